"""MXFP8 (OCP MX v1.0: e4m3fn elements, one e8m0 scale per 32 consecutive K elements) for the Linear layers of the transformer
blocks — BASELINE configs[4] ("fp8 UNet weights on CDNA4 fp8 MFMA") on gfx950's block-scaled MFMA, csrc/sta_mxfp8.hip.

Which layers: the same 7 per block as sta.fp8 (attn1.to_q/to_k/to_v, both to_out, GEGLU.proj, the FeedForward output Linear);
attn2.to_q/to_k/to_v stay 16 bit (the cross-attention maps are held to 1e-3).

How: weights are quantised once (`MxFp8Linear.from_linear`), activations per call by `sta_mx8_quant_rows`; the GEMM is this project's
own kernel `sta_mx8_gemm` (v_mfma_scale_f32_32x32x64_f8f6f4, twice the 16-bit MFMA rate) with the scales applied inside the MFMA and
an epilogue that writes 16 bit directly (no cast pass), optionally scales columns (attn1's softmax scale * log2 e on q), adds the
bias, or runs GEGLU (value * gelu_erf(gate)) — with the GEGLU result optionally leaving as MXFP8, which the FeedForward output Linear
then reads without a quantiser pass. Inference only (no autograd through the quantiser).

An MXFP8 tensor here is the pair (q, s): q [R, K] torch.float8_e4m3fn, s [R, K/32] torch.uint8 (e8m0: scale = 2^(s - 127)).
"""
import torch
from torch import nn

from . import lib as _lib

F8 = torch.float8_e4m3fn
E4M3_MAX = 448.0
E4M3_EMAX = 8
_DT = {torch.bfloat16: _lib.STA_BF16, torch.float16: _lib.STA_F16}


def _check16(x2d):
    if not x2d.is_cuda or x2d.dtype not in _DT:
        raise RuntimeError("MXFP8 needs 16-bit CUDA/HIP tensors (there is no CPU path; quant_rows_mx_reference is the host restatement)")


def quant_rows_mx(x2d):
    """x [R, K] 16-bit CUDA (K % 32 == 0) -> (q [R, K] e4m3fn, s [R, K/32] uint8 e8m0) through sta_mx8_quant_rows."""
    _check16(x2d)
    x2d = x2d.contiguous()
    R, K = x2d.shape
    if K % 32:
        raise RuntimeError("MXFP8 needs K %% 32 == 0, got %d" % K)
    q = torch.empty((R, K), dtype=F8, device=x2d.device)
    s = torch.empty((R, K // 32), dtype=torch.uint8, device=x2d.device)
    _lib.check(_lib.load().sta_mx8_quant_rows(x2d.data_ptr(), q.data_ptr(), s.data_ptr(), R, K, _DT[x2d.dtype],
                                              torch.cuda.current_stream(x2d.device).cuda_stream), "sta_mx8_quant_rows")
    return q, s


def quant_rows_mx_reference(x2d):
    """The OCP MX rule in plain torch (any device; the tests run it on the CPU): per 32-block X = 2^clamp(floor(log2 amax) - 8, -127,
    127), q = e4m3fn(clamp(x / X, -448, 448)) (torch's cast rounds to nearest even), s = log2 X + 127; an all-zero block gets s = 127.
    x / X is a power-of-two rescale (exact in fp32). The rule puts amax / X in [256, 512), so a block maximum whose quotient is above 448
    saturates (about one block in five for Gaussian data): the price of the OCP rule against a per-row absmax / 448 scale."""
    R, K = x2d.shape
    xb = x2d.float().reshape(R, K // 32, 32)
    amax = xb.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)                               # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, (ex - 1 - E4M3_EMAX).clamp(-127, 127), torch.zeros_like(ex))
    q = torch.ldexp(xb, -e.unsqueeze(-1).float()).clamp(-E4M3_MAX, E4M3_MAX).to(F8)
    return q.reshape(R, K), (e + 127).to(torch.uint8)


def dequant_mx(q, s):
    """(q [R, K], s [R, K/32]) -> fp32 [R, K]."""
    R, K = q.shape
    return torch.ldexp(q.float().reshape(R, K // 32, 32), (s.to(torch.int32) - 127).unsqueeze(-1).float()).reshape(R, K)


def pack_geglu_rows(n2):
    """Row order of the GEGLU projection that sta_mx8_gemm's GEGLU epilogue wants: groups of 64 rows, each 32 value rows h .. h+31
    then the gate rows H + h .. H + h + 31 (H = n2 / 2). Index tensor: packed[i] = original[perm[i]]; unpack by argsort(perm)."""
    H = n2 // 2
    if n2 % 64:
        raise RuntimeError("the GEGLU epilogue needs the projection width %% 64 == 0, got %d" % n2)
    g = torch.arange(H // 32).repeat_interleave(32) * 32 + torch.arange(32).repeat(H // 32)     # h in order
    return torch.stack([g.view(-1, 32), g.view(-1, 32) + H], dim=1).reshape(-1)


def gemm(p, ps, q, qs, out_dtype, bias=None, col_scale=None, geglu=False, mx_out=False):
    """out[m, n] = sum_k P[m, k] Q[n, k] (both MXFP8, fp32 accumulation) -> 16-bit [M, N] (* col_scale[n] + bias[n]);
    geglu=True: Q packed by pack_geglu_rows -> [M, N/2] of value * gelu_erf(gate); mx_out=True: that result as MXFP8 (q, s)."""
    M, K = p.shape
    N = q.shape[0]
    if q.shape[1] != K or ps.shape != (M, K // 32) or qs.shape != (N, K // 32):
        raise RuntimeError("MXFP8 GEMM operand shapes: P %s ps %s Q %s qs %s" % (tuple(p.shape), tuple(ps.shape), tuple(q.shape), tuple(qs.shape)))
    if out_dtype not in _DT:
        raise RuntimeError("MXFP8 GEMM writes fp16 or bf16, not %s" % out_dtype)
    W = N // 2 if geglu else N
    if mx_out:
        out = torch.empty((M, W), dtype=F8, device=p.device)
        out_s = torch.empty((M, W // 32), dtype=torch.uint8, device=p.device)
    else:
        out, out_s = torch.empty((M, W), dtype=out_dtype, device=p.device), None
    if bias is not None:
        bias = bias.to(out_dtype).contiguous()
    if col_scale is not None:
        col_scale = col_scale.float().contiguous()
    flags = (_lib.STA_MX8_GEGLU if geglu else 0) | (_lib.STA_MX8_MX_OUT if mx_out else 0)
    _lib.check(_lib.load().sta_mx8_gemm(p.data_ptr(), ps.data_ptr(), q.data_ptr(), qs.data_ptr(), out.data_ptr(),
                                        None if out_s is None else out_s.data_ptr(), None if bias is None else bias.data_ptr(),
                                        None if col_scale is None else col_scale.data_ptr(), M, N, K, W, flags, _DT[out_dtype],
                                        torch.cuda.current_stream(p.device).cuda_stream), "sta_mx8_gemm")
    return (out, out_s) if mx_out else out


def _as_mx(x, K):
    """x: a 16-bit tensor [..., K] or an already quantised (q, s) pair -> (q [R, K], s [R, K/32], leading shape, dtype or None)."""
    if isinstance(x, tuple):
        q, s = x
        return q.reshape(-1, K), s.reshape(-1, K // 32), tuple(q.shape[:-1]), None
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("MxFp8Linear is an inference layer (BASELINE configs[4] has fixed blend weights)")
    q, s = quant_rows_mx(x.reshape(-1, K))
    return q, s, tuple(x.shape[:-1]), x.dtype


class MxFp8Linear(nn.Module):
    """Drop-in for nn.Linear at inference (same call signature, `in_features` / `out_features`): MXFP8 weight, 16-bit bias.
    forward / forward_geglu / forward_transposed also take an already quantised input (q, s), so one quantisation feeds several
    GEMMs; the output dtype is then `out_dtype`."""

    def __init__(self, wq, ws, bias, dtype):
        super().__init__()
        self.out_features, self.in_features = wq.shape
        self.dtype = dtype
        self.register_buffer("weight_q", wq)
        self.register_buffer("weight_scale", ws)
        self.bias = None if bias is None else nn.Parameter(bias.detach().clone(), requires_grad=False)
        self._geglu = None

    @classmethod
    def from_linear(cls, lin):
        w = lin.weight.detach()
        if lin.in_features % 32:
            raise RuntimeError("MXFP8 needs in_features %% 32 == 0, got %d" % lin.in_features)
        wq, ws = quant_rows_mx(w) if w.is_cuda and w.dtype in _DT else quant_rows_mx_reference(w)
        return cls(wq, ws, lin.bias, w.dtype if w.dtype in _DT else torch.float16)

    def forward(self, x, out_dtype=None):
        q, s, lead, dt = _as_mx(x, self.in_features)
        out = gemm(q, s, self.weight_q, self.weight_scale, out_dtype or dt or self.dtype, bias=self.bias)
        return out.view(*lead, self.out_features)

    def forward_geglu(self, x, mx_out=False, out_dtype=None):
        """GEGLU (reference attention.py:47-49) over this projection: value * gelu_erf(gate), [..., out_features / 2], in ONE GEMM;
        mx_out=True returns it as MXFP8 (q, s) for the next MxFp8Linear."""
        if self._geglu is None or self._geglu[0] is not self.weight_q:
            perm = pack_geglu_rows(self.out_features).to(self.weight_q.device)
            self._geglu = (self.weight_q, self.weight_q.view(torch.uint8)[perm].view(F8), self.weight_scale[perm].contiguous(),
                           None if self.bias is None else self.bias.detach()[perm].contiguous())
        _, wq, ws, b = self._geglu
        q, s, lead, dt = _as_mx(x, self.in_features)
        out = gemm(q, s, wq, ws, out_dtype or dt or self.dtype, bias=b, geglu=True, mx_out=mx_out)
        H = self.out_features // 2
        if mx_out:
            return out[0].view(*lead, H), out[1].view(*lead, H // 32)
        return out.view(*lead, H)

    def forward_transposed(self, x, out_dtype=None):
        """W . x^T: [out_features, R] (the self-attention kernel wants V transposed) — the same GEMM with the operands swapped."""
        q, s, _, dt = _as_mx(x, self.in_features)
        return gemm(self.weight_q, self.weight_scale, q, s, out_dtype or dt or self.dtype)


def convert_transformer_linears_mx_(unet):
    """In place: the same 7 Linear layers per BasicTransformerBlock as sta.fp8.convert_transformer_linears_ become MxFp8Linear.
    Returns (number converted, 16-bit bytes before, bytes after: e4m3 weight + e8m0 scales)."""
    from ldm.modules.attention import BasicTransformerBlock
    n = before = after = 0
    for blk in unet.modules():
        if not isinstance(blk, BasicTransformerBlock):
            continue
        sites = [(blk.attn1, "to_q"), (blk.attn1, "to_k"), (blk.attn1, "to_v"), (blk.attn1.to_out, "0"), (blk.attn2.to_out, "0"),
                 (blk.ff.net[0], "proj"), (blk.ff.net, "2")]
        for parent, name in sites:
            lin = getattr(parent, name)
            if isinstance(lin, nn.Linear):
                q = MxFp8Linear.from_linear(lin)
                before += lin.weight.numel() * lin.weight.element_size()
                after += q.weight_q.numel() + q.weight_scale.numel()
                setattr(parent, name, q)
                n += 1
    return n, before, after
