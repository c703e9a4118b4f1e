"""Transformer blocks of the SD-v1 UNet with the spatial-temporal cross-attention routed through
the gfx950 fused kernels (sta.ops -> csrc/sta_xattn.hip).

Drop-in surface of the reference's ldm/modules/attention.py (same class names, constructor
arguments, parameter names and forward signatures, so SD-v1-4 state_dicts load unchanged):
  CrossAttention          reference :157-215
  BasicTransformerBlock   reference :223-300
  SpatialTransformer      reference :303-346
  GEGLU / FeedForward     reference :42-69

What is different by design:
  * norm2 / to_q run ONCE per block call instead of K+1 times (identical results in the reference);
  * K/V of the K+2 contexts are projected and packed once per prompt, not once per UNet call;
  * the K+1 attentions, the disc mask and the coef-weighted blend are one kernel launch producing the
    pre-projection blend; `to_out` is applied once (affine => equal to the reference's blend of
    projected outputs, attention.py:279-294);
  * everything is out of place, so autograd works without the CUDA-autocast accident the
    reference's in-place writes rely on (SURVEY.md §7 hard part (a)).
"""
import math
import os

import torch
import torch.nn.functional as F
from torch import nn

from ldm.modules.diffusionmodules.util import checkpoint, zero_module, Normalize
from sta import fused as _fused
from sta import ops as _ops
from sta.mxfp8 import MxFp8Linear
from sta import prompt_state as _ps


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)

    def forward(self, x):
        if isinstance(self.proj, MxFp8Linear):
            return self.proj.forward_geglu(x)         # projection + gelu + mul as ONE MXFP8 GEMM (csrc/sta_mxfp8.hip)
        h = self.proj(x)
        if _fused.usable(h):
            return _fused.geglu(h)                     # chunk + gelu + mul in one pass (csrc/sta_unet.hip)
        if _fused.tracked_usable(h):
            return _fused.geglu_tracked(h)             # the same pass under autograd, HIP input gradient
        a, gate = h.chunk(2, dim=-1)
        return a * F.gelu(gate)


class FeedForward(nn.Module):
    def __init__(self, dim, dim_out=None, mult=4, glu=False, dropout=0.0):
        super().__init__()
        inner = int(dim * mult)
        dim_out = dim if dim_out is None else dim_out
        first = GEGLU(dim, inner) if glu else nn.Sequential(nn.Linear(dim, inner), nn.GELU())
        self.net = nn.Sequential(first, nn.Dropout(dropout), nn.Linear(inner, dim_out))

    def forward(self, x):
        net = self.net
        if isinstance(net[0], GEGLU) and isinstance(net[0].proj, MxFp8Linear) and isinstance(net[2], MxFp8Linear):
            # MXFP8 (sta.mxfp8): the GEGLU GEMM writes h as MXFP8 and the output Linear reads it as it is — no quantiser pass
            # between them (net[1] is the inference-time identity Dropout)
            return net[2](net[0].proj.forward_geglu(x, mx_out=True), out_dtype=x.dtype)
        return net(x)


class CrossAttention(nn.Module):
    """Multi-head attention with the reference's parameter layout (to_q/to_k/to_v bias-free,
    to_out = Linear + Dropout). Used directly for self-attention (attn1) and as the parameter
    holder of the fused spatial-temporal path (attn2)."""

    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.0):
        super().__init__()
        inner = dim_head * heads
        context_dim = query_dim if context_dim is None else context_dim
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(context_dim, inner, bias=False)
        self.to_v = nn.Linear(context_dim, inner, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(dropout))

    def forward(self, x, context=None, mask=None, self_attention_region=None):
        if mask is not None or self_attention_region is not None:
            # dead branches on the reference's path (attention.py:187-191, :199-213 hard-code batch 6/2)
            raise NotImplementedError("mask / self_attention_region are not part of the spatial-temporal path")
        h = self.heads
        if context is None and not torch.is_grad_enabled() and _ops.self_attention_supported(x, h):
            return self._self_attention_hip(x)
        if context is None and isinstance(self.to_q, nn.Linear) and _ops.self_attention_train_supported(x, h) \
                and not (self.to_q.weight.requires_grad or self.to_k.weight.requires_grad or self.to_v.weight.requires_grad):
            return self._self_attention_tracked(x)
        context = x if context is None else context
        b, n, _ = x.shape
        q = self.to_q(x).view(b, n, h, -1).transpose(1, 2)
        k = self.to_k(context).view(b, context.shape[1], h, -1).transpose(1, 2)
        v = self.to_v(context).view(b, context.shape[1], h, -1).transpose(1, 2)
        if q.is_cuda:
            # shapes the HIP kernels refuse (N < 64, N % 8, head dims above 160): the reference's own formulation,
            # einsum - softmax - einsum (attention.py:181-196), as plain library GEMMs with an fp32 softmax — no Triton-backed SDPA
            # kernel in the product. No BASELINE config reaches this on the GPU.
            # The [rows, N, M] scores exist in fp32 for one slice of query rows at a time (<= 1 GiB), so memory does not grow as
            # O(N^2) per (batch, head) beyond that slice; under autograd the 16-bit P of every slice is what backward keeps.
            m = k.shape[2]
            rows = max(1, min(n, (1 << 28) // max(1, b * h * m)))
            o = torch.cat([torch.matmul(torch.softmax(torch.matmul(q[:, :, i:i + rows], k.transpose(-1, -2)).float() * self.scale, dim=-1).to(q.dtype), v)
                           for i in range(0, n, rows)], dim=2) if rows < n else \
                torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)).float() * self.scale, dim=-1).to(q.dtype), v)
        else:
            o = F.scaled_dot_product_attention(q, k, v, scale=self.scale)
        return self.to_out(o.transpose(1, 2).reshape(b, n, -1))

    def _self_attention_tracked(self, x):
        """attn1 with autograd (the tracked weight-optimisation epochs, frozen weights): ONE GEMM against [Wq; Wk; Wv], the HIP
        forward that keeps the log-sum-exp, and the HIP backward kernels (sta.ops.SelfAttentionQKV) instead of PyTorch's SDPA —
        whose backward was the largest kernel of the tracked epochs (profiles/r02_config3_breakdown.txt)."""
        ws = (self.to_q.weight, self.to_k.weight, self.to_v.weight)

        def cat():
            # as in _self_attention_hip: softmax scale * log2(e) rides in W_q (fp32 product, rounded once), the kernels run in the
            # log2 domain (scale = ln 2: forward with the running maximum as accumulator initial value, 1112 -> 977 us at level 0,
            # 32 rows); autograd differentiates the GEMM with the folded weight, so dx is unchanged
            wq2 = (ws[0].detach().float() * (self.scale * 1.4426950408889634)).to(ws[0].dtype)
            return torch.cat([wq2, ws[1].detach(), ws[2].detach()])
        o = _ops.SelfAttentionQKV.apply(F.linear(x, _fused.cached_image(self, "wqkv", ws, cat)), self.heads, _ops.LN2)
        return self.to_out(o)

    def _self_attention_hip(self, x, pre_to_out_sfrag=False, pre_to_out=False):
        """attn1 without autograd: the flash-style HIP kernel (csrc/sta_selfattn.hip). `pre_to_out_sfrag`: return the kernel's
        output BEFORE to_out, in its out-fragment order (the block then runs to_out + residual + norm2 as one pass); `pre_to_out`:
        the same row-major (the level-1 pass, plain 16-bit Linears only). q and k come out of ONE
        GEMM against the concatenated [Wq; Wk] (the kernel takes a row stride), V is produced already
        transposed because the PV product wants keys contiguous per channel: ONE plain GEMM W_v . X^T over the
        flattened batch gives [C, B*N], which the kernel reads through (row, batch) strides. (A batched
        `matmul(W_v, x^T)` with the weight broadcast over the batch faults inside the GEMM library from batch 40 up.)"""
        if isinstance(self.to_q, MxFp8Linear):
            return self._self_attention_hip_mx(x)
        if not isinstance(self.to_q, nn.Linear):
            return self._self_attention_hip_fp8(x)
        c = self.to_q.weight.shape[0]
        qk = F.linear(x, self._wqk_cat())                             # [B, N, 2C]
        b, n, _ = x.shape
        vt = torch.mm(self.to_v.weight, x.reshape(b * n, c).t()).view(c, b, n).permute(1, 0, 2)    # [B, C, N] view of [C, B*N]
        o = _ops.self_attention(qk[..., :c], qk[..., c:], vt, self.heads, _ops.LN2, sfrag=pre_to_out_sfrag)
        return o if pre_to_out_sfrag or pre_to_out else self.to_out(o)


    def _wqk_cat(self):
        """[Wq * scale * log2 e; Wk], rebuilt only when a weight tensor changes."""
        wq, wk = self.to_q.weight, self.to_k.weight

        def cat():
            # softmax scale * log2(e) rides in W_q (multiplied in fp32, rounded once): q leaves the GEMM in log2 units and the
            # kernel's exponent is a bare exp2 of the MFMA result (sta_selfattn.hip, PRE)
            wq2 = (wq.detach().float() * (self.scale * 1.4426950408889634)).to(wq.dtype)
            return torch.cat([wq2, wk.detach()])
        return _fused.cached_image(self, "wqk", (wq, wk), cat)

    def _ln_qkv_fragments(self):
        """[Wq'; Wk; Wv] as sta_ln_qkv streams it (csrc/sta_lnqkv.hip), repacked only when a weight tensor changes."""
        wv = self.to_v.weight
        return _fused.cached_image(self, "ln_qkv", (self.to_q.weight, self.to_k.weight, wv), lambda: _fused.pack_ln_qkv_weight(self._wqk_cat(), wv))

    def _self_attention_hip_fp8(self, x):
        """The same with e4m3 weights (sta.fp8, BASELINE configs[4]): x is quantised ONCE per call (sta_quant_rows_fp8) and
        feeds both fp8 GEMMs — [Wq; Wk] (row scales concatenated) and the transposed W_v . x^T."""
        from sta import fp8 as _fp8
        if getattr(self, "_wqk8", None) is None or self._wqk8_src is not self.to_q.weight_q:
            self._wqk8 = _fp8.Fp8Linear(torch.cat([self.to_q.weight_q, self.to_k.weight_q]),          # scale * log2(e) rides in q's fp32 row scales
                                        torch.cat([self.to_q.weight_scale * (self.scale * 1.4426950408889634), self.to_k.weight_scale], dim=1), None)
            self._wqk8_src = self.to_q.weight_q
        b, n, c = x.shape
        xq, sx = _fp8.quant_rows(x.reshape(b * n, c))
        qk = _fp8.scaled_mm(xq, self._wqk8.weight_q.t(), sx, self._wqk8.weight_scale, None, x.dtype).view(b, n, 2 * c)
        vt = self.to_v.forward_transposed(xq, sx, x.dtype).view(c, b, n).permute(1, 0, 2)
        o = _ops.self_attention(qk[..., :c], qk[..., c:], vt, self.heads, _ops.LN2)
        return self.to_out(o)

    def _self_attention_hip_mx(self, x):
        """The same with MXFP8 weights (sta.mxfp8): x is quantised ONCE per call (sta_mx8_quant_rows) and feeds both GEMMs —
        [Wq; Wk] with softmax scale * log2(e) applied to q's fp32 accumulators (col_scale), and W_v . x^T with the operands swapped."""
        from sta import mxfp8 as _mx
        if getattr(self, "_wqk_mx", None) is None or self._wqk_mx_src is not self.to_q.weight_q:
            c = self.to_q.out_features
            self._wqk_mx = (torch.cat([self.to_q.weight_q, self.to_k.weight_q]), torch.cat([self.to_q.weight_scale, self.to_k.weight_scale]),
                            torch.cat([torch.full((c,), self.scale * 1.4426950408889634), torch.ones(c)]).to(x.device))
            self._wqk_mx_src = self.to_q.weight_q
        b, n, c = x.shape
        xq, xs = _mx.quant_rows_mx(x.reshape(b * n, c))
        wq, ws, col_scale = self._wqk_mx
        qk = _mx.gemm(xq, xs, wq, ws, x.dtype, col_scale=col_scale).view(b, n, 2 * c)
        vt = self.to_v.forward_transposed((xq, xs), out_dtype=x.dtype).view(c, b, n).permute(1, 0, 2)
        o = _ops.self_attention(qk[..., :c], qk[..., c:], vt, self.heads, _ops.LN2)
        return self.to_out(o)


class _PromptCache:
    """What a block keeps per prompt for one (N, K) shape: the packed K/V image of the K+2 contexts
    and the disc masks. Buffers are allocated once per shape and refilled in place for later prompts,
    so a captured hipGraph that holds their addresses stays valid across prompts."""
    __slots__ = ("version", "packed", "packed_proj", "qfrag", "ofrag", "mask", "centres")

    def __init__(self):
        self.version = -1
        self.packed = None
        self.packed_proj = None      # forward-only image for the projection-fused kernel (None: shape not taken)
        self.qfrag = False           # that kernel reads norm2's output in query-fragment order (head-pair launches)
        self.ofrag = False           # ... and leaves its output in out-fragment order for the fused to_out + norm3 pass (C = 320)
        self.mask = None
        self.centres = None


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, n_heads, d_head, dropout=0.0, context_dim=None, gated_ff=True, checkpoint=True):
        super().__init__()
        self.attn1 = CrossAttention(query_dim=dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.ff = FeedForward(dim, dropout=dropout, glu=gated_ff)
        self.attn2 = CrossAttention(query_dim=dim, context_dim=context_dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.norm3 = nn.LayerNorm(dim)
        self.checkpoint = checkpoint
        self._caches = {}            # (N, K) -> _PromptCache
        self._last_n = None
        self.keep_maps = False       # parity hook: keep the kernel's [K+2, heads, N, 77] attention maps of the last call
        self.last_maps = None
        self._attn_capture = None    # sta.attnmaps.AttnCapture while one is attached: token maps of this block's calls
        self._attn_loss = None       # sta.attnloss.AttnLayoutLoss while one is attached: differentiable token maps of tracked calls

    # -- per-prompt state (reference: the `time == 981` branch, attention.py:240-263) ---------------
    def _stale(self, cache, centres, time):
        if cache.version != _ps.version() or cache.centres != centres:
            return True
        # Nobody announced prompts through sta.prompt_state: keep the reference's own rule and
        # rebuild at the first timestep of every trajectory (costs the same host sync it pays).
        return _ps.version() == 0 and time is not None and int(time) == _ps.first_timestep()

    @staticmethod
    def _per_image_boxes(bboxs_curr, n_img):
        """bboxs_curr is the reference's list of K [x, y] for one image, or a list of n_img such lists."""
        def is_box(b):                      # [x, y]
            return len(b) == 2 and not isinstance(b[0], (list, tuple))
        if n_img == 1 and (len(bboxs_curr) == 0 or is_box(bboxs_curr[0])):
            boxes = [bboxs_curr]             # the reference's form: K boxes of the one image
        else:
            boxes = list(bboxs_curr)         # one list of boxes per image
        if len(boxes) != n_img or any(len(b) != len(boxes[0]) for b in boxes):
            raise ValueError("need one box list per image, all with the same number of objects (got %d lists for %d images)"
                             % (len(boxes), n_img))
        return tuple(tuple((float(b[0]), float(b[1])) for b in bx) for bx in boxes)

    def prepare_prompt(self, n, context, bboxs_curr, time=None):
        """(Re)build the packed K/V image and the disc masks for N = n pixels. Called lazily from
        forward(), or ahead of time by the sampler before replaying a captured graph."""
        if context.shape[0] % 2:
            raise ValueError("the spatial-temporal block needs CFG pairs [uncond, cond] (even batch), got context %s"
                             % (tuple(context.shape),))
        n_img = context.shape[0] // 2
        centres = self._per_image_boxes(bboxs_curr, n_img)
        K = len(centres[0])
        cache = self._caches.setdefault((n, K, n_img), _PromptCache())
        if not self._stale(cache, centres, time):
            return cache
        dim = math.isqrt(n)
        if dim * dim != n:
            raise ValueError("latent must be square (N=%d)" % n)
        wdtype = self.attn2.to_k.weight.dtype
        with torch.no_grad():
            local = _ps.local_contexts(K, n_img, context.device, wdtype)                  # [I, K, M, Dc]
            ctx = context.to(wdtype).reshape(n_img, 2, context.shape[1], context.shape[2])   # per image: "", global
            ctxs = ctx if local is None else torch.cat([ctx, local], dim=1)                  # + locals
            ctxs = ctxs.reshape(n_img * (K + 2), context.shape[1], context.shape[2])
            k = self.attn2.to_k(ctxs)
            v = self.attn2.to_v(ctxs)
            cache.packed = _ops.pack_kv(k, v, self.attn2.heads, out=cache.packed, n_img=n_img)
            if k.is_cuda and _ops.proj_supported(k.shape[2], self.attn2.heads, k.shape[1], K, N=n, n_img=n_img):
                cache.packed_proj = _ops.pack_kv_proj(k, v, self.attn2.heads, out=cache.packed_proj, n_img=n_img)
                cache.qfrag = _ops.proj_qfrag_supported(k.shape[2], self.attn2.heads, k.shape[1], K, n, n_img)
                cache.ofrag = cache.qfrag and _ops.proj_ofrag_supported(k.shape[2], self.attn2.heads, k.dtype)
            else:
                cache.packed_proj, cache.qfrag, cache.ofrag = None, False, False
            if K:
                m = torch.stack([_ops.disc_mask_bits(c, dim, _ps.disc_radius_sq()) for c in centres]).to(context.device)   # [I, N]
                if cache.mask is None:
                    cache.mask = m
                else:
                    cache.mask.copy_(m)
        cache.version, cache.centres = _ps.version(), centres
        return cache

    def forward(self, x, context=None, time=None, text_index=None, coef=None, bboxs_curr=None, in_bias=None, tail=None):
        """`in_bias` (not in the reference): a per-channel bias the caller still owes to `x` (SpatialTransformer's
        proj_in bias when the projection ran as a bias-free GEMM); it is added inside the first fused pass.
        `tail` (not in the reference): a sta.fused.FfTail from the SpatialTransformer whose LAST block this is — where the fused
        feed-forward path is taken and the shapes allow it, the block's output pass applies proj_out and the transformer's residual
        as well and sets `tail.done`; otherwise the block returns what it returns without `tail`."""
        bboxs_curr = [] if bboxs_curr is None else bboxs_curr
        if context is None:
            raise ValueError("BasicTransformerBlock needs the text context")
        if x.shape[0] % 2 or x.shape[0] != context.shape[0]:
            raise ValueError("the spatial-temporal block needs the CFG batch [uncond, cond] (batch 2 per image), got x %s context %s"
                             % (tuple(x.shape), tuple(context.shape)))
        self._last_n = x.shape[1]
        cache = self.prepare_prompt(x.shape[1], context, bboxs_curr, time)
        if coef is None:
            if len(cache.centres[0]):
                raise ValueError("coef is required when objects are present")
            coef = x.new_zeros(0, dtype=torch.float32)
        al = self._attn_loss
        if al is not None and al.wants(x.shape[1]):
            # the loss's side value cannot leave a checkpointed forward: a recording block keeps its activations (sta.attnloss)
            return self._forward(x, coef, cache, in_bias, tail)
        return checkpoint(lambda xx, cc: self._forward(xx, cc, cache, in_bias, tail), (x, coef), self.parameters(), self.checkpoint)

    def _forward(self, x, coef, cache, in_bias=None, tail=None):
        c = coef if coef.numel() else None
        cap = self._attn_capture                     # None unless an AttnCapture is attached (the one test an ordinary call pays)
        if cap is not None and not cap.wants(x.shape[1]):
            cap = None
        if _fused.usable(x):
            # inference: every residual add runs inside the LayerNorm pass that consumes it (sta_add_layernorm)
            n1, n2, n3 = self.norm1, self.norm2, self.norm3
            a1 = self.attn1
            big = _fused.rowgemm_worthwhile(x)      # enough rows for the persistent row-GEMM passes to fill the chip
            sfrag = big and _ops.self_attention_sfrag_supported(x, a1.heads) and isinstance(a1.to_q, nn.Linear) and isinstance(a1.to_out[0], nn.Linear)
            # level 0: norm1 and the q|k / V^T projections of attn1 are ONE pass (csrc/sta_lnqkv.hip) — norm1's output never reaches HBM
            lnqkv = sfrag and _fused.LN_QKV and all(isinstance(m, nn.Linear) and m.bias is None for m in (a1.to_q, a1.to_k, a1.to_v)) \
                and _fused.ln_qkv_supported(x)
            if lnqkv:
                s, qk, vt = _fused.ln_qkv(x, in_bias, n1.weight, n1.bias, n1.eps, a1._ln_qkv_fragments(), store_sum=in_bias is not None)
            else:
                s, y = _fused.add_layernorm(x, None, in_bias, n1.weight, n1.bias, n1.eps, store_sum=in_bias is not None)
            x = x if s is None else s
            fused_q = cache.packed_proj is not None and not self.keep_maps and cap is None      # a capturing block needs q in HBM
            # the GEGLU projection of the feed-forward as one pass over norm3's output in query-fragment order (csrc/sta_ffgemm.hip)
            # (oversize batches — the [rows, inner] GEGLU output beyond what a launch addresses — take the row-major path)
            ffq = self._ff_fusable(x) and _fused.rowgemm_worthwhile(x, self.ff.net[0].proj.out_features // 2)
            # norm2's output has ONE consumer when to_q runs inside the attention kernel: the pass then writes it in the MFMA
            # operand order that kernel loads (query-fragment order, 1-KiB coalesced loads) instead of row-major
            qfrag = fused_q and cache.qfrag
            to_out_c640 = big and _fused.TO_OUT_LN_C640 and x.shape[-1] == 640
            if sfrag:
                # level 0: the self-attention kernel leaves its output in out-fragment order and attn1.to_out + the residual + norm2
                # are ONE pass over it (csrc/sta_rowgemm.hip) — to_out's result never reaches HBM, y leaves in the order its consumer wants
                if lnqkv:
                    b, n, ch = x.shape
                    o = _ops.self_attention(qk[..., :ch], qk[..., ch:], vt.view(ch, b, n).permute(1, 0, 2), a1.heads, _ops.LN2, sfrag=True)
                else:
                    o = a1._self_attention_hip(y, pre_to_out_sfrag=True)
                x, y = _fused.to_out_add_layernorm_ofrag(x, o, self._wo1_fragments(), a1.to_out[0].bias, n2.weight, n2.bias, n2.eps, a1.heads, y_qfrag=qfrag)
            elif to_out_c640 and isinstance(a1.to_q, nn.Linear) and not isinstance(a1.to_q, MxFp8Linear) and _fused.rows_c640_supported(x, a1.to_out[0]) \
                    and _ops.self_attention_supported(y, a1.heads):
                # level 1: attn1.to_out + the residual + norm2 as ONE pass over the kernel's row-major output (csrc/sta_rows640.hip)
                x, y = _fused.linear_res_c640(x, a1._self_attention_hip(y, pre_to_out=True), a1.to_out[0], n2, y_qfrag=qfrag)
            else:
                x, y = _fused.add_layernorm(x, a1(y), None, n2.weight, n2.bias, n2.eps, qfrag=qfrag)
            if fused_q:
                # to_q runs INSIDE the attention kernel: no [2I, N, C] query round trip through HBM
                ofrag = qfrag and cache.ofrag and isinstance(self.attn2.to_out[0], nn.Linear) and _fused.rows_addressable(x)
                blended = _ops.xattn_forward_proj(y, self._wq_fragments(), cache.packed_proj, cache.mask, c, self.attn2.scale, qfrag=qfrag, ofrag=ofrag)
                if ofrag:
                    # ... and to_out + the residual + norm3 are ONE pass over the kernel's out-fragment output: to_out's [2I, N, C]
                    # result never reaches HBM either (csrc/sta_rowgemm.hip)
                    lin = self.attn2.to_out[0]
                    x, y = _fused.to_out_add_layernorm_ofrag(x, blended, self._wo_fragments(), lin.bias, n3.weight, n3.bias, n3.eps, self.attn2.heads,
                                                             y_qfrag=ffq)
                    return self._ff_tail(x, y, ffq, tail)
            else:
                q = self.attn2.to_q(y)
                self._keep_maps(q, c, cache)
                if cap is not None:
                    cap.record(self, q, cache)
                blended = _ops.xattn_blend(q, c, cache.packed, cache.mask, self.attn2.scale)
            if to_out_c640 and blended.is_contiguous() and _fused.rows_c640_supported(x, self.attn2.to_out[0]):
                # level 1: attn2.to_out + the residual + norm3 as ONE pass (to_out[1] is Dropout(0))
                x, y = _fused.linear_res_c640(x, blended, self.attn2.to_out[0], n3, y_qfrag=ffq)
            else:
                x, y = _fused.add_layernorm(x, self.attn2.to_out(blended), None, n3.weight, n3.bias, n3.eps, qfrag=ffq)
            return self._ff_tail(x, y, ffq, tail)
        al = self._attn_loss                         # an AttnLayoutLoss records only while autograd is enabled: the two branches below
        if al is not None and not al.wants(x.shape[1]):
            al = None
        if _fused.tracked_usable(x):
            # tracked epochs (opt-in, fused.TRACKED): the residual adds run inside the LayerNorm passes as above, each pass an
            # autograd Function whose backward is one HIP input-gradient kernel (parameters are frozen)
            n1, n2, n3 = self.norm1, self.norm2, self.norm3
            x, y = _fused.add_layernorm_tracked(x, None, in_bias, n1.weight, n1.bias, n1.eps)
            x, y = _fused.add_layernorm_tracked(x, self.attn1(y), None, n2.weight, n2.bias, n2.eps)
            q = self.attn2.to_q(y)
            self._keep_maps(q, c, cache)
            if cap is not None:
                cap.record(self, q, cache)
            if al is not None:
                al.record(self, q, cache)
            blended = _ops.xattn_blend(q, c, cache.packed, cache.mask, self.attn2.scale)
            x, y = _fused.add_layernorm_tracked(x, self.attn2.to_out(blended), None, n3.weight, n3.bias, n3.eps)
            return self.ff(y) + x
        if in_bias is not None:
            x = x + in_bias
        x = self.attn1(self.norm1(x)) + x
        q = self.attn2.to_q(self.norm2(x))
        self._keep_maps(q, c, cache)
        if cap is not None:
            cap.record(self, q, cache)
        if al is not None:
            al.record(self, q, cache)
        blended = _ops.xattn_blend(q, c, cache.packed, cache.mask, self.attn2.scale)
        x = self.attn2.to_out(blended) + x
        return self.ff(self.norm3(x)) + x

    def _wq_fragments(self):
        """to_q.weight of attn2 in MFMA operand order, repacked only when the weight tensor changes."""
        w = self.attn2.to_q.weight
        return _fused.cached_image(self, "wq", (w,), lambda: _ops.pack_wq(w, self.attn2.heads))

    def _ff_c640(self, x):
        """Level 1 (C = 640): the GEGLU projection pass of csrc/sta_ffgemm.hip in front of the library output Linear."""
        net = self.ff.net
        return _fused.FF_GEGLU_C640 and isinstance(net[2], nn.Linear) and _fused.ff_geglu_c640_supported(x.shape[-1], net[0].proj.out_features // 2)

    def _ff_fusable(self, x):
        net = self.ff.net
        return isinstance(net[0], GEGLU) and isinstance(net[0].proj, nn.Linear) and (x.numel() // x.shape[-1]) % 16 == 0 \
            and (_fused.ff_geglu_supported(x.shape[-1], net[0].proj.out_features // 2) or self._ff_c640(x))

    def _ff_tail(self, x, y, ffq, tail=None):
        """x + ff(y) (attention.py:299). `ffq`: y is in query-fragment order and the GEGLU projection runs as the fused pass.
        `tail`: see forward — with it the output pass is sta.fused.ff_tail and the result is the SpatialTransformer's."""
        if not ffq:
            return self.ff(y) + x
        proj = self.ff.net[0].proj
        if self._ff_c640(x):
            w1 = _fused.cached_image(self, "w1", (proj.weight,), lambda: _fused.pack_geglu_c640_weight(proj.weight))
            h = _fused.ff_geglu_c640_qfrag(y, w1, proj.bias, proj.out_features // 2)
            if _fused.FF_OUT_RES_C640 and _fused.rows_c640_supported(x, self.ff.net[2]):
                if tail is not None and _fused.ff_tail_supported(x, self.ff.net[2], tail.proj_out):
                    return tail.run(x, h, self.ff.net[2])      # ... + proj_out + the transformer's residual (csrc/sta_rowstail.hip)
                # ... and the output Linear + the block's last residual as one pass over row-major h (net[1] is Dropout(0))
                return _fused.linear_res_c640(x, h, self.ff.net[2])[0]
            return self.ff.net[2](self.ff.net[1](h)) + x
        w1 = _fused.cached_image(self, "w1", (proj.weight,), lambda: _fused.pack_geglu_weight(proj.weight))
        out = self.ff.net[2]
        if isinstance(out, nn.Linear):
            # ... and the output Linear + the block's last residual as one pass over h in fragment order (net[1] is Dropout(0))
            h = _fused.ff_geglu_qfrag(y, w1, proj.bias, proj.out_features // 2, h_frag=True)
            if tail is not None and _fused.ff_tail_supported(x, out, tail.proj_out):
                return tail.run(x, h, out)                      # ... + proj_out + the transformer's residual (csrc/sta_rowstail.hip)
            w2 = _fused.cached_image(self, "w2", (out.weight,), lambda: _fused.pack_ff_out_weight(out.weight))
            return _fused.ff_out_res_hfrag(x, h, w2, out.bias)
        h = _fused.ff_geglu_qfrag(y, w1, proj.bias, proj.out_features // 2)
        return out(self.ff.net[1](h)) + x

    def _wo1_fragments(self):
        """attn1.to_out.weight laid out for the self-attention kernel's out-fragment order."""
        w = self.attn1.to_out[0].weight
        return _fused.cached_image(self, "wo1", (w,), lambda: _fused.pack_to_out_weight(w, self.attn1.heads, _fused.FRAG_SELFATTN))

    def _wo_fragments(self):
        """to_out.weight of attn2 as sta_to_out_ln_ofrag streams it, repacked only when the weight tensor changes."""
        w = self.attn2.to_out[0].weight
        return _fused.cached_image(self, "wo", (w,), lambda: _fused.pack_to_out_weight(w, self.attn2.heads))

    def _keep_maps(self, q, coef, cache):
        """Parity hook (off by default): the per-step attention maps are a local of the reference's forward
        (attention.py:194); the kernel can write them out ([K+2, heads, N, 77] fp32) for the tests that pin them."""
        if self.keep_maps:
            with torch.no_grad():
                _, self.last_maps = _ops.xattn_forward(q.detach(), cache.packed, cache.mask, coef, self.attn2.scale, want_maps=True)


class SpatialTransformer(nn.Module):
    """GroupNorm -> 1x1 conv -> [b, hw, c] tokens -> transformer blocks -> 1x1 conv -> residual."""

    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0.0, context_dim=None):
        super().__init__()
        self.in_channels = in_channels
        inner = n_heads * d_head
        self.norm = Normalize(in_channels)
        self.proj_in = nn.Conv2d(in_channels, inner, kernel_size=1, stride=1, padding=0)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(inner, n_heads, d_head, dropout=dropout, context_dim=context_dim) for _ in range(depth)])
        self.proj_out = zero_module(nn.Conv2d(inner, in_channels, kernel_size=1, stride=1, padding=0))

    def forward(self, x, context=None, time=None, text_index=None, coef=None, bboxs_curr=None):
        b, c, h, w = x.shape
        if _fused.usable(x) and (_fused.is_nhwc(x) or b <= 32):     # NCHW path uses weight-broadcast bmm: see _self_attention_hip
            return self._forward_fused(x, context, time, text_index, coef, bboxs_curr)
        if _fused.tracked_usable(x):
            xn = _fused.groupnorm_silu_tracked(x, self.norm.weight, self.norm.bias, self.norm.num_groups, self.norm.eps, silu=False)
        else:
            xn = self.norm(x)
        t = self.proj_in(xn)
        # 'b c h w -> b (h w) c': a free view when the activation is channels_last (NHWC in memory)
        t = t.permute(0, 2, 3, 1).reshape(b, h * w, -1)
        for blk in self.transformer_blocks:
            t = blk(t, context=context, time=time, text_index=text_index, coef=coef, bboxs_curr=bboxs_curr)
        t = t.reshape(b, h, w, -1).permute(0, 3, 1, 2)          # back to [b, c, h, w] without a copy (NHWC strides)
        return self.proj_out(t) + x

    def _forward_fused(self, x, context, time, text_index, coef, bboxs_curr):
        """Inference path on NCHW activations without a layout copy: the two 1x1 convolutions are GEMMs whose
        transposed operand is a VIEW ('b c (hw)' read as [hw, c]; output written as [b, hw, c] resp. [b, c, hw]),
        so neither the 'b c h w -> b (h w) c' permute copy nor its inverse exists; GroupNorm is one pass and the
        proj_out bias and the residual are one pass (csrc/sta_unet.hip). proj_in's bias rides into the first
        block's fused LayerNorm pass."""
        b, c, h, w = x.shape
        inner = self.proj_in.out_channels
        xn = _fused.groupnorm_silu(x, self.norm.weight, self.norm.bias, self.norm.num_groups, self.norm.eps, silu=False)
        w_in, w_out = self.proj_in.weight[:, :, 0, 0], self.proj_out.weight[:, :, 0, 0]          # [out, in] views
        if _fused.is_nhwc(x):
            # channels_last: 'b c h w -> b (h w) c' IS the memory layout; both projections are plain GEMMs
            rows = xn.permute(0, 2, 3, 1).reshape(b, h * w, c)
            if c <= 640 and _fused.linear_rows_supported(rows, w_in):
                # short reductions over many rows: the HIP row GEMM (csrc/sta_gemm.hip; 134 vs 156 us at C = 320, 78 vs 91 at 640)
                t = _fused.linear_rows(rows, _fused.packed_linear_weight(self, self.proj_in, w_in), inner, bias=self.proj_in.bias)
            else:
                t = F.linear(rows, w_in, self.proj_in.bias)
            # the LAST block's feed-forward output pass can apply proj_out, its bias and the residual `+ x_in` as well (one GEMM over
            # [h | x2]: csrc/sta_rowstail.hip); the block says through `tail.done` whether it did
            x_rows = x.permute(0, 2, 3, 1).reshape(b, h * w, c)
            tail = _fused.FfTail(self, self.proj_out, x_rows, h * w if _fused.GN_STATS_FROM_PRODUCER else None) if inner == c else None
            last = len(self.transformer_blocks) - 1
            for i, blk in enumerate(self.transformer_blocks):
                t = blk(t, context=context, time=time, text_index=text_index, coef=coef, bboxs_curr=bboxs_curr, tail=tail if i == last else None)
            if tail is not None and tail.done:
                out = t.view(b, h, w, c).permute(0, 3, 1, 2)                                       # NHWC view of [b, hw, c]
                if hasattr(t, "_sta_stats"):
                    out._sta_stats = t._sta_stats          # the next GroupNorm's statistics, accumulated by the pass's epilogue
                return out
            if _fused.linear_rows_supported(t, w_out):
                # proj_out, its bias and the residual `+ x_in` (attention.py:346) in the GEMM's epilogue: no separate residual pass
                y = _fused.linear_rows(t, _fused.packed_linear_weight(self, self.proj_out, w_out), c, bias=self.proj_out.bias,
                                       res=x_rows, stats_rows=h * w if _fused.GN_STATS_FROM_PRODUCER else None)
                out = y.view(b, h, w, c).permute(0, 3, 1, 2)                                       # NHWC view of [b, hw, c]
                if hasattr(y, "_sta_stats"):
                    out._sta_stats = y._sta_stats          # the next GroupNorm's statistics, accumulated by the GEMM's epilogue
                return out
            y = F.linear(t, w_out).view(b, h, w, c).permute(0, 3, 1, 2)
            return _fused.add_bias_nchw(y, x, self.proj_out.bias)
        t = torch.bmm(xn.view(b, c, h * w).transpose(1, 2), w_in.t().unsqueeze(0).expand(b, c, inner))     # [b, hw, inner]
        for i, blk in enumerate(self.transformer_blocks):
            t = blk(t, context=context, time=time, text_index=text_index, coef=coef, bboxs_curr=bboxs_curr,
                    in_bias=self.proj_in.bias if i == 0 else None)
        y = torch.bmm(w_out.unsqueeze(0).expand(b, c, inner), t.transpose(1, 2))                            # [b, c, hw]
        return _fused.add_bias_nchw(y.view(b, c, h, w), x, self.proj_out.bias)
