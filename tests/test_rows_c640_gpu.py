"""sta_rows_c640 (csrc/sta_rows640.hip): an output Linear of the level-1 block (C = 640) + the residual add (+ the LayerNorm that
follows) as one pass over row-major activations — both instances (K = 640 with LayerNorm, K = 2560 without) against fp64, against
the library pair they replace, their refusals, graph replay, and the C = 640 BasicTransformerBlock with the switches on and off."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from sta.synth import seeded_fill_  # noqa: E402

C = 640
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
LN_EPS = 1e-5
_cache = {}


def _weights(dtype, K):
    """One weight, bias, LayerNorm pair and packed image per (dtype, K) for every case, made once."""
    if (dtype, K) not in _cache:
        from sta import fused
        g = torch.Generator().manual_seed(640 + K)
        w = (torch.randn(C, K, generator=g) / K ** 0.5).to(dtype).cuda()
        bias = (torch.randn(C, generator=g) * 0.3).to(dtype).cuda()
        lw = (1.0 + 0.2 * torch.randn(C, generator=g)).to(dtype).cuda()
        lb = (0.2 * torch.randn(C, generator=g)).to(dtype).cuda()
        _cache[(dtype, K)] = (w, bias, lw, lb, fused.pack_rows_c640_weight(w))
    return _cache[(dtype, K)]


def _inputs(R, K, dtype):
    g = torch.Generator().manual_seed(R + K)
    return torch.randn(R, K, generator=g).to(dtype).cuda(), torch.randn(R, C, generator=g).to(dtype).cuda()


def _worst(got, ref, eps):
    return ((got.double() - ref.double()).abs() / (eps * (1.0 + ref.double().abs()))).max().item()


# one item (seven and a half waves dropped by the descriptors) | exactly one pass | one pass + a partial pass of one item | four
# passes (the last with 16 rows) in ONE workgroup (grid capped to 1: the ring wraps from the last k-step to k-step 0)
CASES = [(16, 0), (128, 0), (144, 0), (400, 1)]


@pytest.mark.parametrize("R,max_wg", CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("y_qfrag", [False, True])
def test_rows_c640_ln_vs_fp64(R, max_wg, dtype, with_bias, y_qfrag):
    """K = 640: s = x + a W^T + b within 1 eps (1 + |ref|) of fp64 torch on the same 16-bit inputs, y within 3 eps (1 + |ref|) of the
    LayerNorm of the STORED s (row-major or, through ops.from_qfrag, in query-fragment order), and s within 4 eps (1 + |s2|) of the
    pair it replaces (library GEMM + sta_add_layernorm): the bounds of test_to_out_add_layernorm_out_fragment_order."""
    from sta import fused, ops
    w, bias, lw, lb, wp = _weights(dtype, 640)
    b = bias if with_bias else None
    a, x = _inputs(R, 640, dtype)
    s, y = fused.rows_c640(x, a, wp, b, lw, lb, LN_EPS, y_qfrag=y_qfrag, max_workgroups=max_wg)
    torch.cuda.synchronize()
    assert s.shape == x.shape and y.shape == x.shape and s.dtype == dtype and torch.isfinite(s).all() and torch.isfinite(y).all()
    if y_qfrag:
        y = ops.from_qfrag(y)
    eps = EPS[dtype]
    s_ref = x.double() + a.double() @ w.double().t() + (b.double() if with_bias else 0.0)
    y_ref = F.layer_norm(s.double(), (C,), lw.double(), lb.double(), LN_EPS)
    s2, _ = fused.add_layernorm(x, F.linear(a, w, b), None, lw, lb, LN_EPS)
    es, ey, e2 = _worst(s, s_ref, eps), _worst(y, y_ref, eps), _worst(s, s2, eps)
    print("rows_c640 K=640 R=%d %s bias=%s qfrag=%s: err / (eps (1 + |ref|)): s %.3f, y %.3f, s vs pair %.3f" % (R, dtype, with_bias, y_qfrag, es, ey, e2))
    assert es <= 1.0, es
    assert ey <= 3.0, ey
    assert e2 <= 4.0, e2
    if max_wg:
        # the grid cap changes which workgroup takes a pass, not one bit of the result
        s1, y1 = fused.rows_c640(x, a, wp, b, lw, lb, LN_EPS, y_qfrag=False)
        assert torch.equal(s, s1) and torch.equal(y, y1)


@pytest.mark.parametrize("R,max_wg", CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("with_bias", [True, False])
def test_rows_c640_ff_out_vs_fp64(R, max_wg, dtype, with_bias):
    """K = 2560, no LayerNorm: s = x + h W^T + b within 1 eps (1 + |ref|) of fp64 and within 4 eps (1 + |s2|) of the library GEMM
    followed by the elementwise add."""
    from sta import fused
    w, bias, _, _, wp = _weights(dtype, 2560)
    b = bias if with_bias else None
    a, x = _inputs(R, 2560, dtype)
    s, y = fused.rows_c640(x, a, wp, b, max_workgroups=max_wg)
    torch.cuda.synchronize()
    assert y is None and s.shape == x.shape and s.dtype == dtype and torch.isfinite(s).all()
    eps = EPS[dtype]
    s_ref = x.double() + a.double() @ w.double().t() + (b.double() if with_bias else 0.0)
    s2 = F.linear(a, w, b) + x
    es, e2 = _worst(s, s_ref, eps), _worst(s, s2, eps)
    print("rows_c640 K=2560 R=%d %s bias=%s: err / (eps (1 + |ref|)): s %.3f, s vs pair %.3f" % (R, dtype, with_bias, es, e2))
    assert es <= 1.0, es
    assert e2 <= 4.0, e2
    if max_wg:
        assert torch.equal(s, fused.rows_c640(x, a, wp, b)[0])


def test_rows_c640_refusals():
    """Other shapes, a row count that is not a multiple of 16, tensors of 4 GiB and above, an unknown dtype, a LayerNorm at K = 2560:
    -1 with the reason in sta_last_error, the outputs untouched; the level-0 entry points keep refusing C = 640."""
    from sta import fused, lib
    L = lib.load()
    dtype = torch.float16
    w, bias, lw, lb, wp = _weights(dtype, 640)
    R = 32
    a = torch.zeros(R + 16, 2560, dtype=dtype, device="cuda")
    x = torch.zeros(R + 16, C, dtype=dtype, device="cuda")
    s = torch.full((R + 16, C), 7.0, dtype=dtype, device="cuda")
    y = torch.full((R + 16, C), 7.0, dtype=dtype, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(rows, c, k, ln=True, max_wg=0, dt=lib.STA_F16):
        return L.sta_rows_c640(a.data_ptr(), wp.data_ptr(), None, x.data_ptr(), lw.data_ptr() if ln else None, lb.data_ptr() if ln else None,
                               s.data_ptr(), y.data_ptr() if ln else None, rows, c, k, LN_EPS, 0, max_wg, dt, st)
    assert L.sta_rows_c640_packed_w_bytes(C, 640) == C * 640 * 2 and L.sta_rows_c640_packed_w_bytes(C, 2560) == C * 2560 * 2
    assert L.sta_rows_c640_packed_w_bytes(320, 320) == 0 and L.sta_rows_c640_packed_w_bytes(C, 1280) == 0 and L.sta_rows_c640_packed_w_bytes(1280, 1280) == 0
    assert L.sta_to_out_ln_packed_wo_bytes(640, 8) == 0 and L.sta_ff_out_packed_w_bytes(C, 2560) == 0
    assert call(R, 320, 320) == -1 and "K = 640 or 2560 only" in lib.last_error()
    assert call(R, C, 1280) == -1 and "K = 640 or 2560 only" in lib.last_error()
    assert call(R, 1280, 640) == -1 and "K = 640 or 2560 only" in lib.last_error()
    assert call(R + 8, C, 640) == -1 and "multiple of 16" in lib.last_error()
    assert call(0, C, 640) == -1 and "multiple of 16" in lib.last_error()
    assert call((1 << 32) // (640 * 2) // 16 * 16 + 16, C, 640) == -1 and "4 GiB" in lib.last_error()
    assert call((1 << 32) // (2560 * 2) // 16 * 16 + 16, C, 2560, ln=False) == -1 and "4 GiB" in lib.last_error()
    assert call(R, C, 640, dt=7) == -1 and "dtype 7" in lib.last_error()
    assert call(R, C, 640, max_wg=-1) == -1 and "max_workgroups" in lib.last_error()
    assert call(R, C, 640, ln=False) == -1 and "null" in lib.last_error()
    assert call(R, C, 2560, ln=True) == -1 and "no LayerNorm" in lib.last_error()
    assert L.sta_rows_c640_pack_w(w.data_ptr(), wp.data_ptr(), 320, 320, lib.STA_F16, st) == -1 and "K = 640 or 2560 only" in lib.last_error()
    assert L.sta_rows_c640_pack_w(w.data_ptr(), wp.data_ptr(), C, 640, 7, st) == -1 and "dtype 7" in lib.last_error()
    torch.cuda.synchronize()
    assert (s == 7.0).all() and (y == 7.0).all()
    with pytest.raises(ValueError):
        fused.pack_rows_c640_weight(torch.zeros(320, 320, dtype=dtype, device="cuda"))
    lin = torch.nn.Linear(640, 640).to("cuda", dtype)
    assert fused.rows_c640_supported(x[:R], lin) and not fused.rows_c640_supported(x[:R + 8], lin)
    assert not fused.rows_c640_supported(x[:R], torch.nn.Linear(1280, 640).to("cuda", dtype))
    assert not fused.rows_c640_supported(x[:R], torch.nn.Linear(640, 640).to("cuda", torch.bfloat16))


@pytest.mark.parametrize("entry,c,K", [("rows_c640", 640, 640), ("rows_c640", 640, 2560), ("ff_tail", 320, 1600), ("ff_tail", 640, 3200)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_row_pass_packed_weight_layout(entry, c, K, dtype):
    """The packed image both row passes stream (csrc/sta_rows_dev.h::rows_pack_kernel, behind sta_rows_c640_pack_w and sta_ff_tail_pack_w)
    at every shape the two entry points accept, bit for bit against the layout restated in numpy: fragment f * nrt + u (nrt = C / 16),
    lane (g, c), the 8 values W[frag_sigma(u, c)][32 f + 8 g .. + 7]. The weight is a hash of the flat index, as 16-bit patterns (the
    pack is a copy: NaN patterns travel like any other), so a transposed or shifted index shows."""
    from sta import fused
    idx = np.arange(c * K, dtype=np.uint64)
    bits = (((idx * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(0xffff)).astype(np.uint16).view(np.int16).reshape(c, K)
    w = torch.from_numpy(bits).view(dtype).cuda()
    packed = fused.pack_rows_c640_weight(w) if entry == "rows_c640" else fused.pack_ff_tail_weight(w)
    torch.cuda.synchronize()
    nrt, nks = c // 16, K // 32
    assert packed.dtype == torch.uint8 and packed.numel() == c * K * 2
    got = packed.cpu().numpy().view(np.int16).reshape(nks, nrt, 4, 16, 8)              # [f][u][g][c][8]
    u, rho = np.arange(nrt)[:, None], np.arange(16)[None, :]
    sigma = 32 * (u >> 1) + 8 * (rho >> 2) + 4 * (u & 1) + (rho & 3)                     # frag_sigma(u, c): [nrt][16]
    col = 32 * np.arange(nks)[:, None, None] + 8 * np.arange(4)[None, :, None] + np.arange(8)[None, None, :]     # [f][g][8]
    want = bits[sigma[None, :, None, :, None], col[:, None, :, None, :]]
    assert want.shape == got.shape and np.array_equal(got, want)


@pytest.mark.parametrize("K", [640, 2560])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_rows_c640_graph_replay_is_bit_equal(dtype, K):
    """One captured launch replays to the bits of the eager launch (three passes in one workgroup: the counted waits hold in replay)."""
    from sta import fused
    w, bias, lw, lb, wp = _weights(dtype, K)
    a, x = _inputs(272, K, dtype)
    ln = (lw, lb, LN_EPS) if K == 640 else ()

    def run():
        return fused.rows_c640(x, a, wp, bias, *ln, max_workgroups=1)
    s0, y0 = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                           # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s1, y1 = run()
    s1.zero_()
    if y1 is not None:
        y1.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s0, s1) and (y0 is None or torch.equal(y0, y1))


def _block_case(dtype):
    from ldm.modules.attention import BasicTransformerBlock
    g = np.load(os.path.join(gi.GOLDEN, "block_d80.npz"), allow_pickle=False)
    dim, c, heads, K, seed = (int(g[k]) for k in ("dim", "C", "heads", "K", "seed"))
    assert c == C
    x, context, local_ctx = gi.block_inputs(dim, c, K, seed, gi.load_uncond())
    x, context = x.cuda().to(dtype), context.cuda().to(dtype)
    coef, boxes = torch.from_numpy(g["coef"]).cuda(), [list(cc) for cc in g["centres"]]

    def make(state=None):
        blk = BasicTransformerBlock(c, heads, c // heads, context_dim=768, checkpoint=False)
        if state is None:
            seeded_fill_(blk, seed)
        blk = blk.to("cuda", dtype)
        if state is not None:
            blk.load_state_dict(state)
        return blk

    def run(blk):
        with torch.no_grad():
            return blk(x, context=context, time=torch.tensor(981), coef=coef, bboxs_curr=boxes)
    return g, local_ctx, make, run


def _count_passes(monkeypatch):
    from sta import fused
    n, real, real_ln = {"rows": 0, "ln": 0}, fused.rows_c640, fused.add_layernorm
    monkeypatch.setattr(fused, "rows_c640", lambda *a, **k: (n.__setitem__("rows", n["rows"] + 1), real(*a, **k))[1])
    monkeypatch.setattr(fused, "add_layernorm", lambda *a, **k: (n.__setitem__("ln", n["ln"] + 1), real_ln(*a, **k))[1])
    return n


@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_block_c640_rows_vs_reference_golden(dtype, on, monkeypatch):
    """The C = 640 BasicTransformerBlock (every row pass allowed at its 128 rows) against the reference's fp32 block output, the
    bounds of test_block_c640_vs_reference_golden. Switches on: the new pass runs exactly three times (two to_out sites, the
    feed-forward output) and sta_add_layernorm once (norm1); off: never, and the three LayerNorm passes are back."""
    from sta import fused, prompt_state
    monkeypatch.setattr(fused, "ROWGEMM_MIN_ROWS", 0)
    monkeypatch.setattr(fused, "TO_OUT_LN_C640", on)
    monkeypatch.setattr(fused, "FF_OUT_RES_C640", on)
    n = _count_passes(monkeypatch)
    g, local_ctx, make, run = _block_case(dtype)
    prompt_state.begin_prompt([c.cuda() for c in local_ctx], first_timestep=981)
    out = run(make())
    assert n == ({"rows": 3, "ln": 1} if on else {"rows": 0, "ln": 3}), n
    ref = g["out"]
    eps = EPS[dtype]
    err = np.abs(out.float().cpu().numpy() - ref)
    print("block d80 %s rows_c640=%s: max %.4g (bound %.4g) mean %.4g (bound %.4g)"
          % (dtype, on, err.max(), 8 * eps * np.abs(ref).max(), err.mean(), 4 * eps * np.abs(ref).mean()))
    assert err.max() <= 8 * eps * np.abs(ref).max(), (err.max(), np.abs(ref).max())
    assert err.mean() <= 4 * eps * np.abs(ref).mean(), (err.mean(), np.abs(ref).mean())


@pytest.mark.parametrize("which", ["attn1", "attn2", "ff"])
def test_block_c640_rows_repacks_updated_weight(which, monkeypatch):
    """An in-place update of a to_out / net[2] weight is followed by a repack: the block that holds an image of the old weight gives
    the output of a FRESH block loaded from the updated state_dict, bit for bit (same kernels, same inputs)."""
    from sta import fused, prompt_state
    monkeypatch.setattr(fused, "ROWGEMM_MIN_ROWS", 0)
    n = _count_passes(monkeypatch)
    g, local_ctx, make, run = _block_case(torch.float16)
    prompt_state.begin_prompt([c.cuda() for c in local_ctx], first_timestep=981)
    blk = make()
    before = run(blk)
    assert n["rows"] == 3
    lin = {"attn1": blk.attn1.to_out[0], "attn2": blk.attn2.to_out[0], "ff": blk.ff.net[2]}[which]
    with torch.no_grad():
        lin.weight.mul_(0.5)
    got = run(blk)
    want = run(make(blk.state_dict()))
    assert not torch.equal(want, before)            # the update is visible in the output at all
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
