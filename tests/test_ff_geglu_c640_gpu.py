"""sta_ff_geglu_c640_qfrag (csrc/sta_ffgemm.hip): the GEGLU projection + gelu * mul of the level-1 feed-forward (C = 640,
inner = 2560) as one pass — the kernel against fp64, its refusals, and the C = 640 BasicTransformerBlock with the pass on and off."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from sta.synth import seeded_fill_  # noqa: E402

C, INNER = 640, 2560
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
_cache = {}


def _weights(dtype):
    """One weight and bias per dtype for every case (and its packed image), made once."""
    if dtype not in _cache:
        from sta import fused
        g = torch.Generator().manual_seed(640)
        w = (torch.randn(2 * INNER, C, generator=g) / C ** 0.5).to(dtype)
        bias = (torch.randn(2 * INNER, generator=g) * 0.3).to(dtype)
        _cache[dtype] = (w.cuda(), bias.cuda(), fused.pack_geglu_c640_weight(w.cuda()))
    return _cache[dtype]


# one item (the wave's second item and seven waves dropped by the descriptor) | exactly one pass | one pass + a ragged pass of one
# item | three passes and a ragged one in ONE workgroup (grid capped to 1: the ring wraps from the last sub-chunk to sub-chunk 0)
@pytest.mark.parametrize("R,max_wg", [(16, 0), (256, 0), (272, 0), (256 * 3 + 48, 1)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("with_bias", [True, False])
def test_ff_geglu_c640_kernel_vs_fp64(R, max_wg, dtype, with_bias):
    """h = (y Wv^T + bv) * gelu(y Wg^T + bg) from y in query-fragment order against fp64 torch on the same 16-bit inputs (exact-erf
    GELU): every element within 2 eps (1 + |ref|), the bound of the level-0 pass; against the pair it replaces (library GEMM
    rounding its result to 16 bit, then sta_geglu) within 16 eps (1 + |h2|)."""
    from sta import fused, ops
    w, bias, wp = _weights(dtype)
    b = bias if with_bias else None
    g = torch.Generator().manual_seed(R + 7)
    y = torch.randn(R, C, generator=g).to(dtype).cuda()
    h = fused.ff_geglu_c640_qfrag(ops.to_qfrag(y), wp, b, INNER, max_workgroups=max_wg)
    torch.cuda.synchronize()
    assert h.shape == (R, INNER) and h.dtype == dtype and torch.isfinite(h).all()
    proj = y.double() @ w.double().t() + (b.double() if with_bias else 0.0)
    ref = proj[:, :INNER] * F.gelu(proj[:, INNER:])
    eps = EPS[dtype]
    worst = ((h.double() - ref).abs() / (eps * (1.0 + ref.abs()))).max().item()
    h2 = fused.geglu(F.linear(y, w, b))
    worst2 = ((h.float() - h2.float()).abs() / (eps * (1.0 + h2.float().abs()))).max().item()
    print("ff_geglu_c640 R=%d %s bias=%s: max err / (eps (1 + |ref|)): fp64 %.3f, pair %.3f" % (R, dtype, with_bias, worst, worst2))
    assert worst <= 2.0, worst
    assert worst2 <= 16.0, worst2
    if max_wg:
        # the grid cap changes which workgroup takes a pass, not one bit of the result
        assert torch.equal(h, fused.ff_geglu_c640_qfrag(ops.to_qfrag(y), wp, b, INNER))


def test_ff_geglu_c640_refusals():
    """A row count that is not a multiple of 16, other shapes, an output past 4 GiB: non-zero return, the reason in sta_last_error,
    the output untouched; the level-0 entry points keep refusing C = 640."""
    from sta import fused, lib
    L = lib.load()
    dtype = torch.float16
    w, bias, wp = _weights(dtype)
    R = 32
    y = torch.zeros(R + 16, C, dtype=dtype, device="cuda")
    h = torch.full((R + 16, INNER), 7.0, dtype=dtype, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(rows, c, inner, max_wg=0):
        return L.sta_ff_geglu_c640_qfrag(y.data_ptr(), wp.data_ptr(), None, h.data_ptr(), rows, c, inner, max_wg, lib.STA_F16, st)
    assert L.sta_ff_geglu_c640_packed_w_bytes(C, INNER) == 2 * INNER * C * 2
    assert L.sta_ff_geglu_c640_packed_w_bytes(320, 1280) == 0 and L.sta_ff_geglu_c640_packed_w_bytes(1280, 5120) == 0
    assert L.sta_ff_geglu_packed_w_bytes(C, INNER) == 0 and L.sta_ff_out_packed_w_bytes(C, INNER) == 0
    assert call(R + 8, C, INNER) == -1 and "multiple of 16" in lib.last_error()
    assert call(R, 320, 1280) != 0 and "C = 640, inner = 2560 only" in lib.last_error()
    assert call(R, 1280, 5120) != 0 and "C = 640, inner = 2560 only" in lib.last_error()
    big = (1 << 32) // (INNER * 2) // 16 * 16 + 16
    assert call(big, C, INNER) != 0 and "4 GiB" in lib.last_error()
    assert call(R, C, INNER, -1) != 0 and "max_workgroups" in lib.last_error()
    assert L.sta_ff_geglu_c640_pack_w(w.data_ptr(), wp.data_ptr(), 320, 1280, lib.STA_F16, st) != 0 and "C = 640, inner = 2560 only" in lib.last_error()
    assert L.sta_ff_geglu_pack_w(w.data_ptr(), wp.data_ptr(), C, INNER, lib.STA_F16, st) != 0 and "C = 320, inner = 1280 only" in lib.last_error()
    torch.cuda.synchronize()
    assert (h == 7.0).all()
    assert fused.ff_geglu_c640_supported(C, INNER) and not fused.ff_geglu_c640_supported(320, 1280) and not fused.ff_geglu_supported(C, INNER)
    with pytest.raises(ValueError):
        fused.pack_geglu_c640_weight(torch.zeros(2560, 320, dtype=dtype, device="cuda"))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_ff_geglu_c640_graph_replay_is_bit_equal(dtype):
    """One captured launch replays to the bits of the eager launch (two passes in one workgroup: the counted waits hold in replay)."""
    from sta import fused, ops
    w, bias, wp = _weights(dtype)
    g = torch.Generator().manual_seed(3)
    yq = ops.to_qfrag(torch.randn(512, C, generator=g).to(dtype).cuda())
    h0 = fused.ff_geglu_c640_qfrag(yq, wp, bias, INNER, max_workgroups=1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.ff_geglu_c640_qfrag(yq, wp, bias, INNER, max_workgroups=1)        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h1 = fused.ff_geglu_c640_qfrag(yq, wp, bias, INNER, max_workgroups=1)
    h1.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(h0, h1)


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
    n, real, real0 = {"c640": 0, "level0": 0, "geglu": 0}, fused.ff_geglu_c640_qfrag, fused.ff_geglu_qfrag
    real_g = fused.geglu
    monkeypatch.setattr(fused, "ff_geglu_c640_qfrag", lambda *a, **k: (n.__setitem__("c640", n["c640"] + 1), real(*a, **k))[1])
    monkeypatch.setattr(fused, "ff_geglu_qfrag", lambda *a, **k: (n.__setitem__("level0", n["level0"] + 1), real0(*a, **k))[1])
    monkeypatch.setattr(fused, "geglu", lambda *a, **k: (n.__setitem__("geglu", n["geglu"] + 1), real_g(*a, **k))[1])
    return n


@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_block_c640_vs_reference_golden(dtype, on, monkeypatch):
    """The C = 640 BasicTransformerBlock (every row-GEMM pass allowed at its 128 rows) against the reference's fp32 block output,
    the bounds of test_block_vs_reference_golden: switch on, the new pass runs exactly once (and never through the level-0 name);
    switch off, never — the library GEMM + sta_geglu pair is back."""
    from sta import fused, prompt_state
    monkeypatch.setattr(fused, "ROWGEMM_MIN_ROWS", 0)
    monkeypatch.setattr(fused, "FF_GEGLU_C640", on)
    n = _count_passes(monkeypatch)
    g, local_ctx, make, run = _block_case(dtype)
    prompt_state.begin_prompt([c.cuda() for c in local_ctx], first_timestep=981)
    out = run(make())
    assert n == ({"c640": 1, "level0": 0, "geglu": 0} if on else {"c640": 0, "level0": 0, "geglu": 1}), n
    ref = g["out"]
    eps = EPS[dtype]
    err = np.abs(out.float().cpu().numpy() - ref)
    print("block d80 %s FF_GEGLU_C640=%s: max %.4g (bound %.4g) mean %.4g (bound %.4g)"
          % (dtype, on, err.max(), 8 * eps * np.abs(ref).max(), err.mean(), 4 * eps * np.abs(ref).mean()))
    assert err.max() <= 8 * eps * np.abs(ref).max(), (err.max(), np.abs(ref).max())
    assert err.mean() <= 4 * eps * np.abs(ref).mean(), (err.mean(), np.abs(ref).mean())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_block_c640_repacks_updated_weight_and_replays(dtype, monkeypatch):
    """An in-place update of proj.weight is followed by a repack: the block that holds an image of the old weight gives the output
    of a FRESH block loaded from the updated state_dict, bit for bit (same kernels, same inputs). And one graph-captured call of
    the block replays to the bits of its eager call."""
    from sta import fused, prompt_state
    monkeypatch.setattr(fused, "ROWGEMM_MIN_ROWS", 0)
    n = _count_passes(monkeypatch)
    g, local_ctx, make, run = _block_case(dtype)
    prompt_state.begin_prompt([c.cuda() for c in local_ctx], first_timestep=981)
    blk = make()
    before = run(blk)
    assert n["c640"] == 1
    with torch.no_grad():
        blk.ff.net[0].proj.weight.mul_(0.5)
    got = run(blk)
    want = run(make(blk.state_dict()))
    assert not torch.equal(want, before)            # the update is visible in the output at all
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(blk)                                    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    calls = n["c640"]
    with torch.cuda.graph(graph):
        replayed = run(blk)
    assert n["c640"] == calls + 1
    replayed.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed, got)
