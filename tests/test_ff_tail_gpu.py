"""sta_ff_tail (csrc/sta_rowstail.hip): ff.net[2] + the block's last residual + proj_out + the transformer's residual as one GEMM
over [h | x2] against [Wp W2 | Wp] — both instances (C = 320 with h in fragment order, C = 640 row-major) against float64 on the same
16-bit operands and against the float64 two-stage chain, the GroupNorm statistics of its epilogue, its refusals, and the
SpatialTransformer with the switches on and off."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from sta.synth import seeded_fill_  # noqa: E402
from tests.cpu_backend import oracle_ops  # noqa: E402

EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
PASS = {320: 256, 640: 128}
_cache = {}


def _weights(dtype, C):
    """net[2], proj_out (a 1x1 convolution, as in the model), (W', b'), and the packed image per (dtype, C), made once."""
    if (dtype, C) not in _cache:
        from sta import fused
        g = torch.Generator().manual_seed(C)
        net2, proj = torch.nn.Linear(4 * C, C), torch.nn.Conv2d(C, C, 1)
        with torch.no_grad():
            net2.weight.copy_(torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5)
            net2.bias.copy_(torch.randn(C, generator=g) * 0.3)
            proj.weight.copy_(torch.randn(C, C, 1, 1, generator=g) / C ** 0.5)
            proj.bias.copy_(torch.randn(C, generator=g) * 0.3)
        net2, proj = net2.to("cuda", dtype), proj.to("cuda", dtype)
        w, b = fused.ff_tail_weights(net2, proj)
        assert w.dtype == dtype and b.dtype == torch.float32
        wp = proj.weight.detach().reshape(C, C)
        _cache[(dtype, C)] = (net2, proj, w, b, fused.pack_ff_tail_weight(torch.cat([w, wp], dim=1)))
    return _cache[(dtype, C)]


def _inputs(R, C, dtype, offset=0.0):
    g = torch.Generator().manual_seed(R + C)
    h, x2, x_in = (torch.randn(R, n, generator=g) for n in (4 * C, C, C))
    return h.to(dtype).cuda(), x2.to(dtype).cuda(), (x_in + offset).to(dtype).cuda()


def _h_arg(h, C):
    """h as the instance reads it: the fragment order of ff_geglu_qfrag(h_frag=True) at C = 320, row-major at C = 640."""
    from sta import ops
    return ops.to_qfrag(h) if C == 320 else h


def _refs(h, x2, x_in, net2, proj, w, b, with_bias):
    """(float64 of the single GEMM on the kernel's own 16-bit operands, float64 of the two-stage chain with the original weights,
    S = sum_k |W'_k| |h_k|)."""
    C = x2.shape[-1]
    hd, x2d, xd = h.double(), x2.double(), x_in.double()
    wp, w2 = proj.weight.detach().reshape(C, C).double(), net2.weight.detach().double()
    one = xd + hd @ w.double().t() + x2d @ wp.t() + (b.double() if with_bias else 0.0)
    x3 = x2d + hd @ w2.t() + (net2.bias.detach().double() if with_bias else 0.0)
    two = xd + x3 @ wp.t() + (proj.bias.detach().double() if with_bias else 0.0)
    return one, two, hd.abs() @ w.double().abs().t()


# one item (the other waves dropped by the descriptors) | exactly one pass | one pass + a partial pass of one item | three passes + 16
# rows in ONE workgroup (grid capped to 1: several passes per workgroup, the ring wraps from the last k-step to k-step 0, the last
# pass is partial) — in units of the instance's pass height (256 | 128 rows)
CASES = [(0, 16, 0), (1, 0, 0), (1, 16, 0), (3, 16, 1)]


@pytest.mark.parametrize("passes,extra,max_wg", CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("C", [320, 640])
def test_ff_tail_vs_fp64(C, with_bias, dtype, passes, extra, max_wg):
    """Within 1 eps (1 + |ref|) of float64 torch on the same 16-bit operands (h, x2, x_in, the rounded W', Wp, b' in fp32) — the bound
    test_rows_c640_gpu.py uses for s — and within eps (S + 2 (1 + |ref|)), S = sum_k |W'_k| |h_k|, of the float64 two-stage chain with
    the original W2 and Wp: the pre-summed-weight bound of test_conv_up2_subpixel_gpu.py (one rounding of every W' entry: eps S; the
    output rounding and the fp32 accumulation: the rest)."""
    from sta import fused
    R = passes * PASS[C] + extra
    net2, proj, w, b, packed = _weights(dtype, C)
    h, x2, x_in = _inputs(R, C, dtype)
    out = fused.ff_tail(_h_arg(h, C), x2, x_in, packed, b if with_bias else None, max_workgroups=max_wg)
    torch.cuda.synchronize()
    assert out.shape == x2.shape and out.dtype == dtype and torch.isfinite(out).all() and not hasattr(out, "_sta_stats")
    one, two, S = _refs(h, x2, x_in, net2, proj, w, b, with_bias)
    eps = EPS[dtype]
    e1 = ((out.double() - one).abs() / (eps * (1.0 + one.abs()))).max().item()
    e2 = ((out.double() - two).abs() / (eps * (S + 2.0 * (1.0 + two.abs())))).max().item()
    print("ff_tail C=%d R=%d %s bias=%s: err / bound: same operands %.3f, two-stage chain %.3f" % (C, R, dtype, with_bias, e1, e2))
    assert e1 <= 1.0, e1
    assert e2 <= 1.0, e2
    if max_wg:
        # the grid cap changes which workgroup takes a pass, not one bit of the result
        assert torch.equal(out, fused.ff_tail(_h_arg(h, C), x2, x_in, packed, b if with_bias else None))


@pytest.mark.parametrize("n_img,passes_img", [(2, 1), (3, 2)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", [320, 640])
def test_ff_tail_epilogue_statistics(C, dtype, n_img, passes_img):
    """The finalized [B, C, 2] sums / sums of squares against float64 sums of the STORED values, to 1e-5 relative (x_in carries an
    offset of 1, as activations carry channel means: a sum that cancels to nothing has no relative error to speak of). The output is
    the one of the launch without statistics, bit for bit; with the grid capped to one workgroup the sums are the same bits (fixed
    slots, fixed order, no atomics); an in-place update of the output retires them. (Rows past R contribute nothing because there are
    none: with statistics R is a multiple of rows_per_image and that of the pass height — test_ff_tail_refusals; partial passes without
    statistics are CASES' business.)"""
    from sta import fused
    rows_img = passes_img * PASS[C]
    R = n_img * rows_img
    net2, proj, w, b, packed = _weights(dtype, C)
    h, x2, x_in = _inputs(R, C, dtype, offset=1.0)
    out = fused.ff_tail(_h_arg(h, C), x2, x_in, packed, b, stats_rows=rows_img)
    st = fused._producer_stats(out)
    assert st is not None and st.shape == (n_img, C, 2) and st.dtype == torch.float32
    assert torch.equal(out, fused.ff_tail(_h_arg(h, C), x2, x_in, packed, b))
    v = out.double().view(n_img, rows_img, C)
    ref = torch.stack([v.sum(dim=1), (v * v).sum(dim=1)], dim=-1)
    rel = ((st.double() - ref).abs() / ref.abs()).max().item()
    print("ff_tail statistics C=%d %s %d x %d rows: max relative error %.3g" % (C, dtype, n_img, rows_img, rel))
    assert rel <= 1e-5, rel
    one = fused.ff_tail(_h_arg(h, C), x2, x_in, packed, b, stats_rows=rows_img, max_workgroups=1)
    assert torch.equal(one, out) and torch.equal(fused._producer_stats(one), st)
    out.add_(1.0)
    assert fused._producer_stats(out) is None


def test_ff_tail_refusals():
    """A rows-per-image that is no multiple of the pass height (or does not divide R) is refused with an error that names it; other
    shapes, tensors of 4 GiB and above, an unknown dtype (-2: unsupported), a row count that is no multiple of 16, a negative grid cap
    (-1: a bad argument): the reason in sta_last_error, the output untouched."""
    from sta import fused, lib
    L = lib.load()
    dtype = torch.float16
    st = torch.cuda.current_stream().cuda_stream
    for C in (320, 640):
        net2, proj, w, b, packed = _weights(dtype, C)
        R = 2 * PASS[C]
        h, x2, x_in = _inputs(R, C, dtype)
        out = torch.full((R, C), 7.0, dtype=dtype, device="cuda")
        part = torch.zeros((R // 16 + 1) * C * 2 * 8, dtype=torch.float32, device="cuda")

        def call(rows=R, c=C, inner=4 * C, stats=False, rows_img=0, max_wg=0, dt=lib.STA_F16):
            return L.sta_ff_tail(h.data_ptr(), x2.data_ptr(), packed.data_ptr(), b.data_ptr(), x_in.data_ptr(), out.data_ptr(),
                                 part.data_ptr() if stats else None, rows_img, rows, c, inner, max_wg, dt, st)
        assert L.sta_ff_tail_packed_w_bytes(C, 4 * C) == C * 5 * C * 2
        assert L.sta_ff_tail_packed_w_bytes(C, 2 * C) == 0 and L.sta_ff_tail_packed_w_bytes(1280, 5120) == 0
        for bad in (PASS[C] + 16, PASS[C] // 2, 0, 3 * PASS[C]):        # not a multiple of the pass height | ... | zero | does not divide R
            assert call(stats=True, rows_img=bad) == -1 and "rows_per_image=%d" % bad in lib.last_error(), lib.last_error()
        assert call(c=C, inner=2 * C) == -2 and "only" in lib.last_error()
        assert call(c=1280, inner=5120) == -2 and "only" in lib.last_error()
        assert call(rows=R + 8) == -1 and "multiple of 16" in lib.last_error()
        assert call(rows=0) == -1 and "multiple of 16" in lib.last_error()
        assert call(rows=(1 << 32) // (4 * C * 2) // 16 * 16 + 16) == -2 and "4 GiB" in lib.last_error()
        assert call(max_wg=-1) == -1 and "max_workgroups" in lib.last_error()
        assert call(dt=7) == -2 and "dtype 7" in lib.last_error()
        assert L.sta_ff_tail_pack_w(w.data_ptr(), packed.data_ptr(), C, 2 * C, lib.STA_F16, st) == -2 and "only" in lib.last_error()
        assert L.sta_ff_tail_pack_w(w.data_ptr(), packed.data_ptr(), C, 4 * C, 7, st) == -2 and "dtype 7" in lib.last_error()
        torch.cuda.synchronize()
        assert (out == 7.0).all()
        with pytest.raises(RuntimeError, match="rows_per_image=%d" % (PASS[C] + 16)):
            fused.ff_tail(_h_arg(h, C), x2, x_in, packed, b, stats_rows=PASS[C] + 16)
        with pytest.raises(ValueError):
            fused.pack_ff_tail_weight(torch.zeros(C, 3 * C, dtype=dtype, device="cuda"))


# ---- the SpatialTransformer ---------------------------------------------------------------------------------------------------------
def _transformer_case(C, dtype, monkeypatch):
    """A SpatialTransformer of 8 heads of C / 8 at 16 x 16, batch 2 (one CFG pair), two objects: (fp32 CPU output of the eager module,
    make(state) -> a 16-bit CUDA module, run(module) -> its NHWC output). Every row pass is allowed at its 512 rows."""
    from ldm.modules.attention import SpatialTransformer
    from sta import fused, prompt_state
    monkeypatch.setattr(fused, "ROWGEMM_MIN_ROWS", 0)
    monkeypatch.setattr(fused, "LINEAR_MIN_ROWS", 128)
    dim, K, seed = 16, 2, 11
    _, context, local_ctx = gi.block_inputs(dim, C, K, seed, gi.load_uncond())
    x = torch.randn(2, C, dim, dim, generator=torch.Generator().manual_seed(seed))
    coef, boxes = torch.tensor([2.5, 2.5]), [[0.3, 0.4], [0.7, 0.6]]
    cpu = SpatialTransformer(C, 8, C // 8, depth=1, context_dim=768)
    seeded_fill_(cpu, seed)
    assert cpu.proj_out.weight.abs().max() > 0          # (zero_module's zeros were replaced: proj_out does something)
    base = {k: v.clone() for k, v in cpu.state_dict().items()}
    with oracle_ops(), torch.no_grad():
        prompt_state.begin_prompt(local_ctx, first_timestep=981)
        ref = cpu(x, context=context, time=torch.tensor(981), coef=coef, bboxs_curr=boxes)
    prompt_state.begin_prompt([c.cuda() for c in local_ctx], first_timestep=981)
    xd = x.to("cuda", dtype).contiguous(memory_format=torch.channels_last)
    ctx, coefd = context.to("cuda", dtype), coef.cuda()

    def make(state=None):
        m = SpatialTransformer(C, 8, C // 8, depth=1, context_dim=768)
        m.load_state_dict(base if state is None else state)
        return m.to("cuda", dtype)

    def run(m):
        with torch.no_grad():
            return m(xd, context=ctx, time=torch.tensor(981), coef=coefd, bboxs_curr=boxes)
    return ref, make, run


def _spy(monkeypatch):
    """Counts the new pass and lists linear_rows' calls as (N, with residual) — proj_out's is the one with a residual; keeps the
    arguments and the result of the last ff_tail call."""
    from sta import fused
    real_tail, real_rows = fused.ff_tail, fused.linear_rows
    seen = {"tail": 0, "linear_rows": [], "args": None, "real_tail": real_tail}

    def tail(h, x2, x_in, *a, **k):
        seen["tail"] += 1
        seen["args"] = (h, x2, x_in)
        seen["image"], seen["kwargs"] = a, k
        seen["out"] = real_tail(h, x2, x_in, *a, **k)
        return seen["out"]

    def rows(x, wp, N, bias=None, res=None, stats_rows=None):
        seen["linear_rows"].append((N, res is not None))
        return real_rows(x, wp, N, bias=bias, res=res, stats_rows=stats_rows)
    monkeypatch.setattr(fused, "ff_tail", tail)
    monkeypatch.setattr(fused, "linear_rows", rows)
    return seen


def _switch(monkeypatch, on):
    from sta import fused
    monkeypatch.setattr(fused, "FF_TAIL_PROJ_OUT_C320", on)
    monkeypatch.setattr(fused, "FF_TAIL_PROJ_OUT_C640", on)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", [320, 640])
def test_spatial_transformer_tail_on_and_off(C, dtype, monkeypatch):
    """Switch on: the new pass runs once and linear_rows is not called for proj_out (only for proj_in); off: never, and proj_out is the
    row GEMM with the residual (the only linear_rows call that carries one). On stays within the two paths' bounds of off, element by element: eps (S + 2 (1 + |ref|)) for the pass
    (test_ff_tail_vs_fp64) plus eps (sum_k |Wp_k| |x3_k| + 2 (1 + |ref|)) for the pair (x3 rounded once in front of proj_out, then the
    output), both around the float64 two-stage chain on the operands the pass was handed. Against the fp32 run of the eager module on
    is no farther than off by more than 1 eps max |ref|. The next GroupNorm consumes `_sta_stats`: no statistics pass."""
    from sta import fused, lib, ops
    ref, make, run = _transformer_case(C, dtype, monkeypatch)
    seen = _spy(monkeypatch)
    m = make()
    _switch(monkeypatch, False)
    off = run(m)
    assert seen["tail"] == 0 and [c for c in seen["linear_rows"] if c[1]] == [(C, True)], seen
    seen["linear_rows"].clear()
    _switch(monkeypatch, True)
    on = run(m)
    assert seen["tail"] == 1 and (C, False) in seen["linear_rows"] and not [c for c in seen["linear_rows"] if c[1]], seen
    assert on.shape == off.shape == ref.shape and fused.is_nhwc(on) and torch.isfinite(on).all()
    eps = EPS[dtype]
    h, x2, x_in = seen["args"]
    h = (ops.from_qfrag(h) if C == 320 else h).reshape(-1, 4 * C)
    net2, proj = m.transformer_blocks[-1].ff.net[2], m.proj_out
    w, b = fused.ff_tail_weights(net2, proj)
    _, two, S = _refs(h, x2.reshape(-1, C), x_in.reshape(-1, C), net2, proj, w, b, True)
    x3 = x2.reshape(-1, C).double() + h.double() @ net2.weight.double().t() + net2.bias.double()
    bound = eps * (S + x3.abs() @ proj.weight.reshape(C, C).double().abs().t() + 4.0 * (1.0 + two.abs()))
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C).double()
    d = ((rows(on) - rows(off)).abs() / bound).max().item()
    e_on, e_off = (on.float().cpu() - ref).abs().max().item(), (off.float().cpu() - ref).abs().max().item()
    print("SpatialTransformer C=%d %s: on vs off / bound %.3f; max error to the fp32 module: on %.4g, off %.4g (max |ref| %.3g)"
          % (C, dtype, d, e_on, e_off, ref.abs().max().item()))
    assert d <= 1.0, d
    assert e_on <= e_off + eps * ref.abs().max().item(), (e_on, e_off)
    # the next GroupNorm: the one-pass kernel on the producer's sums, never the statistics pass
    assert fused._producer_stats(on) is not None and fused._producer_stats(on).shape == (2, C, 2)
    L = lib.load()
    n = {"stats_pass": 0, "one_pass": 0}
    real_two, real_one = L.sta_groupnorm_silu_nhwc, L.sta_groupnorm_silu_nhwc_cstats
    monkeypatch.setattr(L, "sta_groupnorm_silu_nhwc", lambda *a: (n.__setitem__("stats_pass", n["stats_pass"] + 1), real_two(*a))[1])
    monkeypatch.setattr(L, "sta_groupnorm_silu_nhwc_cstats", lambda *a: (n.__setitem__("one_pass", n["one_pass"] + 1), real_one(*a))[1])
    g = torch.Generator().manual_seed(1)
    gw, gb = (1.0 + 0.2 * torch.randn(C, generator=g)).to(dtype).cuda(), (0.2 * torch.randn(C, generator=g)).to(dtype).cuda()
    y = fused.groupnorm_silu(on, gw, gb, 32, 1e-5)
    assert n == {"stats_pass": 0, "one_pass": 1}, n
    y_ref = F.silu(F.group_norm(on.double(), 32, gw.double(), gb.double(), 1e-5))
    assert ((y.double() - y_ref).abs() <= 4 * eps * (1.0 + y_ref.abs())).all()


@pytest.mark.parametrize("which", ["net2.weight", "net2.bias", "proj_out.weight", "proj_out.bias"])
@pytest.mark.parametrize("C", [320, 640])
def test_spatial_transformer_tail_repacks_updated_tensors(C, which, monkeypatch):
    """An in-place update of any of the four tensors behind (W', b') is followed by a repack: on the operands it was handed, the pass
    of the module that held an image of the old tensors gives the bits of the pass with the image of a FRESH module loaded from the
    updated state_dict, and not those of the old image. (The comparison is made at the pass: the transformer's first GroupNorm takes
    its statistics with LDS atomics and is not bit-reproducible from one call to the next.)"""
    from sta import fused
    _, make, run = _transformer_case(C, torch.float16, monkeypatch)
    seen = _spy(monkeypatch)
    real_tail = seen["real_tail"]
    m = make()
    before = run(m)
    assert seen["tail"] == 1
    old_image = seen["image"]
    mod, name = which.split(".")
    t = getattr(m.transformer_blocks[-1].ff.net[2] if mod == "net2" else m.proj_out, name)
    with torch.no_grad():
        t.mul_(0.5)
    after = run(m)
    assert seen["tail"] == 2
    (h, x2, x_in), got, kw = seen["args"], seen["out"], seen["kwargs"]
    fresh = make(m.state_dict())
    want = real_tail(h, x2, x_in, *fused.ff_tail_image(fresh, fresh.transformer_blocks[-1].ff.net[2], fresh.proj_out), **kw)
    stale = real_tail(h, x2, x_in, *old_image, **kw)
    assert not torch.equal(stale, want) and not torch.equal(after, before)            # the update is visible at all
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
    assert torch.equal(fused._producer_stats(got), fused._producer_stats(want))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C", [320, 640])
def test_ff_tail_graph_replay_is_bit_equal(C, dtype):
    """A captured launch with statistics (the pass + the finalize; two images of two passes each in ONE workgroup: the counted waits
    hold in replay) replays to the bits of the eager launch. (Made at the pass and not around the whole SpatialTransformer, whose
    first GroupNorm is not bit-reproducible from one call to the next.)"""
    from sta import fused
    rows_img = 2 * PASS[C]
    net2, proj, w, b, packed = _weights(dtype, C)
    h, x2, x_in = _inputs(2 * rows_img, C, dtype)
    hf = _h_arg(h, C)

    def run():
        return fused.ff_tail(hf, x2, x_in, packed, b, stats_rows=rows_img, max_workgroups=1)
    eager = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                           # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    st = out._sta_stats[1]
    out.zero_()
    st.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(st, eager._sta_stats[1])
