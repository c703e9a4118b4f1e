"""Wrap-around canvases on the MI355X: the five launches of csrc/sta_window.hip on wrapped grids against the torch restatements of
sta.canvas on a ring and float64, their roll equivariance, the masked identities, and `sample_canvas(wrap="x")` /
`inpaint_canvas(wrap="x")` against the fp32 host trajectory, the three-launch form and graph replay."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from tests.test_canvas_gpu import _cls, _inputs, _model  # noqa: E402
from tests.test_canvas_inpaint_cpu import Q_A, Q_B, _draws, keep_mask  # noqa: E402
from tests.test_canvas_wrap_cpu import COVER2, SHAPES, _grid, _roll_canvas, _roll_windows  # noqa: E402
from tests.test_inpaint_gpu import _blend64  # noqa: E402
from tests.test_solver_gpu import TOLS, _case, _step64  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
P = 2
S_LAT, STEPS, K = 32, 8, 2
CANVAS, STRIDE = (S_LAT, 2 * S_LAT), S_LAT // 2        # wrap = "x": T = 4, the last window runs over the seam
CENTRES = [[0.25, 0.4], [0.9375, 0.6]]                 # canvas-normalised; the second disc (x = 60 of 64) crosses the seam
MODES = ["first", "second", "noise", "both"]           # (m_prev, noise) given: neither, m_prev, noise, both


def _coef(mode):
    from sta.solver import StepCoef
    return StepCoef(5.0, 0.6, 0.8, 0.1, 0.9, -0.05, 0.35, 0.22) if mode == "both" else _case(mode)


def _tensors(g, dtype, seed):
    torch.manual_seed(seed)
    r = lambda: torch.randn((P, 4, g.Hc, g.Wc), device="cuda")
    eps = torch.randn(2 * P * g.T, 4, g.s, g.s, device="cuda").to(dtype)
    return eps, r() * 3, r(), r(), r(), r()          # eps, x, m_prev, noise, x0, qnoise


# ---------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_ring_split_fuse_and_blend_equal_their_restatements(shape, dtype):
    """Bit for bit: both `rows` forms and source types of the split, the fuse (fp32 sum in ascending w, IEEE division, one rounding) and
    fuse(split(x)) == x; the blend's state is sta_latent_blend's (one device definition) and its xin the restatement's split of it."""
    from sta import canvas, solver
    g = _grid(shape)
    eps, x, _, _, x0, qn = _tensors(g, dtype, 100 + g.T)
    for rows, src32 in ((1, x), (2, torch.cat([x, -x]))):
        for src in (src32, src32.to(dtype)):
            got = canvas.window_split(src, g, dtype, rows=rows)
            want = canvas.window_split_reference(src.cpu(), g, dtype, rows=rows)
            assert got.dtype == dtype and got.shape == want.shape == (2 * P * g.T, 4, g.s, g.s) and torch.equal(got.cpu(), want), (rows, src.dtype)
    got = canvas.window_fuse(eps, g)
    assert got.dtype == dtype and got.shape == (2 * P, 4, g.Hc, g.Wc) and torch.equal(got.cpu(), canvas.window_fuse_reference(eps.cpu(), g))
    assert torch.equal(canvas.window_fuse(eps, g), got)
    pair = torch.cat([x, -x]).to(dtype)
    assert torch.equal(canvas.window_fuse(canvas.window_split(pair, g, dtype, rows=2), g), pair)
    for kind in ("mixed", "uniform"):
        bl = solver.Blend(x0, keep_mask(P, g.Hc, g.Wc, kind).cuda(), qn, Q_A, Q_B)
        out, xin = canvas.window_blend(x, bl, g, dtype, want_xin=True)
        assert torch.equal(out, solver.latent_blend(x, bl, dtype=dtype)[0])
        assert xin.dtype == dtype and torch.equal(xin.cpu(), canvas.window_split_reference(out.cpu(), g, dtype))
        ref, _ = canvas.window_blend_reference(x.cpu(), solver.Blend(x0.cpu(), bl.keep.cpu(), qn.cpu(), Q_A, Q_B), g, dtype)
        mag = x.cpu().abs() + x0.cpu().abs() + qn.cpu().abs()
        assert ((out.cpu() - ref).abs() <= 1e-6 * (1 + mag)).all()              # torch does not contract the blend's multiply-adds
        out2, none = canvas.window_blend(x, bl, g, dtype)
        assert none is None and torch.equal(out2, out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_ring_step_launches_vs_fp64(mode, shape, dtype):
    """sta_sampler_step_windows and sta_sampler_step_windows_masked on a ring for every presence of m_prev / noise, held to the float64
    bound of tests/test_canvas_gpu.py and tests/test_canvas_inpaint_gpu.py, 1e-6 (1 + the sum of the absolute terms), on the
    restatement's fp32 overlap means (bit-checked by the fuse test); xin is the split of the kernel's own rounded x_next, bit for bit;
    a launch without the spare tensors and a second launch give the same bits. Measured: at most 2.1e-7."""
    from sta import canvas, solver
    g, c = _grid(shape), _coef(mode)
    eps, x, m_prev, noise, x0, qn = _tensors(g, dtype, 200 + g.T)
    means = canvas._fuse32(eps.cpu(), g)
    rx, rm, ax, am = _step64(means, x.cpu(), m_prev.cpu() if c.c_p else None, noise.cpu() if c.c_n else None, c, magnitudes=True)
    xn, m, xin = canvas.sampler_step_windows(eps, x, m_prev, noise, c, g, want_xin=True)
    keep = keep_mask(P, g.Hc, g.Wc).cuda()
    bl = solver.Blend(x0, keep, qn, Q_A, Q_B)
    bxn, bm, bxin = canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, g, want_xin=True)
    rb, ab = _blend64(rx, ax, x0.cpu(), keep.cpu(), qn.cpu(), Q_A, Q_B)
    for name, got, ref, mag in (("x_next", xn, rx, ax), ("m", m, rm, am), ("masked x_next", bxn, rb, ab), ("masked m", bm, rm, am)):
        err = ((got.cpu().double() - ref).abs() / (1 + mag)).max().item()
        print("%s %s %s %s: max err / (1 + sum |terms|) = %.3g" % (mode, shape, dtype, name, err))
        assert err <= 1e-6, (name, err)
    assert xin.dtype == dtype and torch.equal(xin.cpu(), canvas.window_split_reference(xn.cpu(), g, dtype))
    assert bxin.dtype == dtype and torch.equal(bxin.cpu(), canvas.window_split_reference(bxn.cpu(), g, dtype))
    spare = (m_prev if c.c_p else None, noise if c.c_n else None)
    for again in (canvas.sampler_step_windows(eps, x, *spare, c, g), canvas.sampler_step_windows(eps, x, m_prev, noise, c, g, want_xin=True)):
        assert torch.equal(again[0], xn) and torch.equal(again[1], m) and (again[2] is None or torch.equal(again[2], xin))
    for again in (canvas.sampler_step_windows_masked(eps, x, *spare, c, bl, g),
                  canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, g, want_xin=True)):
        assert torch.equal(again[0], bxn) and torch.equal(again[1], bm) and (again[2] is None or torch.equal(again[2], bxin))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_ring_masked_step_identities(mode, shape, dtype):
    """Bit for bit: keep == 0 everywhere is the unmasked ring launch (x_next, m, xin); where keep == 1 the state is sta_latent_blend's
    value for the same x0, noise, q_a, q_b whatever the UNet said; m is the unmasked launch's for any mask."""
    from sta import canvas, solver
    g, c = _grid(shape), _coef(mode)
    eps, x, m_prev, noise, x0, qn = _tensors(g, dtype, 300 + g.T)
    plain = canvas.sampler_step_windows(eps, x, m_prev, noise, c, g, want_xin=True)
    zero = canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, solver.Blend(x0, torch.zeros(P, 1, g.Hc, g.Wc, device="cuda"), qn, Q_A, Q_B),
                                              g, want_xin=True)
    for name, a, b in zip(("x_next", "m", "xin"), zero, plain):
        assert torch.equal(a, b), name
    keep = keep_mask(P, g.Hc, g.Wc).cuda()
    bl = solver.Blend(x0, keep, qn, Q_A, Q_B)
    xn, m, _ = canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, g)
    assert torch.equal(m, plain[1])
    lb, _ = solver.latent_blend(torch.randn_like(x), bl, dtype=dtype)
    one, nought = (keep == 1).expand_as(xn), (keep == 0).expand_as(xn)
    assert one.any() and nought.any() and ((keep > 0) & (keep < 1)).any()
    assert torch.equal(xn[one], lb[one]) and torch.equal(xn[nought], plain[0][nought])
    eps2 = torch.randn_like(eps.float()).to(dtype)
    assert torch.equal(canvas.sampler_step_windows_masked(eps2, x, m_prev, noise, c, bl, g)[0][one], xn[one])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", COVER2)
def test_ring_launches_are_roll_equivariant(shape, dtype):
    """Every canvas tensor rolled by k strides along the wrapped axis and the windows moved k places round the ring: every output of the
    five launches is the rolled one, bit for bit (at most two covering windows: their fp32 sum does not depend on the order)."""
    from sta import canvas, solver
    g = _grid(shape)
    eps, x, m_prev, noise, x0, qn = _tensors(g, dtype, 400 + g.T)
    keep = keep_mask(P, g.Hc, g.Wc).cuda()
    pair = torch.cat([x, -x]).to(dtype)
    for k in (1, max(g.ny, g.nx) - 1):
        ky, kx = k if "y" in g.wrap else 0, k if "x" in g.wrap else 0
        rc, rw = lambda t: _roll_canvas(t, g, ky, kx).contiguous(), lambda t: _roll_windows(t, g, ky, kx).contiguous()
        assert not torch.equal(rc(x), x) and not torch.equal(rw(eps), eps)
        assert torch.equal(canvas.window_split(rc(x), g, dtype), rw(canvas.window_split(x, g, dtype)))
        assert torch.equal(canvas.window_split(rc(pair), g, dtype, rows=2), rw(canvas.window_split(pair, g, dtype, rows=2)))
        assert torch.equal(canvas.window_fuse(rw(eps), g), rc(canvas.window_fuse(eps, g)))
        bl, bl_r = solver.Blend(x0, keep, qn, Q_A, Q_B), solver.Blend(rc(x0), rc(keep), rc(qn), Q_A, Q_B)
        for mode in MODES:
            c = _coef(mode)
            a = canvas.sampler_step_windows(eps, x, m_prev, noise, c, g, want_xin=True)
            b = canvas.sampler_step_windows(rw(eps), rc(x), rc(m_prev), rc(noise), c, g, want_xin=True)
            assert torch.equal(b[0], rc(a[0])) and torch.equal(b[1], rc(a[1])) and torch.equal(b[2], rw(a[2])), mode
            a = canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, g, want_xin=True)
            b = canvas.sampler_step_windows_masked(rw(eps), rc(x), rc(m_prev), rc(noise), c, bl_r, g, want_xin=True)
            assert torch.equal(b[0], rc(a[0])) and torch.equal(b[1], rc(a[1])) and torch.equal(b[2], rw(a[2])), mode
        a, b = canvas.window_blend(x, bl, g, dtype, want_xin=True), canvas.window_blend(rc(x), bl_r, g, dtype, want_xin=True)
        assert torch.equal(b[0], rc(a[0])) and torch.equal(b[1], rw(a[1]))


# ---------------------------------------------------------------------------------------------------
# trajectories: golden-width UNet, S = 8, a 32 x 64 canvas closed along x, stride 16 (T = 4)
# ---------------------------------------------------------------------------------------------------
def _ring(sampler, device="cuda", centres=CENTRES, keep=None, x0=None):
    c, local_ctx, x_T = _inputs(CANVAS, device)
    common = dict(S=STEPS, canvas=CANVAS, window=S_LAT, stride=STRIDE, conditionings=[c], unconditional_conditionings=gi.load_uncond().to(device),
                  bboxs=[centres], object_names=[["a", "b"]], local_conditionings=[local_ctx], x_T=x_T, unconditional_guidance_scale=7.5, eta=0.0,
                  seed=1, wrap="x")
    if keep is None:
        sampler.sample_canvas(**common)
    else:
        sampler.inpaint_canvas(mask=keep.to(device), x0=x0.to(device), **common)
    assert sampler._canvas is None and getattr(sampler, "_inpaint", None) is None
    return sampler.last_result["x0"].clone()


def _sampler(kind, dtype, device="cuda", **kw):
    return _cls(kind)(_model(dtype, device), **dict(dict(opt_epochs=0, use_graph=False, save_images=False), **kw))


def _masked(kind, dtype, device="cuda", **kw):
    return _sampler(kind, dtype, device, mask_noise=_draws(STEPS, 7, (1, 4) + CANVAS), **kw)


def _kept():
    return keep_mask(1, *CANVAS), torch.randn((1, 4) + CANVAS, generator=torch.Generator().manual_seed(9))


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


_HOST = {}


def _host(kind, masked):
    """The same trajectory in fp32 on the host: oracle-backed blocks and the torch restatements of the window kernels on the ring."""
    from tests.cpu_backend import oracle_ops
    if (kind, masked) not in _HOST:
        with oracle_ops():
            if masked:
                keep, x0 = _kept()
                _HOST[(kind, masked)] = _ring(_masked(kind, torch.float32, "cpu"), "cpu", keep=keep, x0=x0)
            else:
                _HOST[(kind, masked)] = _ring(_sampler(kind, torch.float32, "cpu"), "cpu")
    return _HOST[(kind, masked)]


@pytest.mark.parametrize("dtype,tol_max,tol_mean", TOLS)
@pytest.mark.parametrize("kind", ["plms", "ddim", "dpm"])
def test_ring_canvas_vs_fp32_host_trajectory(kind, dtype, tol_max, tol_mean):
    """sample_canvas(wrap="x") on the GPU (PLMS: ring split + fuse per call; DDIM and DPM-Solver++: one sta_sampler_step_windows
    launch per call) vs the same trajectory in fp32 on the host, inside TOLS of tests/test_solver_gpu.py, the bounds of
    tests/test_canvas_gpu.py: fp16 max 1 %, mean 0.5 %; bf16 max 3 %, mean 2 % of max|x| / mean|x|.
    Measured (max / mean): PLMS fp16 0.25 % / 0.25 %, bf16 1.30 % / 1.19 %; DDIM fp16 0.23 % / 0.25 %, bf16 1.17 % / 1.21 %; DPM-Solver++
    fp16 0.24 % / 0.25 %, bf16 1.16 % / 1.22 %."""
    ref = _host(kind, False)
    got = _ring(_sampler(kind, dtype)).float().cpu()
    assert got.shape == (1, 4) + CANVAS and torch.isfinite(got).all()
    err = (got - ref).abs()
    e_max, e_mean = (err.max() / ref.abs().max()).item(), (err.mean() / ref.abs().mean()).item()
    print("ring canvas %s %s: max %.3f %%, mean %.3f %%" % (kind, dtype, 100 * e_max, 100 * e_mean))
    assert e_max <= tol_max and e_mean <= tol_mean, (e_max, e_mean)


@pytest.mark.parametrize("dtype,tol_max,tol_mean", TOLS)
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_ring_inpaint_canvas_vs_fp32_host_trajectory(kind, dtype, tol_max, tol_mean):
    """inpaint_canvas(wrap="x") with a mixed keep mask on the GPU (sta_window_blend, then one sta_sampler_step_windows_masked
    launch per call) vs the host, inside TOLS, the bounds of tests/test_canvas_inpaint_gpu.py.
    Measured (max / mean): DDIM fp16 0.27 % / 0.22 %, bf16 1.45 % / 1.02 %; DPM-Solver++ fp16 0.27 % / 0.23 %, bf16 1.10 % / 1.10 %."""
    keep, x0 = _kept()
    ref = _host(kind, True)
    got = _ring(_masked(kind, dtype), keep=keep, x0=x0).float().cpu()
    assert got.shape == (1, 4) + CANVAS and torch.isfinite(got).all()
    err = (got - ref).abs()
    e_max, e_mean = (err.max() / ref.abs().max()).item(), (err.mean() / ref.abs().mean()).item()
    print("ring inpaint canvas %s %s: max %.3f %%, mean %.3f %%" % (kind, dtype, 100 * e_max, 100 * e_mean))
    assert e_max <= tol_max and e_mean <= tol_mean, (e_max, e_mean)


@pytest.mark.parametrize("masked", [False, True])
def test_ring_unfused_step_agrees_with_the_fused_launch(masked):
    """canvas_fused_step = False (three launches: the means are rounded to fp16 before the step) against the one-launch form, to the
    1 % of max of tests/test_canvas_gpu.test_unfused_step_agrees_with_the_fused_launch and its masked counterpart (measured: 0.19 %
    unmasked, 0.18 % masked)."""
    keep, x0 = _kept() if masked else (None, None)
    make = _masked if masked else _sampler
    a = _ring(make("ddim", torch.float16), keep=keep, x0=x0)
    b = _ring(make("ddim", torch.float16, canvas_fused_step=False), keep=keep, x0=x0)
    e = _rel(b, a)
    print("ring %s fused vs unfused step: max %.4f %%" % ("masked" if masked else "unmasked", 100 * e))
    assert e <= 0.01


@pytest.mark.parametrize("kind,masked", [("dpm", False), ("plms", False), ("ddim", True), ("dpm", True)])
def test_ring_graph_replay_matches_eager(kind, masked):
    """hipGraph replay of the 2 P T = 8 row UNet call == eager launches on the ring: within 2 % of max, the bound of
    tests/test_canvas_gpu.test_canvas_graph_replay_matches_eager and tests/test_canvas_inpaint_gpu's (measured: 0.25 % DPM-Solver++,
    0.23 % PLMS; masked 0.17 % DDIM, 0.18 % DPM-Solver++)."""
    keep, x0 = _kept() if masked else (None, None)
    make = _masked if masked else _sampler
    eager = _ring(make(kind, torch.float16), keep=keep, x0=x0)
    sampler = make(kind, torch.float16, use_graph=True)
    replay = _ring(sampler, keep=keep, x0=x0)
    e = _rel(replay, eager)
    print("ring %s %s graph replay vs eager: max %.3f %%" % (kind, "masked" if masked else "unmasked", 100 * e))
    assert e <= 0.02, e
    assert len(sampler._graphs._entries) == 1


def test_a_ring_differs_from_the_clamped_canvas():
    """The first and the last column share a UNet window now: the wrapped trajectory is another one (more than 5 % of max, the figure
    tests/test_canvas_gpu.py asks of moved objects; measured 55 %)."""
    sampler = _sampler("ddim", torch.float16)
    ring = _ring(sampler)
    c, local_ctx, x_T = _inputs(CANVAS)
    sampler.sample_canvas(S=STEPS, canvas=CANVAS, window=S_LAT, stride=STRIDE, conditionings=[c], unconditional_conditionings=gi.load_uncond().cuda(),
                          bboxs=[CENTRES], object_names=[["a", "b"]], local_conditionings=[local_ctx], x_T=x_T, unconditional_guidance_scale=7.5,
                          eta=0.0, seed=1)
    d = _rel(ring, sampler.last_result["x0"])
    print("ring vs clamped canvas: max %.3f %%" % (100 * d))
    assert d > 0.05, d
