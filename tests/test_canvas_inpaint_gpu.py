"""Inpainting and outpainting on wide canvases on the MI355X: sta_sampler_step_windows_masked and sta_window_blend (csrc/sta_window.hip)
against float64 restatements and bit for bit against the kernels they combine, `inpaint_canvas` against `sample(mask=)`,
`sample_batch(mask=)`, `sample_canvas` and the fp32 host trajectory, graph replay, the launch structure, the pixel paste and
scripts/outpaint.py end to end on synthetic weights."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from tests.test_canvas_gpu import _cls, _inputs, _model  # noqa: E402
from tests.test_canvas_inpaint_cpu import GRIDS, Q_A, Q_B, Counters, _draws, _grid, keep_mask  # noqa: E402
from tests.test_inpaint_gpu import _blend64  # noqa: E402
from tests.test_solver_gpu import TOLS, _case, _step64, _wopt_model  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
S_LAT, STEPS, K = 32, 8, 2
CENTRES = [[0.25, 0.4], [0.625, 0.6]]                  # canvas-normalised; on a 32 x 64 canvas the second disc straddles x = 0.5
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}     # one unit in the last place, relative (10 / 7 fraction bits)


def _tensors(g, P, dtype, seed):
    torch.manual_seed(seed)
    shape = (P, 4, g.Hc, g.Wc)
    r = lambda: torch.randn(shape, device="cuda")
    eps = torch.randn(2 * P * g.T, 4, g.s, g.s, device="cuda").to(dtype)
    return eps, r() * 3, r(), r(), r(), r()          # eps, x, m_prev, noise, x0, qnoise


# ---------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "uniform"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("mode", ["first", "second", "noise"])
def test_sampler_step_windows_masked_kernel(mode, grid, P, dtype, kind):
    """sta_sampler_step_windows_masked in the three coefficient modes of tests/test_solver_gpu._case, with and without xin, on mixed keep
    masks (0 / 1 blocks that cut through a lane's vector, fractional cells, a canvas of ones) and uniform ones (a canvas of zeros, a
    canvas of ones). x_next and m are held to test_solver_gpu's float64 bound for the step, 1e-6 (1 + sum of |terms|), with the sum
    extended by the blend's terms (test_inpaint_gpu._blend64), evaluated on canvas._fuse32's fp32 means. xin is the split of the
    kernel's own x_next bit for bit; a second launch gives the same bits."""
    from sta import canvas, solver
    g, c = _grid(grid), _case(mode)
    eps, x, m_prev, noise, x0, qn = _tensors(g, P, dtype, P * 100 + g.T + 5)
    keep = keep_mask(P, g.Hc, g.Wc, kind).cuda()
    bl = solver.Blend(x0, keep, qn, Q_A, Q_B)
    xn, m, xin = canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, g, want_xin=True)
    means = canvas._fuse32(eps.cpu(), g)
    rx, rm, ax, am = _step64(means, x.cpu(), m_prev.cpu() if c.c_p else None, noise.cpu() if c.c_n else None, c, magnitudes=True)
    rb, ab = _blend64(rx, ax, x0.cpu(), keep.cpu(), qn.cpu(), Q_A, Q_B)
    for name, got, ref, mag in (("x_next", xn, rb, ab), ("m", m, rm, am)):
        err = (got.cpu().double() - ref).abs()
        print("%s %s P=%d %s %s %s: max err / (1 + mag) = %.3g" % (mode, grid, P, dtype, kind, name, (err / (1 + mag)).max().item()))
        assert (err <= 1e-6 * (1 + mag)).all(), (name, (err / (1 + mag)).max().item())
    assert xin.dtype == dtype and torch.equal(xin.cpu(), canvas.window_split_reference(xn.cpu(), g, dtype))
    xn2, m2, none = canvas.sampler_step_windows_masked(eps, x, m_prev if c.c_p else None, noise if c.c_n else None, c, bl, g)
    assert none is None and torch.equal(xn2, xn) and torch.equal(m2, m)
    xn3, m3, xin3 = canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, g, want_xin=True)
    assert torch.equal(xn3, xn) and torch.equal(m3, m) and torch.equal(xin3, xin)
    # the torch restatement agrees with the kernel (hipcc contracts the multiply-adds, torch does not: not bit for bit)
    cpu = lambda t: t.cpu()
    cx, cm, _ = canvas.step_windows_masked_reference(eps.cpu(), x.cpu(), m_prev.cpu(), noise.cpu(), c,
                                                     solver.Blend(cpu(x0), cpu(keep), cpu(qn), Q_A, Q_B), g)
    assert ((cx.double() - xn.cpu().double()).abs() <= 2e-6 * (1 + ab)).all() and ((cm.double() - m.cpu().double()).abs() <= 2e-6 * (1 + am)).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["first", "second", "noise"])
def test_masked_step_with_one_window_is_sta_sampler_step_masked(mode, dtype):
    """T = 1 (sides 16 and 32): x_next, m and xin equal sta_sampler_step_masked's bit for bit."""
    from sta import canvas, solver
    c = _case(mode)
    for side, P in ((16, 2), (32, 1)):
        g = _grid((side, side, side, 8))
        assert g.T == 1
        eps, x, m_prev, noise, x0, qn = _tensors(g, P, dtype, 11 + side)
        bl = solver.Blend(x0, keep_mask(P, side, side).cuda(), qn, Q_A, Q_B)
        got = canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, g, want_xin=True)
        want = solver.solver_step_masked(eps, x, m_prev, noise, c, bl, want_xin=True)
        for name, a, b in zip(("x_next", "m", "xin"), got, want):
            assert torch.equal(a, b), (name, side)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("mode", ["first", "second", "noise"])
def test_masked_step_identities(mode, grid, P, dtype):
    """Bit for bit: keep == 0 everywhere is sta_sampler_step_windows (x_next, m, xin); where keep == 1, x_next is sta_latent_blend's value
    for the same x0, noise, q_a, q_b whatever eps is; m is the unmasked launch's m for any mask."""
    from sta import canvas, solver
    g, c = _grid(grid), _case(mode)
    eps, x, m_prev, noise, x0, qn = _tensors(g, P, dtype, P * 100 + g.T + 6)
    plain = canvas.sampler_step_windows(eps, x, m_prev, noise, c, g, want_xin=True)
    zero = canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, solver.Blend(x0, torch.zeros(P, 1, g.Hc, g.Wc, device="cuda"), qn, Q_A, Q_B),
                                              g, want_xin=True)
    for name, a, b in zip(("x_next", "m", "xin"), zero, plain):
        assert torch.equal(a, b), name
    keep = keep_mask(P, g.Hc, g.Wc).cuda()
    bl = solver.Blend(x0, keep, qn, Q_A, Q_B)
    xn, m, _ = canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, g)
    assert torch.equal(m, plain[1])
    lb, _ = solver.latent_blend(torch.randn_like(x), bl, dtype=dtype)            # any state: where keep == 1 only x0 and the noise count
    one, nought = (keep == 1).expand_as(xn), (keep == 0).expand_as(xn)
    assert one.any() and nought.any() and ((keep > 0) & (keep < 1)).any()
    assert torch.equal(xn[one], lb[one]) and torch.equal(xn[nought], plain[0][nought])
    eps2 = torch.randn_like(eps.float()).to(dtype)
    assert torch.equal(canvas.sampler_step_windows_masked(eps2, x, m_prev, noise, c, bl, g)[0][one], xn[one])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("grid", GRIDS + [(16, 16, 16, 8), (32, 32, 32, 16)])
def test_window_blend_kernel(grid, P, dtype):
    """sta_window_blend: x_out bit-equal to sta_latent_blend, xin bit-equal to sta_window_split of it; with T = 1 xin is sta_latent_blend's."""
    from sta import canvas, solver
    g = _grid(grid)
    _, x, _, _, x0, qn = _tensors(g, P, dtype, P * 100 + g.T + 7)
    for kind in ("mixed", "uniform"):
        bl = solver.Blend(x0, keep_mask(P, g.Hc, g.Wc, kind).cuda(), qn, Q_A, Q_B)
        out, xin = canvas.window_blend(x, bl, g, dtype, want_xin=True)
        want, pair = solver.latent_blend(x, bl, dtype=dtype, want_xin=True)
        assert torch.equal(out, want)
        assert xin.dtype == dtype and torch.equal(xin, canvas.window_split(out, g, dtype))
        assert torch.equal(xin.cpu(), canvas.window_split_reference(out.cpu(), g, dtype))
        if g.T == 1:
            assert torch.equal(xin, pair)
        out2, none = canvas.window_blend(x, bl, g, dtype)
        assert none is None and torch.equal(out2, out)
    with pytest.raises(TypeError):
        canvas.window_blend(x, bl, g, torch.float32)
    with pytest.raises(ValueError):
        canvas.window_blend(x, solver.Blend(x0[..., :8], bl.keep, qn, Q_A, Q_B), g, dtype)


# ---------------------------------------------------------------------------------------------------
# trajectories
# ---------------------------------------------------------------------------------------------------
def _x0(canvas, seed=9):
    return torch.randn((1, 4) + tuple(canvas), generator=torch.Generator().manual_seed(seed))


def _sampler(kind, dtype, canvas, device="cuda", **kw):
    return _cls(kind)(_model(dtype, device), **dict(dict(opt_epochs=0, use_graph=False, save_images=False,
                                                          mask_noise=_draws(STEPS, 7, (1, 4) + tuple(canvas))), **kw))


def _inpaint(sampler, canvas, stride, keep, x0, centres=CENTRES, device="cuda", **kw):
    c, local_ctx, x_T = _inputs(canvas, device)
    sampler.inpaint_canvas(S=STEPS, canvas=canvas, window=S_LAT, stride=stride, mask=keep.to(device), x0=x0.to(device), conditionings=[c],
                           unconditional_conditionings=gi.load_uncond().to(device), bboxs=[centres], object_names=[["a", "b"]],
                           local_conditionings=[local_ctx], x_T=x_T, unconditional_guidance_scale=7.5, eta=0.0, seed=1, **kw)
    assert sampler._inpaint is None and sampler._canvas is None
    return sampler.last_result["x0"].clone()


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_inpaint_canvas_of_one_window_equals_masked_sample(kind, monkeypatch):
    """Canvas 32 x 32 (one window) against `sample(mask=, x0=)` with the same blend draws, torch.equal. As in
    test_canvas_gpu.test_canvas_of_one_window_equals_sample both sides run with deterministic library convolutions requested (the
    golden-width UNet's 8 x 8 level is not bit-reproducible between two identical calls otherwise)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    canvas = (S_LAT, S_LAT)
    keep, x0 = keep_mask(1, *canvas), _x0(canvas)
    sampler = _sampler(kind, torch.float16, canvas)
    got = _inpaint(sampler, canvas, 16, keep, x0, centres=[[0.3, 0.4], [0.7, 0.6]])
    c, local_ctx, x_T = _inputs(canvas)
    sampler.sample(S=STEPS, conditioning=c, batch_size=1, shape=[4, S_LAT, S_LAT], verbose=False, unconditional_guidance_scale=7.5,
                   unconditional_conditioning=gi.load_uncond().cuda(), eta=0.0, x_T=x_T, text_index=0, curr_text="x",
                   bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], seed=1, prompt_idx=0, object_names=["a", "b"], local_conditionings=local_ctx,
                   mask=keep.cuda(), x0=x0.cuda())
    want = sampler.last_result["x0"]
    print("%s: inpaint_canvas vs sample(mask=) %.4f %% of max" % (kind, 100 * _rel(got, want)))
    assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_inpaint_canvas_of_two_disjoint_windows_equals_masked_sample_batch(kind, monkeypatch):
    """Canvas 32 x 64, stride 32, a different mask per half, against `sample_batch(mask=, x0=)` of the two halves with their remapped
    centres and the halves of x_T, x0 and the blend draws: the same UNet batch and the same arithmetic (a mean over one window), so
    torch.equal, with deterministic library convolutions requested on both sides."""
    from sta.canvas import window_centres
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    canvas = (S_LAT, 2 * S_LAT)
    halves = lambda t: torch.cat([t[..., :S_LAT], t[..., S_LAT:]])
    left = keep_mask(1, S_LAT, S_LAT)
    keep = torch.cat([left, (1.0 - left).flip(-1)], dim=3)
    x0 = _x0(canvas)
    sampler = _sampler(kind, torch.float16, canvas)
    got = _inpaint(sampler, canvas, S_LAT, keep, x0)
    c, local_ctx, x_T = _inputs(canvas)
    sampler.mask_noise = [halves(n) for n in sampler.mask_noise]
    sampler.sample_batch(S=STEPS, shape=[4, S_LAT, S_LAT], conditionings=[c, c], unconditional_conditionings=gi.load_uncond().cuda(),
                         bboxs=window_centres(CENTRES, _grid((S_LAT, 2 * S_LAT, S_LAT, S_LAT))), object_names=[["a", "b"]] * 2,
                         local_conditionings=[local_ctx, local_ctx], x_T=halves(x_T), unconditional_guidance_scale=7.5, eta=0.0, seed=1,
                         mask=halves(keep).cuda(), x0=halves(x0).cuda())
    want = sampler.last_result["x0"]
    for w, half in enumerate((got[..., :S_LAT], got[..., S_LAT:])):
        print("%s window %d: max |canvas - sample_batch| %.4f %% of max" % (kind, w, 100 * _rel(half, want[w:w + 1])))
    assert torch.equal(halves(got), want)


_HOST = {}


def _host(kind, canvas, keep, x0):
    """The same masked canvas trajectory in fp32 on the host: oracle-backed blocks and the torch restatements of the kernels."""
    from tests.cpu_backend import oracle_ops
    if (kind, canvas) not in _HOST:
        with oracle_ops():
            _HOST[(kind, canvas)] = _inpaint(_sampler(kind, torch.float32, canvas, "cpu"), canvas, 16, keep, x0, device="cpu")
    return _HOST[(kind, canvas)]


@pytest.mark.parametrize("dtype,tol_max,tol_mean", TOLS)
@pytest.mark.parametrize("canvas", [(S_LAT, 2 * S_LAT), (2 * S_LAT, S_LAT)])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_overlapping_inpaint_canvas_vs_fp32_host_trajectory(kind, canvas, dtype, tol_max, tol_mean):
    """Canvas 32 x 64 and 64 x 32, stride 16 (T = 3 overlapping windows), S = 8, mixed keep mask, on the GPU (sta_window_blend, then one
    sta_sampler_step_windows_masked launch per call) vs the same sampler on CPU tensors through the restatements, inside TOLS of
    tests/test_solver_gpu.py (fp16 max 1 %, mean 0.5 %; bf16 max 3 %, mean 2 % of max|x| / mean|x|)."""
    keep, x0 = keep_mask(1, *canvas), _x0(canvas)
    ref = _host(kind, canvas, keep, x0)
    got = _inpaint(_sampler(kind, dtype, canvas), canvas, 16, keep, x0).float().cpu()
    assert got.shape == (1, 4) + canvas and torch.isfinite(got).all()
    err = (got - ref).abs()
    e_max, e_mean = (err.max() / ref.abs().max()).item(), (err.mean() / ref.abs().mean()).item()
    print("inpaint canvas %s %s %s: max %.3f %%, mean %.3f %%" % (canvas, kind, dtype, 100 * e_max, 100 * e_mean))
    assert e_max <= tol_max and e_mean <= tol_mean, (e_max, e_mean)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_keep_zero_equals_sample_canvas(kind, monkeypatch):
    """keep == 0 everywhere on the overlapping 32 x 64 canvas: bit for bit `sample_canvas` (deterministic library convolutions requested)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    canvas = (S_LAT, 2 * S_LAT)
    sampler = _sampler(kind, torch.float16, canvas)
    got = _inpaint(sampler, canvas, 16, torch.zeros(1, 1, *canvas), _x0(canvas))
    c, local_ctx, x_T = _inputs(canvas)
    sampler.sample_canvas(S=STEPS, canvas=canvas, window=S_LAT, stride=16, conditionings=[c], unconditional_conditionings=gi.load_uncond().cuda(),
                          bboxs=[CENTRES], object_names=[["a", "b"]], local_conditionings=[local_ctx], x_T=x_T,
                          unconditional_guidance_scale=7.5, eta=0.0, seed=1)
    want = sampler.last_result["x0"]
    print("%s keep == 0 vs sample_canvas: %.4f %% of max" % (kind, 100 * _rel(got, want)))
    assert torch.equal(got, want)
    masked = _inpaint(sampler, canvas, 16, keep_mask(1, *canvas), _x0(canvas))
    assert _rel(masked, want) > 0.05                                            # a mask does something


def test_unfused_masked_step_agrees_with_the_fused_launch():
    """canvas_fused_step = False (latent_blend + window_split, then window_fuse + solver_step_masked + window_split: the means are rounded
    to fp16 before the step) against the one-launch form, to the bound of test_canvas_gpu.test_unfused_step_agrees_with_the_fused_launch:
    1 % of max."""
    canvas = (S_LAT, 2 * S_LAT)
    keep, x0 = keep_mask(1, *canvas), _x0(canvas)
    a = _inpaint(_sampler("ddim", torch.float16, canvas), canvas, 16, keep, x0)
    b = _inpaint(_sampler("ddim", torch.float16, canvas, canvas_fused_step=False), canvas, 16, keep, x0)
    e = _rel(b, a)
    print("masked fused vs unfused step: max %.4f %%" % (100 * e))
    assert e <= 0.01


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_inpaint_canvas_graph_replay_matches_eager(kind):
    """hipGraph replay of the window UNet call == eager launches on the masked overlapping canvas: within 2 % of max, the bound of
    test_canvas_gpu.test_canvas_graph_replay_matches_eager."""
    canvas = (S_LAT, 2 * S_LAT)
    keep, x0 = keep_mask(1, *canvas), _x0(canvas)
    eager = _inpaint(_sampler(kind, torch.float16, canvas), canvas, 16, keep, x0)
    sampler = _sampler(kind, torch.float16, canvas, use_graph=True)
    replay = _inpaint(sampler, canvas, 16, keep, x0)
    e = _rel(replay, eager)
    print("%s masked canvas graph replay vs eager: max %.3f %%" % (kind, 100 * e))
    assert e <= 0.02, e
    assert len(sampler._graphs._entries) == 1


def test_launch_structure(monkeypatch):
    """A fused masked trajectory of S calls makes one window_blend, S - 1 sampler_step_windows_masked and one sampler_step_windows call,
    and none of window_split, window_fuse, latent_blend, solver_step*."""
    canvas = (S_LAT, 2 * S_LAT)
    counters = Counters(monkeypatch)
    _inpaint(_sampler("ddim", torch.float16, canvas), canvas, 16, keep_mask(1, *canvas), _x0(canvas))
    assert counters.count() == {"window_blend": 1, "sampler_step_windows_masked": STEPS - 1, "sampler_step_windows": 1}
    assert counters.calls[0] == "window_blend" and counters.calls[-1] == "sampler_step_windows"


@pytest.mark.parametrize("dtype", DTYPES)
def test_pixel_paste_of_the_canvas_decode(dtype, tmp_path):
    """image= / mask_px=: last_result["image"] is the composite (sta_image_composite) of the ONE decode of the whole 32 x 64 canvas with
    the original, within one unit in the last place of the 16-bit type of image_composite_reference in float64; the saved PNG holds
    the original's 8-bit values exactly where mask_px == 1."""
    from PIL import Image
    from sta import solver
    canvas = (S_LAT, 2 * S_LAT)
    model = _wopt_model(dtype, "cuda")
    keep = keep_mask(1, *canvas)
    keep_px = (keep == 1).float().repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)
    orig_u8 = torch.randint(0, 256, (1, 3, 8 * S_LAT, 16 * S_LAT), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    orig = orig_u8.float() / 255.0
    sampler = _cls("ddim")(model, opt_epochs=0, use_graph=False, save_images=True, outdir=str(tmp_path),
                           mask_noise=_draws(STEPS, 7, (1, 4) + canvas))
    decoded, inner = [], model.decode_first_stage
    model.decode_first_stage = lambda z, *a, **k: (decoded.append(inner(z, *a, **k)), decoded[-1])[1]
    try:
        _inpaint(sampler, canvas, 16, keep, _x0(canvas), image=orig, mask_px=keep_px, prompt_indices=[3])
    finally:
        del model.decode_first_stage
    assert len(decoded) == 1 and decoded[0].shape == (1, 3, 8 * S_LAT, 16 * S_LAT) and decoded[0].dtype == dtype
    img = sampler.last_result["image"]
    ref = solver.image_composite_reference(decoded[0].double().cpu(), orig.double(), keep_px.double())
    err = (img.double().cpu() - ref).abs()
    print("composite %s: max err / ulp = %.3f" % (dtype, (err / (ULP[dtype] * ref.abs() + 2.0 ** -24)).max().item()))
    assert img.dtype == dtype and (err <= ULP[dtype] * ref.abs() + 2.0 ** -24).all()
    png = np.array(Image.open(tmp_path / "final0_s1_index_3.png").convert("RGB"))
    kept = (keep_px[0, 0] == 1).numpy()
    want = orig_u8[0].permute(1, 2, 0).numpy()
    assert png.shape == want.shape and kept.any() and not kept.all()
    assert (png[kept] == want[kept]).all() and (png[~kept] != want[~kept]).mean() > 0.5


# ---------------------------------------------------------------------------------------------------
# entry point
# ---------------------------------------------------------------------------------------------------
def test_outpaint_script_synthetic_end_to_end(tmp_path):
    """scripts/outpaint.py --synthetic on a generated 256^2 PNG placed at x = 128 of a 256 x 512 canvas with a 16-pixel seam (256 x 256
    windows, stride 128: T = 3), K = 2 from a --layout, 4 DDIM steps: one 512 x 256 PNG whose kept footprint (pixel columns 144 .. 367)
    holds the source's 8-bit values and whose new area does not."""
    import subprocess
    import sys
    from PIL import Image
    rng = np.random.default_rng(0)
    src = rng.integers(0, 255, (256, 256, 3), dtype=np.uint8)
    init = str(tmp_path / "in.png")
    Image.fromarray(src).save(init)
    layout = tmp_path / "layout.json"
    layout.write_text(json.dumps({"0": {"cat": [0.1, 0.5], "dog": [0.9, 0.5]}}))
    out = tmp_path / "out"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(repo, "diffusion-spacetime-attn_amd", "scripts", "outpaint.py")
    r = subprocess.run([sys.executable, script, "--synthetic", "--init-img", init, "--prompt", "a cat left of a dog", "--layout", str(layout),
                        "--ddim_steps", "4", "--opt_epochs", "0", "--outdir", str(out), "--canvas", "256x512", "--H", "256", "--W", "256",
                        "--place", "128,0", "--seam", "16"], capture_output=True, text=True, timeout=600, env=dict(os.environ, STA_CONV_FIND="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "256x512 canvas (3 windows)" in r.stdout
    path = out / "final0_s42_index_0.png"
    assert path.exists(), sorted(os.listdir(out))
    got = np.array(Image.open(path).convert("RGB"))
    assert got.shape == (256, 512, 3)
    assert (got[:, 144:368] == src[:, 16:240]).all()
    new = np.concatenate([got[:, :144], got[:, 368:]], axis=1)
    assert np.isfinite(new).all() and new.std() > 0
    assert (got[:, 128:144] != src[:, :16]).mean() > 0.5                        # the seam strip is repainted
