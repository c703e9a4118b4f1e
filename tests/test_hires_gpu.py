"""The layout-guided hi-res fix on the MI355X: the fused upscale launch (sta_latent_upscale_step_windows,
csrc/sta_window.hip) against the float64 evaluation of tests/test_hires_cpu.py, under rolls of a ring, with one window and against the
unfused entry; `DDIMSampler.hires_canvas` against the fp32 host trajectory, graph replay and the `disc_scale` keyword; the entry-point
script with --hires end to end."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from tests.test_canvas_gpu import _cls, _inputs, _model  # noqa: E402
from tests.test_canvas_img2img_gpu import _rel, _reproducible_unet  # noqa: E402
from tests.test_hires_cpu import ALL, C, EPS, P, RINGS, S, S1M, SA, _grid, bounds, float64, tensors  # noqa: E402
from tests.test_solver_gpu import TOLS  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]


def _launch(shape, dtype, z=None, noise=None, seed=3, **kw):
    from sta import canvas
    z0, n0 = tensors(shape, seed)
    out = canvas.upscale_step_windows((z0 if z is None else z).cuda(), (n0 if noise is None else noise).cuda(), SA, S1M, _grid(shape), dtype, **kw)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ALL)
def test_kernel_vs_float64(shape, dtype):
    """x and z_up elementwise within 16 x 2^-24 x (|sa| max|z| + |s1m noise|) (z_up: 16 x 2^-24 x max|z|) of the float64 evaluation with
    the same fp32 weights; xin bit for bit sta_window_split of the launch's own x; z_up / xin NULL leave x as it is."""
    from sta import canvas
    g = _grid(shape)
    assert P * C * g.Hc * g.Wc // 8 in (384, 960, 1536)        # 1.5, 3.75 and 6 blocks of 256 lanes: the last block partly idle twice
    x, z_up, xin = _launch(shape, dtype, want_z_up=True)
    z_ref, x_ref = float64(shape)
    bz, bx = bounds(shape)
    ez, ex = (z_up.cpu().double() - z_ref).abs(), (x.cpu().double() - x_ref).abs()
    print("kernel vs float64 %s %s: z_up %.3g (bound %.3g), x %.3g" % (shape, dtype, ez.max().item(), bz.item(), ex.max().item()))
    assert torch.isfinite(x).all() and (ez <= bz).all() and (ex <= bx).all()
    split = canvas.window_split(x, g, dtype)
    torch.cuda.synchronize()
    assert xin.dtype == dtype and tuple(xin.shape) == (2 * P * g.T, C, S, S) and torch.equal(xin, split)
    assert torch.equal(xin.cpu(), canvas.window_split_reference(x.cpu(), g, dtype))
    x2, none_z, none_xin = _launch(shape, dtype, want_xin=False)
    assert none_z is None and none_xin is None and torch.equal(x2, x)
    x3, z3, none_xin = _launch(shape, None, want_z_up=True, want_xin=False)
    assert none_xin is None and torch.equal(x3, x) and torch.equal(z3, z_up)
    if shape[:4] == (16, 24, 16, 24):                          # identity size: the upscale is the source
        assert torch.equal(z_up.cpu(), tensors(shape)[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", RINGS)
def test_ring_launch_is_roll_equivariant(shape, dtype):
    """Integer factor 2: z rolled by k cells and the noise by 2 k along the wrapped axes rolls x and z_up by 2 k, bit for bit, and xin is
    the split of the rolled x (2 k = 2 is no multiple of the stride 8: the windows see other columns, not moved ones)."""
    from sta import canvas
    g = _grid(shape)
    z, noise = tensors(shape)
    x, z_up, xin = _launch(shape, dtype, want_z_up=True)
    for k in (1, 5):
        ky, kx = k if "y" in shape[4] else 0, k if "x" in shape[4] else 0
        roll = lambda t: t.roll((2 * ky, 2 * kx), (-2, -1))
        xr, zr, xinr = _launch(shape, dtype, z=z.roll((ky, kx), (-2, -1)).contiguous(), noise=roll(noise).contiguous(), want_z_up=True)
        assert not torch.equal(zr, z_up)
        assert torch.equal(xr, roll(x)) and torch.equal(zr, roll(z_up))
        assert torch.equal(xinr, canvas.window_split(roll(x).contiguous(), g, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_window_writes_the_pair(dtype):
    """canvas == window and identity size: z_up == z and xin is the CFG input pair solver._pair(x) in 16 bit."""
    from sta import solver
    shape = (16, 16, 16, 16, "")
    assert _grid(shape).T == 1
    x, z_up, xin = _launch(shape, dtype, want_z_up=True)
    assert torch.equal(z_up.cpu(), tensors(shape)[0]) and torch.equal(xin, solver._pair(x).to(dtype))


def _sampler(dtype, device="cuda", **kw):
    fused_step = kw.pop("canvas_fused_step", True)       # a class attribute, not a constructor keyword
    s = _cls("ddim")(_model(dtype, device), **dict(dict(opt_epochs=0, use_graph=False, save_images=False), **kw))
    s.canvas_fused_step = fused_step
    s.make_schedule(STEPS, ddim_eta=0.0, verbose=False)
    return s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ALL)
def test_fused_entry_agrees_with_the_unfused_entry(shape, dtype, monkeypatch):
    """upscale_step_canvas: one launch against the restatement + sta_window_split (`canvas_fused_step = False`). x agrees within twice the
    bound (each is within the bound of the float64 evaluation); the xin of each is the exact rounding of its own x."""
    from sta import canvas
    g = _grid(shape)
    z, noise = tensors(shape)
    calls = []
    for name in ("upscale_step_windows", "upscale_step_windows_reference", "window_split"):
        inner = getattr(canvas, name)
        monkeypatch.setattr(canvas, name, lambda *a, _n=name, _f=inner, **k: (calls.append(_n), _f(*a, **k))[1])
    fused_s, unfused_s = _sampler(dtype), _sampler(dtype, canvas_fused_step=False)
    a = fused_s.upscale_step_canvas(z.cuda(), 2, noise.cuda(), g, want_z_up=True)
    assert calls == ["upscale_step_windows"]
    b = unfused_s.upscale_step_canvas(z.cuda(), 2, noise.cuda(), g, want_z_up=True)
    assert calls == ["upscale_step_windows", "upscale_step_windows_reference", "window_split"]
    torch.cuda.synchronize()
    sa, s1m = fused_s._encode_coefs()
    bound = 16 * EPS * (abs(float(sa[2])) * z.abs().max().double() + (float(s1m[2]) * noise.double()).abs())
    err = (a[0].cpu().double() - b[0].cpu().double()).abs()
    print("fused vs unfused %s %s: %.3g" % (shape, dtype, err.max().item()))
    assert (err <= 2 * bound).all()
    assert ((a[1].cpu().double() - b[1].cpu().double()).abs() <= 2 * 16 * EPS * z.abs().max().double()).all()
    for x, _, xin in (a, b):
        assert xin.dtype == dtype and torch.equal(xin.cpu(), canvas.window_split_reference(x.cpu(), g, dtype))


# ---------------------------------------------------------------------------------------------------
# hires_canvas: golden-width UNet, S = 4, t_start = 2, a 32 x 32 first pass refined on a 64 x 64 canvas (T = 9; wrapped along x: T = 12)
# ---------------------------------------------------------------------------------------------------
S_LAT, STEPS, K = 32, 4, 2
CANVAS = (2 * S_LAT, 2 * S_LAT)
CENTRES = [[0.25, 0.4], [0.625, 0.6]]
SEAM = [[0.25, 0.4], [0.9375, 0.6]]                    # the second disc crosses the seam of a canvas closed along x


def _first_pass():
    return gi.unet_inputs(K, 5)[2]                      # a seeded 32 x 32 latent, standing in for a finished trajectory's x0


def _noise():
    return torch.randn((1, 4) + CANVAS, generator=torch.Generator().manual_seed(17))


def _hires(s, device="cuda", wrap="", **kw):
    c, local_ctx, _ = _inputs((S_LAT, S_LAT), device)
    out = s.hires_canvas(_first_pass().to(device), CANVAS, S_LAT, 16, **dict(dict(
        t_start=2, wrap=wrap, noise=_noise().to(device), conditionings=[c], unconditional_conditionings=gi.load_uncond().to(device),
        bboxs=[SEAM if wrap else CENTRES], object_names=[["a", "b"]], local_conditionings=[local_ctx], unconditional_guidance_scale=7.5,
        seed=1), **kw))
    assert s._canvas is None and s._start == 0 and s._xin0 is None and s._inpaint is None and s._disc_scale == 1.0
    return out.clone()


_HOST = {}


def _host(wrap):
    """The same two-step refine in fp32 on the host: oracle-backed blocks and the torch restatements, made once per wrap."""
    from tests.cpu_backend import oracle_ops
    if wrap not in _HOST:
        with oracle_ops():
            _HOST[wrap] = _hires(_sampler(torch.float32, "cpu"), "cpu", wrap=wrap)
    return _HOST[wrap]


@pytest.mark.parametrize("dtype,tol_max,tol_mean", TOLS)
@pytest.mark.parametrize("wrap", ["", "x"])
def test_hires_canvas_vs_fp32_host_trajectory(wrap, dtype, tol_max, tol_mean):
    """hires_canvas on the GPU (the fused entry launch, discs of radius 0.4 window sides, the last 2 of 4 DDIM calls on T = 9 clamped
    windows or T = 12 round the ring with a disc across the seam) vs the same in fp32 on the host from the restatement, inside TOLS of
    tests/test_solver_gpu.py: fp16 max 1 %, mean 0.5 %; bf16 max 3 %, mean 2 % of max|x| / mean|x|."""
    ref = _host(wrap)
    got = _hires(_sampler(dtype), wrap=wrap).float().cpu()
    assert got.shape == (1, 4) + CANVAS and torch.isfinite(got).all()
    err = (got - ref).abs()
    e_max, e_mean = (err.max() / ref.abs().max()).item(), (err.mean() / ref.abs().mean()).item()
    print("hires_canvas wrap=%r %s: max %.3f %%, mean %.3f %%" % (wrap, dtype, 100 * e_max, 100 * e_mean))
    assert e_max <= tol_max and e_mean <= tol_mean, (e_max, e_mean)


@pytest.mark.parametrize("wrap", ["", "x"])
def test_hires_canvas_graph_replay_equals_eager(wrap, monkeypatch):
    """hipGraph replay of the window UNet call: bit for bit the eager launches around the reproducible UNet call; with the real UNet
    within the 2 % of max of tests/test_canvas_gpu.test_canvas_graph_replay_matches_eager."""
    dtype = torch.float16
    real = _rel(_hires(_sampler(dtype, use_graph=True), wrap=wrap), _hires(_sampler(dtype), wrap=wrap))
    print("hires_canvas wrap=%r graph replay vs eager, real UNet: max %.3f %%" % (wrap, 100 * real))
    assert real <= 0.02
    _reproducible_unet(_model(dtype), dtype, monkeypatch)
    eager = _hires(_sampler(dtype), wrap=wrap)
    s = _sampler(dtype, use_graph=True)
    replay, again = _hires(s, wrap=wrap), _hires(s, wrap=wrap)
    assert torch.isfinite(replay).all() and torch.equal(replay, eager) and torch.equal(again, eager)


def _block_masks(model):
    from ldm.modules.attention import BasicTransformerBlock
    out = []
    for m in model.modules():
        if isinstance(m, BasicTransformerBlock):
            out += [c.mask.clone() for _, c in sorted(m._caches.items()) if c.mask is not None]
    return out


def test_disc_scale_one_is_bit_identical_to_no_keyword(monkeypatch):
    """decode_canvas(disc_scale=1.0) == decode_canvas(): the blocks' mask bits with the real UNet, and the result around the reproducible
    UNet call; disc_scale = 2.0 sets other bits."""
    dtype = torch.float16
    s = _sampler(dtype)
    c, local_ctx, _ = _inputs((S_LAT, S_LAT))
    x = torch.randn((1, 4) + CANVAS, generator=torch.Generator().manual_seed(5)).cuda()
    run = lambda **kw: s.decode_canvas(x, CANVAS, S_LAT, 16, t_start=2, conditionings=[c], unconditional_conditionings=gi.load_uncond().cuda(),
                                       bboxs=[CENTRES], object_names=[["a", "b"]], local_conditionings=[local_ctx], **kw).clone()
    masks = {}
    for key, kw in (("none", {}), ("one", dict(disc_scale=1.0)), ("two", dict(disc_scale=2.0))):
        run(**kw)
        masks[key] = _block_masks(s.model)
    assert masks["none"] and all(torch.equal(a, b) for a, b in zip(masks["none"], masks["one"]))
    assert any(not torch.equal(a, b) for a, b in zip(masks["none"], masks["two"]))
    _reproducible_unet(_model(dtype), dtype, monkeypatch)
    assert torch.equal(run(), run(disc_scale=1.0))


# ---------------------------------------------------------------------------------------------------
# entry point
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", ["", "x"])
def test_entry_point_script_with_hires(wrap, tmp_path):
    """scripts/txt2img-mscoco.py --hires on the synthetic model, 4 DDIM steps, fixed weights: a 256^2 first pass refined at 512x512 (T = 9
    windows of 256), and a 256x512 first-pass canvas closed along x refined at 512x1024 round the ring (T = 3 x 8); both passes' images
    are written."""
    import json
    import subprocess
    import sys
    from PIL import Image
    prompt = "a cat left of a dog on a street"
    (tmp_path / "mscoco.txt").write_text(prompt)
    (tmp_path / "layout.json").write_text(json.dumps({prompt: {"cat": [0.2, 0.5], "dog": [0.95, 0.5]}}))
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(repo, "diffusion-spacetime-attn_amd", "scripts", "txt2img-mscoco.py")
    first, second, T = ((256, 512), "512x1024", 24) if wrap else ((256, 256), "512x512", 9)
    extra = ["--canvas", "256x512", "--canvas_wrap", "x"] if wrap else []
    out = subprocess.run([sys.executable, script, "--ddim_steps", "4", "--synthetic", "--opt_epochs", "0", "--dataset", str(tmp_path / "mscoco.txt"),
                          "--layout", str(tmp_path / "layout.json"), "--limit", "1", "--outdir", str(tmp_path / "o"), "--H", "256", "--W", "256",
                          "--hires", second, "--hires_strength", "0.5"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, STA_CONV_FIND="0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "hi-res fix for prompts [0]: %s pixels, %d windows each, the last 2 of 4 DDIM calls, discs x 2" % (second, T) in out.stdout
    one, two = tmp_path / "result_outputs" / "final0_s1_index_0.png", tmp_path / "result_outputs" / "hires" / "final0_s1_index_0.png"
    assert one.exists() and two.exists(), out.stdout[-2000:]
    assert Image.open(one).size == (first[1], first[0]) and Image.open(two).size == (2 * first[1], 2 * first[0])
