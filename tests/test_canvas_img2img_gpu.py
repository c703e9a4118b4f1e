"""img2img on canvases on the MI355X: the fused entry launch (sta_vae_encode_step_windows, csrc/sta_window.hip)
against a float64 restatement, bit for bit against the two launches it replaces (sta_vae_encode_step + sta_window_split) and under rolls
of a ring; `DDIMSampler.decode_canvas` against the fp32 host trajectory, `decode`, `decode_batch`, `sample_canvas`, the unfused entry and
graph replay; scripts/img2img.py --canvas end to end."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from tests.test_canvas_gpu import _cls, _inputs, _model  # noqa: E402
from tests.test_canvas_img2img_cpu import P, S1M, SA, SF, _float64, _tensors  # noqa: E402
from tests.test_canvas_inpaint_cpu import _draws, keep_mask  # noqa: E402
from tests.test_canvas_wrap_cpu import SHAPES, _grid, _roll_canvas, _roll_windows  # noqa: E402
from tests.test_solver_gpu import TOLS  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
# (16, 40, 16, 16): 80 lane vectors per canvas, 160 in all: not a multiple of 256 and less than one block; (32, 64, 32, 16): 512 in all,
# two blocks; (24, 40, 16, 8): 240, windows that overlap along both axes
CLAMPED = [(32, 64, 32, 16, ""), (16, 40, 16, 16, ""), (24, 40, 16, 8, "")]
S_LAT, STEPS, K = 32, 4, 2
CANVAS = (S_LAT, 2 * S_LAT)
CENTRES = [[0.25, 0.4], [0.625, 0.6]]                  # canvas-normalised; on a 32 x 64 canvas the second disc straddles x = 0.5
SEAM = [[0.25, 0.4], [0.9375, 0.6]]                    # the second disc (x = 60 of 64) crosses the seam of a canvas closed along x


def _launch(g, h, qw, qb, n_post, n_enc, **kw):
    from sta import canvas
    out = canvas.encode_step_windows(h.cuda().contiguous(memory_format=torch.channels_last), qw.cuda(), qb.cuda(), n_post.cuda(), n_enc.cuda(),
                                     SF, SA, S1M, g, **kw)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CLAMPED + SHAPES)
def test_kernel_vs_float64(shape, dtype):
    """x and z0 within 1e-5 (1 + |ref|) of the float64 restatement of test_vae_encode_step_vs_float64, logvar beyond both clamp limits;
    xin bit for bit the restatement's split of the launch's x; z0 / xin NULL leave x as it is."""
    from sta.canvas import window_split_reference
    g = _grid(shape)
    assert P * g.Hc * g.Wc // 8 in (128, 160, 192, 240, 256, 512) and P == 2
    t = _tensors(g, dtype)
    x, z0, xin = _launch(g, *t, want_z0=True, want_xin=True)
    for got, ref in zip((z0, x), _float64(*t)):
        err = (got.cpu().double() - ref).abs()
        assert torch.isfinite(got).all() and (err <= 1e-5 * (1.0 + ref.abs())).all(), err.max().item()
    assert xin.dtype == dtype and torch.equal(xin.cpu(), window_split_reference(x.cpu(), g, dtype))
    x2, none_z, none_xin = _launch(g, *t, want_z0=False, want_xin=False)
    assert none_z is None and none_xin is None and torch.equal(x2, x)
    x3, z3, none_xin = _launch(g, *t, want_z0=True, want_xin=False)
    assert none_xin is None and torch.equal(x3, x) and torch.equal(z3, z0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CLAMPED + SHAPES)
def test_kernel_is_the_two_launches_it_replaces(shape, dtype):
    """Bit for bit: x, z0, xin of the one launch == sta_vae_encode_step followed by sta_window_split(rows = 1, STA_SRC_F32)."""
    from sta import canvas, fused
    g = _grid(shape)
    h, qw, qb, n_post, n_enc = _tensors(g, dtype, seed=5)
    got = _launch(g, h, qw, qb, n_post, n_enc, want_z0=True, want_xin=True)
    hd = h.cuda().contiguous(memory_format=torch.channels_last)
    x, z0, _ = fused.vae_encode_step(hd, qw.cuda(), qb.cuda(), n_post.cuda(), n_enc.cuda(), SF, SA, S1M, want_z0=True, want_xin=False)
    xin = canvas.window_split(x, g, dtype)
    torch.cuda.synchronize()
    for a, b in zip(got, (x, z0, xin)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_window_gives_the_square_launch_its_xin(dtype):
    """T = 1 (canvas = window): xin == sta_vae_encode_step's CFG input pair, and x, z0 its x, z0."""
    from sta import fused
    g = _grid((24, 24, 24, 8))
    assert g.T == 1
    h, qw, qb, n_post, n_enc = _tensors(g, dtype, seed=6)
    got = _launch(g, h, qw, qb, n_post, n_enc, want_z0=True, want_xin=True)
    want = fused.vae_encode_step(h.cuda().contiguous(memory_format=torch.channels_last), qw.cuda(), qb.cuda(), n_post.cuda(), n_enc.cuda(), SF, SA,
                                 S1M, want_z0=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_ring_launch_is_roll_equivariant(shape, dtype):
    """h and both noises rolled by k strides along the wrapped axes and the windows moved k places round the ring: x, z0 and xin are the
    rolled ones, bit for bit. Nothing is summed over windows here, so this holds at every cover."""
    g = _grid(shape)
    h, qw, qb, n_post, n_enc = _tensors(g, dtype, seed=7)
    x, z0, xin = _launch(g, h, qw, qb, n_post, n_enc, want_z0=True, want_xin=True)
    for k in (1, max(g.ny, g.nx) - 1):
        ky, kx = k if "y" in g.wrap else 0, k if "x" in g.wrap else 0
        rc = lambda t: _roll_canvas(t, g, ky, kx).contiguous()
        assert not torch.equal(rc(h), h)
        xr, zr, xinr = _launch(g, rc(h), qw, qb, rc(n_post), rc(n_enc), want_z0=True, want_xin=True)
        assert torch.equal(xr, rc(x)) and torch.equal(zr, rc(z0)) and torch.equal(xinr, _roll_windows(xin, g, ky, kx))


# ---------------------------------------------------------------------------------------------------
# decode_canvas: golden-width UNet, S = 4, t_start = 2, a 32 x 64 canvas, stride 16
# ---------------------------------------------------------------------------------------------------
def _sampler(dtype, device="cuda", masked=False, **kw):
    if masked:
        kw = dict(dict(mask_noise=_draws(STEPS, 7, (1, 4) + CANVAS)), **kw)
    fused_step = kw.pop("canvas_fused_step", True)       # a class attribute, not a constructor keyword
    s = _cls("ddim")(_model(dtype, device), **dict(dict(opt_epochs=0, use_graph=False, save_images=False), **kw))
    s.canvas_fused_step = fused_step
    s.make_schedule(STEPS, ddim_eta=0.0, verbose=False)
    return s


def _kept():
    return keep_mask(1, *CANVAS), torch.randn((1, 4) + CANVAS, generator=torch.Generator().manual_seed(9))


def _decode_canvas(s, device="cuda", canvas=CANVAS, stride=16, t_start=2, wrap="", masked=False, centres=None, x=None, **kw):
    c, local_ctx, x_T = _inputs(canvas, device)
    x = x_T if x is None else x
    if masked:
        keep, x0 = _kept()
        kw = dict(dict(mask=keep.to(device), x0=x0.to(device)), **kw)
    out = s.decode_canvas(x, canvas, S_LAT, stride, t_start=t_start, conditionings=[c], unconditional_conditionings=gi.load_uncond().to(device),
                          bboxs=[centres or (SEAM if wrap else CENTRES)], object_names=[["a", "b"]], local_conditionings=[local_ctx],
                          unconditional_guidance_scale=7.5, seed=1, wrap=wrap, **kw)
    assert s._canvas is None and s._start == 0 and s._xin0 is None and s._inpaint is None
    return out.clone()


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


_HOST = {}


def _host(wrap, masked):
    """The same decode in fp32 on the host: oracle-backed blocks and the torch restatements of the window kernels."""
    from tests.cpu_backend import oracle_ops
    if (wrap, masked) not in _HOST:
        with oracle_ops():
            _HOST[(wrap, masked)] = _decode_canvas(_sampler(torch.float32, "cpu", masked), "cpu", wrap=wrap, masked=masked)
    return _HOST[(wrap, masked)]


@pytest.mark.parametrize("dtype,tol_max,tol_mean", TOLS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("wrap", ["", "x"])
def test_decode_canvas_vs_fp32_host_trajectory(wrap, masked, dtype, tol_max, tol_mean):
    """decode_canvas on the GPU (the last 2 of 4 DDIM calls, T = 3 clamped windows or T = 4 round the ring with a disc across the seam;
    masked: sta_window_blend before the first call and the masked step after it) vs the same decode in fp32 on the host, inside TOLS of
    tests/test_solver_gpu.py, the bounds tests/test_canvas_gpu.py and tests/test_canvas_inpaint_gpu.py use for DDIM: fp16 max 1 %, mean
    0.5 %; bf16 max 3 %, mean 2 % of max|x| / mean|x|."""
    ref = _host(wrap, masked)
    got = _decode_canvas(_sampler(dtype, masked=masked), wrap=wrap, masked=masked).float().cpu()
    assert got.shape == (1, 4) + CANVAS and torch.isfinite(got).all()
    err = (got - ref).abs()
    e_max, e_mean = (err.max() / ref.abs().max()).item(), (err.mean() / ref.abs().mean()).item()
    print("decode_canvas wrap=%r masked=%s %s: max %.3f %%, mean %.3f %%" % (wrap, masked, dtype, 100 * e_max, 100 * e_mean))
    assert e_max <= tol_max and e_mean <= tol_mean, (e_max, e_mean)


def _reproducible_unet(model, dtype, monkeypatch):
    """The UNet call replaced by the elementwise stand-in of tests/test_canvas_gpu.py, bit-reproducible whatever the library's convolutions
    do (it uses the state, the time, both contexts' rows and the weights column): everything of this feature around the UNet call then
    has to reproduce its counterpart bit for bit."""
    def unet(x_in, text_index, t, c_in, coef=None, bboxs_curr=None):
        b = x_in.shape[0] // 2
        gain = (0.3 + 0.001 * t.float().reshape(2 * b, 1, 1, 1) / 1000 + 0.01 * c_in.float().mean(dim=(1, 2)).reshape(2 * b, 1, 1, 1)
                + 0.02 * coef.float().reshape(b, -1).sum(1).repeat_interleave(2).reshape(2 * b, 1, 1, 1))
        h = x_in.to(dtype).float()
        return (torch.tanh(h * gain) + 0.1 * h.roll(1, dims=-1)).to(dtype).to(x_in.dtype)
    monkeypatch.setattr(model, "apply_model_extra", unet, raising=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", [False, True])
def test_decode_canvas_of_one_window_equals_decode(masked, dtype, monkeypatch):
    canvas = (S_LAT, S_LAT)
    _reproducible_unet(_model(dtype), dtype, monkeypatch)
    kw = {}
    if masked:
        kw = dict(mask=keep_mask(1, *canvas).cuda(), x0=torch.randn((1, 4) + canvas, generator=torch.Generator().manual_seed(9)).cuda())
    s = _sampler(dtype, mask_noise=_draws(STEPS, 7, (1, 4) + canvas))
    got = _decode_canvas(s, canvas=canvas, centres=CENTRES, **kw)
    c, local_ctx, x = _inputs(canvas)
    want = s.decode(x, c, 2, unconditional_guidance_scale=7.5, unconditional_conditioning=gi.load_uncond().cuda(), text_index=0, curr_text="x",
                    bboxs_curr=CENTRES, seed=1, prompt_idx=0, object_names=["a", "b"], local_conditionings=local_ctx, **kw)
    assert torch.isfinite(got).all() and got.abs().max() > 0 and not torch.equal(got, x) and torch.equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_canvas_of_two_disjoint_windows_equals_decode_batch(dtype, monkeypatch):
    from sta.canvas import window_centres
    _reproducible_unet(_model(dtype), dtype, monkeypatch)
    s = _sampler(dtype)
    got = _decode_canvas(s, stride=S_LAT)
    c, local_ctx, x = _inputs(CANVAS)
    want = s.decode_batch(torch.cat([x[..., :S_LAT], x[..., S_LAT:]]), [c, c], gi.load_uncond().cuda(),
                          window_centres(CENTRES, _grid((S_LAT, 2 * S_LAT, S_LAT, S_LAT))), [["a", "b"]] * 2, [local_ctx, local_ctx], 2,
                          unconditional_guidance_scale=7.5, seed=1)
    assert torch.equal(got[..., :S_LAT], want[0:1]) and torch.equal(got[..., S_LAT:], want[1:2])


@pytest.mark.parametrize("wrap", ["", "x"])
def test_decode_canvas_with_t_start_s_equals_sample_canvas(wrap, monkeypatch):
    dtype = torch.float16
    _reproducible_unet(_model(dtype), dtype, monkeypatch)
    s = _sampler(dtype)
    got = _decode_canvas(s, t_start=STEPS, wrap=wrap)
    c, local_ctx, x = _inputs(CANVAS)
    s.sample_canvas(S=STEPS, canvas=CANVAS, window=S_LAT, stride=16, conditionings=[c], unconditional_conditionings=gi.load_uncond().cuda(),
                    bboxs=[SEAM if wrap else CENTRES], object_names=[["a", "b"]], local_conditionings=[local_ctx], x_T=x,
                    unconditional_guidance_scale=7.5, eta=0.0, seed=1, wrap=wrap)
    assert torch.isfinite(got).all() and torch.equal(got, s.last_result["x0"])


def _encoded(s, g, dtype, **kw):
    """(x, z0, xin) of encode_step_canvas from a seeded encoder output on the canvas of grid g."""
    from tests.test_canvas_img2img_cpu import _Quant
    gen = torch.Generator().manual_seed(12)
    h = torch.randn(1, 8, g.Hc, g.Wc, generator=gen).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    n_post, n_enc = torch.randn(1, 4, g.Hc, g.Wc, generator=gen), torch.randn(1, 4, g.Hc, g.Wc, generator=gen)
    vae = _Quant()
    vae.quant_conv.cuda()
    return s.encode_step_canvas(h, vae, 2, n_post, n_enc, g, scale_factor=SF, **kw)


@pytest.mark.parametrize("wrap", ["", "x"])
def test_unfused_entry_agrees_with_the_fused_entry(wrap, monkeypatch):
    """canvas_fused_step = False takes sta_vae_encode_step + window_split: the same x and the same first window inputs, bit for bit. The
    later steps of the three-launch form round the means to fp16 before the step, as on every canvas: the trajectories agree to the 1 %
    of max of tests/test_canvas_gpu.test_unfused_step_agrees_with_the_fused_launch."""
    from sta import canvas
    dtype = torch.float16
    g = _grid(CANVAS + (S_LAT, 16, wrap))
    calls = []
    for name in ("encode_step_windows", "window_split"):
        inner = getattr(canvas, name)
        monkeypatch.setattr(canvas, name, lambda *a, _n=name, _f=inner, **k: (calls.append(_n), _f(*a, **k))[1])
    fused_s, unfused_s = _sampler(dtype), _sampler(dtype, canvas_fused_step=False)
    a = _encoded(fused_s, g, dtype, want_z0=True)
    assert calls == ["encode_step_windows"]
    b = _encoded(unfused_s, g, dtype, want_z0=True)
    assert calls == ["encode_step_windows", "window_split"]
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    with_xin = _decode_canvas(fused_s, wrap=wrap, x=a[0], xin=a[2])
    e = _rel(_decode_canvas(unfused_s, wrap=wrap, x=b[0], xin=b[2]), with_xin)
    print("decode_canvas wrap=%r fused vs unfused step: max %.4f %%" % (wrap, 100 * e))
    assert e <= 0.01


@pytest.mark.parametrize("wrap", ["", "x"])
def test_xin_of_the_fused_entry_gives_the_same_result_as_none(wrap, monkeypatch):
    dtype = torch.float16
    _reproducible_unet(_model(dtype), dtype, monkeypatch)
    s = _sampler(dtype)
    g = _grid(CANVAS + (S_LAT, 16, wrap))
    x, _, xin = _encoded(s, g, dtype)
    c, local_ctx, _ = _inputs(CANVAS)
    run = lambda **kw: s.decode_canvas(x, CANVAS, S_LAT, 16, t_start=2, conditionings=[c], unconditional_conditionings=gi.load_uncond().cuda(),
                                       bboxs=[CENTRES], object_names=[["a", "b"]], local_conditionings=[local_ctx], wrap=wrap, **kw).clone()
    with_xin, without = run(xin=xin), run()
    assert torch.isfinite(with_xin).all() and torch.equal(with_xin, without)
    assert not torch.equal(run(xin=(0.5 * xin.float()).to(dtype)), without)


@pytest.mark.parametrize("masked", [False, True])
def test_decode_canvas_graph_replay_equals_eager(masked, monkeypatch):
    """hipGraph replay of the 2 P T = 6 row UNet call: bit for bit the eager launches around the reproducible UNet call, with one capture
    for both decodes; with the real UNet within the 2 % of max of tests/test_canvas_gpu.test_canvas_graph_replay_matches_eager."""
    dtype = torch.float16
    real = _rel(_decode_canvas(_sampler(dtype, masked=masked, use_graph=True), masked=masked), _decode_canvas(_sampler(dtype, masked=masked), masked=masked))
    print("decode_canvas masked=%s graph replay vs eager, real UNet: max %.3f %%" % (masked, 100 * real))
    assert real <= 0.02
    _reproducible_unet(_model(dtype), dtype, monkeypatch)
    eager = _decode_canvas(_sampler(dtype, masked=masked), masked=masked)
    s = _sampler(dtype, masked=masked, use_graph=True)
    replay = _decode_canvas(s, masked=masked)
    again = _decode_canvas(s, masked=masked)
    assert torch.isfinite(replay).all() and torch.equal(replay, eager) and torch.equal(again, eager)
    assert len(s._graphs._entries) == 1


# ---------------------------------------------------------------------------------------------------
# entry point
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", ["", "x"])
def test_img2img_script_with_a_canvas(wrap, tmp_path):
    """scripts/img2img.py --synthetic --canvas 256x512 with 256 x 256 windows (stride 128: T = 3 clamped, T = 4 round the ring), 4 DDIM
    steps at strength 0.5, one prompt with K = 2, from a 160 x 96 picture, smaller than the canvas: resized, encoded once, one 512 x 256
    PNG named as before."""
    import json
    import subprocess
    import sys
    from PIL import Image
    init = str(tmp_path / "in.png")
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (96, 160, 3), dtype=np.uint8)).save(init)
    (tmp_path / "prompts.txt").write_text("a cat left of a dog\n")
    (tmp_path / "layout.json").write_text(json.dumps({"0": {"cat": [0.2, 0.4], "dog": [0.95, 0.6]}}))
    out = tmp_path / "out"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "diffusion-spacetime-attn_amd", "scripts", "img2img.py")
    r = subprocess.run([sys.executable, script, "--synthetic", "--init-img", init, "--from-file", str(tmp_path / "prompts.txt"), "--layout",
                        str(tmp_path / "layout.json"), "--ddim_steps", "4", "--strength", "0.5", "--opt_epochs", "0", "--outdir", str(out),
                        "--canvas", "256x512", "--window", "256"] + (["--canvas_wrap", wrap] if wrap else []),
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, STA_CONV_FIND="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "160 x 96 resized to the 512 x 256 canvas" in r.stdout and "256x512 canvas (%d windows each)" % (4 if wrap else 3) in r.stdout
    path = out / "final0_s42_index_0.png"
    assert path.exists(), sorted(os.listdir(out))
    assert Image.open(path).size == (512, 256)
