"""sta_latent_guide_windows and attention guidance on canvases on the GPU: the kernel against guide_windows_reference in float64, the
guarantees of its launch (one window bit-equal to sta_latent_guide, bit-reproducible, canvases independent, outputs overwritten
completely and nothing else touched, inert canvases bit-equal), the
gradient that reaches the canvas latent on the miniature against the fp32 host chain, and the samplers end to end."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from tests.test_attnloss_gpu import K, RES, S, _model as _build_model  # noqa: E402
from tests.test_canvas_guidance_cpu import CENTRES, NAMES, STRIP, STRIP_CENTRES, S_LAT, TEXT  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
# (Hc, Wc, s, stride, wrap): 480 vectors per canvas at C = 4 (two workgroups, cover up to 4); 4352 vectors (the cap of 16 workgroups with
# a ragged slice, 10 offsets along x); a ring along x; a ring along both axes
GRIDS = [(24, 40, 16, 8, ""), (64, 136, 64, 8, ""), (16, 48, 16, 8, "x"), (32, 32, 16, 8, "xy")]


def _grid(args):
    from sta.canvas import window_grid
    return window_grid(*args)


def _inputs(grid, dtype, P=2, C=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, grid.Hc, grid.Wc, generator=g)
    gp = (torch.randn(2 * P * grid.T, C, grid.s, grid.s, generator=g) * 3e-3).to(dtype)
    keep = (torch.rand(P, 1, grid.Hc, grid.Wc, generator=g) > 0.6).float()
    keep[:, :, 0, :3] = 0.25                                                    # a soft edge as well
    step = torch.rand(P, generator=g) * 0.2 + 0.01
    count = torch.full((P,), float(C * grid.Hc * grid.Wc))
    count[1:] = float(C * grid.Hc * grid.Wc // 3)                               # a canvas of which a third receives gradient
    return x, gp, keep, step, count


def _raw(grid, gp, x, keep, step, count, x_out, xin, stats, normalize=True, inv_scale=1.0):
    """The binding itself on caller-owned buffers."""
    from sta import canvas, lib
    ptr = lambda t: 0 if t is None else t.data_ptr()
    name = "sta_latent_guide_windows"
    lib.check(getattr(lib.load(), name)(gp.data_ptr(), x.data_ptr(), ptr(keep), step.data_ptr(), count.data_ptr(), x_out.data_ptr(), ptr(xin),
                                        ptr(stats), x.shape[0], x.shape[1], grid.Hc, grid.Wc, *canvas._grid_args(grid), int(normalize),
                                        float(inv_scale), lib.STA_BF16 if gp.dtype == torch.bfloat16 else lib.STA_F16,
                                        torch.cuda.current_stream().cuda_stream), name)
    torch.cuda.synchronize()


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_the_float64_reference(grid, dtype):
    """The tolerances of sta_latent_guide (tests/test_guidance_gpu.py): rms within 1e-5 relative, x_out within 1e-5 (|x| + |s d|)
    elementwise; xin bit-equal to the split of the kernel's x_out; keep on / off, normalize on / off, xin and stats written / NULL."""
    from sta.canvas import guide_windows_reference, latent_guide_windows, window_split_reference
    grid = _grid(grid)
    x, gp, keep, step, count = _inputs(grid, dtype)
    worst_rms = worst_x = 0.0
    for kp in (None, keep):
        for normalize in (True, False):
            inv = 1.0 if normalize else 16.0
            ref, rms_ref = guide_windows_reference(gp, x.double(), step.double(), count.double(), grid, keep=kp, normalize=normalize, inv_scale=inv)
            moved = (ref - x.double()).abs()                                    # |s d|
            assert moved.max() > 1e-3
            for want_xin, want_stats in ((True, True), (False, False)):
                out, xin, rms = latent_guide_windows(gp.cuda(), x.cuda(), step.cuda(), count.cuda(), grid, keep=None if kp is None else kp.cuda(),
                                                     normalize=normalize, inv_scale=inv, want_xin=want_xin, want_stats=want_stats)
                torch.cuda.synchronize()
                assert (xin is None) == (not want_xin) and (rms is None) == (not want_stats)
                err = ((out.cpu().double() - ref).abs() / (x.double().abs() + moved)).max().item()
                worst_x = max(worst_x, err)
                assert err <= 1e-5, (kp is not None, normalize, err)
                if want_stats:
                    e = ((rms.cpu().double() - rms_ref).abs() / rms_ref).max().item()
                    worst_rms = max(worst_rms, e)
                    assert e <= 1e-5, (kp is not None, normalize, e)
                if want_xin:
                    assert xin.dtype == dtype and torch.equal(xin.cpu(), window_split_reference(out.cpu(), grid, dtype))
    print("%s %s: worst rms rel err %.2e, worst x_out err / (|x| + |s d|) %.2e" % (tuple(grid[:4]) + (grid.wrap,), dtype, worst_rms, worst_x))


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_window_is_sta_latent_guide_bit_for_bit(dtype):
    """canvas == window (512 vectors per canvas: two workgroups each): x_out, xin and stats equal sta_latent_guide's bits."""
    from sta.canvas import latent_guide_windows
    from sta.guidance import latent_guide
    grid = _grid((32, 32, 32, 16, ""))
    assert grid.T == 1
    x, gp, keep, step, _ = (t.cuda() for t in _inputs(grid, dtype, P=3, seed=4))
    gp[2:4] = 0.0                                                               # canvas 1 is skipped by both
    for kp in (None, keep):
        for normalize in (True, False):
            want = latent_guide(gp, x, step, keep=kp, normalize=normalize, inv_scale=8.0, want_xin=True)
            got = latent_guide_windows(gp, x, step, float(4 * 32 * 32), grid, keep=kp, normalize=normalize, inv_scale=8.0, want_xin=True)
            torch.cuda.synchronize()
            for a, b in zip(got, want):
                assert torch.equal(a.view(torch.int16 if a.dtype == dtype else torch.int32), b.view(torch.int16 if b.dtype == dtype else torch.int32))
            assert torch.equal(got[0][1], x[1]) and not torch.equal(got[0][0], x[0])


def test_launches_reproducible_and_canvases_independent():
    from sta.canvas import latent_guide_windows
    grid = _grid(GRIDS[0])
    x, gp, keep, step, count = (t.cuda() for t in _inputs(grid, torch.float16, P=3, seed=1))
    one = latent_guide_windows(gp, x, step, count, grid, keep=keep, want_xin=True)
    two = latent_guide_windows(gp, x, step, count, grid, keep=keep, want_xin=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(one, two))
    rows = 2 * grid.T
    gp2 = gp.clone()
    gp2[rows:2 * rows] = gp2[rows:2 * rows] * 2.0 + 1.0                         # canvas 1's gradient changes
    other = latent_guide_windows(gp2, x, step, count, grid, keep=keep, want_xin=True)
    torch.cuda.synchronize()
    for a, c, n in zip(one, other, (1, rows, 1)):
        assert torch.equal(a[:n], c[:n]) and torch.equal(a[2 * n:], c[2 * n:]) and not torch.equal(a[n:2 * n], c[n:2 * n])
    alone = latent_guide_windows(gp[2 * rows:], x[2:3], step[2:3], count[2:3], grid, keep=keep[2:3], want_xin=True)
    torch.cuda.synchronize()
    assert torch.equal(alone[0], one[0][2:3]) and torch.equal(alone[1], one[1][2 * rows:]) and torch.equal(alone[2], one[2][2:3])


@pytest.mark.parametrize("grid", [GRIDS[1], GRIDS[3]])
def test_outputs_are_overwritten_completely_and_nothing_else_is_touched(grid):
    """x_out, xin and stats full of NaN come back finite everywhere and right; guard bands of a known pattern around all three stay
    as they were, and the inputs are unchanged."""
    from sta.canvas import guide_windows_reference, window_split_reference
    dtype = torch.bfloat16
    grid = _grid(grid)
    x, gp, keep, step, count = _inputs(grid, dtype, seed=2)
    P, guard = x.shape[0], 4096
    flat_x = torch.full((guard + x.numel() + guard,), 7.0, device="cuda")
    flat_in = torch.full((guard + gp.numel() + guard,), 5.0, device="cuda", dtype=dtype)
    flat_st = torch.full((guard + P + guard,), -3.0, device="cuda")
    x_out = flat_x[guard:guard + x.numel()].view_as(x)
    xin = flat_in[guard:guard + gp.numel()].view_as(gp)
    stats = flat_st[guard:guard + P]
    for t in (x_out, xin, stats):
        t.fill_(float("nan"))
    xd, gd, kd, sd, cd = x.cuda(), gp.cuda(), keep.cuda(), step.cuda(), count.cuda()
    _raw(grid, gd, xd, kd, sd, cd, x_out, xin, stats)
    assert torch.isfinite(x_out).all() and torch.isfinite(xin).all() and torch.isfinite(stats).all()
    assert (flat_x[:guard] == 7.0).all() and (flat_x[guard + x.numel():] == 7.0).all()
    assert (flat_in[:guard] == 5.0).all() and (flat_in[guard + gp.numel():] == 5.0).all()
    assert (flat_st[:guard] == -3.0).all() and (flat_st[guard + P:] == -3.0).all()
    assert torch.equal(xd.cpu(), x) and torch.equal(gd.cpu(), gp) and torch.equal(kd.cpu(), keep) and torch.equal(sd.cpu(), step)
    ref, rms_ref = guide_windows_reference(gp, x.double(), step.double(), count.double(), grid, keep=keep)
    assert ((x_out.cpu().double() - ref).abs() <= 1e-5 * (x.double().abs() + (ref - x.double()).abs())).all()
    assert ((stats.cpu().double() - rms_ref).abs() <= 1e-5 * rms_ref).all()
    assert torch.equal(xin.cpu(), window_split_reference(x_out.cpu(), grid, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("normalize", [True, False])
def test_inert_canvases_stay_bit_equal(dtype, normalize):
    """Canvas 0: a zero gradient; 1: one Inf, in a window that covers the last slice; 2: one NaN in the first window; 3: count == 0;
    4: an ordinary canvas. The first four come back as they went in (signed zeros included), their xin is the split of x, stats tells
    why; the fifth is updated."""
    from sta.canvas import latent_guide_windows, window_split_reference
    grid = _grid(GRIDS[0])
    x, gp, keep, step, count = _inputs(grid, dtype, P=5, seed=3)
    count[:] = float(4 * grid.Hc * grid.Wc)
    rows = 2 * grid.T
    x[0, 0, 0, 0] = -0.0
    gp[0:rows] = 0.0
    gp[2 * rows - 1, 3, 15, 15] = float("inf")
    gp[2 * rows, 0, 0, 0] = float("nan")
    count[3] = 0.0
    out, xin, rms = latent_guide_windows(gp.cuda(), x.cuda(), step.cuda(), count.cuda(), grid, normalize=normalize, inv_scale=4.0, want_xin=True)
    torch.cuda.synchronize()
    out, xin, rms = out.cpu(), xin.cpu(), rms.cpu()
    assert torch.equal(out[:4].view(torch.int32), x[:4].view(torch.int32))
    assert rms[0].item() == 0.0 and not torch.isfinite(rms[1]) and torch.isnan(rms[2]) and not torch.isfinite(rms[3])
    assert torch.isfinite(rms[4]) and rms[4] > 0 and not torch.equal(out[4], x[4]) and torch.isfinite(out).all()
    assert torch.equal(xin, window_split_reference(out, grid, dtype))


# ---------------------------------------------------------------------------------------------------
# the miniature: a 32 x 64 canvas of T = 3 windows of 32 x 32, K = 2, "a cat left of a dog", readouts at 8 x 8, S = 4
# ---------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(dtype, device="cuda"):
    if (dtype, device) not in _MODELS:
        _MODELS[(dtype, device)] = _build_model(dtype, device, vae=False)
    return _MODELS[(dtype, device)]


def _cls(kind):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    return dict(ddim=DDIMSampler, dpm=DPMSolverSampler)[kind]


def _guidance(model, cls="canvas", **kw):
    from sta import guidance
    kw = dict(dict(resolution=RES, scale=0.1, steps=2, iters=1), **kw)
    return (guidance.CanvasGuidance if cls == "canvas" else guidance.AttnGuidance)(model.model.diffusion_model, **kw)


def _start(canvas, device):
    c, local_ctx, xa = gi.unet_inputs(K, 5)
    x_T = xa if canvas == (S_LAT, S_LAT) else torch.cat([xa, gi.unet_inputs(K, 6)[2]], dim=3)
    return c.to(device), [l.to(device) for l in local_ctx], x_T.to(device)


def _canvas(sampler, canvas, centres, device="cuda", mask=None, x0=None):
    c, local_ctx, x_T = _start(canvas, device)
    kw = dict(S=S, canvas=canvas, window=S_LAT, stride=16, conditionings=[c], unconditional_conditionings=gi.load_uncond().to(device),
              bboxs=[centres], object_names=[NAMES], local_conditionings=[local_ctx], curr_texts=[TEXT], x_T=x_T,
              unconditional_guidance_scale=7.5, eta=0.0, seed=1)
    if mask is None:
        sampler.sample_canvas(**kw)
    else:
        sampler.inpaint_canvas(mask=mask.to(device), x0=x0.to(device), **kw)
    if device == "cuda":
        torch.cuda.synchronize()
    return sampler.last_result["x0"].clone()


class _Tap:
    """Records what every latent_guide_windows call of a run was given and returned."""

    def __init__(self, monkeypatch):
        from sta import canvas
        self.calls = []
        real = canvas.latent_guide_windows

        def tapped(g, x, step, count, grid, **kw):
            out = real(g, x, step, count, grid, **kw)
            self.calls.append(dict(g=g.detach().float().cpu(), x=x.detach().cpu(), x_out=out[0].detach().cpu(), count=torch.as_tensor(count).cpu(),
                                   grid=grid, kw=kw))
            return out
        monkeypatch.setattr(canvas, "latent_guide_windows", tapped)


def _canvas_d(call, inv=1.0):
    """The canvas gradient d of a tapped update: the adjoint gather of its window gradient in fp32 on the host, unscaled."""
    from sta.canvas import guide_windows_reference
    zero = torch.zeros_like(call["x"])
    out, _ = guide_windows_reference(call["g"], zero, 1.0, call["count"], call["grid"], normalize=False, inv_scale=1.0)
    return -out * inv


_HOST = {}


def _host_d(monkeypatch):
    """d of the first update on the fp32 host chain (oracle-backed blocks) and the energies of its two evaluations."""
    if "d" not in _HOST:
        from tests.cpu_backend import oracle_ops
        model = _model(torch.float32, "cpu")
        tap = _Tap(monkeypatch)
        sampler = _cls("ddim")(model, loss_model=None, opt_epochs=0, use_graph=False, save_images=False,
                               canvas_guidance=_guidance(model, steps=1, iters=2))
        with oracle_ops():
            _canvas(sampler, STRIP, STRIP_CENTRES, device="cpu")
        e = sampler.last_guidance["energy"]
        _HOST.update(d=_canvas_d(tap.calls[0]), e0=e[0, 0].item(), e1=e[1, 0].item())
    return _HOST


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_reaches_the_canvas_latent(dtype, monkeypatch):
    """d of the first update on the T = 3 strip against the fp32 host chain, with the bounds of the square case
    (tests/test_guidance_gpu.py::test_gradient_reaches_the_latent): max |d - d_ref| / max |d_ref| <= 0.15, sign agreement >= 95 % on the
    entries above 5 % of the largest, the first energy within 1 % of the host chain's. Window 2 holds no disc: its energy is exactly 0
    and the columns only it covers receive no gradient. With iters = 2 the recorded energy falls. Measured on the first run
    (profiles/canvas_guidance.md's machine): 0.017 (bf16) and 0.003 (fp16) of max |d_ref|, sign agreement 100 %, E 0.74703 / 0.74712 against
    the host's 0.74712, falling to 0.70608 / 0.70615 (host 0.70615) — the bounds stand as they are."""
    ref = _host_d(monkeypatch)
    model = _model(dtype)
    tap = _Tap(monkeypatch)
    sampler = _cls("ddim")(model, loss_model=None, opt_epochs=0, use_graph=True, save_images=False,
                           canvas_guidance=_guidance(model, steps=1, iters=2))
    x0 = _canvas(sampler, STRIP, STRIP_CENTRES)
    call, res = tap.calls[0], sampler.last_guidance
    inv = call["kw"]["inv_scale"]
    assert (inv < 1.0) == (dtype == torch.float16) and call["count"].tolist() == [4 * 32 * 48]
    d = _canvas_d(call, inv)
    e_max = ((d - ref["d"]).abs().max() / ref["d"].abs().max()).item()
    strong = ref["d"].abs() > 0.05 * ref["d"].abs().max()
    agree = (torch.sign(d[strong]) == torch.sign(ref["d"][strong])).float().mean().item()
    print("%s: E %s (host %.5f -> %.5f), per window %s, loss scale %g, max |d - d_ref| / max |d_ref| = %.4f, sign agreement %.4f, rms %s"
          % (dtype, res["energy"][:, 0].tolist(), ref["e0"], ref["e1"], res["window_energy"][:, 0].tolist(), 1.0 / inv, e_max, agree,
             res["rms"][:, 0].tolist()))
    assert res["calls"] == [(0, 0), (0, 1)] and res["skipped"] == 0 and res["window_energy"].shape == (2, 1, 3)
    assert torch.isfinite(d).all() and d.abs().max() > 0 and (d[..., 48:] == 0).all()
    assert (res["window_energy"][:, 0, 2] == 0).all() and (res["window_energy"][:, 0, :2] > 0).all()
    assert not torch.equal(call["x_out"], call["x"]) and torch.equal(call["x_out"][..., 48:], call["x"][..., 48:])
    assert abs(res["energy"][0, 0].item() - ref["e0"]) <= 0.01 * ref["e0"]
    assert e_max <= 0.15, e_max
    assert agree >= 0.95, agree
    assert res["energy"][1, 0] < res["energy"][0, 0]
    assert torch.isfinite(x0).all()


@pytest.mark.parametrize("kind,dtype,fused", [("ddim", torch.bfloat16, True), ("dpm", torch.float16, True), ("ddim", torch.float16, False)])
def test_guided_canvas_end_to_end(kind, dtype, fused):
    """steps = 2, iters = 2 (ordinary calls graph-replayed, evaluations eager): x0 is finite and differs from the unguided x0, E falls
    across the first update, nothing stays attached; a guidance that is switched off changes nothing."""
    from ldm.modules.attention import BasicTransformerBlock
    model = _model(dtype)
    mk = lambda cg: _cls(kind)(model, loss_model=None, opt_epochs=0, use_graph=True, save_images=False, canvas_guidance=cg)
    plain = mk(None)
    plain.canvas_fused_step = fused
    x_plain = _canvas(plain, STRIP, STRIP_CENTRES)
    assert plain.last_guidance is None
    sampler = mk(_guidance(model, steps=2, iters=2))
    sampler.canvas_fused_step = fused
    x0 = _canvas(sampler, STRIP, STRIP_CENTRES)
    res = sampler.last_guidance
    e = res["energy"][:, 0].tolist()
    print("%s %s fused=%s: E before the updates %s, rms %s" % (kind, dtype, fused, ["%.5f" % v for v in e], ["%.3e" % v for v in res["rms"][:, 0].tolist()]))
    assert res["calls"] == [(0, 0), (0, 1), (1, 0), (1, 1)] and res["skipped"] == 0
    assert e[1] < e[0]
    assert torch.isfinite(x0).all() and not torch.equal(x0, x_plain)
    assert all(b._attn_loss is None for b in model.modules() if isinstance(b, BasicTransformerBlock))
    off = _guidance(model, steps=0)
    s_off = mk(off)
    s_off.canvas_fused_step = fused
    _canvas(s_off, STRIP, STRIP_CENTRES)
    assert s_off.last_guidance is None and off.loss.block_calls == 0


def _reproducible_unet(model, dtype, monkeypatch):
    """The UNet call replaced by an elementwise stand-in that is bit-reproducible whatever the library does (the stand-in of
    tests/test_canvas_gpu.py::test_canvas_of_one_window_equals_sample_around_a_reproducible_unet); while a guidance evaluates (its loss
    attached, autograd on) the stand-in also hands the loss a differentiable read-out of its input — softplus of the 4 x 4 block means
    of each channel as the R = 4 token maps at 8 x 8 — in place of what the blocks would record."""
    def unet(x_in, text_index, t, c_in, coef=None, bboxs_curr=None):
        b = x_in.shape[0] // 2
        gain = (0.3 + 0.001 * t.float().reshape(2 * b, 1, 1, 1) / 1000 + 0.01 * c_in.float().mean(dim=(1, 2)).reshape(2 * b, 1, 1, 1)
                + 0.02 * coef.float().reshape(b, -1).sum(1).repeat_interleave(2).reshape(2 * b, 1, 1, 1))
        h = x_in.to(dtype).float()
        for blk in model.model.diffusion_model.modules():
            loss = getattr(blk, "_attn_loss", None)
            if loss is not None and loss.recording and torch.is_grad_enabled():
                side = h.shape[-1] // RES
                pooled = (h[0::2] + 0.5 * h[1::2]).reshape(b, 4, RES, side, RES, side).mean(dim=(3, 5))
                loss._disc, loss._valid = loss._disc.to(h.device), loss._valid.to(h.device)
                loss._sum, loss._nblk = torch.nn.functional.softplus(pooled).reshape(b, 4, RES * RES)[:, :len(loss.sel_ctx)], 1
                break
        return (torch.tanh(h * gain) + 0.1 * h.roll(1, dims=-1)).to(dtype).to(x_in.dtype)
    monkeypatch.setattr(model, "apply_model_extra", unet, raising=False)


@pytest.mark.parametrize("kind,dtype", [("ddim", torch.float16), ("dpm", torch.bfloat16)])
def test_canvas_of_one_window_equals_guided_sample(kind, dtype, monkeypatch):
    """Canvas 32 x 32 (one window) with a CanvasGuidance against `sample` with an AttnGuidance, torch.equal, around a reproducible UNet:
    the library's convolutions are not bit-reproducible between two identical calls (tests/test_canvas_gpu.py), and the eager evaluation
    under autograd cannot ask them to be (MIOpen has no deterministic algorithm for the tracked trunk's strided 1 x 1 convolutions in
    16 bits: 'No suitable algorithm was found'), so the UNet is a stand-in and everything of this feature around it — the per-window
    loss, the loss scale, the update launch against sta_latent_guide, the window inputs it writes, the steps that follow — has to
    reproduce the square path bit for bit."""
    model = _model(dtype)
    _reproducible_unet(model, dtype, monkeypatch)
    kw = dict(loss_model=None, opt_epochs=0, use_graph=False, save_images=False)
    on_canvas = _cls(kind)(model, canvas_guidance=_guidance(model), **kw)
    got = _canvas(on_canvas, (S_LAT, S_LAT), CENTRES)
    square = _cls(kind)(model, latent_guidance=_guidance(model, "square"), **kw)
    c, local_ctx, x_T = _start((S_LAT, S_LAT), "cuda")
    square.sample(S=S, conditioning=c, batch_size=1, shape=[4, S_LAT, S_LAT], verbose=False, unconditional_guidance_scale=7.5,
                  unconditional_conditioning=gi.load_uncond().cuda(), eta=0.0, x_T=x_T, text_index=0, curr_text=TEXT, bboxs_curr=CENTRES, seed=1,
                  prompt_idx=0, object_names=NAMES, local_conditionings=local_ctx)
    torch.cuda.synchronize()
    want = square.last_result["x0"]
    a, b = on_canvas.last_guidance, square.last_guidance
    print("%s %s: E canvas %s, square %s, rms %s; max |x0 - x0'| / max = %.3g"
          % (kind, dtype, a["energy"][:, 0].tolist(), b["energy"][:, 0].tolist(), a["rms"][:, 0].tolist(), ((got - want).abs().max() / want.abs().max()).item()))
    assert a["calls"] == b["calls"] == [(0, 0), (1, 0)] and a["skipped"] == 0 and (a["energy"] > 0).all()
    assert torch.equal(a["energy"], b["energy"]) and torch.equal(a["rms"], b["rms"])
    assert torch.isfinite(got).all() and torch.equal(got, want)
    plain = _cls(kind)(model, **kw)
    assert not torch.equal(_canvas(plain, (S_LAT, S_LAT), CENTRES), got)


def test_guided_inpaint_canvas_leaves_the_kept_region_to_the_blend(monkeypatch):
    """inpaint_canvas with the same blend draws, guided and unguided: the state that enters every guided call equals the unguided run's
    where keep == 1, bit for bit (the blend wrote it, the guidance did not touch it), and differs elsewhere."""
    from sta import canvas
    from tests.test_canvas_inpaint_cpu import _draws, keep_mask
    model = _model(torch.bfloat16)
    keep = keep_mask(1, *STRIP)
    z0 = torch.randn((1, 4) + STRIP, generator=torch.Generator().manual_seed(9))
    mk = lambda cg: _cls("ddim")(model, loss_model=None, opt_epochs=0, use_graph=True, save_images=False,
                                 mask_noise=[t.cuda() for t in _draws(S, 7, (1, 4) + STRIP)], canvas_guidance=cg)
    states = []
    for name in ("window_blend", "sampler_step_windows_masked"):               # the blended state that enters call 0, then calls 1 ..
        real = getattr(canvas, name)
        monkeypatch.setattr(canvas, name, lambda *a, _real=real, **k: (lambda out: (states.append(out[0].detach().cpu()), out)[1])(_real(*a, **k)))
    x_plain = _canvas(mk(None), STRIP, STRIP_CENTRES, mask=keep, x0=z0)
    plain_states, states[:] = list(states), []
    tap = _Tap(monkeypatch)
    sampler = mk(_guidance(model, steps=2))
    x0 = _canvas(sampler, STRIP, STRIP_CENTRES, mask=keep, x0=z0)
    assert len(tap.calls) == 2 and sampler.last_guidance["calls"] == [(0, 0), (1, 0)] and torch.isfinite(x0).all() and not torch.equal(x0, x_plain)
    kept = (keep == 1.0).expand(1, 4, *STRIP)
    for i, call in enumerate(tap.calls):
        assert call["kw"]["keep"] is not None
        assert torch.equal(call["x_out"][kept].view(torch.int32), plain_states[i][kept].view(torch.int32))
        assert torch.equal(call["x_out"][kept].view(torch.int32), call["x"][kept].view(torch.int32))
        assert (call["x_out"] - call["x"])[~kept].abs().max() > 0
