"""Attention guidance on canvases without a GPU: guide_windows_reference against the adjoint of the split (autograd, float64), the one
window identity with guide_reference, `count` by hand, the contributing table, the refusals of sta_latent_guide_windows at every `wrap`
(fake pointers: none of these calls may reach a launch), CanvasGuidance on the host miniature of tests/test_canvas_cpu.py for
the three samplers, the off states and the CLI. The kernel is checked in test_canvas_guidance_gpu.py."""
import ctypes
import os
import sys

import pytest
import torch

from oracle import golden_inputs as gi
from tests.cpu_backend import oracle_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STA_E_ARG, STA_E_UNSUP = -1, -2
PTR = 0x10000                                          # a fake device pointer: non-null, 16-byte aligned, never read
S_LAT, STEPS, K, RES = 32, 4, 2, 8
TEXT, NAMES = "a cat left of a dog", ["cat", "dog"]
CENTRES = [[0.3, 0.4], [0.7, 0.6]]                     # one window: tests/test_guidance_cpu.py's layout
STRIP = (S_LAT, 2 * S_LAT)                             # stride 16: T = 3 windows at x = 0, 16, 32
# both discs (radius 0.2 x 32 = 6.4 latent pixels) lie left of x = 32: inside windows 0 and 1, outside window 2
STRIP_CENTRES = [[20.0 / 64.0, 0.4], [24.0 / 64.0, 0.6]]


def _grid(Hc, Wc, s, stride, wrap=""):
    from sta.canvas import window_grid
    return window_grid(Hc, Wc, s, stride, wrap)


# ---------------------------------------------------------------------------------------------------
# guide_windows_reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(24, 40, 16, 8, ""), (16, 48, 16, 8, "x"), (32, 32, 16, 8, "xy"), (24, 40, 16, 8, "x")])
@pytest.mark.parametrize("masked", [False, True])
def test_restatement_is_the_adjoint_of_the_split(args, masked):
    """d/dx of <window_split(x), g> is the gathered sum d: with normalize off, step 1 and inv_scale 1 the restatement returns x - d
    (1 - keep), and rms = sqrt(sum d^2 / count) — float64, 1e-12."""
    from sta.canvas import guide_windows_reference, window_split_reference
    grid = _grid(*args)
    if args[:4] == (24, 40, 16, 8) and not args[4]:
        assert grid.T == 8
    gen = torch.Generator().manual_seed(grid.T)
    P, C = 2, 4
    x = torch.randn(P, C, grid.Hc, grid.Wc, generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn(2 * P * grid.T, C, grid.s, grid.s, generator=gen, dtype=torch.float64)
    keep = (torch.rand(P, 1, grid.Hc, grid.Wc, generator=gen) > 0.5).double() if masked else None
    if masked:
        keep[:, :, 0, :3] = 0.25
    (adj,) = torch.autograd.grad((window_split_reference(x, grid, rows=1) * g).sum(), x)
    d = adj * (1.0 - keep) if masked else adj
    count = torch.tensor([C * grid.Hc * grid.Wc, 100.0], dtype=torch.float64)
    out, rms = guide_windows_reference(g, x.detach(), 1.0, count, grid, keep=keep, normalize=False, inv_scale=1.0)
    assert torch.allclose(x.detach() - out, d, rtol=0, atol=1e-12)
    assert torch.allclose(rms, (d.reshape(P, -1).square().sum(1) / count).sqrt(), rtol=1e-12, atol=0)
    step = torch.tensor([0.3, 0.7], dtype=torch.float64)
    out, _ = guide_windows_reference(g, x.detach(), step, count, grid, keep=keep)
    assert torch.allclose(out, x.detach() - (step / rms).reshape(P, 1, 1, 1) * d, rtol=0, atol=1e-12)
    if masked:
        kept = (keep == 1.0).expand_as(out)
        assert torch.equal(out[kept], x.detach()[kept])


@pytest.mark.parametrize("normalize", [True, False])
def test_one_window_is_guide_reference(normalize):
    from sta.canvas import guide_windows_reference
    from sta.guidance import guide_reference
    grid = _grid(16, 16, 16, 8)
    assert grid.T == 1
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(3, 4, 16, 16, generator=gen)
    g = torch.randn(6, 4, 16, 16, generator=gen) * 3e-3
    g[2:4] = 0.0                                                                # canvas 1: skipped
    keep = (torch.rand(3, 1, 16, 16, generator=gen) > 0.6).float()
    step = torch.tensor([0.3, 0.7, 0.1])
    for kp in (None, keep):
        want, want_rms = guide_reference(g, x, step, keep=kp, normalize=normalize, inv_scale=0.25)
        got, rms = guide_windows_reference(g, x, step, 4 * 16 * 16, grid, keep=kp, normalize=normalize, inv_scale=0.25)
        assert torch.equal(got, want) and torch.equal(rms, want_rms)
        assert torch.equal(got[1], x[1]) and not torch.equal(got[0], x[0])


def test_count_by_hand_and_count_zero():
    from sta.canvas import guide_count, guide_windows_reference, latent_guide_windows
    tiles = _grid(16, 48, 16, 16)                                               # T = 3, no overlap
    assert guide_count(tiles, [[True, False, True], [True, True, True], [False, False, False]], 4).tolist() == [4 * 16 * 32, 4 * 16 * 48, 0]
    lap = _grid(16, 32, 16, 8)                                                  # T = 3 at x = 0, 8, 16
    assert guide_count(lap, [[True, False, False], [True, True, False], [False, True, False], [True, False, True]], 2).tolist() == \
        [2 * 16 * 16, 2 * 16 * 24, 2 * 16 * 16, 2 * 16 * 32]
    ring = _grid(16, 48, 16, 8, "x")                                            # T = 6; window 5 covers columns 40 .. 47 and 0 .. 7
    assert guide_count(ring, [[False] * 5 + [True]], 4).tolist() == [4 * 16 * 16]
    # count == 0: the canvas is returned as it is, whatever the gradient holds; the other canvas moves
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 16, 32, generator=gen)
    g = torch.randn(2 * 2 * 3, 4, 16, 16, generator=gen)
    for gz in (g, torch.cat([torch.zeros_like(g[:6]), g[6:]])):
        out, rms = guide_windows_reference(gz, x, 0.5, torch.tensor([0.0, 4 * 16 * 32.0]), lap)
        assert torch.equal(out[0], x[0]) and not torch.isfinite(rms[0]) and not torch.equal(out[1], x[1]) and rms[1] > 0
    out, xin, rms = latent_guide_windows(g, x, 0.5, torch.tensor([0.0, 4 * 16 * 32.0]), lap, dtype=torch.bfloat16, want_xin=True)
    from sta.canvas import window_split_reference
    assert torch.equal(out[0], x[0]) and torch.equal(xin, window_split_reference(out, lap, torch.bfloat16)) and xin.dtype == torch.bfloat16
    # a normalised step moves the part that receives gradient by `step` in rms
    moved = (out[1] - x[1]).square().sum().div(4 * 16 * 32).sqrt().item()
    assert abs(moved - 0.5) < 1e-5


# ---------------------------------------------------------------------------------------------------
# the contributing table
# ---------------------------------------------------------------------------------------------------
def _unet():
    from tests.test_canvas_cpu import _sampler
    return _sampler("ddim").model.model.diffusion_model


def test_contributing_table_and_the_disc_keyword():
    from sta.attnloss import AttnLayoutLoss, layout_energy
    from sta.canvas import window_centres
    from sta.guidance import CanvasGuidance
    grid = _grid(*STRIP, S_LAT, 16)
    assert grid.T == 3
    per_window = window_centres(STRIP_CENTRES, grid)
    loss = AttnLayoutLoss(_unet(), resolution=RES)
    loss.begin(per_window, texts=[TEXT] * 3, names=[NAMES] * 3)                 # the default: today's rule, the disc is not looked at
    assert loss._valid.all() and loss._disc[2].sum() == 0
    loss.begin(per_window, texts=[TEXT] * 3, names=[NAMES] * 3, disc_required=True)
    assert loss._valid[:2].all() and not loss._valid[2].any() and (loss._disc[:2].sum(-1) > 0).all()
    maps = torch.rand(3, loss._valid.shape[1], RES * RES, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    e = layout_energy(maps, loss._disc, loss._valid)
    assert e[2].item() == 0.0 and (e[:2] > 0).all()
    (gm,) = torch.autograd.grad(e.sum(), maps)
    assert (gm[2] == 0).all() and gm[:2].abs().max() > 0
    cg = CanvasGuidance(_unet(), resolution=RES, scale=0.1, steps=1).begin([STRIP_CENTRES, CENTRES], texts=[TEXT] * 2, names=[NAMES] * 2, grid=grid)
    assert cg.ready and cg.contributing.tolist() == [[True, True, False], [True, True, True]]
    assert cg._count(4, torch.device("cpu")).tolist() == [4 * 32 * 48, 4 * 32 * 64]
    assert not CanvasGuidance(_unet(), resolution=RES, scale=0.1, steps=1).begin([[]], texts=["a landscape"], names=[[]], grid=grid).ready
    with pytest.raises(ValueError, match="grid="):
        CanvasGuidance(_unet(), resolution=RES).begin([STRIP_CENTRES], texts=[TEXT], names=[NAMES])
    with pytest.raises(ValueError, match="no level of side 12"):
        CanvasGuidance(_unet(), resolution=12).begin([STRIP_CENTRES], texts=[TEXT], names=[NAMES], grid=grid)
    with pytest.raises(RuntimeError, match="bind"):
        cg.update(torch.zeros(2, 4, *STRIP), None, None, None, 0, 0.5)


# ---------------------------------------------------------------------------------------------------
# C-ABI
# ---------------------------------------------------------------------------------------------------
def _ints(v):
    a = (ctypes.c_int * len(v))(*v)
    return a, ctypes.addressof(a)


def _call(L, **kw):
    """P = 1, C = 4, canvas 16 x 40, windows of 16 at x = 0, 16, 24: g / xin 6 x 4 x 16 x 16 x 2 = 0x3000 bytes, x / x_out 0x2800."""
    a = dict(g=PTR, x=PTR + 0x10000, keep=PTR + 0x20000, step=PTR + 0x30000, count=PTR + 0x31000, x_out=PTR + 0x40000, xin=PTR + 0x50000,
             stats=PTR + 0x60000, P=1, C=4, Hc=16, Wc=40, oy=(0,), ox=(0, 16, 24), s=16, wrap=0, normalize=1, inv_scale=1.0, dtype=0)
    a.update(kw)
    keep_y, oy = _ints(a["oy"]) if a["oy"] is not None else (None, 0)
    keep_x, ox = _ints(a["ox"]) if a["ox"] is not None else (None, 0)
    ny, nx = a.get("ny", len(a["oy"] or ())), a.get("nx", len(a["ox"] or ()))
    head = (a["g"], a["x"], a["keep"], a["step"], a["count"], a["x_out"], a["xin"], a["stats"], a["P"], a["C"], a["Hc"], a["Wc"], ny, nx, oy, ox,
            a["s"], a["wrap"])
    rc = L.sta_latent_guide_windows(*head, a["normalize"], a["inv_scale"], a["dtype"], None)
    return rc, L.sta_last_error().decode()


def test_abi_symbols_and_refusals_reach_no_launch():
    from sta import lib
    L = lib.load()
    vp, i, f, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    assert lib.SYMBOLS["sta_latent_guide_windows"] == (i, [vp] * 8 + [l, i, i, i, i, i, vp, vp, i, i, i, f, i, vp])
    assert "sta_latent_guide_windows_ring" not in lib.SYMBOLS and not hasattr(L, "sta_latent_guide_windows_ring")
    header = " ".join(open(os.path.join(ROOT, "include", "sta_unet.h")).read().split())
    assert ("int sta_latent_guide_windows(const void* g, const float* x, const float* keep, const float* step, const float* count, "
            "float* x_out, void* xin, float* stats, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, "
            "int wrap, int normalize, float inv_scale, int dtype, void* stream);") in header
    assert "sta_latent_guide_windows_ring" not in header
    assert "latent_guide_windows_kernel" in lib.NO_SPILL_KERNELS["sta_sampler.hip"]      # the by-value offset tables may not go to scratch
    assert "latent_guide_windows_kernel" in open(os.path.join(lib.CSRC, "sta_window.hip")).read()
    cases = [
        (dict(g=0), "null pointer"), (dict(x=0), "null pointer"), (dict(step=0), "null pointer"), (dict(count=0), "null pointer"),
        (dict(x_out=0), "null pointer"), (dict(oy=None), "null pointer"), (dict(ox=None), "null pointer"),
        (dict(g=PTR + 8), "16-byte aligned"), (dict(x=PTR + 0x10004), "16-byte aligned"), (dict(keep=PTR + 0x20008), "16-byte aligned"),
        (dict(x_out=PTR + 0x40008), "16-byte aligned"), (dict(xin=PTR + 0x50002), "16-byte aligned"), (dict(step=PTR + 0x30002), "16-byte aligned"),
        (dict(count=PTR + 0x31001), "16-byte aligned"), (dict(stats=PTR + 0x60002), "16-byte aligned"),
        (dict(x_out=PTR + 0x10000), "aliases an input"),                       # x_out == x
        (dict(xin=PTR), "aliases an input"),                                   # xin == g
        (dict(x_out=PTR + 0x10000 + 0x2780), "aliases an input"),              # overlaps the tail of x (0x2800 bytes)
        (dict(xin=PTR + 0x2ff0), "aliases an input"),                          # overlaps the tail of g (0x3000 bytes)
        (dict(stats=PTR + 0x31000), "aliases an input"),                       # stats == count
        (dict(stats=PTR + 0x40000), "alias each other"),
        (dict(xin=PTR + 0x40000 + 0x27f0), "alias each other"),
        (dict(P=0), "P=0"), (dict(C=0), "C=0"), (dict(Wc=44), "Wc=44"), (dict(Hc=20), "Hc=20"), (dict(s=12), "s=12"), (dict(Hc=8), "Hc=8"),
        (dict(ox=(0, 12, 24)), "ox[1]=12 is not a multiple of 8"), (dict(ox=(0, 16, 32)), "ox[2]=32 out of range"),
        (dict(ox=(8, 16, 24)), "ox[0]=8 unsorted"), (dict(ox=(0, 24)), "gap between ox[0]=0 and ox[1]=24"),
        (dict(ox=(0, 16)), "gap behind ox[1]=16"), (dict(oy=(), ny=0), "ny=0"),
        (dict(ox=tuple(range(0, 136, 8)), Wc=16 + 8 * 16), "nx=17"),
        (dict(dtype=7), "dtype 7"), (dict(dtype=2), "dtype 2"),
    ]
    for kw, text in cases:                                                      # wrap = 0: the rules of the clamped grid
        rc, err = _call(L, **kw)
        assert rc == STA_E_ARG and text in err, (kw, rc, err)
    for wrap, ring in ((0, {}), (1, dict(Wc=48, ox=(0, 16, 32))), (3, dict(Wc=48, ox=(0, 16, 32), Hc=32, oy=(0, 16)))):
        assert _call(L, wrap=wrap, dtype=7, **ring)[1].startswith("latent_guide_windows: dtype 7")       # one name whatever the wrap
        assert _call(L, wrap=wrap, dtype=7, keep=0, xin=0, stats=0, **ring)[0] == STA_E_ARG      # the optional pointers may be NULL: the dtype is refused
    ring_cases = [
        (dict(wrap=4), "wrap=4"), (dict(wrap=-1), "wrap=-1"),
        (dict(wrap=1, Wc=48, ox=(0, 16)), "the ring does not close behind ox[1]=16"),
        (dict(wrap=1, Wc=48, ox=(0, 16, 48)), "ox[2]=48 is not on the wrapped axis"),
        (dict(wrap=2, ox=(0, 16, 24), oy=(0, 8), Hc=32), "the ring does not close behind oy[1]=8"),
        (dict(wrap=1, Wc=48, ox=(0, 16, 32), x_out=PTR + 0x10000), "aliases an input"),
    ]
    for kw, text in ring_cases:
        rc, err = _call(L, **kw)
        assert rc == STA_E_ARG and text in err and err.startswith("latent_guide_windows: "), (kw, rc, err)


# ---------------------------------------------------------------------------------------------------
# samplers on the host miniature
# ---------------------------------------------------------------------------------------------------
KINDS = ["plms", "ddim", "dpm"]


def _guidance(cls="canvas", **kw):
    from sta import guidance
    kw = dict(dict(resolution=RES, scale=0.1, steps=2, iters=1), **kw)
    return (guidance.CanvasGuidance if cls == "canvas" else guidance.AttnGuidance)(_unet(), **kw)


def _canvas_inputs(canvas):
    c, local_ctx, xa = gi.unet_inputs(K, 5)
    x_T = xa if canvas == (S_LAT, S_LAT) else torch.cat([xa, gi.unet_inputs(K, 6)[2]], dim=3)
    return c, local_ctx, x_T


def _canvas(sampler, canvas, centres, **kw):
    c, local_ctx, x_T = _canvas_inputs(canvas)
    with oracle_ops():
        sampler.sample_canvas(**dict(dict(S=STEPS, canvas=canvas, window=S_LAT, stride=16, conditionings=[c],
                                          unconditional_conditionings=gi.load_uncond(), bboxs=[centres], object_names=[NAMES],
                                          local_conditionings=[local_ctx], curr_texts=[TEXT], x_T=x_T, unconditional_guidance_scale=7.5,
                                          eta=0.0, seed=1), **kw))
    return sampler.last_result["x0"].clone()


def _sample(sampler):
    c, local_ctx, x_T = _canvas_inputs((S_LAT, S_LAT))
    with oracle_ops():
        sampler.sample(S=STEPS, conditioning=c, batch_size=1, shape=[4, S_LAT, S_LAT], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond(), eta=0.0, x_T=x_T, text_index=0, curr_text=TEXT, bboxs_curr=CENTRES, seed=1,
                       prompt_idx=0, object_names=NAMES, local_conditionings=local_ctx)
    return sampler.last_result["x0"].clone()


_PLAIN = {}


def _plain_strip():
    from tests.test_canvas_cpu import _sampler
    if "strip" not in _PLAIN:
        _PLAIN["strip"] = _canvas(_sampler("ddim"), STRIP, STRIP_CENTRES)
    return _PLAIN["strip"]


def test_guided_strip_lowers_the_energy_and_a_window_without_discs_contributes_nothing():
    """T = 3 strip, DDIM, steps = 1, iters = 2: E before update 2 is E after update 1 and lies below E before update 1; window 2 holds no
    disc, its energy is exactly 0 in both evaluations and the canvas energy is the mean over the two contributing windows."""
    from ldm.modules.attention import BasicTransformerBlock
    from tests.test_canvas_cpu import _sampler
    sampler = _sampler("ddim", canvas_guidance=_guidance(steps=1, iters=2))
    x0 = _canvas(sampler, STRIP, STRIP_CENTRES)
    res = sampler.last_guidance
    assert res["calls"] == [(0, 0), (0, 1)] and res["skipped"] == 0
    assert res["energy"].shape == (2, 1) and res["window_energy"].shape == (2, 1, 3) and res["rms"].shape == (2, 1)
    print("E %s, per window %s, rms %s" % (res["energy"][:, 0].tolist(), res["window_energy"][:, 0].tolist(), res["rms"][:, 0].tolist()))
    assert (res["window_energy"][:, 0, 2] == 0).all() and (res["window_energy"][:, 0, :2] > 0).all()
    assert torch.allclose(res["energy"][:, 0], res["window_energy"][:, 0, :2].sum(-1) / 2, rtol=1e-6)
    assert torch.isfinite(res["rms"]).all() and (res["rms"] > 0).all()
    assert res["energy"][1, 0] < res["energy"][0, 0]
    assert torch.isfinite(x0).all() and not torch.equal(x0, _plain_strip())
    assert all(b._attn_loss is None for b in sampler.model.modules() if isinstance(b, BasicTransformerBlock))
    assert sampler._canvas is None


@pytest.mark.parametrize("kind", KINDS)
def test_canvas_of_one_window_equals_guided_sample(kind):
    from tests.test_canvas_cpu import _sampler
    on_canvas = _sampler(kind, canvas_guidance=_guidance())
    got = _canvas(on_canvas, (S_LAT, S_LAT), CENTRES)
    square = _sampler(kind, latent_guidance=_guidance("square"))
    want = _sample(square)
    a, b = on_canvas.last_guidance, square.last_guidance
    assert a["calls"] == b["calls"] == [(0, 0), (1, 0)]
    assert torch.equal(a["energy"], b["energy"]) and torch.equal(a["rms"], b["rms"]) and torch.equal(a["window_energy"][:, :, 0], b["energy"])
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, _sample(_sampler(kind)))


def test_sample_and_sample_batch_never_look_at_canvas_guidance(monkeypatch):
    from sta import guidance
    from tests.test_canvas_cpu import _sampler
    monkeypatch.setattr(guidance.CanvasGuidance, "begin", lambda *a, **k: pytest.fail("CanvasGuidance.begin was called"))
    plain, with_cg = _sampler("ddim"), _sampler("ddim", canvas_guidance=_guidance())
    assert plain.canvas_guidance is None
    assert torch.equal(_sample(plain), _sample(with_cg)) and with_cg.last_guidance is None

    def batch(sampler):
        c, local_ctx, x_T = _canvas_inputs((S_LAT, S_LAT))
        with oracle_ops():
            sampler.sample_batch(S=STEPS, shape=[4, S_LAT, S_LAT], conditionings=[c, c], unconditional_conditionings=gi.load_uncond(),
                                 bboxs=[CENTRES, CENTRES], object_names=[NAMES] * 2, local_conditionings=[local_ctx, local_ctx],
                                 curr_texts=[TEXT] * 2, x_T=torch.cat([x_T, x_T]), unconditional_guidance_scale=7.5, eta=0.0, seed=1)
        return sampler.last_result["x0"].clone()
    assert torch.equal(batch(plain), batch(with_cg)) and with_cg.last_guidance is None


def test_off_states_are_bit_identical_and_latent_guidance_stays_refused(monkeypatch):
    from sta import canvas
    from tests.test_canvas_cpu import _sampler
    calls = []
    real = canvas.latent_guide_windows
    monkeypatch.setattr(canvas, "latent_guide_windows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    plain = _plain_strip()
    for kw in (dict(scale=0.0, steps=3), dict(scale=0.1, steps=0)):
        cg = _guidance(**kw)
        off = _sampler("ddim", canvas_guidance=cg)
        assert torch.equal(_canvas(off, STRIP, STRIP_CENTRES), plain) and off.last_guidance is None and cg.loss.block_calls == 0
    # canvases without objects are not guided
    c, local_ctx, x_T = _canvas_inputs(STRIP)
    none = dict(bboxs=[[]], object_names=[[]], local_conditionings=[[]], curr_texts=["a landscape"])
    cg = _guidance()
    a = _canvas(_sampler("ddim"), STRIP, [], **none)
    b_s = _sampler("ddim", canvas_guidance=cg)
    assert torch.equal(_canvas(b_s, STRIP, [], **none), a) and b_s.last_guidance is None and cg.loss.block_calls == 0
    assert not calls
    # an attached latent_guidance is refused on a canvas as before, with or without a canvas_guidance beside it
    for extra in ({}, dict(canvas_guidance=_guidance())):
        for kind in KINDS:
            with pytest.raises(ValueError, match="an attached latent_guidance reads one square image's attention maps"):
                _canvas(_sampler(kind, latent_guidance=_guidance("square"), **extra), STRIP, STRIP_CENTRES)
    assert not calls


@pytest.mark.parametrize("fused", [True, False])
def test_masked_canvas_does_not_guide_the_kept_region(fused, monkeypatch):
    """inpaint_canvas with a CanvasGuidance: every update gets keep, leaves x where keep == 1 bit for bit and moves the rest; the
    unfused step path (canvas_fused_step = False) is guided the same way."""
    from sta import canvas
    from tests.test_canvas_cpu import _sampler
    from tests.test_canvas_inpaint_cpu import _draws, keep_mask
    seen = []
    real = canvas.latent_guide_windows

    def tapped(g, x, step, count, grid, **kw):
        out = real(g, x, step, count, grid, **kw)
        seen.append(dict(x=x.clone(), x_out=out[0].clone(), xin=out[1], keep=kw.get("keep"), grid=grid))
        return out
    monkeypatch.setattr(canvas, "latent_guide_windows", tapped)
    keep = keep_mask(1, *STRIP)
    c, local_ctx, x_T = _canvas_inputs(STRIP)
    sampler = _sampler("ddim", mask_noise=_draws(STEPS, 7, (1, 4) + STRIP), canvas_guidance=_guidance(steps=2))
    sampler.canvas_fused_step = fused
    with oracle_ops():
        sampler.inpaint_canvas(S=STEPS, canvas=STRIP, window=S_LAT, stride=16, mask=keep, x0=gi.unet_inputs(K, 7)[2].repeat(1, 1, 1, 2),
                               conditionings=[c], unconditional_conditionings=gi.load_uncond(), bboxs=[STRIP_CENTRES], object_names=[NAMES],
                               local_conditionings=[local_ctx], curr_texts=[TEXT], x_T=x_T, unconditional_guidance_scale=7.5, eta=0.0, seed=1)
    assert len(seen) == 2 and sampler.last_guidance["calls"] == [(0, 0), (1, 0)] and torch.isfinite(sampler.last_result["x0"]).all()
    kept = (keep == 1.0).expand(1, 4, *STRIP)
    for call in seen:
        assert call["keep"] is not None and torch.equal(call["keep"], keep)
        assert torch.equal(call["x_out"][kept], call["x"][kept]) and (call["x_out"] - call["x"])[~kept].abs().max() > 0
        assert torch.equal(call["xin"], canvas.window_split_reference(call["x_out"], call["grid"], call["xin"].dtype))


def test_decode_canvas_is_guided_from_its_first_call():
    """img2img on a canvas (DDIMSampler.decode_canvas from call 2 of 4): the guided calls are counted from the start of the decode."""
    from tests.test_canvas_cpu import _sampler
    c, local_ctx, x_T = _canvas_inputs(STRIP)
    sampler = _sampler("ddim", canvas_guidance=_guidance(steps=1))
    sampler.make_schedule(STEPS, ddim_eta=0.0, verbose=False)
    with oracle_ops():
        sampler.decode_canvas(x_T, STRIP, S_LAT, 16, t_start=2, conditionings=[c], unconditional_conditionings=gi.load_uncond(),
                              bboxs=[STRIP_CENTRES], object_names=[NAMES], local_conditionings=[local_ctx], curr_texts=[TEXT],
                              unconditional_guidance_scale=7.5, seed=1)
    assert sampler.last_guidance["calls"] == [(0, 0)] and sampler.last_guidance["skipped"] == 0 and sampler._start == 0


# ---------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------
def test_cli_canvas_guidance_parses_and_refuses(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts"))
    import _txt2img_common as cli
    import sta.pipeline
    monkeypatch.setattr(sta.pipeline, "build_sd_v1", lambda *a, **k: pytest.fail("a model was built"))
    p = cli.build_parser("x.json")
    assert p.parse_args(["--opt_epochs", "0"]).canvas_guidance is None
    opt = p.parse_args(["--opt_epochs", "0", "--canvas", "512x2048", "--canvas_guidance", "0.2", "--attn_guidance_steps", "5",
                        "--attn_guidance_iters", "2", "--attn_res", "32"])
    assert opt.canvas_guidance == 0.2 and opt.attn_guidance is None and opt.attn_guidance_steps == 5 and opt.attn_guidance_iters == 2
    cli.check_options(opt)
    assert cli.canvas_grid(opt).T == 7
    cli.check_options(p.parse_args(["--opt_epochs", "0", "--canvas", "512x2048", "--canvas_wrap", "x", "--canvas_guidance", "0.2", "--dpm_solver"]))
    for bad in (["--canvas_guidance", "0"], ["--canvas_guidance", "-1"], ["--canvas_guidance", "nan"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit, match="--canvas_guidance 0.2 needs --canvas"):
        cli.check_options(p.parse_args(["--opt_epochs", "0", "--canvas_guidance", "0.2"]))
    with pytest.raises(SystemExit, match="--attn_res 64: no transformer level of a 256 x 256 window"):
        cli.check_options(p.parse_args(["--opt_epochs", "0", "--canvas", "256x512", "--H", "256", "--W", "256", "--canvas_guidance", "0.2",
                                        "--attn_res", "64"]))
    # the refused combination stays refused, with its message
    with pytest.raises(SystemExit, match="--attn_guidance reads one square image's attention maps and is not defined on a --canvas"):
        cli.check_options(p.parse_args(["--opt_epochs", "0", "--canvas", "512x2048", "--attn_guidance", "0.1"]))
    with pytest.raises(SystemExit, match="--attn_guidance reads one square image's attention maps and is not defined on a --canvas"):
        cli.check_options(p.parse_args(["--opt_epochs", "0", "--canvas", "512x2048", "--attn_guidance", "0.1", "--canvas_guidance", "0.2"]))
    with pytest.raises(SystemExit, match="--opt_epochs 3"):
        cli.check_options(p.parse_args(["--opt_epochs", "3", "--canvas", "512x2048", "--canvas_guidance", "0.2", "--clip", "synthetic"]))
    import img2img
    import inpaint
    import outpaint
    q = img2img.build_parser(canvas=True)
    o = q.parse_args(["--init-img", "x.png", "--opt_epochs", "0", "--canvas", "1024x1024", "--canvas_guidance", "0.3", "--attn_res", "8"])
    assert o.canvas_guidance == 0.3 and img2img.canvas_grid(o).T == 9
    with pytest.raises(SystemExit, match="needs --canvas"):
        img2img.canvas_grid(q.parse_args(["--init-img", "x.png", "--opt_epochs", "0", "--canvas_guidance", "0.3"]))
    with pytest.raises(SystemExit, match="--attn_res 64: no transformer level of a 256 x 256 window"):
        img2img.canvas_grid(q.parse_args(["--init-img", "x.png", "--opt_epochs", "0", "--canvas", "512x512", "--window", "256", "--canvas_guidance", "0.3",
                                          "--attn_res", "64"]))
    with pytest.raises(SystemExit, match="--attn_guidance"):
        img2img.canvas_grid(q.parse_args(["--init-img", "x.png", "--opt_epochs", "0", "--canvas", "1024x1024", "--attn_guidance", "0.3"]))
    q = outpaint.build_parser()
    o = q.parse_args(["--init-img", "x.png", "--canvas", "512x1024", "--place", "512,0", "--canvas_guidance", "0.3"])
    grid, place = outpaint.check_options(o)
    assert o.canvas_guidance == 0.3 and grid.T == 3 and place == (512, 0)
    with pytest.raises(SystemExit, match="--attn_guidance"):
        outpaint.check_options(q.parse_args(["--init-img", "x.png", "--canvas", "512x1024", "--attn_guidance", "0.3"]))
    q = inpaint.build_parser()
    with pytest.raises(SystemExit, match="--canvas_guidance 0.3 needs --canvas"):
        inpaint.check_options(q.parse_args(["--init-img", "x.png", "--mask_from_layout", "0.2", "--layout", "l.json", "--canvas_guidance", "0.3"]))
