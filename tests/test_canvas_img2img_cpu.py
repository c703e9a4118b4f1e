"""img2img on canvases without a GPU: the two C entry points of the fused entry launch (symbols; argument rules with fake pointers: none
of these calls may reach a launch), the torch restatement `encode_step_windows_reference` against a float64 restatement,
`DDIMSampler.decode_canvas` / `encode_step_canvas` on the host miniature (oracle-backed blocks, golden-width UNet, fp32), the refusals
and the CLI of scripts/img2img.py. The kernel is checked in test_canvas_img2img_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import golden_inputs as gi
from tests.cpu_backend import oracle_ops
from tests.test_canvas_cpu import GRIDS, K, PTR, ROOT, S_LAT, STA_E_ARG, STEPS, _ints
from tests.test_canvas_cpu import _sampler as _any_sampler
from tests.test_canvas_wrap_cpu import SHAPES
from tests.test_img2img_cpu import _png, _script

P = 2
CENTRES = [[0.25, 0.4], [0.625, 0.6]]                  # canvas-normalised; on a 32 x 64 canvas the second disc straddles x = 0.5
SF, SA, S1M = 0.18215, 0.5, 0.8660254                   # the constants of test_vae_encode_step_vs_float64
NAME = "sta_vae_encode_step_windows"


def _grid(args):
    from sta.canvas import window_grid
    return window_grid(*args)


# ---------------------------------------------------------------------------------------------------
# C-ABI
# ---------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound_with_matching_argument_counts():
    from sta import lib
    vp, i, f, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    assert lib.SYMBOLS[NAME] == (i, [vp] * 8 + [l, i, i, i, i, vp, vp, i, i, f, f, f, i, vp])
    assert NAME + "_ring" not in lib.SYMBOLS
    header = " ".join(open(os.path.join(ROOT, "include", "sta_unet.h")).read().split())
    head = ("(const void* h, const float* quant_w, const float* quant_b, const float* n_post, const float* n_enc, float* x, float* z0, "
            "void* xin, long P, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, ")
    tail = "float scale_factor, float sqrt_a, float sqrt_1ma, int dtype, void* stream);"
    decl = "int " + NAME + head + tail
    assert decl in header and NAME + "_ring" not in header, decl
    assert decl.count(",") + 1 == len(lib.SYMBOLS[NAME][1])
    L = lib.load()
    assert hasattr(L, NAME) and not hasattr(L, NAME + "_ring")
    # the kernel lives with the window kernels, in the sampler step's unit (no flags), under the no-scratch rule of its siblings
    assert "vae_encode_step_windows_kernel" in lib.NO_SPILL_KERNELS["sta_sampler.hip"] and "sta_sampler.hip" not in lib.PER_SOURCE_FLAGS
    window = open(os.path.join(lib.CSRC, "sta_window.hip")).read()
    assert "vae_encode_step_windows_kernel" in window and '#include "sta_encode_dev.h"' in window
    # one definition of the per-pixel arithmetic: both units include the device header, neither writes exp() out itself
    encode = open(os.path.join(lib.CSRC, "sta_encode.hip")).read()
    assert '#include "sta_encode_dev.h"' in encode and "expf" not in encode and "expf" not in window
    assert "expf" in open(os.path.join(lib.CSRC, "sta_encode_dev.h")).read()


def _call(L, **kw):
    a = dict(h=PTR, qw=PTR + 0x100000, qb=PTR + 0x200000, n_post=PTR + 0x300000, n_enc=PTR + 0x400000, x=PTR + 0x500000, z0=PTR + 0x600000,
             xin=PTR + 0x700000, P=2, Hc=16, Wc=40, oy=(0,), ox=(0, 16, 24), s=16, wrap=0, dtype=0)
    a.update(kw)
    keep_y, oy = _ints(a["oy"]) if a["oy"] is not None else (None, 0)
    keep_x, ox = _ints(a["ox"]) if a["ox"] is not None else (None, 0)
    args = [a[k] for k in ("h", "qw", "qb", "n_post", "n_enc", "x", "z0", "xin", "P", "Hc", "Wc")] + [len(a["oy"] or ()), len(a["ox"] or ()), oy, ox,
                                                                                                      a["s"], a["wrap"]]
    rc = getattr(L, NAME)(*args, SF, SA, S1M, a["dtype"], None)
    return rc, L.sta_last_error().decode()


@pytest.mark.parametrize("wrap", [0, 1, 2, 3])
def test_argument_rules_reach_no_launch(wrap):
    """Every pointer is fake: a call that reached a launch would fault (or, without a GPU, fail with a launch error, not STA_E_ARG).
    The default grid is valid at every wrap (40 - 24 <= 16: as a ring it closes); an axis is held to the clamped rules or to the ring's."""
    from sta import lib
    L = lib.load()
    bad = [(dict(oy=None), "null pointer"), (dict(ox=None), "null pointer")]
    bad += [({k: 0}, "null pointer") for k in ("h", "qw", "qb", "n_post", "n_enc", "x")]                      # a NULL required tensor
    bad += [({k: PTR + 0x800008}, "16-byte aligned") for k in ("h", "n_post", "n_enc", "x", "z0", "xin")]     # a misaligned pointer
    bad += [(dict(ox=(0, 12, 24)), "ox[1]=12 is not a multiple of 8"),                                        # the grid rules, verbatim
            (dict(ox=(0, 24)), "gap between ox[0]=0 and ox[1]=24"),
            (dict(ox=(8, 16, 24)), "ox[0]=8 unsorted"),
            (dict(P=0), "P=0"), (dict(Wc=44), "Wc=44"), (dict(s=12), "s=12"), (dict(Hc=8), "Hc=8"),
            (dict(ox=tuple(range(0, 136, 8)), Wc=16 + 8 * 16), "nx=17"),
            (dict(dtype=7), "dtype 7"), (dict(dtype=2), "dtype 2")]                                           # a bad dtype
    bad += [(dict(wrap=4), "wrap=4"), (dict(wrap=-1), "wrap=-1")]
    if wrap & 1:                                                                                              # x closes on itself: the ring's rules
        bad += [(dict(ox=(0, 16)), "the ring does not close behind ox[1]=16"),
                (dict(ox=(0, 16, 40)), "ox[2]=40 is not on the wrapped axis"),
                (dict(ox=(0, 16, 32), dtype=7), "dtype 7")]                                                   # o + s > L is allowed there
    else:
        bad += [(dict(ox=(0, 16)), "gap behind ox[1]=16"), (dict(ox=(0, 16, 32)), "ox[2]=32 out of range")]
    if wrap & 2:
        bad += [(dict(oy=(0, 16), Hc=48), "the ring does not close behind oy[1]=16"),
                (dict(oy=(0, 8), Hc=16, dtype=7), "dtype 7")]                                                 # a valid ring reaches the dtype rule
    else:
        bad += [(dict(oy=(0, 8)), "oy[1]=8 out of range")]
    for kw, text in bad:
        rc, err = _call(L, **dict(dict(wrap=wrap), **kw))
        assert rc == STA_E_ARG and text in err, (wrap, kw, rc, err)
        assert err == "null pointer" or err.startswith(NAME[len("sta_"):] + ": "), (wrap, kw, err)            # one name whatever the wrap
    # the optional tensors may be NULL: the call then gets as far as the last rule
    rc, err = _call(L, wrap=wrap, z0=0, xin=0, dtype=7)
    assert rc == STA_E_ARG and "dtype 7" in err


# ---------------------------------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------------------------------
def _tensors(g, dtype, seed=3):
    """h with logvar pushed beyond both clamp limits (through an identity-ish quant_conv), as test_vae_encode_step_vs_float64."""
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(P, 8, g.Hc, g.Wc, generator=gen).to(dtype)
    h[:, 4:, :4] = 40.0
    h[:, 4:, 4:8] = -40.0
    qw = (torch.eye(8) + 0.01 * torch.randn(8, 8, generator=gen)).reshape(8, 8, 1, 1)
    qb = 0.1 * torch.randn(8, generator=gen)
    n_post, n_enc = torch.randn(P, 4, g.Hc, g.Wc, generator=gen), torch.randn(P, 4, g.Hc, g.Wc, generator=gen)
    return h, qw, qb, n_post, n_enc


def _float64(h, qw, qb, n_post, n_enc):
    """The float64 restatement of test_vae_encode_step_vs_float64 -> (z_ref, x_ref)."""
    m = torch.einsum("oi,bihw->bohw", qw.reshape(8, 8).double(), h.double()) + qb.double()[None, :, None, None]
    assert (m[:, 4:] > 20).any() and (m[:, 4:] < -30).any()
    z_ref = SF * (m[:, :4] + torch.exp(0.5 * m[:, 4:].clamp(-30.0, 20.0)) * n_post.double())
    return z_ref, np.float32(SA) * z_ref + np.float32(S1M) * n_enc.double()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [g + ("",) for g in GRIDS] + SHAPES)
def test_restatement_vs_float64_and_its_xin_is_the_split_of_its_x(shape, dtype):
    from sta.canvas import encode_step_windows_reference, window_split_reference
    assert GRIDS == [(32, 64, 32, 16), (16, 40, 16, 16), (24, 40, 16, 8)]
    g = _grid(shape)
    h, qw, qb, n_post, n_enc = _tensors(g, dtype)
    x, z0, xin = encode_step_windows_reference(h, qw, qb, n_post, n_enc, SF, SA, S1M, g, dtype, want_z0=True, want_xin=True)
    assert x.dtype == z0.dtype == torch.float32 and xin.dtype == dtype and tuple(xin.shape) == (2 * P * g.T, 4, g.s, g.s)
    for got, ref in zip((z0, x), _float64(h, qw, qb, n_post, n_enc)):
        err = (got.double() - ref).abs()
        assert (err <= 1e-5 * (1.0 + ref.abs())).all(), err.max().item()
    assert torch.equal(xin, window_split_reference(x, g, dtype))
    x2, none_z, none_xin = encode_step_windows_reference(h, qw, qb, n_post, n_enc, SF, SA, S1M, g, dtype, want_z0=False, want_xin=False)
    assert none_z is None and none_xin is None and torch.equal(x2, x)


# ---------------------------------------------------------------------------------------------------
# DDIMSampler.decode_canvas on the host miniature
# ---------------------------------------------------------------------------------------------------
def _sampler(eta=0.0, **kw):
    fused_step = kw.pop("canvas_fused_step", True)       # a class attribute, not a constructor keyword
    s = _any_sampler("ddim", **kw)
    s.canvas_fused_step = fused_step
    s.make_schedule(STEPS, ddim_eta=eta, verbose=False)
    return s


def _inputs(canvas):
    c, local_ctx, xa = gi.unet_inputs(K, 5)
    x = xa if canvas == (S_LAT, S_LAT) else torch.cat([xa, gi.unet_inputs(K, 6)[2]], dim=3)
    assert tuple(x.shape) == (1, 4) + canvas
    return c, local_ctx, x


def _decode_canvas(s, canvas, stride, x, c, local_ctx, t_start=2, centres=CENTRES, **kw):
    with oracle_ops():
        out = s.decode_canvas(x, canvas, S_LAT, stride, **dict(dict(t_start=t_start, conditionings=[c],
                                                                    unconditional_conditionings=gi.load_uncond(), bboxs=[centres],
                                                                    object_names=[["cat", "dog"]], local_conditionings=[local_ctx],
                                                                    unconditional_guidance_scale=7.5, seed=1), **kw))
    assert s._canvas is None and s._start == 0 and s._xin0 is None and s._inpaint is None
    assert out is s.last_result["x0"] and tuple(s.last_result["W"].shape) == (1, K, STEPS)
    return out.clone()


def _decode(s, x, c, local_ctx, t_start=2, **kw):
    with oracle_ops():
        return s.decode(x, c, t_start, unconditional_guidance_scale=7.5, unconditional_conditioning=gi.load_uncond(), text_index=0,
                        curr_text="", bboxs_curr=CENTRES, seed=1, prompt_idx=0, object_names=["cat", "dog"], local_conditionings=local_ctx,
                        **kw).clone()


def _kept(canvas):
    keep = torch.zeros((1, 1) + canvas)
    keep[..., 8:24, 4:20] = 1.0
    keep[..., 24:28, :] = 0.5
    return keep, torch.randn((1, 4) + canvas, generator=torch.Generator().manual_seed(9))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_decode_canvas_of_one_window_equals_decode(eta, masked):
    canvas = (S_LAT, S_LAT)
    c, local_ctx, x = _inputs(canvas)
    gen = torch.Generator().manual_seed(21)
    draws = [torch.randn((1, 4) + canvas, generator=gen) for _ in range(2 * STEPS)]
    kw = {}
    if masked:
        keep, x0 = _kept(canvas)
        kw = dict(mask=keep, x0=x0)
    s = _sampler(eta, noise=draws[:STEPS], mask_noise=draws[STEPS:])
    got = _decode_canvas(s, canvas, 16, x, c, local_ctx, **kw)
    want = _decode(s, x, c, local_ctx, **kw)
    assert got.shape == (1, 4) + canvas and torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, x)


def test_decode_canvas_of_two_disjoint_windows_equals_decode_batch():
    from sta.canvas import window_centres
    canvas = (S_LAT, 2 * S_LAT)
    c, local_ctx, x = _inputs(canvas)
    s = _sampler()
    got = _decode_canvas(s, canvas, S_LAT, x, c, local_ctx)
    per_window = window_centres(CENTRES, _grid((S_LAT, 2 * S_LAT, S_LAT, S_LAT)))
    with oracle_ops():
        want = s.decode_batch(torch.cat([x[..., :S_LAT], x[..., S_LAT:]]), [c, c], gi.load_uncond(), per_window, [["cat", "dog"]] * 2,
                              [local_ctx, local_ctx], 2, unconditional_guidance_scale=7.5, seed=1)
    assert torch.equal(got[..., :S_LAT], want[0:1]) and torch.equal(got[..., S_LAT:], want[1:2])
    assert not torch.allclose(got[..., :S_LAT], got[..., S_LAT:])


@pytest.mark.parametrize("wrap", ["", "x"])
def test_decode_canvas_with_t_start_s_equals_sample_canvas(wrap):
    canvas = (S_LAT, 2 * S_LAT)
    c, local_ctx, x = _inputs(canvas)
    s = _sampler()
    got = _decode_canvas(s, canvas, 16, x, c, local_ctx, t_start=STEPS, wrap=wrap)
    with oracle_ops():
        s.sample_canvas(S=STEPS, canvas=canvas, window=S_LAT, stride=16, conditionings=[c], unconditional_conditionings=gi.load_uncond(),
                        bboxs=[CENTRES], object_names=[["cat", "dog"]], local_conditionings=[local_ctx], x_T=x,
                        unconditional_guidance_scale=7.5, eta=0.0, seed=1, wrap=wrap)
    assert torch.equal(got, s.last_result["x0"])
    shorter = _decode_canvas(s, canvas, 16, x, c, local_ctx, t_start=2, wrap=wrap)
    assert not torch.equal(shorter, got)


class _Quant:
    """The part of a first stage model encode_step_canvas reads."""

    def __init__(self):
        self.quant_conv = torch.nn.Conv2d(8, 8, 1)
        gen = torch.Generator().manual_seed(4)
        with torch.no_grad():
            self.quant_conv.weight.copy_((torch.eye(8) + 0.01 * torch.randn(8, 8, generator=gen)).reshape(8, 8, 1, 1))
            self.quant_conv.bias.copy_(0.1 * torch.randn(8, generator=gen))


@pytest.mark.parametrize("wrap", ["", "x"])
def test_xin_of_encode_step_canvas_gives_the_same_result_as_none(wrap):
    """encode_step_canvas on the host (the restatement) uses encode_step's coefficient tables, and its xin is what decode_canvas would
    split from x itself: the same trajectory, bit for bit; a different xin changes it (the first call reads xin, not x)."""
    from sta.canvas import encode_step_windows_reference
    canvas = (S_LAT, 2 * S_LAT)
    g = _grid(canvas + (S_LAT, 16, wrap))
    c, local_ctx, _ = _inputs(canvas)
    gen = torch.Generator().manual_seed(12)
    h = torch.randn(1, 8, *canvas, generator=gen)
    n_post, n_enc = torch.randn(1, 4, *canvas, generator=gen), torch.randn(1, 4, *canvas, generator=gen)
    s, vae, t_enc = _sampler(), _Quant(), 2
    x, z0, xin = s.encode_step_canvas(h, vae, t_enc, n_post, n_enc, g, scale_factor=SF, want_z0=True)
    sa, s1m = s._encode_coefs()
    want = encode_step_windows_reference(h, vae.quant_conv.weight, vae.quant_conv.bias, n_post, n_enc, SF, float(sa[t_enc]), float(s1m[t_enc]),
                                         g, want_z0=True)
    assert all(torch.equal(a, b) for a, b in zip((x, z0, xin), want))
    assert torch.equal(x, s.stochastic_encode(z0, t_enc, noise=n_enc))          # the tables of encode_step / stochastic_encode
    assert tuple(xin.shape) == (2 * g.T, 4, S_LAT, S_LAT)
    with_xin = _decode_canvas(s, canvas, 16, x, c, local_ctx, t_start=t_enc, xin=xin, wrap=wrap)
    without = _decode_canvas(s, canvas, 16, x, c, local_ctx, t_start=t_enc, wrap=wrap)
    assert torch.isfinite(with_xin).all() and torch.equal(with_xin, without)
    other = _decode_canvas(s, canvas, 16, x, c, local_ctx, t_start=t_enc, xin=0.5 * xin, wrap=wrap)
    assert not torch.equal(other, without)


@pytest.mark.parametrize("fused", [True, False])
def test_draws_are_consumed_in_the_stated_order_at_eta_above_zero(fused):
    """Calls start .. S - 1 use weight column i, eta draw i - start and blend draw i - start, canvas-shaped, in the order of `_trajectory`:
    blend draw of the first call, its eta draw, the next call's blend draw, ... and no blend after the last step."""
    canvas = (S_LAT, 2 * S_LAT)
    c, local_ctx, x = _inputs(canvas)
    keep, x0 = _kept(canvas)
    log = []

    def draw(kind):
        def f(i, shape, device):
            log.append((kind, i, tuple(shape)))
            return torch.randn(shape, generator=torch.Generator().manual_seed(100 * (kind == "eta") + i))
        return f
    s = _sampler(0.5, noise=draw("eta"), mask_noise=draw("blend"), canvas_fused_step=fused)
    columns = []
    unet = s._window_unet

    def spy(*a, **k):
        grid, fn = unet(*a, **k)
        return grid, lambda xin, t, coef: (columns.append((int(t[0]), coef.clone())), fn(xin, t, coef))[1]
    s._window_unet = spy
    W0 = s.weight_init / K
    _decode_canvas(s, canvas, 16, x, c, local_ctx, t_start=3, mask=keep, x0=x0)
    shape = (1, 4) + canvas
    assert log == [("blend", 0, shape), ("eta", 0, shape), ("blend", 1, shape), ("eta", 1, shape), ("blend", 2, shape), ("eta", 2, shape)]
    assert [t for t, _ in columns] == [int(t) for t in s.tables["t_in"][STEPS - 3:]]          # calls 1 .. S - 1 of the schedule
    assert all(torch.equal(w, torch.full((1, K), W0)) for _, w in columns)
    log.clear()
    _decode_canvas(s, canvas, 16, x, c, local_ctx, t_start=2)
    assert log == [("eta", 0, shape), ("eta", 1, shape)]


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def test_decode_canvas_refusals_come_before_any_unet_call():
    canvas = (S_LAT, 2 * S_LAT)
    c, local_ctx, x = _inputs(canvas)
    calls = []

    def run(skw=None, schedule=True, canvas=canvas, stride=16, x=x, **kw):
        s = _any_sampler("ddim", **(skw or {}))
        if schedule:
            s.make_schedule(STEPS, verbose=False)
        s.model.apply_model_extra = lambda *a, **k: calls.append(1)
        try:
            return _decode_canvas(s, canvas, stride, x, c, local_ctx, **kw)
        finally:
            del s.model.apply_model_extra
            assert s._canvas is None and s._start == 0 and s._xin0 is None and s._inpaint is None
    with pytest.raises(ValueError, match="make_schedule"):
        run(schedule=False)
    for bad in (0, STEPS + 1, -1):
        with pytest.raises(ValueError, match="t_start must be in 1 .. %d" % STEPS):
            run(t_start=bad)
    with pytest.raises(ValueError, match="x_T"):
        run(x=x[..., :S_LAT])
    with pytest.raises(ValueError, match="x_T"):
        run(x=torch.cat([x, x]))
    with pytest.raises(ValueError, match="xin"):
        run(xin=torch.zeros(2 * 3, 4, S_LAT, 16))
    with pytest.raises(ValueError, match="xin"):
        run(xin=torch.zeros(2 * 2, 4, S_LAT, S_LAT))                                # T = 3 on this grid
    # everything sample_canvas / inpaint_canvas refuses
    with pytest.raises(ValueError, match="opt_epochs = 2"):
        run(skw=dict(opt_epochs=2))
    for name in ("attn_capture", "attn_loss", "latent_guidance"):
        with pytest.raises(ValueError, match=name):
            run(skw={name: object()})
    with pytest.raises(ValueError, match="smaller than the window"):
        run(canvas=(16, 2 * S_LAT))
    with pytest.raises(ValueError, match="stride 40"):
        run(stride=40)
    with pytest.raises(ValueError, match="'z'"):
        run(wrap="z")
    with pytest.raises(ValueError, match="1.5 windows"):
        run(wrap="y")
    with pytest.raises(ValueError, match="equal length"):
        run(bboxs=[CENTRES, CENTRES])
    keep, x0 = _kept(canvas)
    with pytest.raises(ValueError, match="mask= and x0="):
        run(mask=keep)
    with pytest.raises(ValueError, match="mask= and x0="):
        run(x0=x0)
    with pytest.raises(ValueError, match="image= and mask_px="):
        run(mask=keep, x0=x0, image=torch.zeros(1, 3, 8 * S_LAT, 16 * S_LAT))
    with pytest.raises(ValueError, match="mask"):
        run(mask=keep[..., :S_LAT], x0=x0)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        run(mask=2 * keep, x0=x0)
    assert not calls


def test_an_externally_set_start_is_still_refused():
    """The permission is decode_canvas's own argument to the shared body: `_start` set from outside raises exactly as before, on all three
    methods; PLMS and DPM-Solver++ keep having no decode*."""
    canvas = (S_LAT, 2 * S_LAT)
    c, local_ctx, x = _inputs(canvas)
    keep, x0 = _kept(canvas)
    kw = dict(S=STEPS, canvas=canvas, window=S_LAT, stride=16, conditionings=[c], unconditional_conditionings=gi.load_uncond(), bboxs=[CENTRES],
              object_names=[["cat", "dog"]], local_conditionings=[local_ctx], x_T=x, unconditional_guidance_scale=7.5, eta=0.0, seed=1)
    for kind in ("ddim", "dpm"):
        s = _any_sampler(kind)
        s._start = 2
        with pytest.raises(ValueError, match=r"sample_canvas: a trajectory that starts at call 2 \(img2img\) is not defined on a canvas"):
            s.sample_canvas(**kw)
        with pytest.raises(ValueError, match=r"inpaint_canvas: a trajectory that starts at call 2 \(img2img\) is not defined on a canvas"):
            s.inpaint_canvas(mask=keep, x0=x0, **kw)
    s = _sampler()
    s._start = 1
    with pytest.raises(ValueError, match="starts at call 1"):
        _decode_canvas(s, canvas, 16, x, c, local_ctx)
    for kind in ("plms", "dpm"):
        s = _any_sampler(kind)
        assert not any(hasattr(s, n) for n in ("decode", "decode_batch", "decode_canvas", "encode_step_canvas"))


def test_the_encoder_of_a_wrapped_canvas_sees_across_the_seam():
    """_encode_canvas: circular padding by 8 canvas_wrap_margin pixels on the wrapped axes, ONE encode, cropped by the margin in latent
    cells; a clamped canvas (or margin 0) is encoded as it is."""
    seen = []

    class Vae:
        def encode_moments_input(self, img):
            seen.append(img.clone())
            return torch.nn.functional.avg_pool2d(img, 8).repeat(1, 3, 1, 1)[:, :8]
    from sta.canvas import window_grid
    s = _any_sampler("ddim")
    img = torch.randn(1, 3, 8 * 32, 8 * 64, generator=torch.Generator().manual_seed(2))
    plain = s._encode_canvas(img, window_grid(32, 64, 32, 16), Vae())
    assert len(seen) == 1 and torch.equal(seen[0], img) and tuple(plain.shape) == (1, 8, 32, 64)
    s.canvas_wrap_margin = 4
    for wrap, (my, mx) in (("x", (0, 4)), ("y", (4, 0)), ("xy", (4, 4))):
        del seen[:]
        g = window_grid(64, 64, 32, 16, wrap)
        pic = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(3))
        h = s._encode_canvas(pic, g, Vae())
        assert len(seen) == 1 and tuple(seen[0].shape) == (1, 3, 512 + 64 * my // 4, 512 + 64 * mx // 4) and tuple(h.shape) == (1, 8, 64, 64)
        assert torch.equal(seen[0], torch.nn.functional.pad(pic, (8 * mx, 8 * mx, 8 * my, 8 * my), mode="circular"))
        assert torch.equal(h, Vae().encode_moments_input(pic))                    # a pointwise-in-cells encoder: the crop undoes the padding
    s.canvas_wrap_margin = 0
    del seen[:]
    s._encode_canvas(img, window_grid(32, 64, 32, 16, "x"), Vae())
    assert torch.equal(seen[0], img)
    with pytest.raises(ValueError, match="canvas"):
        s._encode_canvas(img[..., :256], window_grid(32, 64, 32, 16), Vae())


# ---------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------
def test_cli_flags_parse_and_defaults_are_unchanged():
    mod = _script()
    assert not hasattr(mod.build_parser().parse_args([]), "canvas")              # the parser inpaint.py and outpaint.py build on
    p = mod.build_parser(canvas=True)
    opt = p.parse_args(["--init-img", "a.png"])
    assert (opt.canvas, opt.canvas_stride, opt.canvas_wrap, opt.window) == (None, None, None, 512)
    assert (opt.strength, opt.ddim_steps, opt.scale, opt.opt_epochs, opt.batch_prompts, opt.dtype, opt.f, opt.C) == (0.75, 50, 5.0, 3, 1, "fp16", 8, 4)
    assert mod.canvas_grid(opt) is None and mod.check_options(p.parse_args(["--init-img", "a.png", "--opt_epochs", "0"])) == 37
    opt = p.parse_args(["--init-img", "a.png", "--opt_epochs", "0", "--canvas", "512x2048"])
    g = mod.canvas_grid(opt)
    assert (g.Hc, g.Wc, g.s, g.stride, g.T, g.wrap) == (64, 256, 64, 32, 7, "")
    opt = p.parse_args(["--init-img", "a.png", "--opt_epochs", "1", "--canvas", "256x512", "--window", "256", "--canvas_stride", "128",
                        "--canvas_wrap", "x"])
    g = mod.canvas_grid(opt)
    assert (g.Hc, g.Wc, g.s, g.stride, g.ox, g.wrap) == (32, 64, 32, 16, (0, 16, 32, 48), "x")
    g = mod.canvas_grid(p.parse_args(["--init-img", "a.png", "--opt_epochs", "0", "--canvas", "1024x1024"]))
    assert (g.ny, g.nx, g.T) == (3, 3, 9)                                            # the tiled upscale of a 512^2 picture


@pytest.mark.parametrize("args,what", [
    (["--canvas", "512x2048"], "--opt_epochs 3"),                                    # the default tracks epochs
    (["--canvas", "512x2048", "--opt_epochs", "2", "--clip", "synthetic"], "--opt_epochs 2"),
    (["--canvas", "512x2048", "--opt_epochs", "0", "--attn_guidance", "0.1"], "--attn_guidance"),
    (["--canvas", "512x2048", "--opt_epochs", "0", "--window", "500"], "--window 500"),
    (["--canvas", "512x2048", "--opt_epochs", "0", "--window", "0"], "--window 0"),
    (["--canvas", "512", "--opt_epochs", "0"], "HxW"),
    (["--canvas", "512x2000", "--opt_epochs", "0"], "2000"),
    (["--canvas", "256x2048", "--opt_epochs", "0"], "smaller than the window"),
    (["--canvas", "512x2048", "--opt_epochs", "0", "--canvas_stride", "576"], "stride"),
    (["--canvas", "512x8192", "--opt_epochs", "0", "--canvas_stride", "64"], "at most 16"),
    (["--canvas", "512x2048", "--opt_epochs", "0", "--canvas_wrap", "x", "--canvas_stride", "384"], "not a multiple of the stride"),
    (["--canvas", "512x2048", "--opt_epochs", "0", "--canvas_wrap", "y"], "1.5 windows"),
    (["--canvas_stride", "256", "--opt_epochs", "0"], "needs --canvas"),
    (["--canvas_wrap", "x", "--opt_epochs", "0"], "needs --canvas"),
    (["--canvas", "512x2048", "--opt_epochs", "0", "--strength", "1.0"], "t_enc"),   # the existing refusals hold on a canvas too
    (["--canvas", "512x2048", "--opt_epochs", "0", "--plms"], "PLMS"),
])
def test_cli_canvas_refusals_fire_before_a_model_is_built(args, what, tmp_path, monkeypatch):
    mod = _script()
    built = []
    monkeypatch.setattr("sta.pipeline.build_sd_v1", lambda *a, **k: built.append(1))
    img = _png(str(tmp_path / "a.png"), 96, 64)                                      # not square: fine on a canvas, never looked at here
    with pytest.raises(SystemExit) as e:
        mod.main(["--init-img", img, "--synthetic"] + args)
    assert what in str(e.value) and not built


def test_cli_resizes_the_init_image_to_the_canvas(tmp_path, capsys):
    mod = _script()
    f = _png(str(tmp_path / "one.png"), 100, 70)
    im = mod.load_img(f, (256, 512))
    assert im.shape == (1, 3, 256, 512) and float(im.min()) >= -1.0 and float(im.max()) <= 1.0
    assert "100 x 70 resized to the 512 x 256 canvas" in capsys.readouterr().out
    assert mod.load_img(f).shape == (1, 3, 64, 96)                                   # without a canvas: as before
