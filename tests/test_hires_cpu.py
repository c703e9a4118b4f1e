"""The layout-guided hi-res fix without a GPU: the two C entry points of the fused upscale launch (symbols; argument rules with fake
pointers: none of these calls may reach a launch), the torch restatement `upscale_step_windows_reference` against torch's bilinear
interpolation (integer factors) and against a float64 evaluation of the same formula (every shape), its exact invariants, the
`disc_scale` masks, `DDIMSampler.upscale_step_canvas` / `hires_canvas` on the host miniature and the CLI. The kernel is checked in
test_hires_gpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import golden_inputs as gi
from tests.cpu_backend import oracle_ops
from tests.test_canvas_cpu import K, PTR, ROOT, S_LAT, STA_E_ARG, STEPS, _ints
from tests.test_canvas_cpu import _sampler as _any_sampler

P, C, S, STRIDE = 2, 4, 16, 8
SA, S1M = 0.5, 0.8660254
NAME = "sta_latent_upscale_step_windows"
# (h, w, Hc, Wc, wrap): window 16, stride 8 — 2- and 4-fold overlap, clamped last windows, 2 .. 6 lane vectors per row, taps on both edges
INTEGER = [(16, 24, 32, 48, "")]
RATIONAL = [(16, 16, 24, 40, "")]                       # 1.5 x and 2.5 x
IDENTITY = [(16, 24, 16, 24, "")]
RINGS = [(16, 24, 32, 48, "x"), (16, 24, 32, 48, "y"), (16, 24, 32, 48, "xy")]
ALL = INTEGER + RATIONAL + IDENTITY + RINGS
EPS = 2.0 ** -24
DTYPES = [torch.float16, torch.bfloat16]


def _grid(shape):
    from sta.canvas import window_grid
    return window_grid(shape[2], shape[3], S, STRIDE, shape[4])


_CASES = {}


def tensors(shape, seed=3):
    """(z [P, C, h, w], noise [P, C, Hc, Wc]) float32, seeded; made once per shape and seed, never written to."""
    if (shape, seed) not in _CASES:
        gen = torch.Generator().manual_seed(seed)
        h, w, Hc, Wc, _ = shape
        _CASES[(shape, seed)] = (torch.randn(P, C, h, w, generator=gen), torch.randn(P, C, Hc, Wc, generator=gen))
    return _CASES[(shape, seed)]


def _taps(L_out, L_in, wrapped):
    """The rule of the issue in numpy float32, every operation rounded on its own -> (i0, i1, l0, l1)."""
    f = np.float32
    scale = f(L_in) / f(L_out)
    src = (np.arange(L_out, dtype=f) + f(0.5)) * scale - f(0.5)
    assert src.dtype == f
    if not wrapped:
        src = np.maximum(src, f(0))
    fl = np.floor(src)
    l1 = src - fl
    l0 = f(1) - l1
    i0 = fl.astype(np.int64)
    if wrapped:
        i0 = i0 % L_in
        i1 = (i0 + 1) % L_in
    else:
        i1 = np.minimum(i0 + 1, L_in - 1)
    assert i0.min() >= 0 and i1.max() <= L_in - 1
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l0).double(), torch.from_numpy(l1).double()


_F64 = {}


def float64(shape, seed=3):
    """(z_up, x) of the same formula in float64 with the same float32 weights; made once per case."""
    if (shape, seed) not in _F64:
        z, noise = tensors(shape, seed)
        h, w, Hc, Wc, wrap = shape
        y0, y1, l0y, l1y = _taps(Hc, h, "y" in wrap)
        x0, x1, l0x, l1x = _taps(Wc, w, "x" in wrap)
        zd = z.double()
        r0, r1 = zd[:, :, y0], zd[:, :, y1]
        z_up = l0y[:, None] * (l0x * r0[..., x0] + l1x * r0[..., x1]) + l1y[:, None] * (l0x * r1[..., x0] + l1x * r1[..., x1])
        _F64[(shape, seed)] = (z_up, float(np.float32(SA)) * z_up + float(np.float32(S1M)) * noise.double())
    return _F64[(shape, seed)]


def bounds(shape, seed=3):
    """The issue's bounds -> (for z_up: 16 eps max|z|, for x: 16 eps (|sa| max|z| + |s1m noise|) elementwise)."""
    z, noise = tensors(shape, seed)
    zmax = z.abs().max().double()
    return 16 * EPS * zmax, 16 * EPS * (abs(SA) * zmax + (S1M * noise.double()).abs())


# ---------------------------------------------------------------------------------------------------
# C-ABI
# ---------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound_with_matching_argument_counts():
    from sta import lib
    vp, i, f, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    assert lib.SYMBOLS[NAME] == (i, [vp] * 5 + [l, i, i, i, i, i, i, i, vp, vp, i, i, f, f, i, vp])
    assert NAME + "_ring" not in lib.SYMBOLS
    header = " ".join(open(os.path.join(ROOT, "include", "sta_unet.h")).read().split())
    head = ("(const float* z, const float* noise, float* x, float* z_up, void* xin, long P, int C, int h, int w, int Hc, int Wc, int ny, "
            "int nx, const int* oy, const int* ox, int s, int wrap, ")
    tail = "float sqrt_a, float sqrt_1ma, int dtype, void* stream);"
    decl = "int " + NAME + head + tail
    assert decl in header and NAME + "_ring" not in header, decl
    assert decl.count(",") + 1 == len(lib.SYMBOLS[NAME][1])
    L = lib.load()
    assert hasattr(L, NAME) and not hasattr(L, NAME + "_ring")
    # with the window kernels, in the sampler step's unit (no flags), under the no-scratch rule of its siblings
    assert "latent_upscale_step_windows_kernel" in lib.NO_SPILL_KERNELS["sta_sampler.hip"] and "sta_sampler.hip" not in lib.PER_SOURCE_FLAGS
    window = open(os.path.join(lib.CSRC, "sta_window.hip")).read()
    assert "latent_upscale_step_windows_kernel" in window
    # one device definition of the noising: encode1 and the upscale kernel both call noise1 of sta_encode_dev.h
    dev = open(os.path.join(lib.CSRC, "sta_encode_dev.h")).read()
    assert dev.count("float noise1(") == 1 and dev.count("noise1(") == 2 and "noise1(zu[k]" in window


def _call(L, **kw):
    a = dict(z=PTR, noise=PTR + 0x100000, x=PTR + 0x200000, z_up=PTR + 0x300000, xin=PTR + 0x400000, P=2, C=4, h=16, w=24, Hc=16, Wc=40,
             oy=(0,), ox=(0, 16, 24), s=16, wrap=0, dtype=0)
    a.update(kw)
    keep_y, oy = _ints(a["oy"]) if a["oy"] is not None else (None, 0)
    keep_x, ox = _ints(a["ox"]) if a["ox"] is not None else (None, 0)
    args = [a[k] for k in ("z", "noise", "x", "z_up", "xin", "P", "C", "h", "w", "Hc", "Wc")] + [len(a["oy"] or ()), len(a["ox"] or ()), oy, ox,
                                                                                                 a["s"], a["wrap"]]
    rc = getattr(L, NAME)(*args, SA, S1M, a["dtype"], None)
    return rc, L.sta_last_error().decode()


@pytest.mark.parametrize("wrap", [0, 1, 2, 3])
def test_argument_rules_reach_no_launch(wrap):
    """Every pointer is fake: a call that reached a launch would fault (or, without a GPU, fail with a launch error, not STA_E_ARG).
    The default grid is valid at every wrap (40 - 24 <= 16: as a ring it closes); an axis is held to the clamped rules or to the ring's."""
    from sta import lib
    L = lib.load()
    bad = [(dict(oy=None), "null pointer"), (dict(ox=None), "null pointer")]
    bad += [({k: 0}, "null pointer") for k in ("z", "noise", "x")]                                            # a NULL required tensor
    bad += [({k: PTR + 0x800008}, "16-byte aligned") for k in ("z", "noise", "x", "z_up", "xin")]             # a misaligned pointer
    bad += [(dict(h=24), "smaller than the source"), (dict(w=48), "smaller than the source"),                 # upscale only
            (dict(h=12), "h=12"), (dict(w=20), "w=20"), (dict(h=0), "h=0"), (dict(w=-8), "w=-8"),             # positive multiples of 8
            (dict(Wc=44), "Wc=44"), (dict(s=12), "s=12"), (dict(Hc=8), "Hc=8"), (dict(P=0), "P=0"),
            (dict(C=0), "C=0"), (dict(C=-4), "C=-4"),                                                         # what scatter supports
            (dict(ox=(0, 12, 24)), "ox[1]=12 is not a multiple of 8"),                                        # the grid rules, verbatim
            (dict(ox=(0, 24)), "gap between ox[0]=0 and ox[1]=24"),
            (dict(ox=tuple(range(0, 136, 8)), Wc=16 + 8 * 16), "nx=17"),                                      # > STA_MAX_WINDOW_OFFSETS
            (dict(oy=tuple(range(0, 136, 8)), Hc=16 + 8 * 16), "ny=17"),
            (dict(dtype=7), "dtype 7"), (dict(dtype=2), "dtype 2")]
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
    rc, err = _call(L, wrap=wrap, z_up=0, xin=0, dtype=7)                                                         # the optional tensors may be NULL
    assert rc == STA_E_ARG and "dtype 7" in err


# ---------------------------------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------------------------------
def _restate(shape, seed=3, dtype=torch.float16, z=None, noise=None):
    from sta.canvas import upscale_step_windows_reference
    z0, n0 = tensors(shape, seed)
    return upscale_step_windows_reference(z0 if z is None else z, n0 if noise is None else noise, SA, S1M, _grid(shape), dtype, want_z_up=True)


@pytest.mark.parametrize("shape", INTEGER + IDENTITY)
def test_restatement_vs_torch_bilinear_at_integer_factors(shape):
    """z_up against F.interpolate(mode="bilinear", align_corners=False), which anchors the semantics where it derives the same weights:
    within 16 x 2^-24 x max|z| (16 >= the fp32 roundings on the path: 2 complements, 6 in the two-level interpolation, 3 in the
    noising, and their compounding)."""
    z, _ = tensors(shape)
    x, z_up, xin = _restate(shape)
    want = torch.nn.functional.interpolate(z, size=shape[2:4], mode="bilinear", align_corners=False)
    err = (z_up - want).abs().max().item()
    bound = 16 * EPS * z.abs().max().item()
    print("restatement vs torch %s: %.3g (bound %.3g)" % (shape, err, bound))
    assert z_up.dtype == torch.float32 and err <= bound


@pytest.mark.parametrize("shape", ALL)
def test_restatement_vs_float64(shape):
    """Every shape, the rational and the wrapped ones included, against the float64 evaluation of the same formula with the same fp32
    weights, elementwise within 16 x 2^-24 x (|sa| max|z| + |s1m noise|) (z_up: the same with sa = 1 and no noise)."""
    x, z_up, xin = _restate(shape)
    z_ref, x_ref = float64(shape)
    bz, bx = bounds(shape)
    ez, ex = (z_up.double() - z_ref).abs(), (x.double() - x_ref).abs()
    print("restatement vs float64 %s: z_up %.3g, x %.3g" % (shape, ez.max().item(), ex.max().item()))
    assert x.dtype == z_up.dtype == torch.float32 and tuple(x.shape) == (P, C) + tuple(shape[2:4])
    assert (ez <= bz).all() and (ex <= bx).all()
    if shape[4]:            # a ring is not the clamped upscale: the first column sees the last
        clamped = _restate(shape[:4] + ("",))[1]
        assert not torch.equal(clamped, z_up)


def test_identity_size_returns_z():
    shape = IDENTITY[0]
    z, noise = tensors(shape)
    x, z_up, _ = _restate(shape)
    assert torch.equal(z_up, z)
    sa, s1m = torch.tensor(SA), torch.tensor(S1M)
    assert torch.equal(x, sa * z + s1m * noise)


@pytest.mark.parametrize("dtype", DTYPES + [torch.float32])
@pytest.mark.parametrize("shape", ALL)
def test_xin_is_the_split_of_x(shape, dtype):
    from sta.canvas import upscale_step_windows_reference, window_split_reference
    g = _grid(shape)
    z, noise = tensors(shape)
    x, none_z, xin = upscale_step_windows_reference(z, noise, SA, S1M, g, dtype)
    assert none_z is None and xin.dtype == dtype and tuple(xin.shape) == (2 * P * g.T, C, S, S)
    assert torch.equal(xin, window_split_reference(x, g, dtype))
    x2, z_up, none_xin = upscale_step_windows_reference(z, noise, SA, S1M, g, dtype, want_z_up=True, want_xin=False)
    assert none_xin is None and z_up is not None and torch.equal(x2, x)
    from sta.canvas import upscale_step_windows                # CPU tensors take the restatement
    assert all(torch.equal(a, b) for a, b in zip(upscale_step_windows(z, noise, SA, S1M, g, dtype), (x, xin)) if a is not None)


@pytest.mark.parametrize("shape", RINGS)
def test_ring_restatement_is_roll_equivariant(shape):
    """Integer factor f = 2: z rolled by k cells and the noise by k f along the wrapped axes rolls x and z_up by k f, bit for bit."""
    z, noise = tensors(shape)
    x, z_up, _ = _restate(shape)
    f = 2
    for k in (1, 5):
        ky, kx = k if "y" in shape[4] else 0, k if "x" in shape[4] else 0
        xr, zr, _ = _restate(shape, z=z.roll((ky, kx), (-2, -1)), noise=noise.roll((ky * f, kx * f), (-2, -1)))
        assert not torch.equal(zr, z_up)
        assert torch.equal(xr, x.roll((ky * f, kx * f), (-2, -1))) and torch.equal(zr, z_up.roll((ky * f, kx * f), (-2, -1)))


def test_restatement_refusals():
    from sta.canvas import upscale_step_windows_reference, window_grid
    g = window_grid(32, 48, 16, 8)
    z, noise = torch.zeros(1, 4, 16, 24), torch.zeros(1, 4, 32, 48)
    for bad_z, text in ((torch.zeros(1, 4, 40, 24), "smaller than the source"), (torch.zeros(1, 4, 16, 56), "smaller than the source"),
                        (torch.zeros(1, 4, 12, 24), "multiples of 8"), (torch.zeros(4, 16, 24), "float32 latent"),
                        (torch.zeros(1, 4, 16, 24, dtype=torch.float16), "float32 latent")):
        with pytest.raises(ValueError, match=text):
            upscale_step_windows_reference(bad_z, noise, SA, S1M, g)
    with pytest.raises(ValueError, match="noise"):
        upscale_step_windows_reference(z, noise[..., :40], SA, S1M, g)


# ---------------------------------------------------------------------------------------------------
# disc_scale
# ---------------------------------------------------------------------------------------------------
def test_disc_scale_one_reproduces_the_masks_bit_for_bit():
    from sta import ops, prompt_state
    centres = [(0.3, 0.4), (0.7, 0.6), (0.05, 0.95), (0.5, 0.5), (0.2, 0.2)]
    try:
        prompt_state.begin_prompt(None, disc_radius=0.2 * 1.0)
        r2 = prompt_state.disc_radius_sq()
        assert r2 == 0.04 and np.float32(r2) == np.float32(0.04)
        for dim in (8, 16, 32, 64):
            axis = torch.arange(dim, dtype=torch.float32) / dim
            for k, (cx, cy) in enumerate(centres):          # the rule as it has always been written
                want = (((axis - cx) ** 2)[None, :] + ((axis - cy) ** 2)[:, None]) < 0.04
                assert torch.equal(ops.disc_masks(centres, dim, r2)[k].bool().reshape(dim, dim), want)
            assert torch.equal(ops.disc_masks(centres, dim, r2), ops.disc_masks(centres, dim))
            assert torch.equal(ops.disc_mask_bits(centres, dim, r2), ops.disc_mask_bits(centres, dim))
        prompt_state.begin_prompt(None, disc_radius=0.2 * 2.0)
        assert prompt_state.disc_radius_sq() == 0.4 * 0.4
        prompt_state.begin_prompt(None)                         # every announcement sets it: `sample` and `sample_batch` never scale
        assert prompt_state.disc_radius_sq() == 0.04
        for bad in (0.0, -0.2, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="disc_radius"):
                prompt_state.begin_prompt(None, disc_radius=bad)
    finally:
        prompt_state.begin_prompt(None)


@pytest.mark.parametrize("wrap", ["", "x"])
def test_disc_scale_two_on_a_2x_canvas_is_the_canvas_wide_disc(wrap):
    """A 32^2 first pass refined on a 64 x 64 canvas of 32 x 32 windows with disc_scale = 2: every window's mask, at every level, is the
    crop at the window's position of the disc of radius 0.2 CANVAS sides (0.4 window sides). Centres are multiples of 1/64 in window
    units, so every term of the fp32 rule is exact and the float64 evaluation decides the same way."""
    from sta import ops, prompt_state
    from sta.canvas import check_disc_scale, window_centres, window_grid, windows
    g = window_grid(64, 64, 32, 16, wrap)
    s, scale = g.s, check_disc_scale(g, g.Hc / 32)
    assert scale == 2.0
    centres = [(kx / 64.0 * s / g.Wc, ky / 64.0 * s / g.Hc) for kx, ky in ((16, 32), (77, 40), (119, 13), (40, 108), (3, 70))]
    hits = 0
    try:
        prompt_state.begin_prompt(None, disc_radius=0.2 * scale)
        r2 = prompt_state.disc_radius_sq()
        for (y0, x0), wc in zip(windows(g), window_centres(centres, g)):
            for f in (1, 2, 4, 8):
                d = s // f
                got = ops.disc_masks(wc, d, r2).reshape(len(centres), d, d)
                r = torch.arange(d, dtype=torch.float64)
                Y, X = (y0 + f * r)[:, None], (x0 + f * r)[None, :]             # canvas positions of the level's pixels, latent pixels
                for k, (x, y) in enumerate(centres):
                    dx, dy = X / g.Wc - x, Y / g.Hc - y                         # in canvas sides
                    if "x" in wrap:
                        dx = (dx + 0.5) % 1.0 - 0.5                             # the nearest image round the ring
                    want = dx ** 2 + dy ** 2 < 0.04
                    assert torch.equal(got[k].bool(), want.expand(d, d)), (y0, x0, f, k)
                    hits += int(want.sum())
                if f == 1:
                    assert not torch.equal(got, ops.disc_masks(wc, d).reshape(len(centres), d, d))
    finally:
        prompt_state.begin_prompt(None)
    assert hits > 0


def test_the_wrap_refusal_of_a_large_disc():
    from sta.canvas import check_disc_scale, window_grid
    g = window_grid(16, 48, 16, 8, "x")                        # L - s = 32
    assert check_disc_scale(g, 5) == 5.0                       # 0.4 x 5 x 16 = 32: fits
    with pytest.raises(ValueError, match="wrapped x axis: length 48"):
        check_disc_scale(g, 5.5)
    assert check_disc_scale(window_grid(16, 48, 16, 8), 50) == 50.0            # clamped axes have no such rule
    with pytest.raises(ValueError, match="wrapped y axis"):
        check_disc_scale(window_grid(48, 128, 16, 8, "xy"), 5.5)
    for bad in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="disc_scale"):
            check_disc_scale(g, bad)


# ---------------------------------------------------------------------------------------------------
# samplers on the host miniature: a 16 x 32 first pass refined on a 32 x 64 canvas of 32 x 32 windows (T = 3; wrapped along x: T = 4)
# ---------------------------------------------------------------------------------------------------
CANVAS = (S_LAT, 2 * S_LAT)
CENTRES = [[0.25, 0.4], [0.625, 0.6]]


def _sampler(eta=0.0, **kw):
    fused_step = kw.pop("canvas_fused_step", True)
    s = _any_sampler("ddim", **kw)
    s.canvas_fused_step = fused_step
    s.make_schedule(STEPS, ddim_eta=eta, verbose=False)
    return s


def _first_pass(shape=(S_LAT // 2, S_LAT)):
    return torch.randn((1, 4) + shape, generator=torch.Generator().manual_seed(31))


def _kw(**kw):
    c, local_ctx, _ = gi.unet_inputs(K, 5)
    return dict(dict(conditionings=[c], unconditional_conditionings=gi.load_uncond(), bboxs=[CENTRES], object_names=[["cat", "dog"]],
                     local_conditionings=[local_ctx], unconditional_guidance_scale=7.5, seed=1), **kw)


@pytest.mark.parametrize("wrap", ["", "x"])
def test_hires_canvas_is_upscale_step_canvas_then_decode_canvas(wrap):
    from sta import prompt_state
    from sta.canvas import upscale_step_windows_reference, window_grid
    z, t_start = _first_pass(), 2
    s = _sampler()
    seen = []
    inner = prompt_state.begin_prompt
    spy = lambda *a, **k: (seen.append(k.get("disc_radius")), inner(*a, **k))[1]
    prompt_state.begin_prompt = spy
    try:
        with oracle_ops():
            got = s.hires_canvas(z, CANVAS, S_LAT, 16, t_start=t_start, wrap=wrap, **_kw()).clone()
    finally:
        prompt_state.begin_prompt = inner
    assert seen == [0.2 * 2.0] and s._disc_scale == 1.0 and s._canvas is None
    g = window_grid(*CANVAS, S_LAT, 16, wrap)
    torch.manual_seed(1)
    noise = torch.randn((1, 4) + CANVAS)                      # the documented draw: seeded, canvas-shaped, on the latent's device
    x, z_up, xin = s.upscale_step_canvas(z, t_start, noise, g, want_z_up=True)
    sa, s1m = s._encode_coefs()
    want = upscale_step_windows_reference(z, noise, float(sa[t_start]), float(s1m[t_start]), g, want_z_up=True)
    assert all(torch.equal(a, b) for a, b in zip((x, z_up, xin), want))
    assert torch.equal(x, s.stochastic_encode(z_up, t_start, noise=noise))                  # the tables of encode_step / stochastic_encode
    with oracle_ops():
        two = s.decode_canvas(x, CANVAS, S_LAT, 16, t_start=t_start, xin=xin, wrap=wrap, disc_scale=2.0, **_kw()).clone()
        plain = s.decode_canvas(x, CANVAS, S_LAT, 16, t_start=t_start, xin=xin, wrap=wrap, **_kw()).clone()
        one = s.decode_canvas(x, CANVAS, S_LAT, 16, t_start=t_start, xin=xin, wrap=wrap, disc_scale=1.0, **_kw()).clone()
        given = s.hires_canvas(z, CANVAS, S_LAT, 16, t_start=t_start, wrap=wrap, noise=noise, disc_scale=2.0, **_kw()).clone()
    assert got.shape == (1, 4) + CANVAS and torch.isfinite(got).all()
    assert torch.equal(got, two) and torch.equal(given, got)
    assert torch.equal(one, plain) and not torch.equal(plain, two)                          # the discs matter, and 1.0 is today's
    # canvas_fused_step = False on the CPU is the restatement too
    u = _sampler(canvas_fused_step=False)
    assert all(torch.equal(a, b) for a, b in zip(u.upscale_step_canvas(z, t_start, noise, g, want_z_up=True), (x, z_up, xin)))


def test_hires_canvas_at_t_start_s_noises_to_the_last_table_entry():
    z = _first_pass()
    s = _sampler()
    seen = []
    inner = s.upscale_step_canvas
    s.upscale_step_canvas = lambda z, t, *a, **k: (seen.append(t), inner(z, t, *a, **k))[1]
    with oracle_ops():
        out = s.hires_canvas(z, CANVAS, S_LAT, 16, t_start=STEPS, **_kw())
    assert seen == [len(s.tables["a"]) - 1] and torch.isfinite(out).all()


def test_an_explicit_disc_scale_lifts_the_refusal_of_a_non_uniform_upscale():
    s = _sampler()
    with pytest.raises(ValueError, match="not a uniform upscale"):
        s.hires_canvas(_first_pass((32, 32)), CANVAS, S_LAT, 16, t_start=2, **_kw())
    with oracle_ops():
        out = s.hires_canvas(_first_pass((32, 32)), CANVAS, S_LAT, 16, t_start=2, disc_scale=1.5, **_kw())
    assert out.shape == (1, 4) + CANVAS and torch.isfinite(out).all()


def test_draws_are_consumed_in_the_documented_order(monkeypatch):
    """(1) the encode draw: torch.manual_seed(seed), torch.randn of one canvas; (2) decode_canvas's: blend draw of a call, its eta draw."""
    z = _first_pass()
    log = []

    def draw(kind):
        def f(i, shape, device):
            log.append((kind, i, tuple(shape)))
            return torch.randn(shape, generator=torch.Generator().manual_seed(100 * (kind == "eta") + i))
        return f
    s = _sampler(0.5, noise=draw("eta"), mask_noise=draw("blend"))
    randn, seed = torch.randn, torch.manual_seed
    monkeypatch.setattr(torch, "manual_seed", lambda v: (log.append(("seed", v)), seed(v))[1])
    monkeypatch.setattr(torch, "randn", lambda *a, **k: (log.append(("randn", tuple(a[0]))) if "generator" not in k else None, randn(*a, **k))[1])
    shape = (1, 4) + CANVAS
    with oracle_ops():
        s.hires_canvas(z, CANVAS, S_LAT, 16, t_start=2, **_kw(seed=7))
    assert log[:2] == [("seed", 7), ("randn", shape)]
    assert [e for e in log[2:] if e[0] in ("eta", "blend", "randn")] == [("eta", 0, shape), ("eta", 1, shape)]
    del log[:]
    keep = torch.zeros((1, 1) + CANVAS)
    keep[..., 8:24, 4:20] = 1.0
    x0 = randn(shape, generator=torch.Generator().manual_seed(9))
    with oracle_ops():
        s.hires_canvas(z, CANVAS, S_LAT, 16, t_start=2, mask=keep, x0=x0, **_kw(seed=7))
    assert [e for e in log if e[0] != "seed"] == [("randn", shape), ("blend", 0, shape), ("eta", 0, shape), ("blend", 1, shape), ("eta", 1, shape)]


def test_refusals_come_before_any_unet_call():
    z = _first_pass()
    calls = []

    def run(method="hires_canvas", skw=None, schedule=True, z=z, canvas=CANVAS, stride=16, **kw):
        s = _any_sampler("ddim", **(skw or {}))
        if schedule:
            s.make_schedule(STEPS, verbose=False)
        s.model.apply_model_extra = lambda *a, **k: calls.append(1)
        try:
            with oracle_ops():
                if method == "hires_canvas":
                    return s.hires_canvas(z, canvas, S_LAT, stride, **_kw(**dict(dict(t_start=2), **kw)))
                return getattr(s, method)(**_kw(**dict(dict(S=STEPS, canvas=canvas, window=S_LAT, stride=stride, x_T=torch.zeros((1, 4) + canvas)), **kw)))
        finally:
            del s.model.apply_model_extra
            assert s._canvas is None and s._start == 0 and s._xin0 is None and s._inpaint is None and s._disc_scale == 1.0
    with pytest.raises(ValueError, match="make_schedule"):
        run(schedule=False)
    for bad in (0, STEPS + 1, -1):
        with pytest.raises(ValueError, match="t_start must be in 1 .. %d" % STEPS):
            run(t_start=bad)
    with pytest.raises(ValueError, match="smaller than the first pass"):
        run(z=torch.zeros(1, 4, 40, 64))
    with pytest.raises(ValueError, match="not a uniform upscale"):
        run(z=torch.zeros(1, 4, 32, 32))                                        # 1 x and 2 x
    with pytest.raises(ValueError, match="wrapped x axis"):
        run(wrap="x", disc_scale=3.0)                                           # L - s = 32 < 0.4 x 3 x 32
    with pytest.raises(ValueError, match="disc_scale"):
        run(disc_scale=0.0)
    with pytest.raises(ValueError, match="noise"):
        run(noise=torch.zeros(1, 4, 32, 32))
    with pytest.raises(ValueError, match="multiples of 8"):
        run(z=torch.zeros(1, 4, 12, 24))
    # everything decode_canvas refuses
    with pytest.raises(ValueError, match="opt_epochs = 2"):
        run(skw=dict(opt_epochs=2))
    with pytest.raises(ValueError, match="attn_loss"):
        run(skw=dict(attn_loss=object()))
    with pytest.raises(ValueError, match="stride 40"):
        run(stride=40)
    with pytest.raises(ValueError, match="equal length"):
        run(bboxs=[CENTRES, CENTRES])
    with pytest.raises(ValueError, match="mask= and x0="):
        run(mask=torch.zeros((1, 1) + CANVAS))
    # the new keyword on the other canvas methods
    for method in ("sample_canvas", "inpaint_canvas"):
        extra = dict(mask=torch.zeros((1, 1) + CANVAS), x0=torch.zeros((1, 4) + CANVAS)) if method == "inpaint_canvas" else {}
        with pytest.raises(ValueError, match="wrapped x axis"):
            run(method, wrap="x", disc_scale=3.0, eta=0.0, **extra)
        with pytest.raises(ValueError, match="disc_scale"):
            run(method, disc_scale=-1.0, eta=0.0, **extra)
    assert not calls
    for kind in ("plms", "dpm"):
        assert not any(hasattr(_any_sampler(kind), n) for n in ("hires_canvas", "upscale_step_canvas"))


# ---------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------
def _cli():
    sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts"))
    import _txt2img_common as cli
    return cli


def test_cli_flags_parse_and_defaults_are_unchanged():
    cli = _cli()
    p = cli.build_parser("x.json")
    opt = p.parse_args([])
    assert (opt.hires, opt.hires_strength, opt.hires_stride) == (None, None, None)
    assert (opt.H, opt.W, opt.C, opt.f, opt.ddim_steps, opt.scale, opt.ddim_eta, opt.opt_epochs, opt.n_iter, opt.n_samples, opt.seed,
            opt.batch_prompts, opt.dtype, opt.canvas, opt.canvas_stride, opt.canvas_wrap, opt.canvas_guidance, opt.attn_guidance, opt.attn_res,
            opt.plms, opt.dpm_solver) == (512, 512, 4, 8, 50, 7.5, 0.0, 3, 2, 1, 42, 1, "fp16", None, None, None, None, None, 16, False, False)
    assert cli.hires_plan(p.parse_args(["--opt_epochs", "0"])) is None
    opt = p.parse_args(["--opt_epochs", "0", "--hires", "1024x1024", "--hires_strength", "0.4"])
    cli.check_options(opt)
    g, t_start, disc_scale = cli.hires_plan(opt)
    assert (g.Hc, g.Wc, g.s, g.stride, g.T, g.wrap, t_start, disc_scale) == (128, 128, 64, 32, 9, "", 20, 2.0)
    opt = p.parse_args(["--opt_epochs", "3", "--clip", "synthetic", "--plms", "--canvas", "512x2048", "--opt_epochs", "0", "--hires", "1024x4096",
                        "--hires_strength", "1.0", "--hires_stride", "256", "--canvas_wrap", "x", "--canvas_guidance", "0.1", "--ddim_steps", "10"])
    cli.check_options(opt)
    g, t_start, disc_scale = cli.hires_plan(opt)
    assert (g.Hc, g.Wc, g.s, g.stride, g.ny, g.nx, g.wrap, t_start, disc_scale) == (128, 512, 64, 32, 3, 16, "x", 10, 2.0)
    g, _, disc_scale = cli.hires_plan(p.parse_args(["--H", "256", "--W", "256", "--hires", "640x640", "--hires_strength", "0.5", "--dpm_solver"]))
    assert (g.Hc, g.s, disc_scale) == (80, 32, 2.5)
    # --canvas_guidance without --canvas: the second pass is the canvas it guides
    cli.check_options(p.parse_args(["--opt_epochs", "0", "--hires", "1024x1024", "--hires_strength", "0.4", "--canvas_guidance", "0.1"]))


@pytest.mark.parametrize("args,what", [
    (["--hires", "256x256", "--hires_strength", "0.5"], "smaller than the first pass"),
    (["--canvas", "512x2048", "--hires", "1024x2048", "--hires_strength", "0.5"], "not a uniform upscale"),
    (["--canvas", "512x2048", "--hires", "512x1024", "--hires_strength", "0.5"], "smaller than the first pass"),
    (["--hires", "1024x2048", "--hires_strength", "0.5"], "not a uniform upscale"),
    (["--hires", "1024x1024"], "--hires_strength"),
    (["--hires", "1024x1024", "--hires_strength", "0.0"], "(0, 1]"),
    (["--hires", "1024x1024", "--hires_strength", "1.5"], "(0, 1]"),
    (["--hires", "1024x1024", "--hires_strength", "0.01"], "t_start"),
    (["--hires", "1024", "--hires_strength", "0.5"], "HxW"),
    (["--hires", "1000x1000", "--hires_strength", "0.5"], "1000"),
    (["--hires", "1024x1024", "--hires_strength", "0.5", "--hires_stride", "100"], "100"),
    (["--hires", "1024x1024", "--hires_strength", "0.5", "--hires_stride", "576"], "stride"),
    (["--hires", "1024x1024", "--hires_strength", "0.5", "--W", "768"], "square"),
    (["--hires", "1024x1024", "--hires_strength", "0.5", "--attn_maps"], "--attn_maps"),
    (["--hires", "1024x1024", "--hires_strength", "0.5", "--opt_epochs", "3", "--attn_loss", "0.5"], "--attn_loss"),
    (["--H", "256", "--W", "256", "--hires", "512x512", "--hires_strength", "0.5", "--canvas_guidance", "0.1", "--attn_res", "64"], "--attn_res 64"),
    (["--hires", "512x512", "--hires_strength", "0.5", "--canvas_wrap", "x"], "needs --canvas"),
    (["--hires_strength", "0.5"], "needs --hires"),
    (["--hires_stride", "256"], "needs --hires"),
])
def test_cli_refusals_fire_before_a_model_is_built(args, what, monkeypatch):
    import sta.pipeline
    cli = _cli()
    monkeypatch.setattr(sta.pipeline, "build_sd_v1", lambda *a, **k: pytest.fail("a model was built"))
    monkeypatch.setattr(sys, "argv", ["txt2img-gpt.py", "--synthetic"] + (args if "--opt_epochs" in args else ["--opt_epochs", "0"] + args))
    with pytest.raises(SystemExit) as e:
        cli.run("gpt", "x.json")
    assert what in str(e.value)


def test_img2img_cli_disc_scale(tmp_path, monkeypatch):
    from tests.test_img2img_cpu import _png, _script
    mod = _script()
    p = mod.build_parser(canvas=True)
    assert p.parse_args(["--init-img", "a.png"]).disc_scale == 1.0
    assert not hasattr(mod.build_parser().parse_args([]), "disc_scale")
    opt = p.parse_args(["--init-img", "a.png", "--opt_epochs", "0", "--canvas", "1024x1024", "--disc_scale", "2.0"])
    assert opt.disc_scale == 2.0 and mod.canvas_grid(opt).T == 9
    built = []
    monkeypatch.setattr("sta.pipeline.build_sd_v1", lambda *a, **k: built.append(1))
    img = _png(str(tmp_path / "a.png"), 96, 64)
    for args, what in ((["--disc_scale", "2.0"], "needs --canvas"),
                       (["--canvas", "512x1024", "--canvas_wrap", "x", "--disc_scale", "3"], "wrapped x axis"),
                       (["--canvas", "512x1024", "--disc_scale", "0"], "disc_scale")):
        with pytest.raises(SystemExit) as e:
            mod.main(["--init-img", img, "--synthetic", "--opt_epochs", "0"] + args)
        assert what in str(e.value) and not built
