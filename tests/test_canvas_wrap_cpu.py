"""Wrap-around canvases (360 degree panoramas, tileable images) without a GPU: the ring grid, the per-window centres against the CYCLIC
canvas-level disc, the torch restatements of the window kernels on a ring (fuse of split, roll equivariance), the argument rules of the
five C entry points on a wrapped grid (fake pointers: none of these calls may reach a launch), `sample_canvas(wrap=)` / `inpaint_canvas(wrap=)`
of the samplers on the host miniature, the padded decode and the CLI. The kernels are checked in test_canvas_wrap_gpu.py."""
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
# (Hc, Wc, s, stride, wrap): cover 2 along x (nx = 6) and along y, T = 16 with cover 4 on both axes, cover 4 along x (nx = 8), and a
# ring without overlap (the unwrapped grid's offsets)
SHAPES = [(16, 48, 16, 8, "x"), (48, 16, 16, 8, "y"), (32, 32, 16, 8, "xy"), (32, 64, 32, 8, "x"), (16, 32, 16, 16, "x")]
COVER2 = [SHAPES[0], SHAPES[1], SHAPES[4]]             # at most two covering windows: fp32 a + b commutes, a roll is bit-exact
DTYPES = [torch.float16, torch.bfloat16]
Q_A, Q_B = 0.8253, 0.5647
S_LAT, STEPS, K = 32, 4, 2
FIVE = ("sta_window_split", "sta_window_fuse", "sta_sampler_step_windows", "sta_sampler_step_windows_masked", "sta_window_blend")
WINDOW_ENTRY_POINTS = FIVE + ("sta_vae_encode_step_windows", "sta_latent_guide_windows", "sta_latent_upscale_step_windows")


def _grid(args):
    from sta.canvas import window_grid
    return window_grid(*args)


# ---------------------------------------------------------------------------------------------------
# grid
# ---------------------------------------------------------------------------------------------------
def test_ring_grid_offsets():
    from sta.canvas import Grid, window_grid, windows
    g = window_grid(16, 48, 16, 8, "x")
    assert g.oy == (0,) and g.ox == (0, 8, 16, 24, 32, 40) and (g.ny, g.nx, g.T, g.wrap) == (1, 6, 6, "x")
    g = window_grid(48, 16, 16, 8, wrap="y")
    assert g.ox == (0,) and g.oy == (0, 8, 16, 24, 32, 40) and (g.ny, g.nx, g.T, g.wrap) == (6, 1, 6, "y")
    g = window_grid(32, 32, 16, 8, "xy")
    assert g.oy == g.ox == (0, 8, 16, 24) and g.T == 16 and windows(g)[7] == (8, 24)       # w = j nx + i; window 7 runs over the x seam
    g = window_grid(32, 64, 32, 8, "x")
    assert g.ox == tuple(range(0, 64, 8)) and g.oy == (0,) and g.T == 8
    g = window_grid(16, 32, 16, 16, "x")
    assert g.ox == window_grid(16, 32, 16, 16).ox == (0, 16) and g.T == 2                    # no overlap: the unwrapped offsets
    assert window_grid(16, 128, 16, 8, "x").nx == 16                                         # 16 offsets are the most an axis takes
    assert window_grid(24, 48, 16, 8, "x").oy == (0, 8)                                      # the other axis stays clamped
    # the clamped grids are what they were, and a Grid without the trailing field is one
    for args, oy, ox in (((32, 64, 32, 16), (0,), (0, 16, 32)), ((16, 40, 16, 16), (0,), (0, 16, 24)), ((24, 40, 16, 8), (0, 8), (0, 8, 16, 24))):
        g = window_grid(*args)
        assert g == window_grid(*args, "") == Grid(*args, oy, ox, len(oy), len(ox), len(oy) * len(ox)) and g.wrap == ""
        assert g[:9] == args + (oy, ox, len(oy), len(ox), len(oy) * len(ox))
    assert window_grid(16, 48, 16, 8, "x") != window_grid(16, 48, 16, 8)


@pytest.mark.parametrize("shape", SHAPES + [(24, 48, 16, 8, "x"), (48, 24, 16, 8, "y")])
def test_ring_cover_count_agrees_with_brute_force(shape):
    from sta.canvas import cover_count
    g = _grid(shape)
    n = cover_count(g)
    dist = lambda at, o, L, wrapped: (at - o) % L if wrapped else at - o
    for Y in range(g.Hc):
        for X in range(g.Wc):
            want = sum(1 for oy in g.oy for ox in g.ox
                       if 0 <= dist(Y, oy, g.Hc, "y" in g.wrap) < g.s and 0 <= dist(X, ox, g.Wc, "x" in g.wrap) < g.s)
            assert n[Y, X].item() == want and want >= 1
    if g.Hc in (16, 32, 48) and g.Wc in (16, 32, 48, 64):                 # the five shapes: a constant cover, a power of two
        cover = (g.s // g.stride) ** len(g.wrap)
        assert (n == cover).all() and cover in (1, 2, 4, 16)


@pytest.mark.parametrize("args,numbers", [
    ((16, 40, 16, 16, "x"), ("40", "16", "x")),            # L % stride
    ((40, 16, 16, 16, "y"), ("40", "16", "y")),
    ((32, 56, 32, 24, "x"), ("56", "24")),
    ((16, 136, 16, 8, "x"), ("17", "16")),                 # 17 offsets
    ((136, 16, 16, 8, "y"), ("17", "16")),
    ((16, 16, 16, 8, "x"), ("16", "1.5")),                 # L < 1.5 s
    ((32, 40, 32, 8, "x"), ("40", "32", "1.5")),
    ((40, 32, 32, 8, "xy"), ("40", "32", "1.5")),
    ((16, 48, 16, 8, "z"), ("'z'",)),                      # unknown wrap
    ((16, 48, 16, 8, "yx"), ("'yx'",)),
    ((16, 48, 16, 8, None), ("None",)),
    ((16, 44, 16, 8, "x"), ("44",)),                       # the rules of every grid come first
    ((16, 48, 16, 24, "x"), ("24", "16")),
])
def test_ring_grid_refusals_carry_their_numbers(args, numbers):
    from sta.canvas import window_grid
    with pytest.raises(ValueError) as e:
        window_grid(*args)
    for n in numbers:
        assert n in str(e.value), (args, str(e.value))


# ---------------------------------------------------------------------------------------------------
# layout: the remapped centres rasterise the cyclic canvas-level disc
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 48, 16, 8, "x"), (48, 16, 16, 8, "y"), (32, 32, 16, 8, "xy"), (32, 64, 32, 8, "x"), (32, 128, 32, 32, "x")])
def test_window_masks_equal_the_cyclic_canvas_disc(shape):
    """Centres are multiples of 1/64 in window units and pixels of every level multiples of 1/16, so no pixel lies within 3e-5 of a
    disc's edge ((a^2 + b^2) / 4096 is never within 0.16 / 4096 of 0.04): for every pixel of every level (sides s, s/2, s/4, s/8) of
    every window, the window's mask bit equals the CYCLIC canvas-level disc, the minimum over the images of the centre one axis length
    away on a wrapped axis, evaluated in float64. Two centres lie within 0.2 s of the seam."""
    from sta import ops
    from sta.canvas import window_centres, window_grid, windows
    g = window_grid(*shape)
    s = g.s
    wx, wy = "x" in g.wrap, "y" in g.wrap
    nx64, ny64 = 64 * g.Wc // s, 64 * g.Hc // s                                  # the axis lengths in 1/64 of a window
    ks = [(6, 32), (nx64 - 5, 20), (40, ny64 - 7), (nx64 // 2 + 3, 9), (77 % nx64, 40 % ny64)]
    centres = [(kx / 64.0 * s / g.Wc, ky / 64.0 * s / g.Hc) for kx, ky in ks]
    per_window = window_centres(centres, g)
    assert len(per_window) == g.T and all(len(c) == len(centres) for c in per_window)
    hits = {k: set() for k in range(len(ks))}
    for w, ((y0, x0), wc) in enumerate(zip(windows(g), per_window)):
        for f in (1, 2, 4, 8):
            d = s // f
            got = ops.disc_masks(wc, d).reshape(len(centres), d, d)
            r = torch.arange(d, dtype=torch.float64)
            Y, X = ((y0 + f * r) % g.Hc if wy else y0 + f * r)[:, None], ((x0 + f * r) % g.Wc if wx else x0 + f * r)[None, :]
            for k, (kx, ky) in enumerate(ks):
                dx2 = torch.stack([(X / s - kx / 64.0 - i * g.Wc / s) ** 2 for i in ((-1, 0, 1) if wx else (0,))]).min(0).values
                dy2 = torch.stack([(Y / s - ky / 64.0 - i * g.Hc / s) ** 2 for i in ((-1, 0, 1) if wy else (0,))]).min(0).values
                want = dx2 + dy2 < 0.04
                assert torch.equal(got[k].bool(), want), (y0, x0, f, k)
                if f == 1 and want.any():
                    hits[k].add(w)
    assert all(hits.values())
    if wx:                       # centre 0 lies 6/64 s right of the x seam: windows on both sides of the seam hold bits of it
        first, last = [w for w, (y0, x0) in enumerate(windows(g)) if x0 == 0], [w for w, (y0, x0) in enumerate(windows(g)) if x0 == g.ox[-1]]
        assert hits[0] & set(first) and hits[0] & set(last)
    if wy:
        first, last = [w for w, (y0, x0) in enumerate(windows(g)) if y0 == 0], [w for w, (y0, x0) in enumerate(windows(g)) if y0 == g.oy[-1]]
        assert hits[2] & set(first) and hits[2] & set(last)


def test_centres_take_the_representative_nearest_the_window():
    from sta.canvas import window_centres, window_grid
    g = window_grid(32, 64, 32, 32, "x")
    left, right = window_centres([(0.0625, 0.5), (0.9375, 0.25)], g)              # canvas x = 4 and 60 latent pixels
    assert left == [[0.125, 0.5], [-0.125, 0.25]] and right == [[1.125, 0.5], [0.875, 0.25]]
    plain = window_centres([(0.0625, 0.5), (0.9375, 0.25)], window_grid(32, 64, 32, 32))
    assert plain == [[[0.125, 0.5], [1.875, 0.25]], [[-0.875, 0.5], [0.875, 0.25]]]      # the clamped grid is what it was


# ---------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fuse_of_split_is_the_identity_on_a_ring(shape, dtype):
    """The covers are powers of two (1, 2, 4, 16): the fp32 sum of equal 16-bit values and its division by their count are exact."""
    from sta.canvas import window_fuse_reference, window_split_reference
    g = _grid(shape)
    torch.manual_seed(1)
    x = (torch.randn(2, 4, g.Hc, g.Wc) * 3).to(dtype)
    for src in (x, x.float()):
        xin = window_split_reference(src, g, dtype)
        assert xin.shape == (2 * 2 * g.T, 4, g.s, g.s) and xin.dtype == dtype and torch.equal(xin[0::2], xin[1::2])
        back = window_fuse_reference(xin, g)
        assert back.dtype == dtype and torch.equal(back[0::2], x) and torch.equal(back[1::2], x)
    pair = torch.stack([x, -x], 1).reshape(4, 4, g.Hc, g.Wc)                   # rows = 2: row r goes to row r
    xin = window_split_reference(pair, g, dtype, rows=2)
    assert torch.equal(xin[1::2], -xin[0::2]) and torch.equal(window_fuse_reference(xin, g), pair)
    # the last window of canvas 1 by hand: it runs over the seam of every wrapped axis
    y0, x0 = g.oy[-1], g.ox[-1]
    ys, xs = [(y0 + d) % g.Hc for d in range(g.s)], [(x0 + d) % g.Wc for d in range(g.s)]
    if g.stride < g.s:
        assert ("x" in g.wrap and xs[-1] < xs[0]) or ("y" in g.wrap and ys[-1] < ys[0])
    assert torch.equal(xin[2 * (g.T + g.T - 1)], x[1][:, ys][:, :, xs])


def _roll_canvas(t, g, ky, kx):
    return None if t is None else t.roll((ky * g.stride, kx * g.stride), (-2, -1))


def _roll_windows(t, g, ky, kx):
    """[2 P T, C, s, s] with the windows of every canvas moved ky places along j and kx places along i, cyclically."""
    if t is None:
        return None
    return t.reshape(-1, g.ny, g.nx, 2, *t.shape[1:]).roll((ky, kx), (1, 2)).reshape(t.shape)


@pytest.mark.parametrize("shape", COVER2)
@pytest.mark.parametrize("dtype", DTYPES)
def test_restatements_are_roll_equivariant(shape, dtype):
    """Rolling every canvas tensor by k strides along the wrapped axis and moving the windows k places round the ring rolls every
    output of the five restatements, bit for bit (at most two covering windows: their fp32 sum does not depend on the order)."""
    from sta import canvas, solver
    from tests.test_solver_gpu import _case
    g = _grid(shape)
    P = 2
    torch.manual_seed(5)
    r = lambda: torch.randn(P, 4, g.Hc, g.Wc)
    eps = torch.randn(2 * P * g.T, 4, g.s, g.s).to(dtype)
    x, m_prev, noise, x0, qn = r() * 3, r(), r(), r(), r()
    keep = (torch.rand(P, 1, g.Hc, g.Wc) * 1.5).clamp(max=1.0).round(decimals=1)
    for k in (1, max(g.ny, g.nx) - 1):
        ky, kx = k if "y" in g.wrap else 0, k if "x" in g.wrap else 0
        rc, rw = lambda t: _roll_canvas(t, g, ky, kx), lambda t: _roll_windows(t, g, ky, kx)
        assert torch.equal(canvas.window_split_reference(rc(x), g, dtype), rw(canvas.window_split_reference(x, g, dtype)))
        assert torch.equal(canvas.window_fuse_reference(rw(eps), g), rc(canvas.window_fuse_reference(eps, g)))
        bl, bl_r = solver.Blend(x0, keep, qn, Q_A, Q_B), solver.Blend(rc(x0), rc(keep), rc(qn), Q_A, Q_B)
        for mode in ("first", "second", "noise"):
            c = _case(mode)
            a = canvas.step_windows_reference(eps, x, m_prev, noise, c, g, want_xin=True)
            b = canvas.step_windows_reference(rw(eps), rc(x), rc(m_prev), rc(noise), c, g, want_xin=True)
            assert torch.equal(b[0], rc(a[0])) and torch.equal(b[1], rc(a[1])) and torch.equal(b[2], rw(a[2])), mode
            a = canvas.step_windows_masked_reference(eps, x, m_prev, noise, c, bl, g, want_xin=True)
            b = canvas.step_windows_masked_reference(rw(eps), rc(x), rc(m_prev), rc(noise), c, bl_r, g, want_xin=True)
            assert torch.equal(b[0], rc(a[0])) and torch.equal(b[1], rc(a[1])) and torch.equal(b[2], rw(a[2])), mode
        a, b = canvas.window_blend_reference(x, bl, g, dtype, want_xin=True), canvas.window_blend_reference(rc(x), bl_r, g, dtype, want_xin=True)
        assert torch.equal(b[0], rc(a[0])) and torch.equal(b[1], rw(a[1]))
        assert not torch.equal(rc(x), x) and not torch.equal(rw(eps), eps)


def test_ring_without_overlap_is_the_clamped_grid():
    from sta import canvas
    from tests.test_solver_gpu import _case
    ring, plain = _grid((16, 32, 16, 16, "x")), _grid((16, 32, 16, 16))
    torch.manual_seed(6)
    eps = torch.randn(2 * 2 * 2, 4, 16, 16).to(torch.float16)
    x, m_prev = torch.randn(2, 4, 16, 32) * 3, torch.randn(2, 4, 16, 32)
    for a, b in zip(canvas.step_windows_reference(eps, x, m_prev, None, _case("second"), ring, want_xin=True),
                    canvas.step_windows_reference(eps, x, m_prev, None, _case("second"), plain, want_xin=True)):
        assert torch.equal(a, b)


def test_fuse_on_a_ring_agrees_with_an_fp64_mean():
    """Cover 4 along x: half a unit in the last place of fp16 plus the fp32 accumulation's own error (3 adds and a division)."""
    from sta.canvas import window_fuse_reference, windows
    g = _grid((32, 64, 32, 8, "x"))
    torch.manual_seed(2)
    eps = torch.randn(2 * g.T, 4, g.s, g.s).to(torch.float16)
    got = window_fuse_reference(eps, g)
    acc, mag = torch.zeros(2, 4, g.Hc, g.Wc, dtype=torch.float64), torch.zeros(2, 4, g.Hc, g.Wc, dtype=torch.float64)
    for w, (y0, x0) in enumerate(windows(g)):
        for d in range(g.s):
            acc[..., :, (x0 + d) % g.Wc] += eps[2 * w:2 * w + 2, :, :, d].double()
            mag[..., :, (x0 + d) % g.Wc] += eps[2 * w:2 * w + 2, :, :, d].double().abs()
    err = (got.double() - acc / 4).abs()
    assert (err <= 2.0 ** -11 * (acc / 4).abs() + 4 * 2.0 ** -24 * mag / 4 + 2.0 ** -25).all()


# ---------------------------------------------------------------------------------------------------
# C-ABI
# ---------------------------------------------------------------------------------------------------
def _ints(v):
    a = (ctypes.c_int * len(v))(*v)
    return a, ctypes.addressof(a)


def _call(L, name, **kw):
    a = dict(src=PTR, xin=PTR + 0x100000, eps=PTR, out=PTR + 0x100000, x=PTR + 0x200000, m_prev=PTR + 0x300000, noise=PTR + 0x400000,
             x_next=PTR + 0x500000, m=PTR + 0x600000, x0=PTR + 0x700000, keep=PTR + 0x800000, qnoise=PTR + 0x900000, P=1, rows=1, C=4, Hc=16,
             Wc=48, oy=(0,), ox=(0, 8, 16, 24, 32, 40), s=16, wrap=1, src_dtype=2, dtype=0, alpha_t=0.8)
    a.update(kw)
    keep_y, oy = _ints(a["oy"]) if a["oy"] is not None else (None, 0)
    keep_x, ox = _ints(a["ox"]) if a["ox"] is not None else (None, 0)
    ny, nx = a.get("ny", len(a["oy"] or ())), a.get("nx", len(a["ox"] or ()))
    grid = (ny, nx, oy, ox, a["s"], a["wrap"])
    coef = (7.5, 0.5, a["alpha_t"], 1.0, 0.1, 0.0, 0.2, 0.0)
    if name == "sta_window_split":
        rc = L.sta_window_split(a["src"], a["xin"], a["P"], a["rows"], a["C"], a["Hc"], a["Wc"], *grid, a["src_dtype"], a["dtype"], None)
    elif name == "sta_window_fuse":
        rc = L.sta_window_fuse(a["eps"], a["out"], a["P"], a["C"], a["Hc"], a["Wc"], *grid, a["dtype"], None)
    elif name == "sta_sampler_step_windows":
        rc = L.sta_sampler_step_windows(a["eps"], a["x"], a["m_prev"], a["noise"], a["x_next"], a["m"], a["xin"], a["P"], a["C"], a["Hc"],
                                        a["Wc"], *grid, *coef, a["dtype"], None)
    elif name == "sta_sampler_step_windows_masked":
        rc = L.sta_sampler_step_windows_masked(a["eps"], a["x"], a["m_prev"], a["noise"], a["x0"], a["keep"], a["qnoise"], a["x_next"],
                                               a["m"], a["xin"], a["P"], a["C"], a["Hc"], a["Wc"], *grid, *coef, Q_A, Q_B, a["dtype"], None)
    else:
        rc = L.sta_window_blend(a["x"], a["x0"], a["keep"], a["qnoise"], a["x_next"], a["xin"], a["P"], a["C"], a["Hc"], a["Wc"], *grid,
                                Q_A, Q_B, a["dtype"], None)
    return rc, L.sta_last_error().decode()


def test_ring_abi_symbols_and_signatures():
    """One entry point per launch: `int wrap` directly after s in each of them, no `_ring` sibling left in the binding table, the header
    or the library."""
    from sta import lib
    L = lib.load()
    vp, i, f, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    grid = [i, i, vp, vp, i, i]                                                 # ny, nx, oy, ox, s, wrap
    assert lib.SYMBOLS["sta_window_split"] == (i, [vp, vp, l, i, i, i, i] + grid + [i, i, vp])
    assert lib.SYMBOLS["sta_window_fuse"] == (i, [vp, vp, l, i, i, i] + grid + [i, vp])
    assert lib.SYMBOLS["sta_sampler_step_windows"] == (i, [vp] * 7 + [l, i, i, i] + grid + [f] * 8 + [i, vp])
    assert lib.SYMBOLS["sta_sampler_step_windows_masked"] == (i, [vp] * 10 + [l, i, i, i] + grid + [f] * 10 + [i, vp])
    assert lib.SYMBOLS["sta_window_blend"] == (i, [vp] * 6 + [l, i, i, i] + grid + [f, f, i, vp])
    assert not [name for name in lib.SYMBOLS if name.endswith("_ring")]
    for name in WINDOW_ENTRY_POINTS:
        args = lib.SYMBOLS[name][1]
        assert [args[k:k + 6] for k in range(len(args) - 5)].count(grid) == 1, name            # the grid with its wrap, once
        assert getattr(L, name).argtypes == args and getattr(L, name).restype is i
        assert not hasattr(L, name + "_ring"), name                             # the library exports no sibling
    header = " ".join(open(os.path.join(ROOT, "include", "sta_unet.h")).read().split())
    for decl in ("int sta_window_split(const void* src, void* xin, long P, int rows, int C, int Hc, int Wc, int ny, int nx, const int* oy, "
                 "const int* ox, int s, int wrap, int src_dtype, int dtype, void* stream);",
                 "int sta_window_fuse(const void* eps, void* out, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, "
                 "const int* ox, int s, int wrap, int dtype, void* stream);",
                 "int sta_sampler_step_windows(const void* eps, const float* x, const float* m_prev, const float* noise, float* x_next, "
                 "float* m, void* xin, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, "
                 "float scale, float sigma_t, float alpha_t, float c_x, float c_m, float c_p, float c_e, float c_n, int dtype, void* stream);",
                 "int sta_sampler_step_windows_masked(const void* eps, const float* x, const float* m_prev, const float* noise, "
                 "const float* x0, const float* keep, const float* qnoise, float* x_next, float* m, void* xin, long P, int C, int Hc, int Wc, "
                 "int ny, int nx, const int* oy, const int* ox, int s, int wrap, float scale, float sigma_t, float alpha_t, float c_x, "
                 "float c_m, float c_p, float c_e, float c_n, float q_a, float q_b, int dtype, void* stream);",
                 "int sta_window_blend(const float* x, const float* x0, const float* keep, const float* noise, float* x_out, void* xin, "
                 "long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, float q_a, float q_b, "
                 "int dtype, void* stream);"):
        assert decl in header, decl
    assert "_ring(" not in header
    assert "`int wrap` directly after s" in header.split("#define STA_MAX_WINDOW_OFFSETS")[0]   # documented in the section's comment block
    assert L.sta_version() == 0x000600
    for want in ("window_split_kernel", "window_fuse_kernel", "sampler_step_windows_kernel", "sampler_step_windows_masked_kernel",
                 "window_blend_kernel"):                                        # by substring: every wrap instantiation falls under the rule
        assert want in lib.NO_SPILL_KERNELS["sta_sampler.hip"]


@pytest.mark.parametrize("name", FIVE)
def test_ring_argument_rules_reach_no_launch(name):
    """Every rule of a wrapped axis -> STA_E_ARG with its numbers; the rules of a non-wrapped axis are the clamped grid's; an accepted
    grid is shown by the refusal that comes after the grid's (dtype 7), never by a launch. The texts carry the entry point's name."""
    from sta import lib
    L = lib.load()
    ring6, ring17 = (0, 8, 16, 24, 32, 40), tuple(range(0, 136, 8))
    refused = [
        (dict(wrap=4), "wrap=4"), (dict(wrap=-1), "wrap=-1"), (dict(wrap=7), "wrap=7"),
        (dict(ox=(8, 16, 24, 32, 40)), "ox[0]=8 unsorted"),                                    # the first offset is 0
        (dict(ox=(0, 8, 12, 24, 32, 40)), "ox[2]=12 is not a multiple of 8"),
        (dict(ox=(0, 16, 8, 24, 32, 40)), "ox[2]=8 unsorted"),
        (dict(ox=(0, 16, 16, 32)), "ox[2]=16 unsorted"),
        (dict(ox=(0, 16, 32, 48)), "ox[3]=48 is not on the wrapped axis (length 48)"),         # every offset < L
        (dict(ox=(0, -8, 16, 32)), "ox[1]=-8 is not on the wrapped axis"),
        (dict(ox=(0, 24, 40)), "gap between ox[0]=0 and ox[1]=24 (s=16)"),                     # consecutive ones at most s apart
        (dict(ox=(0, 16)), "the ring does not close behind ox[1]=16 (s=16, wrapped length 48)"),   # L - o[n - 1] <= s
        (dict(ox=(0,)), "the ring does not close behind ox[0]=0"),
        (dict(Wc=8, ox=(0,)), "s=16 Hc=16 Wc=8"),                                              # s <= L
        (dict(ox=(), nx=0), "nx=0"),
        (dict(ox=ring17, Wc=136), "nx=17"),
        (dict(oy=(0, 8)), "oy[1]=8 out of range"),                                             # y is not wrapped: today's rules and texts
        (dict(oy=(8,)), "oy[0]=8 out of range"),
        (dict(wrap=2), "ox[5]=40 out of range (s=16, length 48)"),                             # x is not wrapped under wrap = 2
        (dict(wrap=0), "ox[5]=40 out of range"),
        (dict(wrap=0, ox=(0, 16)), "gap behind ox[1]=16"),
        (dict(wrap=2, ox=(0,), Wc=16, Hc=48, oy=(0, 16)), "the ring does not close behind oy[1]=16"),
        (dict(wrap=3, ox=(0,), Wc=16, Hc=48, oy=(0, 16, 32, 48)), "oy[3]=48 is not on the wrapped axis"),
        (dict(wrap=3, Hc=48, oy=(0, 16, 32), ox=(0, 24, 40)), "gap between ox[0]=0 and ox[1]=24"),
        (dict(oy=None), "null pointer"), (dict(ox=None), "null pointer"), (dict(P=0), "P=0"), (dict(C=0), "C=0"), (dict(Wc=44), "Wc=44"),
        (dict(s=12), "s=12"),
    ]
    for kw, text in refused:
        rc, err = _call(L, name, **kw)
        assert rc == STA_E_ARG and text in err, (name, kw, rc, err)
        assert err == "null pointer" or err.startswith(name[len("sta_"):] + ": "), (name, kw, err)
    accepted = [dict(), dict(ox=(0, 16, 32)), dict(ox=(0, 16, 24, 40)), dict(ox=(0, 8, 24, 32)),       # o + s > L is allowed
                dict(ox=tuple(range(0, 128, 8)), Wc=128),                                              # 16 offsets
                dict(wrap=2, ox=(0,), Wc=16, Hc=48, oy=ring6), dict(wrap=3, Hc=48, oy=ring6), dict(wrap=3, Hc=32, Wc=32, oy=(0, 8, 16, 24), ox=(0, 8, 16, 24)),
                dict(wrap=0, ox=(0, 16, 32)), dict(wrap=1, Wc=16, ox=(0,)), dict(wrap=2, ox=(0, 16, 32))]
    for kw in accepted:
        rc, err = _call(L, name, dtype=7, **kw)
        assert rc == STA_E_UNSUP and err == "dtype 7", (name, kw, rc, err)
    rc, err = _call(L, name, **{dict(sta_window_split="src", sta_window_fuse="eps", sta_window_blend="x").get(name, "eps"): 0})
    assert rc == STA_E_ARG and "null pointer" in err
    if "masked" in name or "blend" in name:
        rc, err = _call(L, name, keep=0)
        assert rc == STA_E_ARG and "null pointer" in err
    rc, err = _call(L, name, **{"out" if name == "sta_window_fuse" else "xin": PTR + 0x100008})       # an output each of the five takes
    assert rc == STA_E_ARG and "16-byte aligned" in err


# ---------------------------------------------------------------------------------------------------
# samplers on the host miniature (the helpers of tests/test_canvas_cpu.py)
# ---------------------------------------------------------------------------------------------------
_MODEL = []
KINDS = ["plms", "ddim", "dpm"]
CANVAS = (S_LAT, 2 * S_LAT)
CENTRES = [[0.25, 0.4], [0.625, 0.6]]                  # 16 and 40 of 64 latent pixels: no disc reaches the seam


def _sampler(kind, **kw):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    from tests.test_solver_cpu import _model
    if not _MODEL:
        _MODEL.append(_model()[0])
    cls = dict(ddim=DDIMSampler, plms=PLMSSampler, dpm=DPMSolverSampler)[kind]
    return cls(_MODEL[0], **dict(dict(loss_model=None, opt_epochs=0, use_graph=False, save_images=False), **kw))


def _inputs():
    c, local_ctx, xa = gi.unet_inputs(K, 5)
    return c, local_ctx, torch.cat([xa, gi.unet_inputs(K, 6)[2]], dim=3)


def _canvas(sampler, canvas, stride, centres, x_T, c, local_ctx, method="sample_canvas", **kw):
    with oracle_ops():
        getattr(sampler, method)(**dict(dict(S=STEPS, canvas=canvas, window=S_LAT, stride=stride, conditionings=[c],
                                             unconditional_conditionings=gi.load_uncond(), bboxs=[centres], object_names=[["cat", "dog"]],
                                             local_conditionings=[local_ctx], x_T=x_T, unconditional_guidance_scale=7.5, eta=0.0, seed=1), **kw))
    assert sampler._canvas is None
    return sampler.last_result["x0"].clone()


_RING = {}


def _ring_canvas(kind):
    """sample_canvas(wrap="x") on the 32 x 64 canvas with stride 16 (T = 4, the last window runs over the seam), once per sampler."""
    if kind not in _RING:
        c, local_ctx, x_T = _inputs()
        _RING[kind] = _canvas(_sampler(kind), CANVAS, 16, CENTRES, x_T, c, local_ctx, wrap="x")
    return _RING[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_ring_without_overlap_equals_sample_canvas(kind):
    """Stride 32 on 32 x 64: the wrapped grid has the clamped grid's offsets and no disc reaches the seam, so every window sees the same
    masks: bit for bit the unwrapped `sample_canvas`."""
    c, local_ctx, x_T = _inputs()
    got = _canvas(_sampler(kind), CANVAS, S_LAT, CENTRES, x_T, c, local_ctx, wrap="x")
    want = _canvas(_sampler(kind), CANVAS, S_LAT, CENTRES, x_T, c, local_ctx)
    assert torch.isfinite(got).all() and got.abs().max() > 0 and torch.equal(got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_sample_canvas_on_a_ring_is_roll_equivariant(kind):
    """x_T rolled by one stride along x and the centres moved by stride / Wc (the second disc then crosses the seam): the rolled result,
    to the 1e-5 of max that tests/test_canvas_cpu.py allows its host-chain comparisons (the windows change places in the UNet batch)."""
    c, local_ctx, x_T = _inputs()
    base = _ring_canvas(kind)
    moved = [[(x + 16 / 64) % 1.0, y] for x, y in CENTRES]
    assert moved == [[0.5, 0.4], [0.875, 0.6]]
    got = _canvas(_sampler(kind), CANVAS, 16, moved, x_T.roll(16, -1), c, local_ctx, wrap="x")
    err = (got - base.roll(16, -1)).abs().max().item()
    print("%s: max |rolled run - roll of the run| = %.3g of max %.3g" % (kind, err, base.abs().max().item()))
    assert torch.isfinite(got).all() and err <= 1e-5 * base.abs().max().item()
    assert (got - base).abs().max() > 0.05 * base.abs().max()                   # and it is not the unrolled one


def test_a_ring_differs_from_the_clamped_canvas_and_the_unfused_step_agrees():
    c, local_ctx, x_T = _inputs()
    ring = _ring_canvas("ddim")
    plain = _canvas(_sampler("ddim"), CANVAS, 16, CENTRES, x_T, c, local_ctx)
    assert (ring - plain).abs().max() > 0.01 * plain.abs().max()               # the first and last columns share a window now
    unfused = _canvas(_sampler("ddim", canvas_fused_step=False), CANVAS, 16, CENTRES, x_T, c, local_ctx, wrap="x")
    assert (unfused - ring).abs().max() <= 1e-5 * ring.abs().max()


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_inpaint_canvas_on_a_ring_with_nothing_kept_is_sample_canvas(kind):
    c, local_ctx, x_T = _inputs()
    draws = [torch.randn((1, 4) + CANVAS, generator=torch.Generator().manual_seed(7 + i)) for i in range(STEPS)]
    got = _canvas(_sampler(kind, mask_noise=draws), CANVAS, 16, CENTRES, x_T, c, local_ctx, method="inpaint_canvas", wrap="x",
                  mask=torch.zeros((1, 1) + CANVAS), x0=torch.randn((1, 4) + CANVAS))
    assert torch.equal(got, _ring_canvas(kind))


def test_ring_refusals_come_before_any_unet_call():
    c, local_ctx, x_T = _inputs()
    calls = []

    def run(kind="ddim", skw=None, canvas=CANVAS, stride=16, method="sample_canvas", margin=None, **kw):
        sampler = _sampler(kind, **(skw or {}))
        if margin is not None:
            sampler.canvas_wrap_margin = margin
        sampler.model.apply_model_extra = lambda *a, **k: calls.append(1)
        try:
            return _canvas(sampler, canvas, stride, CENTRES, x_T, c, local_ctx, method=method, **kw)
        finally:
            del sampler.model.apply_model_extra
            assert sampler._canvas is None and getattr(sampler, "_inpaint", None) is None
    masked = dict(method="inpaint_canvas", mask=torch.zeros((1, 1) + CANVAS), x0=x_T)
    for extra in (dict(), masked):
        with pytest.raises(ValueError, match="'z'"):
            run(wrap="z", **extra)
        with pytest.raises(ValueError, match="64 is not a multiple of the stride 24"):
            run(stride=24, wrap="x", **extra)
        with pytest.raises(ValueError, match="1.5 windows"):
            run(wrap="y", **extra)                                                # 32 rows of 32-row windows
        with pytest.raises(ValueError, match="canvas_wrap_margin = 72"):
            run(wrap="x", margin=72, **extra)
        with pytest.raises(ValueError, match="canvas_wrap_margin = -1"):
            run(wrap="x", margin=-1, **extra)
    # what a canvas refuses, it refuses on a ring
    with pytest.raises(ValueError, match="opt_epochs = 2"):
        run(wrap="x", skw=dict(opt_epochs=2))
    for name in ("attn_capture", "attn_loss", "latent_guidance"):
        with pytest.raises(ValueError, match=name):
            run(wrap="x", skw={name: object()})
    with pytest.raises(ValueError, match="mask="):
        run(wrap="x", mask=torch.zeros((1, 1) + CANVAS), x0=x_T)
    with pytest.raises(ValueError, match="x_T"):
        run(wrap="x", canvas=(S_LAT, 3 * S_LAT))
    with pytest.raises(NotImplementedError, match="inpainting"):
        run("plms", wrap="x", **masked)
    assert not calls


# ---------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------
def _stub(S, **attrs):
    from tests.test_img2img_cpu import _stub_sampler
    s, calls = _stub_sampler(S=S)
    for k, v in attrs.items():
        setattr(s, k, v)
    return s, calls


def _stub_canvas(s, S, canvas, x_T, wrap, method="sample_canvas", **kw):
    cond = torch.zeros(1, 77, 8)
    getattr(s, method)(S=S, canvas=canvas, window=16, stride=8, conditionings=[cond], unconditional_conditionings=cond,
                       bboxs=[[[0.3, 0.4], [0.7, 0.6]]], object_names=[["cat", "dog"]], local_conditionings=[[cond, cond]], x_T=x_T,
                       unconditional_guidance_scale=7.5, eta=0.0, seed=0, wrap=wrap, **kw)
    return s.last_result["x0"].clone(), s.last_result["image"].clone()


@pytest.mark.parametrize("canvas,wrap,margin", [((16, 48), "x", 8), ((48, 16), "y", 8), ((32, 32), "xy", 8), ((16, 48), "x", 3),
                                                ((16, 48), "x", 48), ((16, 48), "x", 0), ((16, 48), "", 8)])
def test_decode_of_a_ring_is_pad_decode_crop(canvas, wrap, margin):
    """One decode, of the latent padded circularly by the margin on both sides of every wrapped axis; the image is the crop of 8 margin
    pixels per side. Margin 0, or no wrap: the latent itself."""
    S = 4
    s, _ = _stub(S, canvas_wrap_margin=margin)
    seen, inner = [], s.model.first_stage_model.decode
    s.model.first_stage_model.decode = lambda z: (seen.append(z.clone()), inner(z))[1]
    x0, image = _stub_canvas(s, S, canvas, torch.randn((1, 4) + canvas), wrap)
    Hc, Wc = canvas
    mx, my = margin if "x" in wrap else 0, margin if "y" in wrap else 0
    padded = torch.cat([x0[..., Wc - mx:], x0, x0[..., :mx]], dim=-1)
    padded = torch.cat([padded[..., Hc - my:, :], padded, padded[..., :my, :]], dim=-2)
    assert len(seen) == 1 and seen[0].shape == (1, 4, Hc + 2 * my, Wc + 2 * mx)
    scale = (seen[0] / padded).flatten()[0]                                      # decode_first_stage's own 1 / scale_factor
    assert torch.allclose(seen[0], padded * scale, rtol=1e-6, atol=0)
    dec = inner(seen[0])
    want = torch.clamp((dec[..., 8 * my:8 * (my + Hc), 8 * mx:8 * (mx + Wc)] + 1.0) / 2.0, min=0.0, max=1.0)
    assert image.shape == (1, 3, 8 * Hc, 8 * Wc) and torch.equal(image, want)


def _smear(z):
    """A decoder stand-in that knows nothing of the wrap: nearest upsampling, then a 33-tap blur along both axes with zeros beyond its
    input's border (sums of shifted copies: the same arithmetic at every position)."""
    u = torch.nn.functional.interpolate(z[:, :3], scale_factor=8.0)
    for dim in (-1, -2):
        n, pad = u.shape[dim], [0, 0, 0, 0]
        pad[0 if dim == -1 else 2] = pad[1 if dim == -1 else 3] = 16
        p = torch.nn.functional.pad(u, pad)
        u = sum((1.0 + 0.1 * k) * p.narrow(dim, k, n) for k in range(33)) / 33.0
    return 0.2 * u


@pytest.mark.parametrize("canvas,wrap", [((16, 48), "x"), ((32, 32), "xy")])
def test_a_rolled_latent_decodes_to_the_rolled_image(canvas, wrap):
    """The blur reaches 16 pixels, the default margin gives it 64 of the other side: a latent rolled along a wrapped axis decodes to the
    rolled image, bit for bit; without the padding (margin 0) it does not. The stub trajectory is elementwise, so the rolled x_T gives
    the rolled latent exactly (cover 2 per axis here only for (16, 48); (32, 32) has cover 4 and its latents are compared to 1e-6)."""
    S = 4
    x_T = torch.randn((1, 4) + canvas, generator=torch.Generator().manual_seed(3))
    shift, dims = ((8,), (-1,)) if wrap == "x" else ((8, 16), (-1, -2))

    def run(x, margin):
        s, _ = _stub(S, canvas_wrap_margin=margin)
        s.model.first_stage_model.decode = _smear
        return _stub_canvas(s, S, canvas, x, wrap)
    for margin, same in ((8, True), (0, False)):
        x0, image = run(x_T, margin)
        x0_r, image_r = run(x_T.roll(shift, dims), margin)
        if wrap == "x":
            assert torch.equal(x0_r, x0.roll(shift, dims))
            assert torch.equal(image_r, image.roll(tuple(8 * k for k in shift), dims)) == same
        else:
            assert torch.allclose(x0_r, x0.roll(shift, dims), rtol=0, atol=1e-6 * float(x0.abs().max()))
            close = torch.allclose(image_r, image.roll(tuple(8 * k for k in shift), dims), rtol=0, atol=1e-5)
            assert close == same
        assert image.std() > 0.01


def test_pixel_paste_runs_on_the_cropped_image():
    from sta import solver
    S, canvas = 4, (16, 48)
    draws = [torch.randn((1, 4) + canvas, generator=torch.Generator().manual_seed(5 + i)) for i in range(S)]
    s, _ = _stub(S, mask_noise=draws)
    keep = torch.zeros((1, 1) + canvas)
    keep[..., 4:12, 40:] = 1.0                                                   # a footprint on the right border, at the seam
    keep_px = keep.repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)
    orig = torch.rand(1, 3, 128, 384, generator=torch.Generator().manual_seed(6))
    x0, image = _stub_canvas(s, S, canvas, torch.randn((1, 4) + canvas), "x", method="inpaint_canvas", mask=keep, x0=torch.randn((1, 4) + canvas),
                             image=orig, mask_px=keep_px)
    dec = s.model.decode_first_stage(torch.cat([x0[..., -8:], x0, x0[..., :8]], dim=-1))[..., 64:-64]
    assert image.shape == orig.shape and torch.equal(image, solver.image_composite_reference(dec, orig, keep_px))
    assert torch.equal(image[..., 32:96, 320:], orig[..., 32:96, 320:])


# ---------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------
def test_cli_canvas_wrap_parses_and_refuses(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts"))
    import _txt2img_common as cli
    import sta.pipeline
    monkeypatch.setattr(sta.pipeline, "build_sd_v1", lambda *a, **k: pytest.fail("a model was built"))
    p = cli.build_parser("x.json")
    opt = p.parse_args(["--opt_epochs", "0", "--canvas", "512x2048"])
    assert opt.canvas_wrap is None and cli.canvas_grid(opt).wrap == "" and cli.canvas_grid(opt).T == 7
    opt = p.parse_args(["--opt_epochs", "0", "--canvas", "512x2048", "--canvas_wrap", "x"])
    cli.check_options(opt)
    g = cli.canvas_grid(opt)
    assert (g.Hc, g.Wc, g.s, g.stride, g.T, g.wrap) == (64, 256, 64, 32, 8, "x") and g.ox == tuple(range(0, 256, 32))
    g = cli.canvas_grid(p.parse_args(["--opt_epochs", "1", "--canvas", "1024x512", "--canvas_stride", "128", "--canvas_wrap", "y", "--plms"]))
    assert (g.ny, g.nx, g.stride, g.wrap) == (8, 1, 16, "y")
    g = cli.canvas_grid(p.parse_args(["--opt_epochs", "0", "--canvas", "768x1024", "--canvas_wrap", "xy", "--dpm_solver"]))
    assert (g.ny, g.nx, g.T, g.wrap) == (3, 4, 12, "xy")
    with pytest.raises(SystemExit):                                              # argparse: not one of x, y, xy
        p.parse_args(["--canvas", "512x2048", "--canvas_wrap", "z"])
    for bad, text in ((["--canvas_wrap", "x"], "--canvas_wrap x needs --canvas"),
                      (["--canvas", "512x2048", "--canvas_stride", "384", "--canvas_wrap", "x"], "256 is not a multiple of the stride 48"),
                      (["--canvas", "1280x512", "--canvas_stride", "384", "--canvas_wrap", "y"], "160 is not a multiple of the stride 48"),
                      (["--canvas", "512x512", "--canvas_wrap", "x"], "1.5 windows"),
                      (["--canvas", "512x2048", "--canvas_wrap", "y"], "1.5 windows"),
                      (["--canvas", "512x2048", "--canvas_wrap", "xy"], "1.5 windows"),
                      (["--canvas", "512x8192", "--canvas_stride", "64", "--canvas_wrap", "x"], "at most 16"),
                      (["--canvas", "512x2048", "--canvas_wrap", "x", "--attn_maps"], "--attn_maps")):
        with pytest.raises(SystemExit, match=text):
            cli.check_options(p.parse_args(["--opt_epochs", "0"] + bad))
    with pytest.raises(SystemExit, match="--opt_epochs"):
        cli.check_options(p.parse_args(["--opt_epochs", "3", "--canvas", "512x2048", "--canvas_wrap", "x", "--clip", "synthetic"]))


def _script():
    import importlib.util
    path = os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts", "outpaint.py")
    spec = importlib.util.spec_from_file_location("outpaint_script_wrap", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules.pop("img2img", None)          # the script's sibling import: keep it out of other tests' namespace
    return mod


def test_outpaint_on_a_ring_erodes_the_seam_on_wrapped_borders():
    mod = _script()
    p = mod.build_parser()
    opt = p.parse_args(["--init-img", "a.png", "--canvas", "256x512", "--H", "256", "--W", "256", "--canvas_wrap", "x", "--seam", "16"])
    g, place = mod.check_options(opt)
    assert (g.Hc, g.Wc, g.s, g.stride, g.T, g.wrap) == (32, 64, 32, 16, 4, "x") and place == (0, 0)
    assert mod.check_options(p.parse_args(["--init-img", "a.png", "--canvas", "256x512", "--H", "256", "--W", "256"]))[0].wrap == ""
    # on the left border of a wrapped x axis both vertical sides are eroded (2 cells each); top and bottom lie on real borders
    keep, keep_px, at = mod.keep_masks(256, (0, 0), 16, g, 8)
    want = torch.zeros(1, 1, 32, 64)
    want[:, :, :, 2:30] = 1.0
    assert torch.equal(keep, want) and at == (0, 0) and keep_px.sum() == 256 * 224 and keep_px[0, 0, :, 16:240].min() == 1
    keep, _, at = mod.keep_masks(256, (256, 0), 16, g, 8)                        # and on the right border
    want = torch.zeros(1, 1, 32, 64)
    want[:, :, :, 34:62] = 1.0
    assert torch.equal(keep, want) and at == (0, 32)
    plain = _grid((32, 64, 32, 16))
    assert mod.keep_masks(256, (0, 0), 16, plain, 8)[0][0, 0, :, :30].min() == 1      # the clamped canvas keeps its border side
    # y wrapped: top and bottom are eroded on the borders, the vertical sides only inside
    tall = _grid((64, 32, 32, 16, "y"))
    keep, keep_px, at = mod.keep_masks(256, (0, 256), 8, tall, 8)
    assert at == (32, 0) and keep.sum() == 30 * 32 and keep[0, 0, 33:63].min() == 1 and keep[0, 0, 63].max() == 0
    # a footprint that would cross the seam is refused like one outside the canvas
    with pytest.raises(SystemExit, match="does not lie inside"):
        mod.keep_masks(256, (384, 0), 16, g, 8)
    with pytest.raises(SystemExit, match="does not lie inside"):
        mod.keep_masks(256, (0, 384), 8, tall, 8)
    with pytest.raises(SystemExit, match="nothing of the 256 x 256 picture kept"):
        mod.keep_masks(256, (0, 0), 128, g, 8)
    for bad, text in ((["--canvas", "256x256", "--canvas_wrap", "x"], "1.5 windows"),
                      (["--canvas", "256x640", "--canvas_stride", "192", "--canvas_wrap", "x"], "80 is not a multiple of the stride 24"),
                      (["--canvas_wrap", "x"], "needs --canvas")):
        with pytest.raises(SystemExit, match=text):
            mod.check_options(p.parse_args(["--init-img", "a.png", "--H", "256", "--W", "256"] + bad))
