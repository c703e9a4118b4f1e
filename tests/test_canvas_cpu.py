"""Wide canvases as overlapping windows without a GPU: the window grid, the per-window centres against the canvas-level disc, the torch
restatements of the window kernels (sta.canvas), the refusals of the three C entry points (fake pointers: none of these calls may reach a
launch), `sample_canvas` of the three samplers on the host miniature (oracle-backed blocks, golden-width UNet, fp32) and the CLI. The
kernels are checked in test_canvas_gpu.py."""
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
GRIDS = [(32, 64, 32, 16), (16, 40, 16, 16), (24, 40, 16, 8)]
S_LAT, STEPS, K = 32, 4, 2


# ---------------------------------------------------------------------------------------------------
# grid
# ---------------------------------------------------------------------------------------------------
def test_window_grid_offsets():
    from sta.canvas import window_grid, windows
    g = window_grid(32, 64, 32, 16)
    assert g.oy == (0,) and g.ox == (0, 16, 32) and (g.ny, g.nx, g.T) == (1, 3, 3)
    g = window_grid(16, 40, 16, 16)
    assert g.ox == (0, 16, 24) and g.oy == (0,) and g.T == 3                   # the last window is clamped to the edge
    g = window_grid(24, 40, 16, 8)
    assert (g.ny, g.nx, g.T) == (2, 4, 8) and g.oy == (0, 8) and g.ox == (0, 8, 16, 24)
    assert windows(g)[5] == (8, 8)                                              # w = j nx + i
    g = window_grid(32, 32, 32, 16)
    assert g.T == 1 and g.oy == g.ox == (0,)
    assert window_grid(16, 16 + 8 * 15, 16, 8).nx == 16                         # 16 offsets are the most an axis takes


@pytest.mark.parametrize("grid", GRIDS + [(32, 32, 32, 16), (64, 32, 32, 16)])
def test_cover_count_agrees_with_brute_force(grid):
    from sta.canvas import cover_count, window_grid
    g = window_grid(*grid)
    n = cover_count(g)
    for Y in range(g.Hc):
        for X in range(g.Wc):
            want = sum(1 for oy in g.oy for ox in g.ox if oy <= Y < oy + g.s and ox <= X < ox + g.s)
            assert n[Y, X].item() == want and want >= 1
    assert n.max().item() <= 9


@pytest.mark.parametrize("args,numbers", [
    ((32, 60, 32, 16), ("60",)),                       # canvas width not a multiple of 8
    ((36, 64, 32, 16), ("36",)),
    ((32, 64, 28, 8), ("28",)),                        # window not a multiple of 8
    ((32, 64, 32, 12), ("12",)),                       # stride not a multiple of 8
    ((32, 64, 32, 40), ("40", "32")),                  # stride > s: gaps
    ((32, 64, 32, 4), ("4",)),                         # stride < 8
    ((32, 64, 32, 0), ("0",)),
    ((16, 64, 32, 16), ("16", "32")),                  # canvas smaller than the window
    ((32, 24, 32, 16), ("24", "32")),
    ((16, 16 + 8 * 16, 16, 8), ("17", "16")),          # 17 offsets along x
    ((16 + 8 * 16, 16, 16, 8), ("17", "16")),
])
def test_window_grid_refusals_carry_their_numbers(args, numbers):
    from sta.canvas import window_grid
    with pytest.raises(ValueError) as e:
        window_grid(*args)
    for n in numbers:
        assert n in str(e.value), (args, str(e.value))


# ---------------------------------------------------------------------------------------------------
# layout: the remapped centres rasterise the canvas-level disc
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(32, 64, 32, 16), (64, 32, 32, 16), (32, 128, 32, 24)])
def test_window_masks_equal_the_canvas_disc(grid):
    """Centres are multiples of 1/64 in window units, so every term of the fp32 rule is exact: for every canvas pixel of every level
    (sides s, s/2, s/4, s/8 per window) and every covering window, the window's mask bit equals the canvas-level disc
    (X / s - x Wc / s)^2 + (Y / s - y Hc / s)^2 < 0.04, evaluated here in float64 (exact for these values)."""
    from sta import ops
    from sta.canvas import window_centres, window_grid, windows
    g = window_grid(*grid)
    s = g.s
    # x Wc / s and y Hc / s multiples of 1/64
    centres = [(kx / 64.0 * s / g.Wc, ky / 64.0 * s / g.Hc) for kx, ky in ((16, 32), (77, 40), (g.Wc * 2 - 9, 13), (40, g.Hc * 2 - 20), (-8, 70))]
    per_window = window_centres(centres, g)
    assert len(per_window) == g.T and all(len(c) == len(centres) for c in per_window)
    hits = 0
    for (y0, x0), wc in zip(windows(g), per_window):
        for (x, y), (wx, wy) in zip(centres, wc):
            assert wx == (x * g.Wc - x0) / s and wy == (y * g.Hc - y0) / s
        for f in (1, 2, 4, 8):
            d = s // f
            got = ops.disc_masks(wc, d).reshape(len(centres), d, d)
            r = torch.arange(d, dtype=torch.float64)
            Y, X = (y0 + f * r)[:, None], (x0 + f * r)[None, :]             # canvas positions of the level's pixels, latent pixels
            for k, (x, y) in enumerate(centres):
                want = (X / s - x * g.Wc / s) ** 2 + (Y / s - y * g.Hc / s) ** 2 < 0.04
                assert torch.equal(got[k].bool(), want), (y0, x0, f, k)
                hits += int(want.sum())
    assert hits > 0


def test_an_object_far_outside_a_window_sets_no_bit():
    from sta import ops
    from sta.canvas import window_centres, window_grid
    g = window_grid(32, 64, 32, 32)
    left, right = window_centres([(0.125, 0.5)], g)                            # canvas x = 8 latent pixels
    assert left == [[0.25, 0.5]] and right == [[-0.75, 0.5]]
    for d in (32, 16, 8, 4):
        assert ops.disc_masks(left, d).sum() > 0 and ops.disc_masks(right, d).sum() == 0


# ---------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fuse_of_split_is_the_identity(grid, dtype):
    """The sum of up to 9 equal 16-bit values is exact in fp32 and so is its division by their count."""
    from sta.canvas import window_fuse_reference, window_grid, window_split_reference
    g = window_grid(*grid)
    torch.manual_seed(1)
    x = (torch.randn(2, 4, g.Hc, g.Wc) * 3).to(dtype)
    for src in (x, x.float()):
        xin = window_split_reference(src, g, dtype)
        assert xin.shape == (2 * 2 * g.T, 4, g.s, g.s) and xin.dtype == dtype
        assert torch.equal(xin[0::2], xin[1::2])
        back = window_fuse_reference(xin, g)
        assert back.dtype == dtype and torch.equal(back[0::2], x) and torch.equal(back[1::2], x)
    pair = torch.stack([x, -x], 1).reshape(4, 4, g.Hc, g.Wc)                   # rows = 2: row r goes to row r
    xin = window_split_reference(pair, g, dtype, rows=2)
    assert torch.equal(xin[1::2], -xin[0::2]) and torch.equal(window_fuse_reference(xin, g), pair)
    y0, x0 = g.oy[-1], g.ox[-1]                                                 # the last window of canvas 1 holds that corner
    assert torch.equal(xin[2 * (g.T + g.T - 1)], x[1, :, y0:y0 + g.s, x0:x0 + g.s])


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_fuse_agrees_with_an_fp64_mean(grid, dtype):
    """Half a unit in the last place of the output type, plus the fp32 accumulation's own error (at most 8 adds and one division of
    fp32, 2^-24 each): half an ulp is at most 2^-11 (fp16) / 2^-8 (bf16) / 2^-24 (fp32) of the value."""
    from sta.canvas import cover_count, window_fuse_reference, window_grid, windows
    g = window_grid(*grid)
    torch.manual_seed(2)
    eps = torch.randn(2 * g.T, 4, g.s, g.s).to(dtype)
    got = window_fuse_reference(eps, g)
    acc = torch.zeros(2, 4, g.Hc, g.Wc, dtype=torch.float64)
    mag = torch.zeros_like(acc)
    for w, (y0, x0) in enumerate(windows(g)):
        acc[..., y0:y0 + g.s, x0:x0 + g.s] += eps[2 * w:2 * w + 2].double()
        mag[..., y0:y0 + g.s, x0:x0 + g.s] += eps[2 * w:2 * w + 2].double().abs()
    n = cover_count(g).double()
    half_ulp = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}[dtype]      # 10 / 7 / 23 fraction bits
    err = (got.double() - acc / n).abs()
    bound = half_ulp * (acc / n).abs() + 9 * 2.0 ** -24 * mag / n + (2.0 ** -25 if dtype == torch.float16 else 0.0)   # + fp16 subnormals
    assert (err <= bound).all(), (err - bound).max().item()


@pytest.mark.parametrize("mode", ["first", "second", "noise"])
def test_step_windows_with_one_window_is_the_plain_step(mode):
    from sta import solver
    from sta.canvas import step_windows_reference, window_grid
    from tests.test_solver_gpu import _case
    c = _case(mode)
    g = window_grid(16, 16, 16, 8)
    torch.manual_seed(3)
    eps = torch.randn(4, 4, 16, 16).to(torch.float16)
    x, m_prev, noise = torch.randn(2, 4, 16, 16) * 3, torch.randn(2, 4, 16, 16), torch.randn(2, 4, 16, 16)
    xn, m, xin = step_windows_reference(eps, x, m_prev, noise, c, g, want_xin=True)
    rx, rm, rxin = solver.solver_step(eps, x, m_prev, noise, c, want_xin=True)
    assert torch.equal(xn, rx) and torch.equal(m, rm) and torch.equal(xin, rxin) and xin.dtype == torch.float16


def test_step_windows_on_overlapping_windows():
    """The step of the fp32 means; xin is the split of x_next."""
    from sta import solver
    from sta.canvas import _fuse32, step_windows_reference, window_fuse_reference, window_grid, window_split_reference
    from tests.test_solver_gpu import _case
    c = _case("second")
    g = window_grid(24, 40, 16, 8)
    torch.manual_seed(4)
    eps = torch.randn(2 * 2 * g.T, 4, 16, 16).to(torch.bfloat16)
    x, m_prev = torch.randn(2, 4, 24, 40), torch.randn(2, 4, 24, 40)
    xn, m, xin = step_windows_reference(eps, x, m_prev, None, c, g, want_xin=True)
    rx, rm = solver.step_reference(_fuse32(eps, g), x, m_prev, None, c)
    assert torch.equal(xn, rx) and torch.equal(m, rm)
    assert torch.equal(xin, window_split_reference(xn, g, torch.bfloat16))
    assert torch.equal(window_fuse_reference(eps, g), _fuse32(eps, g).to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------
# C-ABI
# ---------------------------------------------------------------------------------------------------
def _ints(v):
    a = (ctypes.c_int * len(v))(*v)
    return a, ctypes.addressof(a)


def _call(L, name, **kw):
    a = dict(src=PTR, xin=PTR + 0x100000, eps=PTR, out=PTR + 0x100000, x=PTR + 0x200000, m_prev=PTR + 0x300000, noise=PTR + 0x400000,
             x_next=PTR + 0x500000, m=PTR + 0x600000, P=1, rows=1, C=4, Hc=16, Wc=40, oy=(0,), ox=(0, 16, 24), s=16, wrap=0, src_dtype=2, dtype=0)
    a.update(kw)
    keep_y, oy = _ints(a["oy"]) if a["oy"] is not None else (None, 0)
    keep_x, ox = _ints(a["ox"]) if a["ox"] is not None else (None, 0)
    ny, nx = a.get("ny", len(a["oy"] or ())), a.get("nx", len(a["ox"] or ()))
    grid = (ny, nx, oy, ox, a["s"], a["wrap"])
    if name == "sta_window_split":
        rc = L.sta_window_split(a["src"], a["xin"], a["P"], a["rows"], a["C"], a["Hc"], a["Wc"], *grid, a["src_dtype"], a["dtype"], None)
    elif name == "sta_window_fuse":
        rc = L.sta_window_fuse(a["eps"], a["out"], a["P"], a["C"], a["Hc"], a["Wc"], *grid, a["dtype"], None)
    else:
        rc = L.sta_sampler_step_windows(a["eps"], a["x"], a["m_prev"], a["noise"], a["x_next"], a["m"], a["xin"], a["P"], a["C"], a["Hc"],
                                        a["Wc"], *grid, 7.5, 0.5, a.get("alpha_t", 0.8), 1.0, 0.1, 0.0, 0.2, 0.0, a["dtype"], None)
    return rc, L.sta_last_error().decode()


def test_abi_symbols_and_refusals_reach_no_launch():
    from sta import lib
    L = lib.load()
    vp, i, f, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    assert lib.SYMBOLS["sta_window_split"] == (i, [vp, vp, l, i, i, i, i, i, i, vp, vp, i, i, i, i, vp])
    assert lib.SYMBOLS["sta_window_fuse"] == (i, [vp, vp, l, i, i, i, i, i, vp, vp, i, i, i, vp])
    assert lib.SYMBOLS["sta_sampler_step_windows"] == (i, [vp] * 7 + [l, i, i, i, i, i, vp, vp, i, i] + [f] * 8 + [i, vp])
    assert not [name for name in lib.SYMBOLS if name.endswith("_ring")]         # one entry point per launch: `wrap` is an argument
    header = " ".join(open(os.path.join(ROOT, "include", "sta_unet.h")).read().split())
    for decl in ("int sta_window_split(const void* src, void* xin, long P, int rows, int C, int Hc, int Wc, int ny, int nx, const int* oy, "
                 "const int* ox, int s, int wrap, int src_dtype, int dtype, void* stream);",
                 "int sta_window_fuse(const void* eps, void* out, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, "
                 "int s, int wrap, int dtype, void* stream);",
                 "int sta_sampler_step_windows(const void* eps, const float* x, const float* m_prev, const float* noise, float* x_next, "
                 "float* m, void* xin, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, "
                 "float scale, float sigma_t, float alpha_t, float c_x, float c_m, float c_p, float c_e, float c_n, int dtype, void* stream);",
                 "#define STA_MAX_WINDOW_OFFSETS 16"):
        assert decl in header, decl
    assert lib.MAX_WINDOW_OFFSETS == 16 and L.sta_version() == 0x000600
    # built as part of the sampler step's translation unit (its helpers and its flags: no fast-math flag), like sta_guide.hip:
    # tests/test_abi_dtype_cpu.py and tests/test_guidance_cpu.py pin the list of translation units
    assert lib.INCLUDED_SOURCES["sta_window.hip"] == "sta_sampler.hip" and "sta_sampler.hip" not in lib.PER_SOURCE_FLAGS
    assert '#include "sta_window.hip"' in open(os.path.join(lib.CSRC, "sta_sampler.hip")).read()
    assert os.path.isfile(os.path.join(lib.CSRC, "sta_window.hip"))
    assert "window_fuse_kernel" in lib.NO_SPILL_KERNELS["sta_sampler.hip"]      # the by-value offset tables may not go to scratch
    common = [
        (dict(oy=None), STA_E_ARG, "null pointer"),
        (dict(ox=None), STA_E_ARG, "null pointer"),
        (dict(P=0), STA_E_ARG, "P=0"),
        (dict(C=0), STA_E_ARG, "C=0"),
        (dict(Wc=44), STA_E_ARG, "Wc=44"),
        (dict(Hc=20), STA_E_ARG, "Hc=20"),
        (dict(s=12), STA_E_ARG, "s=12"),
        (dict(s=0), STA_E_ARG, "s=0"),
        (dict(Hc=8), STA_E_ARG, "Hc=8"),                                       # canvas smaller than the window
        (dict(ox=(0, 12, 24)), STA_E_ARG, "ox[1]=12 is not a multiple of 8"),
        (dict(ox=(0, 16, 32)), STA_E_ARG, "ox[2]=32 out of range"),
        (dict(ox=(8, 16, 24)), STA_E_ARG, "ox[0]=8 unsorted"),
        (dict(ox=(0, 24, 16)), STA_E_ARG, "gap between ox[0]=0 and ox[1]=24"),
        (dict(ox=(0, 16, 16)), STA_E_ARG, "ox[2]=16 unsorted"),
        (dict(ox=(0, 24)), STA_E_ARG, "gap between ox[0]=0 and ox[1]=24"),
        (dict(ox=(0, 16)), STA_E_ARG, "gap behind ox[1]=16"),
        (dict(ox=(0, -8, 24)), STA_E_ARG, "ox[1]=-8 out of range"),
        (dict(oy=(0, 8), Hc=16), STA_E_ARG, "oy[1]=8 out of range"),
        (dict(oy=(), ny=0), STA_E_ARG, "ny=0"),
        (dict(ox=tuple(range(0, 136, 8)), Wc=16 + 8 * 16), STA_E_ARG, "nx=17"),
        (dict(dtype=7), STA_E_UNSUP, "dtype 7"),
    ]
    own = {
        "sta_window_split": [(dict(src=0), STA_E_ARG, "null pointer"), (dict(xin=0), STA_E_ARG, "null pointer"),
                             (dict(src=PTR + 8), STA_E_ARG, "16-byte aligned"), (dict(xin=PTR + 0x100004), STA_E_ARG, "16-byte aligned"),
                             (dict(rows=3), STA_E_ARG, "rows=3"), (dict(rows=0), STA_E_ARG, "rows=0"),
                             (dict(src_dtype=1, dtype=0), STA_E_UNSUP, "src_dtype 1"), (dict(src_dtype=5), STA_E_UNSUP, "src_dtype 5")],
        "sta_window_fuse": [(dict(eps=0), STA_E_ARG, "null pointer"), (dict(out=0), STA_E_ARG, "null pointer"),
                            (dict(eps=PTR + 2), STA_E_ARG, "16-byte aligned"), (dict(out=PTR + 0x100008), STA_E_ARG, "16-byte aligned")],
        "sta_sampler_step_windows": [(dict(eps=0), STA_E_ARG, "null pointer"), (dict(x=0), STA_E_ARG, "null pointer"),
                                     (dict(x_next=0), STA_E_ARG, "null pointer"), (dict(m=0), STA_E_ARG, "null pointer"),
                                     (dict(x=PTR + 0x200004), STA_E_ARG, "16-byte aligned"), (dict(m_prev=PTR + 0x300008), STA_E_ARG, "16-byte aligned"),
                                     (dict(noise=PTR + 0x400002), STA_E_ARG, "16-byte aligned"), (dict(xin=PTR + 0x100008), STA_E_ARG, "16-byte aligned"),
                                     (dict(alpha_t=0.0), STA_E_ARG, "alpha_t == 0")],
    }
    for name in own:
        for kw, code, text in common + own[name]:
            rc, err = _call(L, name, **kw)
            assert rc == code and text in err, (name, kw, rc, err)
        assert _call(L, name, dtype=7)[1] == "dtype 7"                          # the same text every entry point gives
    assert _call(L, "sta_sampler_step_windows", dtype=7, m_prev=0, noise=0, xin=0)[1] == "dtype 7"      # the optional pointers may be NULL
    assert _call(L, "sta_window_split", dtype=7, src_dtype=7)[0] == STA_E_UNSUP


# ---------------------------------------------------------------------------------------------------
# samplers on the host miniature
# ---------------------------------------------------------------------------------------------------
_MODEL = []
KINDS = ["plms", "ddim", "dpm"]
CENTRES = [[0.3, 0.4], [0.7, 0.6]]


def _sampler(kind, **kw):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    from tests.test_solver_cpu import _model
    if not _MODEL:
        _MODEL.append(_model()[0])
    cls = dict(ddim=DDIMSampler, plms=PLMSSampler, dpm=DPMSolverSampler)[kind]
    return cls(_MODEL[0], **dict(dict(loss_model=None, opt_epochs=0, use_graph=False, save_images=False), **kw))


def _canvas(sampler, canvas, stride, centres, x_T, c, local_ctx, **kw):
    with oracle_ops():
        sampler.sample_canvas(**dict(dict(S=STEPS, canvas=canvas, window=S_LAT, stride=stride, conditionings=[c],
                                          unconditional_conditionings=gi.load_uncond(), bboxs=[centres], object_names=[["cat", "dog"]],
                                          local_conditionings=[local_ctx], x_T=x_T, unconditional_guidance_scale=7.5, eta=0.0, seed=1), **kw))
    return sampler.last_result["x0"]


@pytest.mark.parametrize("kind", KINDS)
def test_canvas_of_one_window_equals_sample(kind):
    c, local_ctx, x_T = gi.unet_inputs(K, 5)
    sampler = _sampler(kind)
    got = _canvas(sampler, (S_LAT, S_LAT), 16, CENTRES, x_T, c, local_ctx).clone()
    assert sampler._canvas is None and tuple(sampler.last_result["W"].shape) == (1, K, STEPS)
    with oracle_ops():
        sampler.sample(S=STEPS, conditioning=c, batch_size=1, shape=[4, S_LAT, S_LAT], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond(), eta=0.0, x_T=x_T, text_index=0, curr_text="", bboxs_curr=CENTRES, seed=1,
                       prompt_idx=0, object_names=["cat", "dog"], local_conditionings=local_ctx)
    want = sampler.last_result["x0"]
    assert got.shape == (1, 4, S_LAT, S_LAT) and torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_canvas_of_two_disjoint_windows_equals_sample_batch(kind):
    """Canvas 32 x 64, stride 32: no overlap, so each half is the window's own trajectory — sample_batch of the two windows with their
    remapped centres and the halves of x_T, to 1e-5 of max (the UNet batch is the same; only the order of the bookkeeping differs)."""
    from sta.canvas import window_centres, window_grid
    c, local_ctx, xa = gi.unet_inputs(K, 5)
    xb = gi.unet_inputs(K, 6)[2]
    x_T = torch.cat([xa, xb], dim=3)
    centres = [[0.25, 0.4], [0.625, 0.6]]                                       # the second disc straddles the seam at x = 0.5
    sampler = _sampler(kind)
    got = _canvas(sampler, (S_LAT, 2 * S_LAT), S_LAT, centres, x_T, c, local_ctx).clone()
    assert got.shape == (1, 4, S_LAT, 2 * S_LAT)
    g = window_grid(S_LAT, 2 * S_LAT, S_LAT, S_LAT)
    per_window = window_centres(centres, g)
    assert per_window == [[[0.5, 0.4], [1.25, 0.6]], [[-0.5, 0.4], [0.25, 0.6]]]
    with oracle_ops():
        sampler.sample_batch(S=STEPS, shape=[4, S_LAT, S_LAT], conditionings=[c, c], unconditional_conditionings=gi.load_uncond(),
                             bboxs=per_window, object_names=[["cat", "dog"]] * 2, local_conditionings=[local_ctx, local_ctx],
                             x_T=torch.cat([xa, xb]), unconditional_guidance_scale=7.5, eta=0.0, seed=1)
    want = sampler.last_result["x0"]
    for w, half in enumerate((got[..., :S_LAT], got[..., S_LAT:])):
        err = (half - want[w:w + 1]).abs().max().item()
        print("%s window %d: max |canvas - sample_batch| = %.3g of max %.3g" % (kind, w, err, want[w].abs().max().item()))
        assert err <= 1e-5 * want[w].abs().max().item()
    assert not torch.allclose(got[..., :S_LAT], got[..., S_LAT:])


def test_overlapping_canvas_and_the_unfused_step_agree_on_the_host():
    """T = 3 overlapping windows, DDIM: finite, and the three-launch form (means rounded to the UNet's type — fp32 here, so nothing is
    rounded) gives the same trajectory as the fused step up to fp32 rounding."""
    c, local_ctx, xa = gi.unet_inputs(K, 5)
    x_T = torch.cat([xa, gi.unet_inputs(K, 6)[2]], dim=3)
    centres = [[0.25, 0.4], [0.625, 0.6]]
    sampler = _sampler("ddim")
    a = _canvas(sampler, (S_LAT, 2 * S_LAT), 16, centres, x_T, c, local_ctx).clone()
    sampler.canvas_fused_step = False
    b = _canvas(sampler, (S_LAT, 2 * S_LAT), 16, centres, x_T, c, local_ctx)
    assert torch.isfinite(a).all() and (a - b).abs().max() <= 1e-5 * a.abs().max()


def test_sample_canvas_refusals():
    c, local_ctx, x_T = gi.unet_inputs(K, 5)
    calls = []

    def run(kind="ddim", skw=None, **kw):
        sampler = _sampler(kind, **(skw or {}))
        sampler.model.apply_model_extra = lambda *a, **k: calls.append(1)
        try:
            return _canvas(sampler, (S_LAT, S_LAT), 16, CENTRES, x_T, c, local_ctx, **kw)
        finally:
            del sampler.model.apply_model_extra
    with pytest.raises(ValueError, match="opt_epochs = 2"):
        run(skw=dict(opt_epochs=2))
    for name in ("attn_capture", "attn_loss", "latent_guidance"):
        for kind in KINDS:
            with pytest.raises(ValueError, match=name):
                run(kind, skw={name: object()})
    with pytest.raises(ValueError, match="mask="):
        run(mask=torch.zeros(1, 1, S_LAT, S_LAT), x0=x_T)
    with pytest.raises(ValueError, match="x0="):
        run(x0=x_T)
    sampler = _sampler("ddim")
    sampler._start = 2
    with pytest.raises(ValueError, match="call 2"):
        _canvas(sampler, (S_LAT, S_LAT), 16, CENTRES, x_T, c, local_ctx)
    with pytest.raises(ValueError, match="smaller than the window"):
        _canvas(_sampler("plms"), (16, S_LAT), 16, CENTRES, x_T, c, local_ctx)
    with pytest.raises(ValueError, match="x_T"):
        _canvas(_sampler("plms"), (S_LAT, 2 * S_LAT), 16, CENTRES, x_T, c, local_ctx)
    assert not calls


# ---------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------
def test_cli_canvas_parses_and_refuses(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts"))
    import _txt2img_common as cli
    import sta.pipeline
    monkeypatch.setattr(sta.pipeline, "build_sd_v1", lambda *a, **k: pytest.fail("a model was built"))
    p = cli.build_parser("x.json")
    opt = p.parse_args(["--opt_epochs", "0"])
    assert opt.canvas is None and opt.canvas_stride is None and cli.canvas_grid(opt) is None
    cli.check_options(opt)
    opt = p.parse_args(["--opt_epochs", "0", "--canvas", "512x2048"])
    cli.check_options(opt)
    g = cli.canvas_grid(opt)
    assert (g.Hc, g.Wc, g.s, g.stride, g.T) == (64, 256, 64, 32, 7)
    g = cli.canvas_grid(p.parse_args(["--opt_epochs", "1", "--canvas", "1024x512", "--canvas_stride", "128", "--plms"]))
    assert (g.ny, g.nx, g.stride) == (5, 1, 16)
    g = cli.canvas_grid(p.parse_args(["--opt_epochs", "0", "--canvas", "256x640", "--H", "256", "--W", "256", "--dpm_solver", "--mxfp8"]))
    assert (g.s, g.ox) == (32, (0, 16, 32, 48))
    for bad, text in ((["--canvas", "512"], "HxW"), (["--canvas", "512x"], "HxW"), (["--canvas", "ax2048"], "HxW"),
                      (["--canvas", "512x2048", "--W", "768"], "square"),
                      (["--canvas", "512x2000"], "2000"), (["--canvas", "256x2048"], "smaller than the window"),
                      (["--canvas", "512x2048", "--canvas_stride", "100"], "100"),
                      (["--canvas", "512x2048", "--canvas_stride", "576"], "stride"),
                      (["--canvas", "512x8192", "--canvas_stride", "64"], "at most 16"),
                      (["--canvas_stride", "256"], "needs --canvas"),
                      (["--canvas", "512x2048", "--attn_maps"], "--attn_maps"),
                      (["--canvas", "512x2048", "--attn_guidance", "0.1"], "--attn_guidance")):
        with pytest.raises(SystemExit, match=text):
            cli.check_options(p.parse_args(["--opt_epochs", "0"] + bad))
    with pytest.raises(SystemExit, match="--opt_epochs"):
        cli.check_options(p.parse_args(["--opt_epochs", "3", "--canvas", "512x2048", "--clip", "synthetic"]))
    with pytest.raises(SystemExit, match="--attn_loss"):
        cli.check_options(p.parse_args(["--opt_epochs", "1", "--canvas", "512x2048", "--attn_loss", "0.5"]))
