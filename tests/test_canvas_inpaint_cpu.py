"""Inpainting and outpainting on wide canvases without a GPU: the torch restatements of the masked window kernels (sta.canvas), the
refusals of the two new C entry points (fake pointers: none of these calls may reach a launch), `inpaint_canvas` on the host miniature
and on a stub UNet (draw order, launch structure, the pixel paste), and scripts/outpaint.py's parser, refusals and keep masks. The
kernels are checked in test_canvas_inpaint_gpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import golden_inputs as gi
from tests.cpu_backend import oracle_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STA_E_ARG, STA_E_UNSUP = -1, -2
PTR = 0x10000                                          # a fake device pointer: non-null, 16-byte aligned, never read
GRIDS = [(32, 64, 16, 16), (16, 40, 16, 16), (24, 40, 16, 8), (32, 64, 32, 16)]
Q_A, Q_B = 0.8253, 0.5647
S_LAT, STEPS, K = 32, 4, 2
CENTRES = [[0.3, 0.4], [0.7, 0.6]]


def keep_mask(P, Hc, Wc, kind="mixed"):
    """keep [P, 1, Hc, Wc]. "mixed": canvas 0 has 0 / 1 blocks whose edges (rows 3 and Hc - 5, columns 5 and Wc - 6) are no multiples
    of 8, so one lane's 8-element vector mixes kept and repainted elements, and a few fractional cells; a second canvas is all 1.
    "uniform": canvas 0 all 0, a second canvas all 1."""
    keep = torch.zeros(P, 1, Hc, Wc)
    if kind == "mixed":
        keep[0, 0, 3:Hc - 5, 5:Wc - 6] = 1.0
        keep[0, 0, 6:9, 11:14] = 0.0                   # a repainted hole inside the kept block
        keep[0, 0, 1, 1:4] = 0.25
        keep[0, 0, Hc - 2, Wc - 5:Wc - 2] = 0.5
        keep[0, 0, 4, 7] = 0.75
    keep[1:] = 1.0
    return keep


def _grid(args):
    from sta.canvas import window_grid
    return window_grid(*args)


# ---------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("mode", ["first", "second", "noise"])
def test_masked_restatement_is_the_step_then_the_blend(mode, grid):
    from sta import canvas, solver
    from tests.test_solver_gpu import _case
    c, g = _case(mode), _grid(grid)
    torch.manual_seed(g.T)
    P = 2
    shape = (P, 4, g.Hc, g.Wc)
    eps = torch.randn(2 * P * g.T, 4, g.s, g.s).to(torch.float16)
    x, m_prev, noise, x0, qn = torch.randn(shape) * 3, torch.randn(shape), torch.randn(shape), torch.randn(shape), torch.randn(shape)
    bl = solver.Blend(x0, keep_mask(P, g.Hc, g.Wc), qn, Q_A, Q_B)
    xn, m, xin = canvas.step_windows_masked_reference(eps, x, m_prev, noise, c, bl, g, want_xin=True)
    px, pm, _ = canvas.step_windows_reference(eps, x, m_prev, noise, c, g)
    assert torch.equal(xn, solver.blend_reference(px, bl)) and torch.equal(m, pm)
    assert xin.dtype == torch.float16 and torch.equal(xin, canvas.window_split_reference(xn, g, torch.float16))
    assert canvas.step_windows_masked_reference(eps, x, m_prev, noise, c, bl, g)[2] is None
    # the dispatching entry point takes the restatement for CPU tensors
    for a, b in zip(canvas.sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, g, want_xin=True), (xn, m, xin)):
        assert torch.equal(a, b)
    one = (bl.keep == 1).expand_as(xn)
    assert torch.equal(xn[one], (Q_A * x0 + Q_B * qn)[one]) and not torch.equal(xn, px)
    xb, xin0 = canvas.window_blend_reference(x, bl, g, torch.bfloat16, want_xin=True)
    assert torch.equal(xb, solver.blend_reference(x, bl)) and torch.equal(xin0, canvas.window_split_reference(xb, g, torch.bfloat16))
    wb, wxin = canvas.window_blend(x, bl, g, torch.bfloat16, want_xin=True)
    assert torch.equal(wb, xb) and torch.equal(wxin, xin0) and canvas.window_blend(x, bl, g)[1] is None


def test_masked_restatement_with_one_window_is_solver_step_masked():
    from sta import canvas, solver
    from tests.test_solver_gpu import _case
    c, g = _case("noise"), _grid((16, 16, 16, 8))
    torch.manual_seed(3)
    shape = (2, 4, 16, 16)
    eps = torch.randn(4, 4, 16, 16).to(torch.float16)
    x, noise, x0, qn = torch.randn(shape) * 3, torch.randn(shape), torch.randn(shape), torch.randn(shape)
    bl = solver.Blend(x0, keep_mask(2, 16, 16), qn, Q_A, Q_B)
    got = canvas.step_windows_masked_reference(eps, x, None, noise, c, bl, g, want_xin=True)
    want = solver.solver_step_masked(eps, x, None, noise, c, bl, want_xin=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    xb, xin = canvas.window_blend_reference(x, bl, g, torch.float16, want_xin=True)
    wb, wxin = solver.latent_blend(x, bl, dtype=torch.float16, want_xin=True)
    assert torch.equal(xb, wb) and torch.equal(xin, wxin)


# ---------------------------------------------------------------------------------------------------
# C-ABI
# ---------------------------------------------------------------------------------------------------
def _ints(v):
    a = (ctypes.c_int * len(v))(*v)
    return a, ctypes.addressof(a)


def _call(L, name, **kw):
    a = dict(eps=PTR, x=PTR + 0x200000, m_prev=PTR + 0x300000, noise=PTR + 0x400000, x_next=PTR + 0x500000, m=PTR + 0x600000,
             xin=PTR + 0x100000, x0=PTR + 0x700000, keep=PTR + 0x800000, qnoise=PTR + 0x900000, x_out=PTR + 0x500000, P=1, C=4, Hc=16,
             Wc=40, oy=(0,), ox=(0, 16, 24), s=16, wrap=0, alpha_t=0.8, dtype=0)
    a.update(kw)
    keep_y, oy = _ints(a["oy"]) if a["oy"] is not None else (None, 0)
    keep_x, ox = _ints(a["ox"]) if a["ox"] is not None else (None, 0)
    grid = (len(a["oy"] or ()), len(a["ox"] or ()), oy, ox, a["s"], a["wrap"])
    if name == "sta_sampler_step_windows_masked":
        rc = L.sta_sampler_step_windows_masked(a["eps"], a["x"], a["m_prev"], a["noise"], a["x0"], a["keep"], a["qnoise"], a["x_next"], a["m"],
                                               a["xin"], a["P"], a["C"], a["Hc"], a["Wc"], *grid, 7.5, 0.5, a["alpha_t"], 1.0, 0.1, 0.0, 0.2,
                                               0.0, Q_A, Q_B, a["dtype"], None)
    else:
        rc = L.sta_window_blend(a["x"], a["x0"], a["keep"], a["qnoise"], a["x_out"], a["xin"], a["P"], a["C"], a["Hc"], a["Wc"], *grid, Q_A,
                                Q_B, a["dtype"], None)
    return rc, L.sta_last_error().decode()


def test_abi_symbols_and_refusals_reach_no_launch():
    from sta import lib
    L = lib.load()
    vp, i, f, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    assert lib.SYMBOLS["sta_sampler_step_windows_masked"] == (i, [vp] * 10 + [l, i, i, i, i, i, vp, vp, i, i] + [f] * 10 + [i, vp])
    assert lib.SYMBOLS["sta_window_blend"] == (i, [vp] * 6 + [l, i, i, i, i, i, vp, vp, i, i, f, f, i, vp])
    header = " ".join(open(os.path.join(ROOT, "include", "sta_unet.h")).read().split())
    for decl in ("int sta_sampler_step_windows_masked(const void* eps, const float* x, const float* m_prev, const float* noise, "
                 "const float* x0, const float* keep, const float* qnoise, float* x_next, float* m, void* xin, long P, int C, int Hc, "
                 "int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, float scale, float sigma_t, float alpha_t, float c_x, "
                 "float c_m, float c_p, float c_e, float c_n, float q_a, float q_b, int dtype, void* stream);",
                 "int sta_window_blend(const float* x, const float* x0, const float* keep, const float* noise, float* x_out, void* xin, "
                 "long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, float q_a, float q_b, int dtype, "
                 "void* stream);"):
        assert decl in header, decl
    # one definition of the blend, shared by the square-image kernels and the canvas kernels
    csrc = lambda n: open(os.path.join(lib.CSRC, n)).read()
    assert csrc("sta_blend_dev.h").count("float blend1(") == 1
    for n in ("sta_inpaint.hip", "sta_window.hip"):
        assert '#include "sta_blend_dev.h"' in csrc(n) and "float blend1(" not in csrc(n) and "blend1(" in csrc(n)
    for kernel in ("sampler_step_windows_masked_kernel", "window_blend_kernel"):
        assert kernel in lib.NO_SPILL_KERNELS["sta_sampler.hip"]                # the by-value offset tables may not go to scratch
    common = [
        (dict(oy=None), STA_E_ARG, "null pointer"),
        (dict(ox=None), STA_E_ARG, "null pointer"),
        (dict(x=0), STA_E_ARG, "null pointer"),
        (dict(x0=0), STA_E_ARG, "null pointer"),
        (dict(keep=0), STA_E_ARG, "null pointer"),
        (dict(qnoise=0), STA_E_ARG, "null pointer"),
        (dict(x=PTR + 0x200004), STA_E_ARG, "16-byte aligned"),
        (dict(x0=PTR + 0x700008), STA_E_ARG, "16-byte aligned"),
        (dict(keep=PTR + 0x800004), STA_E_ARG, "16-byte aligned"),
        (dict(qnoise=PTR + 0x900002), STA_E_ARG, "16-byte aligned"),
        (dict(xin=PTR + 0x100008), STA_E_ARG, "16-byte aligned"),
        (dict(P=0), STA_E_ARG, "P=0"),
        (dict(C=0), STA_E_ARG, "C=0"),
        (dict(Wc=44), STA_E_ARG, "Wc=44"),
        (dict(s=12), STA_E_ARG, "s=12"),
        (dict(Hc=8), STA_E_ARG, "Hc=8"),
        (dict(ox=(0, 12, 24)), STA_E_ARG, "ox[1]=12 is not a multiple of 8"),
        (dict(ox=(0, 16, 32)), STA_E_ARG, "ox[2]=32 out of range"),
        (dict(ox=(0, 24)), STA_E_ARG, "gap between ox[0]=0 and ox[1]=24"),
        (dict(ox=(0, 16)), STA_E_ARG, "gap behind ox[1]=16"),
        (dict(ox=tuple(range(0, 136, 8)), Wc=16 + 8 * 16), STA_E_ARG, "nx=17"),
        (dict(dtype=7), STA_E_UNSUP, "dtype 7"),
    ]
    own = {
        "sta_sampler_step_windows_masked": [(dict(eps=0), STA_E_ARG, "null pointer"), (dict(x_next=0), STA_E_ARG, "null pointer"),
                                            (dict(m=0), STA_E_ARG, "null pointer"), (dict(eps=PTR + 2), STA_E_ARG, "16-byte aligned"),
                                            (dict(m_prev=PTR + 0x300008), STA_E_ARG, "16-byte aligned"),
                                            (dict(noise=PTR + 0x400002), STA_E_ARG, "16-byte aligned"),
                                            (dict(m=PTR + 0x600004), STA_E_ARG, "16-byte aligned"), (dict(alpha_t=0.0), STA_E_ARG, "alpha_t == 0")],
        "sta_window_blend": [(dict(x_out=0), STA_E_ARG, "null pointer"), (dict(x_out=PTR + 0x500004), STA_E_ARG, "16-byte aligned")],
    }
    for name in own:
        for kw, code, text in common + own[name]:
            rc, err = _call(L, name, **kw)
            assert rc == code and text in err, (name, kw, rc, err)
        assert _call(L, name, dtype=7)[1] == "dtype 7"                          # the same text every entry point gives
        assert _call(L, name, dtype=7, xin=0)[1] == "dtype 7"                   # xin is optional
    assert _call(L, "sta_sampler_step_windows_masked", dtype=7, m_prev=0, noise=0, xin=0)[1] == "dtype 7"      # so are m_prev and noise
    assert _call(L, "sta_sampler_step_windows_masked", dtype=7, m_prev=0)[1] == "dtype 7"
    assert _call(L, "sta_sampler_step_windows_masked", dtype=7, noise=0)[1] == "dtype 7"


def test_the_sampler_step_is_defined_once():
    """The element step, forward and backward, and the helpers of the elementwise kernels have one definition, csrc/sta_step_dev.h; the
    square, masked and canvas kernels use it and define none of it themselves (sta_guide.hip has no step: it uses the helpers)."""
    from sta import lib
    csrc = lambda n: open(os.path.join(lib.CSRC, n)).read()
    header = csrc("sta_step_dev.h")
    step_defs = ("float step1(", "void step1_bwd(")
    helper_defs = ("typedef float F4", "struct StepCoef", "void load8(", "void store8(", " round8(const float", "void store_pair(")
    for d in step_defs + helper_defs:
        assert header.count(d) == 1, d
    for n in ("sta_sampler.hip", "sta_inpaint.hip", "sta_window.hip", "sta_guide.hip"):
        text = csrc(n)
        assert '#include "sta_step_dev.h"' in text, n
        for d in step_defs + helper_defs + ("struct V8T",):      # V8T: once for the whole library, see the next test
            assert d not in text, (n, d)
        assert "load8(" in text and "store8(" in text and "V8T<T>" in text, n
    assert all("step1(" in csrc(n) for n in ("sta_sampler.hip", "sta_inpaint.hip", "sta_window.hip"))
    assert all("step1_bwd<T>(" in csrc(n) for n in ("sta_sampler.hip", "sta_inpaint.hip"))
    assert "step1" not in csrc("sta_guide.hip")
    # no kernel restates the step's arithmetic: sigma_t and the c_* coefficients are read in the header alone
    for n in ("sta_sampler.hip", "sta_inpaint.hip", "sta_window.hip"):
        for field in ("c.sigma_t", "c.c_x", "c.c_m", "c.c_p", "c.c_e", "c.c_n", "c.scale"):
            assert field not in csrc(n), (n, field)


def test_the_trunk_glue_arithmetic_is_defined_once():
    """The LayerNorm row helpers, the query-fragment LDS tile and the NHWC GroupNorm geometry have one definition, csrc/sta_trunk_dev.h
    (V8T: csrc/sta_internal.h); the forward, backward and fused-projection sources include it and restate none of its constants."""
    import glob
    import re
    from sta import lib
    texts = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(lib.CSRC, "*.hip")) + glob.glob(os.path.join(lib.CSRC, "*.h"))}
    definitions = {"V8T": r"struct V8T\b", "GN_NT": r"constexpr int GN_NT\b", "GN_MAXG": r"constexpr int GN_MAXG\b",
                   "gn_nhwc_chunks": r"\bint gn_nhwc_chunks\(int", "the 272-byte tile constant": r"constexpr int \w+ = 272\b"}
    homes = {"V8T": "sta_internal.h"}
    for what, pattern in definitions.items():
        found = {n: len(re.findall(pattern, t)) for n, t in texts.items() if re.search(pattern, t)}
        assert found == {homes.get(what, "sta_trunk_dev.h"): 1}, (what, found)
    for n, t in texts.items():      # nor is 272 a factor of an offset anywhere else
        if n != "sta_trunk_dev.h":
            assert not re.search(r"\*\s*272\b|\b272\s*\*|CHUNK = 272", t), n
        assert "gn_nhwc_chunks_bwd" not in t and "add_layernorm_qfrag_wide_kernel" not in t, n
    for n in ("sta_unet.hip", "sta_unet_bwd.hip", "sta_lnqkv.hip"):
        assert '#include "sta_trunk_dev.h"' in texts[n], n
        assert "gn_part_at(" in texts[n] or n == "sta_lnqkv.hip", n
    for n in ("sta_unet.hip", "sta_lnqkv.hip"):
        assert "qfrag_tile_at(" in texts[n] and "QFRAG_CHUNK" in texts[n], n


# ---------------------------------------------------------------------------------------------------
# inpaint_canvas on the host miniature
# ---------------------------------------------------------------------------------------------------
def _draws(S, seed, shape):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=gen) for _ in range(S)]


def _inpaint_canvas(sampler, canvas, stride, x_T, c, local_ctx, **kw):
    with oracle_ops():
        sampler.inpaint_canvas(**dict(dict(S=STEPS, canvas=canvas, window=S_LAT, stride=stride, conditionings=[c],
                                           unconditional_conditionings=gi.load_uncond(), bboxs=[CENTRES], object_names=[["cat", "dog"]],
                                           local_conditionings=[local_ctx], x_T=x_T, unconditional_guidance_scale=7.5, eta=0.0, seed=1), **kw))
    return sampler.last_result["x0"]


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_inpaint_canvas_of_one_window_equals_masked_sample(kind):
    from tests.test_canvas_cpu import _sampler
    c, local_ctx, x_T = gi.unet_inputs(K, 5)
    x0 = gi.unet_inputs(K, 6)[2]
    keep = keep_mask(1, S_LAT, S_LAT)
    sampler = _sampler(kind, mask_noise=_draws(STEPS, 7, (1, 4, S_LAT, S_LAT)))
    got = _inpaint_canvas(sampler, (S_LAT, S_LAT), 16, x_T, c, local_ctx, mask=keep, x0=x0).clone()
    assert sampler._canvas is None and sampler._inpaint is None
    with oracle_ops():
        sampler.sample(S=STEPS, conditioning=c, batch_size=1, shape=[4, S_LAT, S_LAT], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond(), eta=0.0, x_T=x_T, text_index=0, curr_text="", bboxs_curr=CENTRES, seed=1,
                       prompt_idx=0, object_names=["cat", "dog"], local_conditionings=local_ctx, mask=keep, x0=x0)
    want = sampler.last_result["x0"]
    assert torch.isfinite(got).all() and torch.equal(got, want)
    with oracle_ops():
        sampler.sample_canvas(S=STEPS, canvas=(S_LAT, S_LAT), window=S_LAT, stride=16, conditionings=[c],
                              unconditional_conditionings=gi.load_uncond(), bboxs=[CENTRES], object_names=[["cat", "dog"]],
                              local_conditionings=[local_ctx], x_T=x_T, unconditional_guidance_scale=7.5, eta=0.0, seed=1)
    assert not torch.equal(sampler.last_result["x0"], got)                      # the mask does something


def test_inpaint_canvas_refusals():
    from tests.test_canvas_cpu import _sampler
    c, local_ctx, x_T = gi.unet_inputs(K, 5)
    keep, calls = keep_mask(1, S_LAT, S_LAT), []
    ok = dict(mask=keep, x0=x_T)

    def run(kind="ddim", skw=None, canvas=(S_LAT, S_LAT), prep=None, **kw):
        sampler = _sampler(kind, **(skw or {}))
        sampler.model.apply_model_extra = lambda *a, **k: calls.append(1)
        if prep:
            prep(sampler)
        try:
            return _inpaint_canvas(sampler, canvas, 16, x_T, c, local_ctx, **dict(ok, **kw))
        finally:
            del sampler.model.apply_model_extra
            assert getattr(sampler, "_inpaint", None) is None and sampler._canvas is None
    # everything sample_canvas refuses
    with pytest.raises(ValueError, match="opt_epochs = 2"):
        run(skw=dict(opt_epochs=2))
    for name in ("attn_capture", "attn_loss", "latent_guidance"):
        for kind in ("ddim", "dpm"):
            with pytest.raises(ValueError, match=name):
                run(kind, skw={name: object()})
    with pytest.raises(ValueError, match="call 2"):
        run(prep=lambda s: setattr(s, "_start", 2))
    with pytest.raises(ValueError, match="smaller than the window"):
        run(canvas=(16, S_LAT))
    with pytest.raises(ValueError, match="x_T"):
        run(canvas=(S_LAT, 2 * S_LAT), mask=keep_mask(1, S_LAT, 2 * S_LAT), x0=torch.zeros(1, 4, S_LAT, 2 * S_LAT))
    # its own
    with pytest.raises(ValueError, match="mask= and x0="):
        run(mask=None)
    with pytest.raises(ValueError, match="mask= and x0="):
        run(x0=None)
    with pytest.raises(ValueError, match="mask"):
        run(mask=keep_mask(1, S_LAT, 2 * S_LAT))                                # not the canvas's shape
    with pytest.raises(ValueError, match=r"x0 \(1, 4, 32, 64\)"):
        run(mask=keep_mask(1, S_LAT, 2 * S_LAT), x0=torch.zeros(1, 4, S_LAT, 2 * S_LAT))
    with pytest.raises(ValueError, match="batch of 1"):
        run(mask=keep_mask(2, S_LAT, S_LAT), x0=torch.cat([x_T, x_T]))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        run(mask=keep * 1.5)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        run(mask=keep - 0.5)
    image, mask_px = torch.rand(1, 3, 8 * S_LAT, 8 * S_LAT), torch.ones(1, 1, 8 * S_LAT, 8 * S_LAT)
    with pytest.raises(ValueError, match="image= and mask_px="):
        run(image=image)
    with pytest.raises(ValueError, match="image= and mask_px="):
        run(mask_px=mask_px)
    with pytest.raises(ValueError, match="image"):
        run(image=image[..., :128], mask_px=mask_px[..., :128])                 # not 8 Hc x 8 Wc
    assert not calls
    # sample_canvas keeps refusing a mask, and masked PLMS stays unsupported
    with pytest.raises(ValueError, match="mask="):
        with oracle_ops():
            _sampler("ddim").sample_canvas(S=STEPS, canvas=(S_LAT, S_LAT), window=S_LAT, conditionings=[c],
                                           unconditional_conditionings=gi.load_uncond(), bboxs=[CENTRES], object_names=[["cat", "dog"]],
                                           local_conditionings=[local_ctx], x_T=x_T, mask=keep, x0=x_T)
    with pytest.raises(NotImplementedError, match="inpainting"):
        run("plms")
    assert not calls


# ---------------------------------------------------------------------------------------------------
# inpaint_canvas around a stub UNet: draw order, launch structure, identities, the pixel paste
# ---------------------------------------------------------------------------------------------------
def _stub(S, eta=0.0, **attrs):
    from tests.test_img2img_cpu import _stub_sampler
    s, calls = _stub_sampler(S=S, eta=eta)
    for k, v in attrs.items():
        setattr(s, k, v)
    return s, calls


def _stub_canvas(s, S, canvas, x_T, eta=0.0, method="inpaint_canvas", **kw):
    cond = torch.zeros(1, 77, 8)
    getattr(s, method)(S=S, canvas=canvas, window=16, stride=8, conditionings=[cond], unconditional_conditionings=cond, bboxs=[CENTRES],
                       object_names=[["cat", "dog"]], local_conditionings=[[cond, cond]], x_T=x_T, unconditional_guidance_scale=7.5, eta=eta,
                       seed=0, **kw)
    return s.last_result["x0"].clone()


class Counters:
    """The sta.canvas / sta.solver entry points a trajectory may call, wrapped by counters."""
    NAMES = (("canvas", "window_blend"), ("canvas", "sampler_step_windows_masked"), ("canvas", "sampler_step_windows"),
             ("canvas", "window_split"), ("canvas", "window_fuse"), ("solver", "latent_blend"), ("solver", "solver_step"),
             ("solver", "solver_step_masked"))

    def __init__(self, monkeypatch):
        from sta import canvas, solver
        self.calls = []
        for mod, name in self.NAMES:
            inner = getattr(dict(canvas=canvas, solver=solver)[mod], name)
            monkeypatch.setattr(dict(canvas=canvas, solver=solver)[mod], name,
                                lambda *a, _inner=inner, _name=name, **k: (self.calls.append(_name), _inner(*a, **k))[1])

    def count(self):
        return {name: self.calls.count(name) for name in dict.fromkeys(self.calls)}


def test_launch_structure_and_draw_order(monkeypatch):
    """A fused masked trajectory of S calls: one window_blend, S - 1 sampler_step_windows_masked, one sampler_step_windows, nothing
    else; the draws are canvas-shaped and interleave as in `sample(mask=)`: blend 0, eta 0, blend 1, eta 1, ..., eta S - 1."""
    S, canvas = 5, (16, 40)
    order = []
    s, unet_calls = _stub(S, eta=0.5, mask_noise=lambda i, shape, device: (order.append(("blend", i, shape)), torch.zeros(shape))[1],
                          noise=lambda i, shape, device: (order.append(("eta", i, shape)), torch.zeros(shape))[1])
    x_T = torch.randn(1, 4, *canvas)
    counters = Counters(monkeypatch)
    _stub_canvas(s, S, canvas, x_T, eta=0.5, mask=keep_mask(1, *canvas), x0=torch.randn(1, 4, *canvas))
    assert counters.count() == {"window_blend": 1, "sampler_step_windows_masked": S - 1, "sampler_step_windows": 1}
    assert counters.calls[0] == "window_blend" and counters.calls[-1] == "sampler_step_windows" and len(unet_calls) == S
    shape = (1, 4) + canvas
    assert order == [("blend", 0, shape)] + [e for i in range(S) for e in [("eta", i, shape)] + ([("blend", i + 1, shape)] if i + 1 < S else [])]
    # the three-launch form
    counters.calls.clear()
    s.canvas_fused_step = False
    _stub_canvas(s, S, canvas, x_T, eta=0.5, mask=keep_mask(1, *canvas), x0=torch.randn(1, 4, *canvas))
    assert counters.count() == {"latent_blend": 1, "window_split": S, "window_fuse": S, "solver_step_masked": S - 1, "solver_step": 1}


def test_unfused_masked_step_agrees_on_the_host():
    S, canvas = 6, (24, 40)
    x_T, x0 = torch.randn(1, 4, *canvas), torch.randn(1, 4, *canvas)
    qn = _draws(S, 3, (1, 4) + canvas)
    a = _stub_canvas(_stub(S, mask_noise=qn)[0], S, canvas, x_T, mask=keep_mask(1, *canvas), x0=x0)
    b = _stub_canvas(_stub(S, mask_noise=qn, canvas_fused_step=False)[0], S, canvas, x_T, mask=keep_mask(1, *canvas), x0=x0)
    assert torch.isfinite(a).all() and (a - b).abs().max() <= 1e-5 * a.abs().max()


def test_keep_zero_is_sample_canvas_and_keep_one_feeds_q_sample_of_x0():
    from tests.test_inpaint_cpu import _spy
    S, canvas = 4, (16, 40)
    x_T, x0 = torch.randn(1, 4, *canvas), torch.randn(1, 4, *canvas)
    qn = _draws(S, 4, (1, 4) + canvas)
    zero = _stub_canvas(_stub(S, mask_noise=qn)[0], S, canvas, x_T, mask=torch.zeros(1, 1, *canvas), x0=x0)
    plain = _stub_canvas(_stub(S)[0], S, canvas, x_T, method="sample_canvas")
    assert torch.equal(zero, plain)
    s, _ = _stub(S, mask_noise=qn)
    seen = _spy(s)
    _stub_canvas(s, S, canvas, x_T, mask=torch.ones(1, 1, *canvas), x0=x0)
    assert len(seen) == S
    for i, first_window in enumerate(seen):                                     # window 0 of call i: q_sample of x0 at the call's timestep
        q_a, q_b = s._blend_coefs(i)
        assert torch.equal(first_window, (q_a * x0 + q_b * qn[i])[..., :16, :16])


def test_pixel_space_paste_on_a_canvas():
    """image= / mask_px=: last_result["image"] is the composite of ONE decode of the whole canvas; the saved 8-bit pixels are the
    original's where mask_px == 1."""
    from sta import solver
    S, canvas = 4, (16, 40)
    s, _ = _stub(S, mask_noise=_draws(S, 5, (1, 4) + canvas))
    orig_u8 = torch.randint(0, 256, (1, 3, 128, 320), dtype=torch.uint8)
    orig = orig_u8.float() / 255.0
    keep = keep_mask(1, *canvas)
    keep_px = (keep == 1).float().repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)
    saved = []
    s.save_images, s._save = True, lambda image, epoch, seed, prompt_idx, index=0: saved.append(s._to_u8(image.half(), index))
    _stub_canvas(s, S, canvas, torch.randn(1, 4, *canvas), mask=keep, x0=torch.randn(1, 4, *canvas), image=orig, mask_px=keep_px)
    img = s.last_result["image"]
    assert img.shape == (1, 3, 128, 320)
    assert torch.equal(img, solver.image_composite_reference(s.model.decode_first_stage(s.last_result["x0"]), orig, keep_px))
    kept = (keep_px[0, 0] == 1).numpy()
    want = orig_u8[0].permute(1, 2, 0).numpy()
    assert len(saved) == 1 and kept.any() and not kept.all() and (saved[0][kept] == want[kept]).all()


# ---------------------------------------------------------------------------------------------------
# scripts/outpaint.py
# ---------------------------------------------------------------------------------------------------
def _script():
    import importlib.util
    path = os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts", "outpaint.py")
    spec = importlib.util.spec_from_file_location("outpaint_script", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules.pop("img2img", None)          # the script's sibling import: keep it out of other tests' namespace
    return mod


def test_outpaint_parser():
    mod = _script()
    p = mod.build_parser()
    opt = p.parse_args(["--init-img", "a.png", "--canvas", "512x2048"])
    assert (opt.strength, opt.opt_epochs, opt.place, opt.seam, opt.H, opt.W) == (1.0, 0, "0,0", 0, 512, 512) and not opt.dpm_solver
    g, place = mod.check_options(opt)
    assert (g.Hc, g.Wc, g.s, g.stride, g.T) == (64, 256, 64, 32, 7) and place == (0, 0)
    opt = p.parse_args(["--init-img", "a.png", "--canvas", "256x640", "--H", "256", "--W", "256", "--canvas_stride", "128", "--place", "384,0",
                        "--seam", "16", "--dpm_solver", "--opt_epochs", "1"])
    g, place = mod.check_options(opt)
    assert (g.s, g.ox) == (32, (0, 16, 32, 48)) and place == (384, 0) and opt.dpm_solver


@pytest.mark.parametrize("args,what", [
    (["--plms"], "PLMS"),
    (["--strength", "0.5"], "--strength"),
    (["--opt_epochs", "3"], "--opt_epochs"),
    (["--attn_maps"], "--attn_maps"),
    (["--attn_loss", "0.5", "--opt_epochs", "1"], "--attn_loss"),
    (["--attn_guidance", "0.1"], "--attn_guidance"),
    (["--n_samples", "2"], "n_samples"),
    (["--place", "100,0"], "--place X 100"),
    (["--place", "0,12"], "--place Y 12"),
    (["--place", "64"], "X,Y"),
    (["--seam", "12"], "--seam 12"),
    (["--place", "320,0"], "does not lie inside"),                              # 320 + 256 > 512
    (["--place", "0,64"], "does not lie inside"),
    (["--place", "128,0", "--seam", "128"], "nothing of the 256 x 256 picture kept"),
    (["--canvas", "256x256"], "nothing to paint"),
    # every canvas refusal of _txt2img_common.canvas_grid
    (["--canvas", "512"], "HxW"),
    (["--canvas", "256x500"], "500"),
    (["--canvas", "128x512"], "smaller than the window"),
    (["--canvas_stride", "100"], "100"),
    (["--canvas_stride", "320"], "stride"),
    (["--canvas", "256x8192", "--canvas_stride", "64"], "at most 16"),
    (["--W", "512"], "square"),
])
def test_outpaint_cli_refusals(args, what, tmp_path, monkeypatch):
    from tests.test_img2img_cpu import _png
    mod = _script()
    monkeypatch.setattr("sta.pipeline.build_sd_v1", lambda *a, **k: pytest.fail("a model was built"))
    img = _png(str(tmp_path / "a.png"), 256, 256)
    base = ["--init-img", img, "--synthetic", "--H", "256", "--W", "256"]
    if "--canvas" not in args:
        base += ["--canvas", "256x512"]
    with pytest.raises(SystemExit) as e:
        mod.main(base + args)
    assert what in str(e.value), str(e.value)


def test_outpaint_needs_a_canvas_and_an_image(monkeypatch):
    mod = _script()
    monkeypatch.setattr("sta.pipeline.build_sd_v1", lambda *a, **k: pytest.fail("a model was built"))
    with pytest.raises(SystemExit, match="--canvas HxW is required"):
        mod.main(["--init-img", "a.png", "--synthetic"])
    with pytest.raises(SystemExit, match="--canvas_stride 256 needs --canvas"):
        mod.main(["--init-img", "a.png", "--synthetic", "--canvas_stride", "256"])
    with pytest.raises(SystemExit, match="--init-img is required"):
        mod.main(["--synthetic", "--canvas", "512x1024"])


def test_outpaint_keep_masks_by_hand():
    """Picture 256, --place 128,0, --seam 16 on a 256 x 512 canvas: keep = 1 exactly on latent rows 0 .. 31, columns 18 .. 45 (the two
    vertical sides are interior and lose 2 cells each; top and bottom lie on the canvas border); keep_px the same in pixels."""
    mod = _script()
    g = _grid((32, 64, 32, 16))
    keep, keep_px, at = mod.keep_masks(256, (128, 0), 16, g, 8)
    want = torch.zeros(1, 1, 32, 64)
    want[:, :, 0:32, 18:46] = 1.0
    assert torch.equal(keep, want) and at == (0, 16)
    want_px = torch.zeros(1, 1, 256, 512)
    want_px[:, :, :, 144:368] = 1.0
    assert torch.equal(keep_px, want_px)
    assert torch.equal(keep.repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1), keep_px)
    # on the left border only the right side is eroded; without a seam the footprint is kept whole
    keep, _, at = mod.keep_masks(256, (0, 0), 16, g, 8)
    assert keep[0, 0, :, :30].min() == 1 and keep[0, 0, :, 30:].max() == 0 and at == (0, 0)
    keep, _, at = mod.keep_masks(256, (256, 0), 0, g, 8)
    assert keep[0, 0, :, 32:].min() == 1 and keep[0, 0, :, :32].max() == 0 and at == (0, 32)
    # a tall canvas: top and bottom interior
    keep, keep_px, at = mod.keep_masks(256, (0, 128), 8, _grid((64, 32, 32, 16)), 8)
    assert at == (16, 0) and keep.sum() == 30 * 32 and keep[0, 0, 17:47].min() == 1 and keep_px.sum() == 240 * 256
    assert np.isclose(float(keep.mean()), 30 * 32 / (64 * 32))
