"""Attention-guided latent updates without a GPU: guide_reference by hand, the refusals of sta_latent_guide (fake pointers: none of
these calls may reach a launch), the host chain on the miniature of tests/test_attnloss_cpu.py (oracle-backed blocks, fp32) for the
three samplers and both block modes, the off states, the clean-up and the CLI. The kernel is checked in test_guidance_gpu.py."""
import ctypes
import os
import sys

import pytest
import torch

from oracle import golden_inputs as gi
from tests.cpu_backend import oracle_ops
from tests.test_attnloss_cpu import CENTRES, K, LAT, RES, S, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STA_E_ARG, STA_E_UNSUP = -1, -2
P = 0x10000                                            # a fake device pointer: non-null, 16-byte aligned, never read
ACP_751 = None                                         # alphas_cumprod[751] of the model's schedule, filled by _run


# ---------------------------------------------------------------------------------------------------
# guide_reference
# ---------------------------------------------------------------------------------------------------
def _hand():
    """2 images, n = 16 (2 channels of hw = 8): x, the gradient pair, keep."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 2, 2, 4, generator=g)
    gp = torch.randn(4, 2, 2, 4, generator=g)
    keep = torch.zeros(2, 1, 2, 4)
    keep[0, 0, 0, :2] = 1.0
    keep[1, 0, 1, 1:] = 0.5
    return x, gp, keep


def test_guide_reference_by_hand():
    from sta.guidance import guide_reference
    x, gp, keep = _hand()
    step = torch.tensor([0.3, 0.7])
    for kp in (None, keep):
        d = gp[0::2] + gp[1::2]
        if kp is not None:
            d = d * (1.0 - kp)
        rms = torch.stack([d[i].pow(2).sum().div(16).sqrt() for i in range(2)])
        out, got_rms = guide_reference(gp, x, step, keep=kp, normalize=True)
        assert torch.allclose(got_rms, rms, rtol=1e-6, atol=0)
        for i in range(2):
            assert torch.allclose(out[i], x[i] - step[i] / rms[i] * d[i], rtol=1e-6, atol=1e-7)
            # a normalised step moves the image by exactly step in rms
            assert abs((out[i] - x[i]).pow(2).mean().sqrt().item() - step[i].item()) < 1e-6
        out, _ = guide_reference(gp, x, step, keep=kp, normalize=False, inv_scale=0.25)
        for i in range(2):
            assert torch.allclose(out[i], x[i] - step[i] * 0.25 * d[i], rtol=1e-6, atol=1e-7)
        if kp is not None:
            assert torch.equal(out[0, :, 0, :2], x[0, :, 0, :2])                # keep == 1: not guided, in every channel
    # a power-of-two loss scale cancels exactly in the normalised update and is undone by inv_scale in the plain one
    a, _ = guide_reference(gp, x, step)
    b, _ = guide_reference(gp * 1024.0, x, step)
    assert torch.equal(a, b)
    a, _ = guide_reference(gp, x, step, normalize=False)
    b, _ = guide_reference(gp * 1024.0, x, step, normalize=False, inv_scale=1.0 / 1024.0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("normalize", [True, False])
def test_guide_reference_skips_zero_and_non_finite_rows(normalize):
    from sta.guidance import guide_reference, latent_guide
    x, gp, _ = _hand()
    gp[0:2] = 0.0                                                               # image 0: an all-zero gradient
    gp[3, 1, 0, 2] = float("inf")                                               # image 1: one Inf
    out, rms = guide_reference(gp, x, 0.5, normalize=normalize)
    assert torch.equal(out, x) and rms[0].item() == 0.0 and not torch.isfinite(rms[1])
    gp[3, 1, 0, 2] = float("nan")
    out, rms = guide_reference(gp, x, 0.5, normalize=normalize)
    assert torch.equal(out, x) and torch.isnan(rms[1])
    gp[3, 1, 0, 2] = 1.0                                                        # image 1 live again: image 0 still untouched
    out, xin, rms = latent_guide(gp, x, 0.5, normalize=normalize, dtype=torch.bfloat16, want_xin=True)
    assert torch.equal(out[0], x[0]) and not torch.equal(out[1], x[1]) and rms[1] > 0
    assert xin.dtype == torch.bfloat16 and torch.equal(xin[0::2], out.to(torch.bfloat16)) and torch.equal(xin[1::2], xin[0::2])


# ---------------------------------------------------------------------------------------------------
# C-ABI
# ---------------------------------------------------------------------------------------------------
def _call(L, g=P, x=P + 0x1000, keep=P + 0x2000, step=P + 0x3000, x_out=P + 0x4000, xin=P + 0x5000, stats=P + 0x6000, b=1, n=64, hw=32,
          normalize=1, inv_scale=1.0, dtype=0):
    rc = L.sta_latent_guide(g, x, keep, step, x_out, xin, stats, b, n, hw, normalize, inv_scale, dtype, None)
    return rc, L.sta_last_error().decode()


def test_abi_symbol_and_refusals_reach_no_launch():
    from sta import lib
    L = lib.load()
    res, args = lib.SYMBOLS["sta_latent_guide"]
    vp, i, f, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    assert res is i and args == [vp] * 7 + [l, l, l, i, f, i, vp]
    header = open(os.path.join(ROOT, "include", "sta_unet.h")).read()
    assert "int sta_latent_guide(const void* g, const float* x, const float* keep, const float* step, float* x_out, void* xin, float* stats," in header
    # built as part of the sampler step's translation unit, not a source of its own (tests/test_abi_dtype_cpu.py pins lib.SOURCES)
    assert lib.INCLUDED_SOURCES["sta_guide.hip"] == "sta_sampler.hip"
    names = [os.path.basename(s) for s in lib.SOURCES]
    assert "sta_guide.hip" not in names and "sta_sampler.hip" in names and len(names) == 19
    assert '#include "sta_guide.hip"' in open(os.path.join(lib.CSRC, "sta_sampler.hip")).read()
    assert os.path.isfile(os.path.join(lib.CSRC, "sta_guide.hip"))
    cases = [
        (dict(g=0), STA_E_ARG, "null pointer"),
        (dict(x=0), STA_E_ARG, "null pointer"),
        (dict(step=0), STA_E_ARG, "null pointer"),
        (dict(x_out=0), STA_E_ARG, "null pointer"),
        (dict(n=60, hw=4), STA_E_ARG, "n=60"),
        (dict(n=64, hw=4), STA_E_ARG, "hw=4"),
        (dict(n=64, hw=24), STA_E_ARG, "hw=24"),
        (dict(n=64, hw=0), STA_E_ARG, "hw=0"),
        (dict(b=0), STA_E_ARG, "b=0"),
        (dict(g=P + 8), STA_E_ARG, "16-byte aligned"),
        (dict(x=P + 0x1004), STA_E_ARG, "16-byte aligned"),
        (dict(keep=P + 0x2008), STA_E_ARG, "16-byte aligned"),
        (dict(x_out=P + 0x4008), STA_E_ARG, "16-byte aligned"),
        (dict(xin=P + 0x5002), STA_E_ARG, "16-byte aligned"),
        (dict(step=P + 0x3002), STA_E_ARG, "16-byte aligned"),
        (dict(x_out=P + 0x1000), STA_E_ARG, "aliases an input"),               # x_out == x
        (dict(xin=P), STA_E_ARG, "aliases an input"),                          # xin == g
        (dict(x_out=P + 0x1000 + 0x80), STA_E_ARG, "aliases an input"),        # overlaps the tail of x (64 floats = 0x100 bytes)
        (dict(stats=P + 0x4000), STA_E_ARG, "alias each other"),
        (dict(dtype=7), STA_E_UNSUP, "dtype 7"),
    ]
    for kw, code, text in cases:
        rc, err = _call(L, **kw)
        assert rc == code and text in err, (kw, rc, err)
    assert _call(L, dtype=7)[1] == "dtype 7"                                    # the same text every entry point gives
    assert _call(L, dtype=7, keep=0, xin=0, stats=0)[1] == "dtype 7"            # the optional pointers may be NULL


# ---------------------------------------------------------------------------------------------------
# host miniature (DDIM S = 4, first call at t = 751)
# ---------------------------------------------------------------------------------------------------
_RUNS = {}


def _run(kind="ddim", opt_epochs=0, hooks=False, **gkw):
    """One sample() on the miniature -> dict(sampler, guidance, x0, entered: names of the UNet stages whose forward was entered
    while an update's evaluation ran). gkw: AttnGuidance keywords, or `guidance=None`."""
    key = (kind, opt_epochs, hooks, tuple(sorted(gkw.items())))
    if key in _RUNS:
        return _RUNS[key]
    global ACP_751
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    from sta.attnloss import AttnLayoutLoss
    from sta.guidance import AttnGuidance
    model = _model()
    ACP_751 = float(model.alphas_cumprod[751])
    unet = model.model.diffusion_model
    guidance = None if "guidance" in gkw else AttnGuidance(unet, resolution=RES, **gkw)
    cls = dict(ddim=DDIMSampler, plms=PLMSSampler, dpm=DPMSolverSampler)[kind]
    extra = dict(attn_loss=AttnLayoutLoss(unet, resolution=RES)) if opt_epochs > 1 else {}
    sampler = cls(model, loss_model=None, opt_epochs=opt_epochs, use_graph=False, save_images=False, latent_guidance=guidance, **extra)
    entered, handles = [], []
    if hooks:
        stages = [("in%d" % i, m) for i, m in enumerate(unet.input_blocks)] + [("mid", unet.middle_block)] + \
                 [("out%d" % i, m) for i, m in enumerate(unet.output_blocks)]
        for name, m in stages:
            handles.append(m.register_forward_pre_hook(lambda mod, args, name=name: entered.append(name) if torch.is_grad_enabled() else None))
    c, local_ctx, x_T = gi.unet_inputs(K, 5)
    try:
        with oracle_ops():
            sampler.sample(S=S, conditioning=c, batch_size=1, shape=[4, LAT, LAT], verbose=False, unconditional_guidance_scale=7.5,
                           unconditional_conditioning=gi.load_uncond(), eta=0.0, x_T=x_T[:, :, :LAT, :LAT], text_index=0,
                           curr_text="a cat left of a dog", bboxs_curr=CENTRES, seed=1, prompt_idx=0, object_names=["cat", "dog"],
                           local_conditionings=local_ctx)
    finally:
        for h in handles:
            h.remove()
    _RUNS[key] = dict(sampler=sampler, guidance=guidance, model=model, x0=sampler.last_result["x0"], entered=entered)
    return _RUNS[key]


def _first_order(r, eta):
    """(E0 - E1, the first-order prediction step rms numel) of the first guided call of a run with iters = 2. The update moves x by
    `step` in rms along -g, so E falls by step |g|^2 / (rms sqrt(numel)) = step rms numel to first order; the step the sampler
    applies is eta (1 - alphas_cumprod[t]), at t = 751 0.947 eta."""
    res = r["sampler"].last_guidance
    e0, e1, rms = res["energy"][0, 0].item(), res["energy"][1, 0].item(), res["rms"][0, 0].item()
    return e0 - e1, eta * (1.0 - ACP_751) * rms * 4 * LAT * LAT


@pytest.mark.parametrize("blocks", ["all", "down"])
def test_small_step_matches_first_order(blocks):
    """eta = 0.01, steps = 1, iters = 2: the energy before update 2 is the energy after update 1, and its drop is the first-order
    prediction within 5 %. Measured: blocks="all" E 0.80166 -> 0.79905, drop 0.00261 against 0.00260 predicted (rms 6.72e-5; with a
    bare step eta, without the schedule factor 0.947, the figures are 0.00277 against 0.00275); blocks="down" 0.00337 against 0.00336."""
    r = _run("ddim", scale=0.01, steps=1, iters=2, blocks=blocks)
    res = r["sampler"].last_guidance
    assert res["calls"] == [(0, 0), (0, 1)] and res["skipped"] == 0 and res["energy"].shape == (2, 1) and res["rms"].shape == (2, 1)
    assert torch.isfinite(res["rms"]).all() and (res["rms"] > 0).all()
    drop, want = _first_order(r, 0.01)
    print("blocks=%s: E0 %.5f, E0 - E1 %.5f, first order %.5f (rel %.4f), rms %.3e"
          % (blocks, res["energy"][0, 0].item(), drop, want, abs(drop - want) / want, res["rms"][0, 0].item()))
    if blocks == "all":
        assert abs(res["energy"][0, 0].item() - 0.80166) < 2e-5 and abs(res["rms"][0, 0].item() - 6.72e-5) < 5e-7
    assert want > 0 and abs(drop - want) <= 0.05 * want, (drop, want)
    assert torch.isfinite(r["x0"]).all()


def test_larger_step_lowers_the_energy():
    """eta = 0.1: E1 < E0 - 0.02 (measured: 0.80166 -> 0.77528, a drop of 0.0264)."""
    res = _run("ddim", scale=0.1, steps=1, iters=2, blocks="all")["sampler"].last_guidance
    e0, e1 = res["energy"][0, 0].item(), res["energy"][1, 0].item()
    print("eta = 0.1: E0 %.5f E1 %.5f drop %.5f" % (e0, e1, e0 - e1))
    assert e1 < e0 - 0.02, (e0, e1)


def test_down_mode_runs_the_encoder_up_to_the_last_recording_block_only():
    """blocks="down" at 8 x 8 on a 32 x 32 latent: the evaluations enter input stages 0 .. 8 (the two level-2 stages 7 and 8 hold the
    recording blocks), never a later input stage, the middle block or an output block; blocks="all" enters every stage."""
    r = _run("ddim", hooks=True, scale=0.01, steps=1, iters=2, blocks="down")
    assert r["entered"] == ["in%d" % i for i in range(9)] * 2, r["entered"]
    assert r["guidance"].loss.block_calls == 2 * 2                              # two recording blocks, two evaluations
    assert torch.isfinite(r["sampler"].last_guidance["rms"]).all()
    full = _run("ddim", hooks=True, scale=0.01, steps=1, iters=2, blocks="all")
    assert len(full["entered"]) == 2 * (12 + 1 + 12) and full["guidance"].loss.block_calls == 2 * 5


def test_off_states_are_bit_identical_and_nothing_stays_attached(monkeypatch):
    from ldm.modules.attention import BasicTransformerBlock
    from sta import guidance
    plain = _run("ddim", guidance=None)
    assert plain["sampler"].last_guidance is None
    calls = []
    real = guidance.latent_guide
    monkeypatch.setattr(guidance, "latent_guide", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for kw in (dict(scale=0.0, steps=3), dict(scale=0.1, steps=0)):
        off = _run("ddim", **kw)
        assert torch.equal(off["x0"], plain["x0"]) and off["sampler"].last_guidance is None and not calls
        assert off["guidance"].loss.block_calls == 0
    on = _run("ddim", scale=0.1, steps=2, iters=1, blocks="all")
    assert len(calls) == 2 and not torch.equal(on["x0"], plain["x0"]) and torch.isfinite(on["x0"]).all()
    for r in (plain, on):
        assert all(b._attn_loss is None for b in r["model"].modules() if isinstance(b, BasicTransformerBlock))


def test_an_exception_inside_update_detaches_the_collector(monkeypatch):
    from ldm.modules.attention import BasicTransformerBlock
    from sta import guidance

    def boom(*a, **k):
        raise ZeroDivisionError("inside update")
    monkeypatch.setattr(guidance, "latent_guide", boom)
    _RUNS.pop(("ddim", 0, False, (("blocks", "down"), ("scale", 0.05), ("steps", 1))), None)
    model = {}
    orig = guidance.AttnGuidance.__init__
    monkeypatch.setattr(guidance.AttnGuidance, "__init__", lambda self, unet, **k: (model.setdefault("unet", unet), orig(self, unet, **k))[1])
    with pytest.raises(ZeroDivisionError):
        _run("ddim", scale=0.05, steps=1, blocks="down")
    blocks = [b for b in model["unet"].modules() if isinstance(b, BasicTransformerBlock)]
    assert len(blocks) == 16 and all(b._attn_loss is None for b in blocks)


def test_tracked_epochs_are_never_guided(monkeypatch):
    """opt_epochs = 2 with an attention loss: the tracked epoch (autograd on) calls update zero times, the kept one `steps` times."""
    from sta import guidance
    seen = []
    orig = guidance.AttnGuidance.update
    monkeypatch.setattr(guidance.AttnGuidance, "update", lambda self, *a, **k: (seen.append(torch.is_grad_enabled()), orig(self, *a, **k))[1])
    traj = []
    from ldm.models.diffusion.plms import SolverSamplerBase
    orig_traj = SolverSamplerBase._trajectory
    monkeypatch.setattr(SolverSamplerBase, "_trajectory", lambda self, *a, **k: (traj.append((torch.is_grad_enabled(), len(seen))), orig_traj(self, *a, **k))[1])
    r = _run("ddim", opt_epochs=2, scale=0.05, steps=3, iters=1, blocks="down")
    assert [t[0] for t in traj] == [True, False]                               # the tracked epoch, then the kept one
    assert traj[1][1] == 0 and seen == [False] * 3                             # nothing before the kept trajectory started
    assert r["sampler"].last_guidance["calls"] == [(0, 0), (1, 0), (2, 0)] and len(r["sampler"].last_result["losses"]) == 1


@pytest.mark.parametrize("kind", ["plms", "dpm"])
def test_plms_and_dpm_solver_miniatures(kind):
    """steps = 2, iters = 2 at eta = 0.1: steps x iters entries, finite, and E before update 2 below E before update 1."""
    r = _run(kind, scale=0.1, steps=2, iters=2, blocks="down")
    res = r["sampler"].last_guidance
    assert res["calls"] == [(0, 0), (0, 1), (1, 0), (1, 1)] and res["skipped"] == 0
    assert torch.isfinite(r["x0"]).all() and torch.isfinite(res["energy"]).all() and torch.isfinite(res["rms"]).all()
    print(kind, res["energy"].reshape(-1).tolist())
    assert res["energy"][1, 0] < res["energy"][0, 0]
    assert not torch.equal(r["x0"], _run(kind, guidance=None)["x0"])


def test_prompts_without_objects_and_bad_arguments():
    from sta.guidance import AttnGuidance
    unet = _model().model.diffusion_model
    g = AttnGuidance(unet, resolution=RES, scale=0.1, steps=2)
    g.begin([[]], texts=["a landscape"], names=[[]])
    assert not g.ready
    with pytest.raises(ValueError, match="blocks"):
        AttnGuidance(unet, blocks="up")
    with pytest.raises(ValueError, match="iters"):
        AttnGuidance(unet, iters=0)
    with pytest.raises(RuntimeError, match="bind"):
        g.update(torch.zeros(1, 4, 32, 32), None, None, None, 0, 0.5)


# ---------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------
def _cli():
    sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts"))
    import _txt2img_common as c
    return c


def test_cli_attn_guidance_parses_and_refuses(monkeypatch):
    c = _cli()
    p = c.build_parser("x.json")
    opt = p.parse_args(["--opt_epochs", "0"])
    assert opt.attn_guidance is None and opt.attn_guidance_steps == 10 and opt.attn_guidance_iters == 1
    opt = p.parse_args(["--opt_epochs", "0", "--attn_guidance", "0.2", "--attn_guidance_steps", "5", "--attn_guidance_iters", "2"])
    assert opt.attn_guidance == 0.2 and opt.attn_guidance_steps == 5 and opt.attn_guidance_iters == 2 and opt.attn_res == 16
    for bad in (["--attn_guidance", "0"], ["--attn_guidance", "-1"], ["--attn_guidance", "nan"], ["--attn_guidance_iters", "0"],
                ["--attn_guidance_steps", "-1"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    import sta.pipeline
    monkeypatch.setattr(sta.pipeline, "build_sd_v1", lambda *a, **k: pytest.fail("a model was built"))
    c.check_options(opt)
    with pytest.raises(SystemExit, match="square image"):
        c.check_options(p.parse_args(["--opt_epochs", "0", "--attn_guidance", "0.1", "--H", "512", "--W", "768"]))
    with pytest.raises(SystemExit, match="square image"):
        c.check_options(p.parse_args(["--opt_epochs", "0", "--attn_guidance", "0.1", "--H", "480", "--W", "480"]))
    with pytest.raises(SystemExit, match="no transformer level"):
        c.check_options(p.parse_args(["--opt_epochs", "0", "--attn_guidance", "0.1", "--attn_res", "64", "--H", "256", "--W", "256"]))
    # the other entry points take the same flags through the same check
    import img2img
    import inpaint
    for mod, extra in ((img2img, []), (inpaint, ["--mask_from_layout", "0.2", "--layout", "l.json"])):
        q = mod.build_parser()
        o = q.parse_args(["--init-img", "x.png", "--attn_guidance", "0.3", "--attn_res", "8"] + extra)
        assert o.attn_guidance == 0.3 and o.attn_guidance_steps == 10 and o.attn_res == 8
        with pytest.raises(SystemExit):
            q.parse_args(["--init-img", "x.png", "--attn_guidance", "0"] + extra)
        mod.check_options(o)
        with pytest.raises(SystemExit, match="no transformer level"):           # a 256 x 256 image has levels 32, 16, 8, 4
            c.check_guidance_option(q.parse_args(["--init-img", "x.png", "--attn_guidance", "0.3", "--attn_res", "64"] + extra), side=256)
