"""DPM-Solver++ and DDIM on the MI355X: the sampler-step kernel (csrc/sta_sampler.hip) against a float64 restatement, and the
samplers' trajectories, graph replay, prompt batching and tracked epochs against the reference goldens and the host chain."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from sta.synth import seeded_fill_  # noqa: E402

G = gi.GOLDEN


def _load(name):
    return np.load(os.path.join(G, name), allow_pickle=False)


def _step64(eps, x, m_prev, noise, c, magnitudes=False):
    """float64 restatement of include/sta_unet.h sta_sampler_step; `magnitudes`: also the sums of the absolute terms of m and
    x_next, the scale an fp32 evaluation's rounding is relative to (the terms may cancel)."""
    b = x.shape[0]
    ev = eps.double().reshape(b, 2, *x.shape[1:])
    e = ev[:, 0] + c.scale * (ev[:, 1] - ev[:, 0])
    m = (x.double() - c.sigma_t * e) / c.alpha_t
    xn = c.c_x * x.double() + c.c_m * m + c.c_e * e
    if m_prev is not None:
        xn = xn + c.c_p * m_prev.double()
    if noise is not None:
        xn = xn + c.c_n * noise.double()
    if not magnitudes:
        return xn, m
    ae = ev[:, 0].abs() + abs(c.scale) * (ev[:, 1].abs() + ev[:, 0].abs())
    am = (x.double().abs() + abs(c.sigma_t) * ae) / abs(c.alpha_t)
    axn = abs(c.c_x) * x.double().abs() + abs(c.c_m) * am + abs(c.c_e) * ae
    if m_prev is not None:
        axn = axn + abs(c.c_p) * m_prev.double().abs()
    if noise is not None:
        axn = axn + abs(c.c_n) * noise.double().abs()
    return xn, m, axn, am


def _case(mode):
    from sta.solver import StepCoef
    if mode == "first":
        return StepCoef(7.5, 0.9976, 0.0683, 0.998, 0.0232, 0.0, 0.0, 0.0)
    if mode == "second":
        return StepCoef(7.5, 0.95, 0.31, 0.997, 0.0417, -0.0133, 0.0, 0.0)
    return StepCoef(5.0, 0.6, 0.8, 0.0, 0.9, 0.0, 0.35, 0.22)          # DDIM with noise


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("b", [1, 16, 64])
@pytest.mark.parametrize("side", [64, 96])
@pytest.mark.parametrize("mode", ["first", "second", "noise"])
def test_sampler_step_kernel_vs_fp64(dtype, b, side, mode):
    from sta import solver
    torch.manual_seed(b * 1000 + side)
    c = _case(mode)
    shape = (b, 4, side, side)
    eps = torch.randn((2 * b, 4, side, side), device="cuda").to(dtype)
    x = torch.randn(shape, device="cuda") * 3
    m_prev = torch.randn(shape, device="cuda") if c.c_p else None
    noise = torch.randn(shape, device="cuda") if c.c_n else None
    xn, m, xin = solver.solver_step(eps, x, m_prev, noise, c, want_xin=True)
    rx, rm, ax, am = _step64(eps, x, m_prev, noise, c, magnitudes=True)
    for got, ref, mag in ((xn, rx, ax), (m, rm, am)):
        err = (got.double() - ref).abs()
        assert (err <= 1e-6 * (1 + mag)).all(), (err / (1 + mag)).max().item()       # a few fp32 roundings of the terms
    pair = torch.stack([xn, xn], 1).reshape(2 * b, 4, side, side).to(dtype)
    assert torch.equal(xin, pair)                            # bit-equal to pair(x_next, x_next).to(dtype)
    # the CPU restatement of solver_step agrees with the kernel
    cx, cm, _ = solver.solver_step(eps.cpu().float(), x.cpu(), None if m_prev is None else m_prev.cpu(),
                                   None if noise is None else noise.cpu(), c)
    assert ((cx.double() - xn.cpu().double()).abs() <= 2e-6 * (1 + ax.cpu())).all()
    assert ((cm.double() - m.cpu().double()).abs() <= 2e-6 * (1 + am.cpu())).all()
    # backward: SolverStepFn (sta_sampler_step_bwd) vs autograd of the float64 restatement
    e_ = eps.float().requires_grad_(True)
    x_ = x.clone().requires_grad_(True)
    mp_ = None if m_prev is None else m_prev.clone().requires_grad_(True)
    gx, gm = torch.randn(shape, device="cuda"), torch.randn(shape, device="cuda")
    a, bm, _ = solver.solver_step(e_, x_, mp_, noise, c, dtype=dtype)
    torch.autograd.backward([a, bm], [gx, gm])
    e64 = eps.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    mp64 = None if m_prev is None else m_prev.double().requires_grad_(True)
    ra, rb = _step64(e64, x64, mp64, noise, c)
    torch.autograd.backward([ra, rb], [gx.double(), gm.double()])
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    gmag = gx.double().abs() * abs(c.c_x) + (gm.double().abs() + abs(c.c_m) * gx.double().abs()) / abs(c.alpha_t)
    assert ((x_.grad.double() - x64.grad).abs() <= 1e-6 * (1 + gmag)).all()
    assert ((e_.grad.double() - e64.grad).abs() <= ulp * e64.grad.abs() + 1e-6).all()      # dL/deps rounded to the UNet's dtype
    if mp_ is not None:
        assert torch.allclose(mp_.grad.double(), mp64.grad, rtol=1e-6, atol=1e-6)


def _golden_unet(dtype):
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    meta = json.load(open(os.path.join(G, "unet_state_dict_keys.json")))
    unet = UNetModel(**meta["cfg"]).eval()
    seeded_fill_(unet, 21)
    for p in unet.parameters():
        p.requires_grad_(False)
    return unet.to("cuda", dtype)


def _golden_run(sampler, g, prefix, S, W, graph=False):
    from sta import prompt_state
    c, local_ctx, x_T = gi.unet_inputs(int(g["K"]), int(g["input_seed"]))
    sampler.make_schedule(S, ddim_eta=float(g[prefix + "eta"]) if prefix + "eta" in g else 0.0, verbose=False)
    tr = sampler._time_range()
    with torch.no_grad():
        prompt_state.begin_prompt([l.cuda() for l in local_ctx], first_timestep=int(tr[0]))
        return sampler._trajectory(x_T.cuda(), c.cuda(), gi.load_uncond().cuda(), float(g["scale"]), tr, torch.from_numpy(W).cuda(),
                                   [list(cc) for cc in g["centres"]], 0, graph=graph)


def _within(img, ref, tol_max, tol_mean, what):
    err = np.abs(img.float().cpu().numpy() - ref)
    print("%s: max %.3f %%, mean %.3f %%" % (what, 100 * err.max() / np.abs(ref).max(), 100 * err.mean() / np.abs(ref).mean()))
    assert err.max() <= tol_max * np.abs(ref).max(), (what, err.max(), np.abs(ref).max())
    assert err.mean() <= tol_mean * np.abs(ref).mean(), (what, err.mean(), np.abs(ref).mean())


TOLS = [(torch.float16, 0.01, 0.005), (torch.bfloat16, 0.03, 0.02)]


@pytest.mark.parametrize("dtype,tol_max,tol_mean", TOLS)
def test_dpm_solver_trajectory_vs_reference_golden(dtype, tol_max, tol_mean):
    """Final x of the reference's DPM-Solver++(2M) at S = 20 and S = 10 (per-call weight columns, CFG 7.5) on the GPU vs the
    reference's fp32 CPU run. Tolerances as test_plms_trajectory_vs_reference_golden: fp16 max 1 %, mean 0.5 %; bf16 max 3 %,
    mean 2 % of max|x| / mean|x| (measured: fp16 0.22 % / 0.22 % at S = 20, 0.31 % / 0.23 % at S = 10; bf16 1.41 % / 1.05 %,
    1.47 % / 1.20 %)."""
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    g = _load("dpm_traj.npz")
    model = LatentDiffusion(unet_config=_golden_unet(dtype)).cuda()
    sampler = DPMSolverSampler(model, opt_epochs=0, use_graph=False, save_images=False)
    for S in (20, 10):
        img = _golden_run(sampler, g, "S%d_" % S, S, g["S%d_W" % S])
        _within(img, g["S%d_x0" % S], tol_max, tol_mean, "dpm S=%d %s" % (S, dtype))


@pytest.mark.parametrize("dtype,tol_max,tol_mean", TOLS)
def test_ddim_trajectory_vs_reference_golden(dtype, tol_max, tol_mean):
    """DDIM at eta 0 (S = 20) and eta 0.5 (S = 10, the reference's recorded noise) on the GPU vs the reference's fp32 CPU run;
    same tolerances (measured: fp16 0.23 % / 0.22 % at eta 0, 0.25 % / 0.23 % at eta 0.5; bf16 1.33 % / 1.05 %, 1.29 % / 1.21 %)."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.ddpm import LatentDiffusion
    g = _load("ddim_traj.npz")
    model = LatentDiffusion(unet_config=_golden_unet(dtype)).cuda()
    for tag in ("eta0", "eta05"):
        noise = [torch.from_numpy(n) for n in g[tag + "_noise"]] if tag + "_noise" in g else None
        sampler = DDIMSampler(model, opt_epochs=0, use_graph=False, save_images=False, noise=noise)
        img = _golden_run(sampler, g, tag + "_", int(g[tag + "_S"]), g[tag + "_W"])
        _within(img, g[tag + "_x0"], tol_max, tol_mean, "ddim %s %s" % (tag, dtype))


def _sample(sampler, S, c, x_T, local_ctx, rep=0):
    sampler.sample(S=S, conditioning=c.cuda() * (1 + rep), batch_size=1, shape=[4, 32, 32], verbose=False,
                   unconditional_guidance_scale=7.5, unconditional_conditioning=gi.load_uncond().cuda(), eta=0.0,
                   x_T=x_T.cuda(), text_index=0, curr_text="x", bboxs_curr=[[0.3, 0.4], [0.7, 0.6 - 0.1 * rep]], seed=1,
                   prompt_idx=0, object_names=["a", "b"], local_conditionings=[l.cuda() for l in local_ctx])
    return sampler.last_result["x0"].clone()


def test_solver_graph_replay_matches_eager():
    """hipGraph replay == eager launches for DPM-Solver++ and DDIM, including a graph cache first filled by PLMS (integer
    timesteps) and then used by DPM-Solver++ (fractional model times: a separate capture, not a truncating copy)."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    c, local_ctx, x_T = gi.unet_inputs(2, 41)
    model = LatentDiffusion(unet_config=_golden_unet(torch.float16)).cuda()
    res = {}
    for cls in (DPMSolverSampler, DDIMSampler):
        for graph in (False, True):
            res[(cls.__name__, graph)] = _sample(cls(model, opt_epochs=0, use_graph=graph, save_images=False), 10, c, x_T, local_ctx)
    plms = PLMSSampler(model, opt_epochs=0, use_graph=True, save_images=False)
    _sample(plms, 10, c, x_T, local_ctx)
    dpm = DPMSolverSampler(model, opt_epochs=0, use_graph=True, save_images=False)
    dpm._graphs = plms._graphs                                   # the same process-wide cache of captures
    shared = _sample(dpm, 10, c, x_T, local_ctx)
    assert len(plms._graphs._entries) == 2 and {k[2] for k in plms._graphs._entries} == {torch.long, torch.float32}
    for name in ("DPMSolverSampler", "DDIMSampler"):
        a, b = res[(name, False)].float(), res[(name, True)].float()
        assert (a - b).abs().max() <= 0.02 * a.abs().max(), (name, (a - b).abs().max(), a.abs().max())
    a = res[("DPMSolverSampler", False)].float()
    assert (a - shared.float()).abs().max() <= 0.02 * a.abs().max()
    # a second prompt re-uses the capture with refilled K/V buffers
    other = _sample(dpm, 10, c, x_T, local_ctx, rep=1)
    assert (other.float() - shared.float()).abs().max() > 0.05 * shared.float().abs().max()


def test_dpm_solver_sample_batch_equals_prompt_by_prompt():
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    model = LatentDiffusion(unet_config=_golden_unet(torch.float16)).cuda()
    I, K = 4, 2
    cs, locs, xts, boxes = [], [], [], []
    for i in range(I):
        c, local_ctx, x_T = gi.unet_inputs(K, 50 + i)
        cs.append(c.cuda()), locs.append([l.cuda() for l in local_ctx]), xts.append(x_T.cuda())
        boxes.append([[0.3 + 0.1 * i, 0.4], [0.7, 0.6 - 0.1 * i]])
    uc = gi.load_uncond().cuda()
    sampler = DPMSolverSampler(model, opt_epochs=0, use_graph=False, save_images=False)
    sampler.sample_batch(S=8, shape=[4, 32, 32], conditionings=cs, unconditional_conditionings=uc, bboxs=boxes,
                         object_names=[["a", "b"]] * I, local_conditionings=locs, x_T=torch.cat(xts), seed=1)
    batch = sampler.last_result["x0"].clone()
    for i in range(I):
        sampler.sample(S=8, conditioning=cs[i], batch_size=1, shape=[4, 32, 32], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=uc, x_T=xts[i], text_index=0, curr_text="x", bboxs_curr=boxes[i], seed=1,
                       prompt_idx=i, object_names=["a", "b"], local_conditionings=locs[i])
        one = sampler.last_result["x0"]
        assert (batch[i:i + 1] - one).abs().max() <= 0.01 * one.abs().max(), (i, (batch[i:i + 1] - one).abs().max())


def _wopt_model(dtype, device):
    from ldm.models.autoencoder import AutoencoderKL
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    meta = json.load(open(os.path.join(G, "unet_state_dict_keys.json")))
    unet = UNetModel(**dict(meta["cfg"], use_checkpoint=False)).eval()
    seeded_fill_(unet, 21)
    vae = AutoencoderKL(ddconfig=dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32,
                                      ch_mult=[1, 2, 4, 4], num_res_blocks=1, attn_resolutions=[], dropout=0.0))
    seeded_fill_(vae, 3)
    model = LatentDiffusion(unet_config=unet.to(dtype), first_stage_config=vae.to(dtype)).to(device)
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def _wopt_epoch(model, loss_model, device, loss_scale=None):
    """Two epochs x 4 DPM-Solver++ calls; returns (result, dLoss/dW of the tracked epoch)."""
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    c, local_ctx, x_T = gi.unet_inputs(2, 6)
    sampler = DPMSolverSampler(model, loss_model=loss_model, opt_epochs=2, save_images=False, use_graph=device != "cpu",
                               loss_scale=loss_scale)
    grads = []
    orig_step = torch.optim.Adam.step
    torch.optim.Adam.step = lambda self, *a, **k: (grads.append(self.param_groups[0]["params"][0].grad.clone()), orig_step(self, *a, **k))[1]
    try:
        sampler.sample(S=4, conditioning=c.to(device), batch_size=1, shape=[4, 32, 32], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond().to(device), x_T=x_T.to(device), text_index=0, curr_text="two things",
                       bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], seed=1, prompt_idx=0, object_names=["The cat", "dog"],
                       local_conditionings=[l.to(device) for l in local_ctx])
    finally:
        torch.optim.Adam.step = orig_step
    return sampler, grads[0][0].float().cpu()


_DPM_REF = {}


@pytest.mark.parametrize("recompute", ["call", "none"])
def test_dpm_solver_tracked_epoch_gradient(recompute):
    """A tracked DPM-Solver++ epoch (S = 4, K = 2, bf16) through SolverStepFn (sta_sampler_step_bwd), the HIP backward kernels, the
    VAE decoder and the CLIP-loss front end: dLoss/dW against the fp32 host chain with the oracle op, under per-call recomputation
    and eagerly; the Adam step moves W (measured max |dW - dW_ref| / max |dW_ref|: 0.009 per call, 0.047 eager)."""
    from ldm.models.diffusion.plms import DCLIPLoss
    from sta.pipeline import set_recompute
    from sta.synth import SyntheticCLIP
    from tests.cpu_backend import oracle_ops
    if not _DPM_REF:
        with oracle_ops():
            s, g = _wopt_epoch(_wopt_model(torch.float32, "cpu"), DCLIPLoss(SyntheticCLIP()), "cpu")
        _DPM_REF.update(grad=g, loss=s.last_result["losses"][0])
    model = _wopt_model(torch.bfloat16, "cuda")
    assert set_recompute(model, recompute) == recompute
    sampler, g = _wopt_epoch(model, DCLIPLoss(SyntheticCLIP().cuda()), "cuda")
    r = sampler.last_result
    if recompute == "call":
        assert sampler.last_kept_calls >= 1
    step = (r["W"].cpu() - 2.5).abs()
    assert (step > 0).all() and (step <= 0.005 + 1e-5).all(), step
    ref = _DPM_REF["grad"]
    assert abs(r["losses"][0] - _DPM_REF["loss"]) <= 0.01 * abs(_DPM_REF["loss"]), (r["losses"][0], _DPM_REF["loss"])
    e_max = ((g - ref).abs().max() / ref.abs().max()).item()
    print("dpm recompute=%s: max |dW - dW_ref| / max |dW_ref| = %.3f" % (recompute, e_max))
    assert e_max <= 0.15, e_max


def test_dpm_solver_fp16_tracked_epoch_with_loss_scale():
    """fp16 tracked DPM-Solver++ epoch with the sampler's default loss scale: a finite, non-zero dLoss/dW."""
    from ldm.models.diffusion.plms import DCLIPLoss
    from sta.pipeline import set_recompute
    from sta.synth import SyntheticCLIP
    model = _wopt_model(torch.float16, "cuda")
    set_recompute(model, "none")
    sampler, g = _wopt_epoch(model, DCLIPLoss(SyntheticCLIP().cuda()), "cuda")
    assert torch.isfinite(g).all() and (g != 0).all(), g
    assert sampler._loss_scale(sampler.last_result["losses"][0]) > 1.0
