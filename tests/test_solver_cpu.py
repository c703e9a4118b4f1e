"""DPM-Solver++ and DDIM samplers on CPU: schedule tables and trajectories against the reference's own samplers
(tests/golden/{dpm_schedule,dpm_traj,ddim_traj}.npz, tools/gen_solver_golden.py), and the CLI's sampler choice.

The HIP entry points of the UNet are swapped for the oracle's fused form (tests/cpu_backend.py) and the sampler step runs as
its torch restatement (sta.solver.step_reference); the kernels are checked in tests/test_solver_gpu.py.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import golden_inputs as gi
from sta.synth import seeded_fill_
from tests.cpu_backend import oracle_ops

G = gi.GOLDEN
ROOT = os.path.dirname(G.rstrip("/")).rsplit("/tests", 1)[0]


def _load(name):
    return np.load(os.path.join(G, name), allow_pickle=False)


def _model():
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    meta = json.load(open(os.path.join(G, "unet_state_dict_keys.json")))
    unet = UNetModel(**meta["cfg"]).eval()
    checksum = seeded_fill_(unet, 21)
    return LatentDiffusion(unet_config=unet), checksum


def _alphas_cumprod():
    from ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(unet_config=torch.nn.Identity()).alphas_cumprod


def _expected_orders(S):
    return [1] + [2] * (S - 2) + [1 if S < 15 else 2]


def test_dpm_schedule_tables_match_reference():
    from sta import solver
    g = _load("dpm_schedule.npz")
    acp = _alphas_cumprod()
    np.testing.assert_allclose(acp.numpy(), g["alphas_cumprod"], rtol=1e-6)
    for S in (10, 20, 25, 50):
        t = solver.dpm_tables(acp, S)
        np.testing.assert_array_equal(t["t"], g["S%d_t" % S])
        np.testing.assert_array_equal(t["t_in"], g["S%d_t_in" % S][:S])
        assert float(t["t_in"][0]) == 999.0 and int(t["t_in"][0]) == 999
        for k, ref in (("alpha", "alpha"), ("sigma", "sigma"), ("lam", "lambda")):
            np.testing.assert_allclose(t[k], g["S%d_%s" % (S, ref)], rtol=2e-6, atol=1e-6, err_msg="%s S=%d" % (k, S))
        assert list(t["order"]) == _expected_orders(S)
        # the step coefficients restated in float64 from the reference's alpha / sigma / lambda (dpm_solver.py:525-530, 779-784)
        a, s, l = (g["S%d_%s" % (S, k)].astype(np.float64) for k in ("alpha", "sigma", "lambda"))
        for i in range(S):
            h = l[i + 1] - l[i]
            np.testing.assert_allclose(t["c_x"][i], s[i + 1] / s[i], rtol=1e-5)
            np.testing.assert_allclose([t["sigma_t"][i], t["alpha_t"][i]], [s[i], a[i]], rtol=1e-5)
            if t["order"][i] == 1:
                np.testing.assert_allclose([t["c_m"][i], t["c_p"][i]], [-a[i + 1] * np.expm1(-h), 0.0], rtol=1e-4, atol=1e-9)
            else:
                r0 = (l[i] - l[i - 1]) / h
                phi = a[i + 1] * np.expm1(-h)
                np.testing.assert_allclose([t["c_m"][i], t["c_p"][i]], [-phi * (1 + 0.5 / r0), phi * 0.5 / r0], rtol=1e-4)
    g2 = _load("dpm_traj.npz")
    for S in (20, 10):       # the model input times the reference's wrapper handed to the UNet
        np.testing.assert_array_equal(solver.dpm_tables(acp, S)["t_in"], g2["S%d_t_in" % S])


def test_ddim_schedule_tables_match_reference():
    from sta import solver
    g = _load("ddim_traj.npz")
    acp = _alphas_cumprod()
    for tag in ("eta0", "eta05"):
        S, eta = int(g[tag + "_S"]), float(g[tag + "_eta"])
        t = solver.ddim_tables(acp, S, eta)
        np.testing.assert_array_equal(t["timesteps"], g[tag + "_timesteps"])
        np.testing.assert_array_equal(t["t_in"], np.flip(g[tag + "_timesteps"]))
        np.testing.assert_allclose(t["a"], g[tag + "_alphas"], rtol=1e-6)
        np.testing.assert_allclose(t["a_prev"], g[tag + "_alphas_prev"], rtol=1e-6)
        np.testing.assert_allclose(t["sigma"], g[tag + "_sigmas"], rtol=1e-5, atol=1e-7)
        idx = np.arange(S)[::-1]
        np.testing.assert_allclose(t["sigma_t"], g[tag + "_s1m"][idx], rtol=1e-6)
        np.testing.assert_allclose(t["alpha_t"], np.sqrt(g[tag + "_alphas"][idx]), rtol=1e-6)
        np.testing.assert_allclose(t["c_m"], np.sqrt(g[tag + "_alphas_prev"][idx]), rtol=1e-6)
        ce = np.sqrt(1 - g[tag + "_alphas_prev"] - g[tag + "_sigmas"] ** 2)[idx]
        np.testing.assert_allclose(t["c_e"], ce, rtol=1e-5)
        np.testing.assert_allclose(t["c_n"], g[tag + "_sigmas"][idx], rtol=1e-5, atol=1e-7)
        assert (t["c_n"] > 0).all() == (eta > 0)


def _run_golden(sampler, g, prefix, S, W):
    """The sampler's own trajectory on the golden UNet; returns (final x, the state x at the input of every call)."""
    from sta import prompt_state
    c, local_ctx, x_T = gi.unet_inputs(int(g["K"]), int(g["input_seed"]))
    np.testing.assert_array_equal(x_T.numpy(), g["x_T"])
    model = sampler.model
    seen, inner = [], model.apply_model_extra

    def spy(x_in, *a, **k):
        seen.append(x_in[:1].clone())
        return inner(x_in, *a, **k)

    model.apply_model_extra = spy
    sampler.make_schedule(S, ddim_eta=float(g[prefix + "eta"]) if prefix + "eta" in g else 0.0, verbose=False)
    tr = sampler._time_range()
    with oracle_ops(), torch.no_grad():
        prompt_state.begin_prompt(local_ctx, first_timestep=int(tr[0]))
        x = sampler._trajectory(x_T.clone(), c, gi.load_uncond(), float(g["scale"]), tr, torch.from_numpy(W),
                                [list(cc) for cc in g["centres"]], 0)
    del model.apply_model_extra
    assert len(seen) == S
    return x, seen


def _check(x, seen, g, prefix):
    keep = list(g[prefix + "keep"])
    for j, i in enumerate(keep):
        ref = g[prefix + "xs"][j]
        err = np.abs(seen[i].numpy() - ref).max() / max(1.0, np.abs(ref).max())
        assert err < 2e-3, (prefix, i, err)
    ref = g[prefix + "x0"]
    err = np.abs(x.numpy() - ref).max() / np.abs(ref).max()
    assert err < 2e-3, (prefix, err)
    return err


@pytest.mark.parametrize("S", [20, 10])
def test_dpm_solver_trajectory_matches_reference(S):
    """S DPM-Solver++(2M) steps = S UNet calls with CFG 7.5 and a different weight column per call; S = 10 takes the
    first-order update at the last call (lower_order_final)."""
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    g = _load("dpm_traj.npz")
    model, checksum = _model()
    assert abs(checksum - float(g["checksum"])) <= 1e-6 * abs(float(g["checksum"]))
    sampler = DPMSolverSampler(model, opt_epochs=0, use_graph=False, save_images=False)
    x, seen = _run_golden(sampler, g, "S%d_" % S, S, g["S%d_W" % S])
    _check(x, seen, g, "S%d_" % S)


@pytest.mark.parametrize("tag", ["eta0", "eta05"])
def test_ddim_trajectory_matches_reference(tag):
    """DDIM with the reference's recorded noise (eta 0.5) replayed through the sampler's noise source."""
    from ldm.models.diffusion.ddim import DDIMSampler
    g = _load("ddim_traj.npz")
    model, _ = _model()
    noise = [torch.from_numpy(n) for n in g[tag + "_noise"]] if tag + "_noise" in g else None
    sampler = DDIMSampler(model, opt_epochs=0, use_graph=False, save_images=False, noise=noise)
    x, seen = _run_golden(sampler, g, tag + "_", int(g[tag + "_S"]), g[tag + "_W"])
    _check(x, seen, g, tag + "_")


def test_ddim_without_noise_source_draws_randn_only_when_eta_positive():
    from ldm.models.diffusion.ddim import DDIMSampler
    model, _ = _model()
    calls = []
    s = DDIMSampler(model, noise=lambda i, shape, device: calls.append(i) or torch.zeros(shape))
    s.make_schedule(4, ddim_eta=0.0, verbose=False)
    assert all(s._coef(i, 7.5).c_n == 0 for i in range(4))
    s.make_schedule(4, ddim_eta=0.5, verbose=False)
    assert all(s._coef(i, 7.5).c_n > 0 for i in range(4))
    assert s._noise(2, torch.zeros(1, 4, 8, 8)).shape == (1, 4, 8, 8) and calls == [2]


def test_dpm_solver_sample_keyword_surface_and_result():
    """sample(...) with opt_epochs=0: the reference's keywords, W[K, S] = 5/K, S calls, result kept for callers."""
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    model, _ = _model()
    c, local_ctx, x_T = gi.unet_inputs(2, 5)
    sampler = DPMSolverSampler(model, opt_epochs=0, use_graph=False, save_images=False)
    n, inner = [0], model.apply_model_extra
    model.apply_model_extra = lambda *a, **k: (n.__setitem__(0, n[0] + 1), inner(*a, **k))[1]
    with oracle_ops():
        sampler.sample(S=4, conditioning=c, batch_size=1, shape=[4, 16, 16], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond(), eta=0.3, x_T=x_T[:, :, :16, :16], text_index=0, curr_text="x",
                       bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], seed=1, prompt_idx=0, object_names=["a", "b"], local_conditionings=local_ctx)
    r = sampler.last_result
    assert n[0] == 4
    assert r["x0"].shape == (1, 4, 16, 16) and torch.isfinite(r["x0"]).all()
    assert r["W"].shape == (2, 4) and torch.allclose(r["W"], torch.full((2, 4), 2.5))


def test_dpm_solver_weight_optimisation_moves_W():
    """opt_epochs=2 with a differentiable stand-in loss: one Adam step (lr 5e-3) from the first epoch moves every column."""
    from ldm.models.autoencoder import AutoencoderKL
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler

    class Loss(torch.nn.Module):
        def forward_2(self, image, text):
            return image.mean().reshape(1)

        def forward_3(self, image, text):
            return (image ** 2).mean().reshape(1)

    model, _ = _model()
    unet = model.model.diffusion_model
    for p in unet.parameters():
        p.requires_grad_(False)
    vae = AutoencoderKL(ddconfig=dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32,
                                      ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[], dropout=0.0))
    seeded_fill_(vae, 3)
    for p in vae.parameters():
        p.requires_grad_(False)
    model = LatentDiffusion(unet_config=unet, first_stage_config=vae)
    c, local_ctx, x_T = gi.unet_inputs(2, 6)
    sampler = DPMSolverSampler(model, loss_model=Loss(), opt_epochs=2, use_graph=False, save_images=False)
    with oracle_ops():
        sampler.sample(S=4, conditioning=c, batch_size=1, shape=[4, 8, 8], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond(), x_T=x_T[:, :, :8, :8], text_index=0, curr_text="x",
                       bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], seed=1, prompt_idx=0, object_names=["The cat", "dog"],
                       local_conditionings=local_ctx)
    r = sampler.last_result
    assert len(r["losses"]) == 1 and r["W"].shape == (2, 4)
    step = (r["W"] - 2.5).abs()
    assert torch.allclose(step, torch.full_like(step, 0.005), atol=1e-4)


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts"))
    import _txt2img_common as c
    return c


def test_cli_picks_the_sampler_as_the_reference():
    c = _cli()
    p = c.build_parser("x.json")
    assert c.sampler_choice(p.parse_args(["--dpm_solver", "--ddim_eta", "0.7"])) == ("DPMSolverSampler", 0.0)
    assert c.sampler_choice(p.parse_args(["--dpm_solver", "--plms"]))[0] == "DPMSolverSampler"
    assert c.sampler_choice(p.parse_args(["--plms"])) == ("PLMSSampler", 0.0)
    assert c.sampler_choice(p.parse_args([])) == ("DDIMSampler", 0.0)
    assert c.sampler_choice(p.parse_args(["--ddim_eta", "0.5"])) == ("DDIMSampler", 0.5)
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    assert c.sampler_class("DPMSolverSampler") is DPMSolverSampler and c.sampler_class("DDIMSampler") is DDIMSampler
    assert c.sampler_class("PLMSSampler") is PLMSSampler
    c.check_options(p.parse_args(["--dpm_solver", "--opt_epochs", "0"]))     # no longer refused
    assert "only --plms works" not in open(c.__file__).read()
