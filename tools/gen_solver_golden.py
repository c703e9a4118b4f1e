"""Regenerate tests/golden/{dpm_traj,ddim_traj,dpm_schedule}.npz by running the REFERENCE's own samplers on CPU.

Run in the build container only (needs the reference tree, oracle/ref_harness.py):   python tools/gen_solver_golden.py

The reference's sampler wrappers call `apply_model(x, t, c)` without the blend weights and object boxes, so neither ran on its
spatial-temporal UNet. Here the reference's own solver code is driven through FakeLatentDiffusion.apply_model_extra with CFG and
column k of W at the k-th UNet call:
  * DPM_Solver(model_fn, NoiseScheduleVP('discrete'), predict_x0=True).sample(steps=S, skip_type="time_uniform", method="multistep",
    order=2, lower_order_final=True), model_fn from the reference's model_wrapper (classifier-free guidance);
  * DDIMSampler.p_sample_ddim with its `apply_model` routed to apply_model_extra; the noise it draws (noise_like) is recorded.
The blocks set up their per-prompt state only at time == 981 (attention.py:240): one discarded priming call at 981 first, as
oracle/gen_golden.py G5b does. Same golden UNet (reduced width, seeded weights) and inputs as G5 (plms_traj.npz).
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffusion-spacetime-attn_amd"))
sys.path.insert(0, REPO)

from oracle import ref_harness as rh  # noqa: E402
from oracle.gen_golden import CENTRES, UNET_CFG, UNET_SEED  # noqa: E402
from oracle.golden_inputs import unet_inputs  # noqa: E402
from sta.synth import seeded_fill_  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
K, SCALE, INPUT_SEED = 2, 7.5, 41


def weights(S):
    """a different column per call, so that a wrong call -> column mapping is caught"""
    return torch.tensor([[5.0 / K * (1.0 + 0.2 * np.sin(0.7 * i + k)) for i in range(S)] for k in range(K)], dtype=torch.float32)


class _Calls:
    """apply_model_extra with the per-call weight column; records the state x and the model time of every call."""

    def __init__(self, fake, W, centres):
        self.fake, self.W, self.centres = fake, W, centres
        self.k, self.xs, self.ts = 0, [], []

    def __call__(self, x_in, t_in, c_in):
        self.xs.append(x_in[:1].clone())
        self.ts.append(float(t_in[0]))
        out = self.fake.apply_model_extra(x_in, 0, t_in, c_in, coef=self.W[:, self.k], bboxs_curr=self.centres)
        self.k += 1
        return out


def _prime(unet, x_T, uncond, c, W, centres):
    unet(torch.cat([x_T, x_T]), 0, torch.tensor([981, 981]), context=torch.cat([uncond, c]), coef=W[:, 0], bboxs_curr=centres)


def gen_dpm():
    uncond = rh.load_uncond()
    c, local_ctx, x_T = unet_inputs(K, INPUT_SEED)
    centres = [list(cc) for cc in CENTRES[:K]]
    out = dict(x_T=x_T.numpy(), input_seed=INPUT_SEED, scale=SCALE, K=K, centres=np.asarray(centres))
    with rh.reference_env(local_ctx) as ref, torch.no_grad():
        import ldm.models.diffusion.dpm_solver.dpm_solver as ref_dpm
        unet = ref.unet.UNetModel(**UNET_CFG).eval()
        out["checksum"] = seeded_fill_(unet, UNET_SEED)
        fake = rh.FakeLatentDiffusion(ref, unet)
        for S in (20, 10):
            W = weights(S)
            _prime(unet, x_T, uncond, c, W, centres)
            calls = _Calls(fake, W, centres)
            ns = ref_dpm.NoiseScheduleVP("discrete", alphas_cumprod=fake.alphas_cumprod)
            model_fn = ref_dpm.model_wrapper(calls, ns, model_type="noise", guidance_type="classifier-free", condition=c,
                                             unconditional_condition=uncond, guidance_scale=SCALE)
            solver = ref_dpm.DPM_Solver(model_fn, ns, predict_x0=True, thresholding=False)
            x0 = solver.sample(x_T.clone(), steps=S, skip_type="time_uniform", method="multistep", order=2, lower_order_final=True)
            assert calls.k == S, calls.k
            keep = [1, 2, S // 2, S - 1]
            t = solver.get_time_steps("time_uniform", ns.T, 1.0 / ns.total_N, S, "cpu")
            out.update({"S%d_W" % S: W.numpy(), "S%d_t_in" % S: np.asarray(calls.ts, dtype=np.float32), "S%d_t" % S: t.numpy(),
                        "S%d_alpha" % S: ns.marginal_alpha(t).numpy(), "S%d_sigma" % S: ns.marginal_std(t).numpy(),
                        "S%d_lambda" % S: ns.marginal_lambda(t).numpy(), "S%d_keep" % S: np.asarray(keep),
                        "S%d_xs" % S: np.stack([calls.xs[i].numpy() for i in keep]), "S%d_x0" % S: x0.numpy()})
            print("dpm S=%d x0 |mean| %.4f max %.3f, times %s" % (S, x0.abs().mean().item(), x0.abs().max().item(), calls.ts[:3]))
    np.savez_compressed(os.path.join(OUT, "dpm_traj.npz"), **out)


def gen_ddim():
    uncond = rh.load_uncond()
    c, local_ctx, x_T = unet_inputs(K, INPUT_SEED)
    centres = [list(cc) for cc in CENTRES[:K]]
    out = dict(x_T=x_T.numpy(), input_seed=INPUT_SEED, scale=SCALE, K=K, centres=np.asarray(centres))
    cases = [("eta0", 0.0, 20), ("eta05", 0.5, 10)]
    with rh.reference_env(local_ctx) as ref, torch.no_grad():
        import ldm.models.diffusion.ddim as ref_ddim
        unet = ref.unet.UNetModel(**UNET_CFG).eval()
        out["checksum"] = seeded_fill_(unet, UNET_SEED)
        fake = rh.FakeLatentDiffusion(ref, unet)
        for tag, eta, S in cases:
            W = weights(S)
            _prime(unet, x_T, uncond, c, W, centres)
            calls = _Calls(fake, W, centres)

            class Model:                       # the sampler's model: its apply_model(x, t, c) carries the weights and boxes
                def __getattr__(self, name):
                    return getattr(fake, name)

                def apply_model(self, x, t, cond):
                    return calls(x, t, cond)

            s = object.__new__(ref_ddim.DDIMSampler)
            s.model, s.ddpm_num_timesteps, s.schedule = Model(), fake.num_timesteps, "linear"
            s.register_buffer = lambda name, attr, s=s: setattr(s, name, attr)   # CPU instead of the forced "cuda"
            s.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=False)
            drawn = []
            saved = ref_ddim.noise_like

            def noise_like(shape, device, repeat=False):
                n = saved(shape, device, repeat)
                drawn.append(n.clone())
                return n

            ref_ddim.noise_like = noise_like
            torch.manual_seed(1234)
            try:
                img = x_T.clone()
                time_range = np.flip(s.ddim_timesteps)
                for i, step in enumerate(time_range):      # loop header of ddim.py:128-140
                    ts = torch.full((1,), int(step), dtype=torch.long)
                    img, _ = s.p_sample_ddim(img, c, ts, index=S - i - 1, unconditional_guidance_scale=SCALE,
                                             unconditional_conditioning=uncond)
            finally:
                ref_ddim.noise_like = saved
            keep = [1, 2, S // 2, S - 1]
            f = lambda v: np.asarray(v, dtype=np.float64)
            out.update({tag + "_S": S, tag + "_eta": eta, tag + "_W": W.numpy(), tag + "_timesteps": np.asarray(s.ddim_timesteps),
                        tag + "_alphas": f(s.ddim_alphas), tag + "_alphas_prev": f(s.ddim_alphas_prev), tag + "_sigmas": f(s.ddim_sigmas),
                        tag + "_s1m": f(s.ddim_sqrt_one_minus_alphas), tag + "_keep": np.asarray(keep),
                        tag + "_xs": np.stack([calls.xs[i].numpy() for i in keep]), tag + "_x0": img.numpy()})
            if eta > 0:
                out[tag + "_noise"] = torch.stack(drawn).numpy()
            print("ddim %s x0 |mean| %.4f max %.3f" % (tag, img.abs().mean().item(), img.abs().max().item()))
    np.savez_compressed(os.path.join(OUT, "ddim_traj.npz"), **out)


def gen_schedule():
    out = {}
    with rh.reference_env() as ref:
        import ldm.models.diffusion.dpm_solver.dpm_solver as ref_dpm
        fake = rh.FakeLatentDiffusion(ref, None)
        ns = ref_dpm.NoiseScheduleVP("discrete", alphas_cumprod=fake.alphas_cumprod)
        solver = ref_dpm.DPM_Solver(lambda x, t: x, ns, predict_x0=True)
        for S in (10, 20, 25, 50):
            t = solver.get_time_steps("time_uniform", ns.T, 1.0 / ns.total_N, S, "cpu")
            out["S%d_t" % S] = t.numpy()
            out["S%d_t_in" % S] = ((t - 1.0 / ns.total_N) * 1000.0).numpy()
            out["S%d_alpha" % S] = ns.marginal_alpha(t).numpy()
            out["S%d_sigma" % S] = ns.marginal_std(t).numpy()
            out["S%d_lambda" % S] = ns.marginal_lambda(t).numpy()
        out["alphas_cumprod"] = fake.alphas_cumprod.numpy()
    np.savez_compressed(os.path.join(OUT, "dpm_schedule.npz"), **out)
    print("dpm_schedule.npz", out["S20_t_in"][:3])


if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_schedule()
    gen_dpm()
    gen_ddim()
