"""DDIM sampler on the spatial-temporal UNet, with per-object, per-step blend-weight optimisation.

Counterpart of the reference's ldm/models/diffusion/ddim.py (DDIMSampler.sample :57-98, ddim_sampling :100-148,
p_sample_ddim :150-205), whose p_sample_ddim calls apply_model without the blend weights and object boxes (ddim.py:172-177), so it
never ran on the spatial-temporal UNet. Same schedule (make_ddim_timesteps / make_ddim_sampling_parameters, integer timesteps
flip(1, 21, ..., 981) for S = 50), CFG batch [uncond, cond], `eta` -> sigma; S steps = S UNet calls, call i uses column i of
W[K, S]. The step after each call is one sta_sampler_step launch (sta.solver).

Noise (eta > 0): by default torch.randn on the device after each call, in the reference's order (noise_like, ddim.py:199).
`noise=` replaces it: a list of pre-drawn tensors (index = call) or a callable (i, shape, device) -> tensor.
"""
import torch

from ldm.models.diffusion.plms import SolverSamplerBase
from sta import solver


class DDIMSampler(SolverSamplerBase):
    t_dtype = torch.long

    def __init__(self, model, schedule="linear", noise=None, **kwargs):
        super().__init__(model, schedule=schedule, **kwargs)
        self.noise = noise

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        if ddim_discretize != "uniform":
            raise NotImplementedError("only the uniform DDIM discretisation is on this path")
        self.tables = solver.ddim_tables(self.model.alphas_cumprod, ddim_num_steps, eta=ddim_eta)
        self.ddim_timesteps = self.tables["timesteps"]
        self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sigmas = self.tables["a"], self.tables["a_prev"], self.tables["sigma"]
        if verbose:
            print("DDIM: %d calls, eta %s" % (ddim_num_steps, ddim_eta))

    def _coef(self, i, scale):
        return solver.ddim_coefs(self.tables, i, scale)

    def _noise(self, i, x):
        if self.noise is None:
            return torch.randn(x.shape, device=x.device)
        if callable(self.noise):
            return self.noise(i, tuple(x.shape), x.device)
        return self.noise[i].to(x.device)
