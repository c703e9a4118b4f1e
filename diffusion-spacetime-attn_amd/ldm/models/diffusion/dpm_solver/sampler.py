"""DPM-Solver++ sampler on the spatial-temporal UNet, with per-object, per-call blend-weight optimisation.

Counterpart of the reference's ldm/models/diffusion/dpm_solver/sampler.py (DPMSolverSampler :9-82), which runs
`DPM_Solver(model_fn, NoiseScheduleVP('discrete'), predict_x0=True).sample(steps=S, skip_type="time_uniform", method="multistep",
order=2, lower_order_final=True)` — but whose model wrapper calls apply_model without the blend weights and object boxes, so it
never ran on the spatial-temporal UNet. Here the same solver drives apply_model_extra with CFG and column i of W[K, S] at call i:
  * S steps = S UNet calls at the model input times (t - 1/N) 1000, t = linspace(1, 1/N, S + 1)[:S] (999.0, 949.05, ... for S = 20);
  * call 0 and (S < 15) the last call take the first-order update, every other call the second-order multistep one;
  * the step after each call — CFG combine, data prediction, update, next input — is one sta_sampler_step launch (sta.solver).
`--ddim_eta` is ignored, as in the reference. Weight optimisation, loss scaling, graphs: as PLMSSampler.
"""
import numpy as np

from ldm.models.diffusion.plms import SolverSamplerBase
from sta import solver


class DPMSolverSampler(SolverSamplerBase):
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        self.tables = solver.dpm_tables(self.model.alphas_cumprod, ddim_num_steps, lower_order_final=True)
        if verbose:
            print("DPM-Solver++(2M): %d calls at model times %s" % (ddim_num_steps, self.tables["t_in"]))

    def _coef(self, i, scale):
        return solver.dpm_coefs(self.tables, i, scale)

    def _blend_coefs(self, i):
        """Inpainting: the marginal of the call's continuous time, x = alpha(t_i) x0 + sigma(t_i) n (float32 schedule values). The
        reference never combined its mask path with this solver; the blend is DDIM's, at the solver's own noise level."""
        return float(np.float32(self.tables["alpha_t"][i])), float(np.float32(self.tables["sigma_t"][i]))
