"""Regenerate tests/golden/{vae_encoder.npz,vae_encoder_state_dict.json,ddim_img2img.npz} by running the REFERENCE's own code on CPU.

Run in the build container only (needs the reference tree, oracle/ref_harness.py):   python tools/gen_img2img_golden.py

The reference's Encoder (ldm/modules/diffusionmodules/model.py:368-459) at full SD-v1 width (ddconfig of v1-inference.yaml: ch 128,
ch_mult 1 2 4 4, 2 res blocks, z 4, double_z), quant_conv (autoencoder.py:302) and DiagonalGaussianDistribution
(ldm/modules/distributions/distributions.py:24-37) in fp32 on a 128 x 128 image, B = 2: every level of that image is inside the HIP
kernels' supported sets (tests/test_img2img_gpu.py lowers the work-item gates). The weights come from sta.synth.seeded_fill_
(seed 5) under the AutoencoderKL state_dict names (encoder.*, quant_conv.*) and are not stored; the image is stored as uint8 and
the posterior noise is stored. The second file lists the encoder's state_dict names and shapes.
The third is the reference's img2img sampling (scripts/img2img.py: DDIMSampler.make_schedule, stochastic_encode, the decode loop of
ddim.py:223-245) on G5's reduced UNet and inputs (tools/gen_solver_golden.py), K = 2, S = 10, strength 0.6 (t_enc = 6), at eta 0 and
eta 0.5 (the noise noise_like draws is recorded): p_sample_ddim's apply_model is routed to apply_model_extra with the weight column
of the full-trajectory call (S - t_enc + j at decode call j), after the discarded priming call at 981 the blocks need.
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "diffusion-spacetime-attn_amd"))
sys.path.insert(0, REPO)

from oracle import ref_harness as rh  # noqa: E402
from sta.synth import seeded_fill_, seeded_tensor  # noqa: E402
from oracle.gen_golden import CENTRES, UNET_CFG, UNET_SEED  # noqa: E402
from oracle.golden_inputs import unet_inputs  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
DDCONFIG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
                attn_resolutions=[], dropout=0.0)
SEED, B, SIZE = 5, 2, 128


def main():
    img_u8 = ((seeded_tensor("img2img_image", (B, 3, SIZE, SIZE), SEED) * 0.5 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)
    n_post = seeded_tensor("img2img_n_post", (B, 4, SIZE // 8, SIZE // 8), SEED)
    with rh.reference_env() as ref, torch.no_grad():
        import ldm.modules.diffusionmodules.model as ref_model
        from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
        part = torch.nn.ModuleDict(dict(encoder=ref_model.Encoder(**DDCONFIG),
                                        quant_conv=torch.nn.Conv2d(2 * DDCONFIG["z_channels"], 2 * 4, 1))).eval()
        seeded_fill_(part, SEED)
        x = img_u8.float() / 255.0 * 2.0 - 1.0
        h = part["encoder"](x)
        moments = part["quant_conv"](h)
        post = DiagonalGaussianDistribution(moments)
        z = post.mean + post.std * n_post                # sample() with the stored noise (distributions.py:35-37)
        names = [[k, list(v.shape)] for k, v in part.state_dict().items()]
    np.savez_compressed(os.path.join(OUT, "vae_encoder.npz"), image_u8=img_u8.numpy(), n_post=n_post.numpy(), h=h.numpy(),
                        moments=moments.numpy(), z=z.numpy(), seed=np.int64(SEED))
    with open(os.path.join(OUT, "vae_encoder_state_dict.json"), "w") as fh:
        json.dump(dict(ddconfig=DDCONFIG, names=names), fh, indent=0)
    print("wrote vae_encoder.npz (h %s, |z| max %.3f), %d state_dict entries" % (tuple(h.shape), float(z.abs().max()), len(names)))


def gen_ddim_img2img(S=10, strength=0.6):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from gen_solver_golden import INPUT_SEED, K, SCALE, _Calls, _prime, weights
    uncond = rh.load_uncond()
    c, local_ctx, x_T = unet_inputs(K, INPUT_SEED)
    centres = [list(cc) for cc in CENTRES[:K]]
    t_enc = int(strength * S)
    x0 = seeded_tensor("img2img_x0", tuple(x_T.shape), SEED)
    n_enc = seeded_tensor("img2img_n_enc", tuple(x_T.shape), SEED)
    W = weights(S)
    out = dict(x0=x0.numpy(), n_enc=n_enc.numpy(), input_seed=INPUT_SEED, scale=SCALE, K=K, centres=np.asarray(centres), S=S,
               strength=strength, t_enc=t_enc, W=W.numpy())
    with rh.reference_env(local_ctx) as ref, torch.no_grad():
        import ldm.models.diffusion.ddim as ref_ddim
        unet = ref.unet.UNetModel(**UNET_CFG).eval()
        out["checksum"] = seeded_fill_(unet, UNET_SEED)
        fake = rh.FakeLatentDiffusion(ref, unet)
        for tag, eta in (("eta0", 0.0), ("eta05", 0.5)):
            _prime(unet, x_T, uncond, c, W, centres)
            calls = _Calls(fake, W, centres)
            calls.k = S - t_enc                    # decode call j uses column S - t_enc + j

            class Model:
                def __getattr__(self, name):
                    return getattr(fake, name)

                def apply_model(self, x, t, cond):
                    return calls(x, t, cond)

            s = object.__new__(ref_ddim.DDIMSampler)
            s.model, s.ddpm_num_timesteps, s.schedule = Model(), fake.num_timesteps, "linear"
            s.register_buffer = lambda name, attr, s=s: setattr(s, name, attr)
            s.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=False)
            z_enc = s.stochastic_encode(x0, torch.tensor([t_enc]), noise=n_enc)
            drawn = []
            saved = ref_ddim.noise_like

            def noise_like(shape, device, repeat=False):
                n = saved(shape, device, repeat)
                drawn.append(n.clone())
                return n

            ref_ddim.noise_like = noise_like
            torch.manual_seed(4321)
            try:
                img = z_enc.clone()
                time_range = np.flip(s.ddim_timesteps[:t_enc])
                for i, step in enumerate(time_range):      # the loop of DDIMSampler.decode, ddim.py:235-244
                    ts = torch.full((1,), int(step), dtype=torch.long)
                    img, _ = s.p_sample_ddim(img, c, ts, index=t_enc - i - 1, unconditional_guidance_scale=SCALE,
                                             unconditional_conditioning=uncond)
            finally:
                ref_ddim.noise_like = saved
            out.update({tag + "_eta": eta, tag + "_z_enc": z_enc.numpy(), tag + "_timesteps": np.asarray(time_range).copy(),
                        tag + "_xs": np.stack([x.numpy() for x in calls.xs]), tag + "_x": img.numpy()})
            if eta > 0:
                out[tag + "_noise"] = torch.stack(drawn).numpy()
            print("ddim img2img %s: %d calls, x |mean| %.4f" % (tag, len(calls.xs), img.abs().mean().item()))
    np.savez_compressed(os.path.join(OUT, "ddim_img2img.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
    gen_ddim_img2img()
