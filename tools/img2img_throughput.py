"""img2img on one MI355X: the stride-2 Downsample kernel, the whole VAE encoder, and img2img images/s next to txt2img DDIM-50.

Imports bench.py (environment, sys.path) like tools/sampler_throughput.py. Three parts, one JSON line:
  * s2     sta_conv3x3_s2_nhwc against F.pad + the library stride-2 convolution (NHWC) at every shape the kernel supports
           (the SD-v1 encoder's three Downsample inputs at 512^2 and 768^2), --s2-batch images: median us of --reps timed launches
           after warm-up, TFLOP/s, and the share of the launch's bound: max(flop / MFMA peak, bytes / HBM peak) with bytes = input +
           output + weights once (2 (4 Cin + Cout) bytes per output pixel, 230 flop/B at 128 channels: HBM-bound below the ridge;
           MFMA-bound at 256 and 512);
  * enc    the SD-v1 encoder (synthetic weights, NHWC, 16-bit) on 16 and 64 images of 512^2: the HIP path against the library path
           (sta.fused.CONV3X3 = False and CONV_S2 = False: every 3x3 convolution and Downsample through MIOpen, F.pad included);
  * steps  images/s at 64 prompts per step: img2img (strength 0.75, DDIM 50 -> 37 UNet calls, K = 2, fixed weights: one encoder call,
           one sta_vae_encode_step, decode_batch) against txt2img DDIM-50 (sample_batch) in the same process, the two alternating.

    python tools/img2img_throughput.py [--dtype fp16] [--s2-batch 16] [--reps 20] [--images 64] [--rounds 2] [--skip-steps]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402,F401  (environment and sys.path of the bench run)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MFMA_PEAK = 2.5e15        # dense fp16 / bf16 flop/s of an MI355X
HBM_PEAK = 8.0e12         # bytes/s
S2_SHAPES = [(512, 128), (256, 256), (128, 512), (768, 128), (384, 256), (192, 512)]


def _time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def s2_leg(dt, B, reps):
    from sta import fused
    out = []
    for HW, C in S2_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(HW + C)
        x = torch.randn(B, C, HW, HW, device="cuda", generator=g).to(dt).contiguous(memory_format=torch.channels_last)
        w = (torch.randn(C, C, 3, 3, device="cuda", generator=g) / (9 * C) ** 0.5).to(dt)
        wl = w.contiguous(memory_format=torch.channels_last)
        b = torch.zeros(C, device="cuda", dtype=dt)
        with torch.no_grad():
            wp = fused.pack_conv3x3_weight(w)
            hip = _time(lambda: fused.conv3x3_s2_nhwc(x, wp, C, bias=b), reps)
            lib_us = _time(lambda: F.conv2d(F.pad(x, (0, 1, 0, 1)), wl, b, stride=2), reps)
        Ho = HW // 2
        flop = 2.0 * 9 * C * C * Ho * Ho * B
        nbytes = 2.0 * (B * (HW * HW * C + Ho * Ho * C) + 9 * C * C)
        t_bound = max(flop / MFMA_PEAK, nbytes / HBM_PEAK)
        bound = "MFMA" if flop / MFMA_PEAK >= nbytes / HBM_PEAK else "HBM"
        rec = {"H": HW, "C": C, "B": B, "hip_us": round(hip, 1), "pad_conv_us": round(lib_us, 1), "speedup": round(lib_us / hip, 3),
               "hip_tflops": round(flop / hip / 1e6, 1), "pad_conv_tflops": round(flop / lib_us / 1e6, 1), "bound": bound,
               "hip_share_of_bound": round(t_bound * 1e6 / hip, 3)}
        print("[s2] %s" % rec, file=sys.stderr, flush=True)
        out.append(rec)
        del x, w, wl
        torch.cuda.empty_cache()
    return out


def enc_leg(dt, reps):
    from ldm.models.autoencoder import AutoencoderKL
    from sta import fused, pipeline, synth
    vae = AutoencoderKL().add_encoder()
    synth.seeded_fill_(pipeline.encoder_part(vae), 5)
    vae = vae.to("cuda", dt).to(memory_format=torch.channels_last)
    out = {}
    for n in (16, 64):
        img = torch.rand(n, 3, 512, 512, device="cuda") * 2 - 1
        with torch.no_grad():
            hip = _time(lambda: vae.encode_moments_input(img), reps, warm=2)
            fused.CONV3X3, fused.CONV_S2 = False, False
            try:
                lib_us = _time(lambda: vae.encode_moments_input(img), reps, warm=2)
            finally:
                fused.CONV3X3, fused.CONV_S2 = True, True
        out["images%d" % n] = {"hip_ms": round(hip / 1e3, 2), "library_ms": round(lib_us / 1e3, 2), "speedup": round(lib_us / hip, 3),
                               "hip_ms_per_64_images": round(hip / 1e3 * 64 / n, 2)}
        print("[enc] %d images: %s" % (n, out["images%d" % n]), file=sys.stderr, flush=True)
        del img
        torch.cuda.empty_cache()
    del vae
    return out


def steps_leg(dt, I, rounds, K=2, S=50, strength=0.75):
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts, use_shipped_miopen_db
    use_shipped_miopen_db(0)
    dev = torch.device("cuda", 0)
    model = build_sd_v1(dev, dt, with_vae=True, init_weights=True, seed=0, channels_last=True, with_encoder=True)
    vae = model.first_stage_model
    prompts = load_prompts(64)
    lat, centres = 64, [list(c) for c in DEFAULT_CENTRES[:K]]
    t_enc = int(strength * S)
    g = torch.Generator(device=dev).manual_seed(1)
    img = (torch.rand(1, 3, 512, 512, device=dev, generator=g) * 2 - 1).expand(I, -1, -1, -1).contiguous()
    x_T1 = torch.randn([1, 4, lat, lat], generator=g, device=dev)
    recs = [prompts[i % len(prompts)] for i in range(I)]
    names = [(r["objects"] + ["object"] * K)[:K] for r in recs]
    conds = [conditionings(model, r["prompt"], nm, dt) for r, nm in zip(recs, names)]
    kw = dict(conditionings=[c[1] for c in conds], unconditional_conditionings=[c[0] for c in conds], bboxs=[centres] * I, object_names=names,
              local_conditionings=[c[2] for c in conds], curr_texts=[r["prompt"] for r in recs], unconditional_guidance_scale=7.5, seed=1)
    txt = DDIMSampler(model, opt_epochs=0, use_graph=True, save_images=False)
    i2i = DDIMSampler(model, opt_epochs=0, use_graph=True, save_images=False)
    n_post = torch.randn(I, 4, lat, lat, generator=g, device=dev)
    n_enc = torch.randn(I, 4, lat, lat, generator=g, device=dev)

    def run_txt():
        txt.sample_batch(S=S, shape=[4, lat, lat], x_T=x_T1.expand(I, -1, -1, -1), **kw)

    def run_i2i():
        i2i.make_schedule(S, ddim_eta=0.0, verbose=False)
        with torch.no_grad():
            h = vae.encode_moments_input(img)
            x, _, xin = i2i.encode_step(h, vae, t_enc, n_post, n_enc)
        i2i.decode_batch(x, t_start=t_enc, xin=xin, **kw)

    run_txt()
    run_i2i()                        # warm-up: graph captures, first-use solver searches
    legs = {"txt2img_ddim50": [], "img2img_ddim50_s075": []}
    for _ in range(rounds):
        for name, fn in (("txt2img_ddim50", run_txt), ("img2img_ddim50_s075", run_i2i)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            legs[name].append(time.perf_counter() - t0)
            print("[steps] %s %.3f s" % (name, legs[name][-1]), file=sys.stderr, flush=True)
    out = {k: {"images_per_s": round(I / min(v), 3), "s_per_step": [round(x, 3) for x in v]} for k, v in legs.items()}
    out["img2img_vs_txt2img"] = round(out["img2img_ddim50_s075"]["images_per_s"] / out["txt2img_ddim50"]["images_per_s"], 3)
    out["unet_calls_per_image"] = {"txt2img_ddim50": S, "img2img_ddim50_s075": t_enc}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--s2-batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    from sta import lib
    lib.load()
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    res = {"dtype": a.dtype, "mfma_peak": MFMA_PEAK, "hbm_peak": HBM_PEAK}
    res["s2"] = s2_leg(dt, a.s2_batch, a.reps)
    res["enc"] = enc_leg(dt, max(3, a.reps // 4))
    if not a.skip_steps:
        res["steps"] = steps_leg(dt, a.images, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
