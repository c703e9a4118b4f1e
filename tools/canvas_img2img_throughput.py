"""What img2img on a canvas costs: one 512 x 2048 canvas with stride 256, clamped (T = 7) and wrapped along x (T = 8), at the settings of
tools/canvas_wrap_throughput.py — DDIM, 50 steps, t_start = 25, K = 2, fixed blend weights, synthetic weights, hipGraph replay, latents only.

Three figures, all from this one run.
(a) The entry launch, timed with HIP events around it: the fused sta_vae_encode_step_windows against sta_vae_encode_step +
    sta_window_split issued back to back, the two forms alternating. Every event-timed launch sits on a floor of several us, so for
    a launch of this size the ratio says little more than which side of 1 it is on; the bytes each form moves are counted from the shapes.
(b) Seconds per `decode_canvas` trajectory (25 UNet calls of 2 T window rows) against `decode_batch` of T 512 x 512 images at the same
    t_start, which runs the same UNet batch per call: the ratio is the cost of the window work.
(c) The VAE encoder's time on the whole canvas picture (on the wrapped canvas: with its circular padding of 8 canvas_wrap_margin pixels).

    python tools/canvas_img2img_throughput.py [--steps 50] [--t_start 25] [--reps 3] [--warmup 1] [--dtype fp16] [--out profiles/canvas_img2img_throughput.json]
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from canvas_throughput import timed  # noqa: E402  (imports bench.py for the environment and sys.path of the bench run)

import torch  # noqa: E402


def event_us(fns, warmup=20, reps=200):
    """Median device microseconds of each callable, HIP events around one issue of it, the callables alternating."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    pairs = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            pairs[k].append((a, b))
    torch.cuda.synchronize()
    return [round(1e3 * statistics.median(a.elapsed_time(b) for a, b in p), 2) for p in pairs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--t_start", type=int, default=25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "canvas_img2img_throughput.json"))
    a = ap.parse_args()
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta import canvas, fused, lib
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, use_shipped_miopen_db
    dev = torch.device("cuda", 0)
    lib.load()
    use_shipped_miopen_db(0)
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    model = build_sd_v1(dev, dt, init_weights=True, seed=0, channels_last=True, with_encoder=True)
    vae = model.first_stage_model
    vae.encoder.to(memory_format=torch.channels_last)
    K, s = 2, 64
    grids = {"clamped_T7": canvas.window_grid(64, 256, s, 32), "wrapped_T8": canvas.window_grid(64, 256, s, 32, "x")}
    names = ["cat", "dog"]
    uc, c, local = conditionings(model, "a cat left of a dog on a street", names, dt)
    centres = [list(v) for v in DEFAULT_CENTRES[:K]]
    gen = torch.Generator(device=dev).manual_seed(1)
    image = torch.rand([1, 3, 512, 2048], generator=gen, device=dev) * 2 - 1
    n_post, n_enc = (torch.randn([1, 4, 64, 256], generator=gen, device=dev) for _ in range(2))
    sampler = DDIMSampler(model, opt_epochs=0, use_graph=True, save_images=False)
    sampler.make_schedule(a.steps, ddim_eta=0.0, verbose=False)
    t_enc = min(a.t_start, a.steps - 1)
    sa, s1m = sampler._encode_coefs()
    qc = vae.quant_conv
    res = {"run": True, "workload": "DDIM-%d, t_start=%d, K=2, fixed weights, synthetic weights, hipGraph, %s; canvas 512x2048 px, windows 512 px, "
                                    "stride 256 px, clamped (T=7) and wrap=x (T=8); latents only" % (a.steps, a.t_start, a.dtype),
           "note": "every event-timed launch sits on a floor of several us: at this size the entry ratio is dominated by that floor",
           "reps": a.reps, "warmup": a.warmup, "entry_launch": {}, "encoder": {}, "legs": {}}

    for name, grid in grids.items():
        # (c) the one encode of the canvas picture
        def encode():
            with torch.no_grad():
                return sampler._encode_canvas(image, grid, vae)
        for _ in range(2):
            encode()
        torch.cuda.synchronize()
        runs = []
        for _ in range(max(a.reps, 3)):
            t0 = time.perf_counter()
            h = encode()
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        res["encoder"][name] = {"ms": [round(1e3 * r, 2) for r in runs], "best_ms": round(1e3 * min(runs), 2),
                                "pixels": [int(v) for v in (image.shape[-2], image.shape[-1] + (16 * sampler.canvas_wrap_margin if grid.wrap else 0))]}
        # (a) the entry launch: fused against the pair it replaces
        h = h.contiguous(memory_format=torch.channels_last)
        args = (qc.weight.detach().reshape(8, 8).float().contiguous(), qc.bias.detach().float().contiguous(), n_post, n_enc, model.scale_factor,
                float(sa[t_enc]), float(s1m[t_enc]))
        one = lambda: canvas.encode_step_windows(h, *args, grid)
        two = lambda: canvas.window_split(fused.vae_encode_step(h, *args, want_xin=False)[0], grid, dt)
        a_out, b_out = one(), two()
        assert torch.equal(a_out[2], b_out), "the fused entry and the pair it replaces disagree"
        us_one, us_two = event_us([one, two])
        px, esz = grid.Hc * grid.Wc, 2
        xin_bytes = 2 * grid.T * 4 * s * s * esz
        res["entry_launch"][name] = {"fused_us": us_one, "encode_step_plus_split_us": us_two, "fused_over_pair": round(us_one / us_two, 3),
                                     "fused_bytes": px * (8 * esz + 3 * 16) + xin_bytes, "pair_bytes": px * (8 * esz + 4 * 16) + xin_bytes}
        print("[entry %s] %s" % (name, res["entry_launch"][name]), file=sys.stderr, flush=True)
        x, _, xin = a_out

        # (b) trajectories, latents only: the decode of the canvas is no part of the comparison
        def canvas_leg():
            sampler.decode_canvas(x, (grid.Hc, grid.Wc), s, grid.stride, t_start=a.t_start, conditionings=[c], unconditional_conditionings=uc,
                                  bboxs=[centres], object_names=[names], local_conditionings=[local], unconditional_guidance_scale=7.5, seed=1,
                                  xin=xin, wrap=grid.wrap)
        x_batch = torch.randn([grid.T, 4, s, s], generator=gen, device=dev)

        def batch_leg():
            sampler.decode_batch(x_batch, [c] * grid.T, uc, canvas.window_centres(centres, grid), [names] * grid.T, [local] * grid.T, a.t_start,
                                 unconditional_guidance_scale=7.5, seed=1)
        model.first_stage_model = None
        try:
            for leg, fn in (("decode_batch_%dx512" % grid.T, batch_leg), ("decode_canvas_" + name, canvas_leg)):
                runs, ms, n = timed(fn, a.warmup, a.reps)
                res["legs"][leg] = {"s_per_trajectory": [round(r, 4) for r in runs], "best_s": round(min(runs), 4),
                                    "ms_per_call": round(1e3 * min(runs) / a.t_start, 3), "launches_between_unet_calls": n,
                                    "their_device_us_per_call": round(1e3 * ms / a.t_start, 2)}
                print("[%s] %s" % (leg, res["legs"][leg]), file=sys.stderr, flush=True)
        finally:
            model.first_stage_model = vae
        base = res["legs"]["decode_batch_%dx512" % grid.T]["best_s"]
        res.setdefault("trajectory", {})[name] = {
            "decode_canvas_vs_decode_batch": round(res["legs"]["decode_canvas_" + name]["best_s"] / base, 4),
            "window_work_ms_per_call": round(1e3 * (res["legs"]["decode_canvas_" + name]["best_s"] - base) / a.t_start, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
