"""What closing a canvas on itself costs: one 512 x 2048 canvas with stride 256, wrapped along x (`wrap="x"`: T = 8 windows, the last one
runs over the seam) and clamped (T = 7), in the same run and at the settings of tools/canvas_throughput.py — DDIM, 50 steps, K = 2, fixed
blend weights, synthetic weights, hipGraph replay, latents only.

Two figures. The step launch between the UNet calls, timed with HIP events around it (sta_sampler_step_windows at wrap = 1 against
wrap = 0; every event-timed launch sits on a floor of several us, so the ratio of the two is an UPPER bound on the ratio
of the kernels). And the wall time of whole trajectories of the wrapped canvas against `sample_batch` of eight 512 x 512 images, which runs
the same UNet batch of 16 rows per call: the ratio is the cost of the window work on the ring. The clamped launch is also what the
previous build's profiles/canvas_throughput.json holds (canvas_fused_step.their_device_us_per_call), for a comparison across builds.

    python tools/canvas_wrap_throughput.py [--wrap x] [--steps 50] [--reps 3] [--warmup 1] [--dtype fp16] [--out profiles/canvas_wrap.json]
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from canvas_throughput import timed  # noqa: E402  (imports bench.py for the environment and sys.path of the bench run)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wrap", choices=["x"], default="x", help="the wrapped axis of the 512 x 2048 canvas (its height is one window)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "canvas_wrap.json"))
    a = ap.parse_args()
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta import canvas, lib
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, use_shipped_miopen_db
    dev = torch.device("cuda", 0)
    lib.load()
    use_shipped_miopen_db(0)
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    model = build_sd_v1(dev, dt, with_vae=False, init_weights=True, seed=0, channels_last=True)
    K, s = 2, 64
    ring, clamped = canvas.window_grid(64, 256, s, 32, a.wrap), canvas.window_grid(64, 256, s, 32)
    names = ["cat", "dog"]
    uc, c, local = conditionings(model, "a cat left of a dog on a street", names, dt)
    centres = [list(v) for v in DEFAULT_CENTRES[:K]]
    gen = torch.Generator(device=dev).manual_seed(1)
    x_canvas = torch.randn([1, 4, ring.Hc, ring.Wc], generator=gen, device=dev)
    x_batch = torch.randn([ring.T, 4, s, s], generator=gen, device=dev)
    sampler = DDIMSampler(model, opt_epochs=0, use_graph=True, save_images=False)

    def canvas_leg(grid):
        return lambda: sampler.sample_canvas(S=a.steps, canvas=(grid.Hc, grid.Wc), window=s, stride=grid.stride, conditionings=[c],
                                             unconditional_conditionings=uc, bboxs=[centres], object_names=[names],
                                             local_conditionings=[local], x_T=x_canvas, unconditional_guidance_scale=7.5, seed=1, wrap=grid.wrap)

    def batch_leg():
        sampler.sample_batch(S=a.steps, shape=[4, s, s], conditionings=[c] * ring.T, unconditional_conditionings=uc,
                             bboxs=canvas.window_centres(centres, ring), object_names=[names] * ring.T,
                             local_conditionings=[local] * ring.T, x_T=x_batch, unconditional_guidance_scale=7.5, seed=1)

    res = {"run": True, "workload": "DDIM-%d, K=2, fixed weights, synthetic weights, hipGraph, %s; canvas 512x2048 px, windows 512 px, stride 256 px: "
                                    "wrap=%s (T=%d) vs clamped (T=%d) vs sample_batch of %d 512x512 images; latents only"
                                    % (a.steps, a.dtype, a.wrap, ring.T, clamped.T, ring.T),
           "note": "every event-timed launch sits on a floor of several us: the launch ratio is an upper bound on the kernels' ratio",
           "reps": a.reps, "warmup": a.warmup, "legs": {}}
    for name, fn in (("sample_batch_8x512", batch_leg), ("canvas_wrapped_T8", canvas_leg(ring)), ("canvas_clamped_T7", canvas_leg(clamped))):
        runs, ms, n = timed(fn, a.warmup, a.reps)
        res["legs"][name] = {"s_per_trajectory": [round(r, 4) for r in runs], "best_s": round(min(runs), 4),
                             "ms_per_call": round(1e3 * min(runs) / a.steps, 3), "launches_between_unet_calls": n,
                             "their_device_us_per_call": round(1e3 * ms / a.steps, 2)}
        print("[%s] %s" % (name, res["legs"][name]), file=sys.stderr, flush=True)
    legs = res["legs"]
    res["step_launch_us"] = {"wrapped": legs["canvas_wrapped_T8"]["their_device_us_per_call"],
                             "clamped": legs["canvas_clamped_T7"]["their_device_us_per_call"],
                             "wrapped_over_clamped_upper_bound": round(legs["canvas_wrapped_T8"]["their_device_us_per_call"]
                                                                       / legs["canvas_clamped_T7"]["their_device_us_per_call"], 3)}
    base = legs["sample_batch_8x512"]["best_s"]
    res["trajectory"] = {"wrapped_vs_sample_batch_of_8": round(legs["canvas_wrapped_T8"]["best_s"] / base, 4),
                         "window_work_ms_per_call": round(1e3 * (legs["canvas_wrapped_T8"]["best_s"] - base) / a.steps, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
