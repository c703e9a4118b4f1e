"""What the window work of a canvas costs: one 512 x 2048 canvas (stride 256: T = 7 windows) against `sample_batch` of seven 512 x 512
images at the same settings — DDIM, 50 steps, K = 2, fixed blend weights, synthetic weights, hipGraph replay. Both run the same UNet
batch of 14 rows per call, so the ratio is the cost of the window gather, the overlap mean and the scatter of the next inputs.

Two canvas legs: the fused step (one sta_sampler_step_windows launch per call) and the fast path forced off (`canvas_fused_step = False`:
sta_window_fuse + sta_sampler_step + sta_window_split per call), to show what the fused launch buys. The latent is timed (no decode:
the decoders differ in shape, not in window work). Besides the wall time of whole trajectories, one more trajectory per leg runs with HIP
events around every launch between the UNet calls (event-timed launches have a floor of some 15 us each). Imports bench.py for the environment and sys.path of the bench run.

    python tools/canvas_throughput.py [--steps 50] [--reps 3] [--warmup 1] [--dtype fp16] [--out profiles/canvas_throughput.json]
Prints one JSON line and writes it to --out.
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


class LaunchTimer:
    """HIP events around every launch the samplers make between UNet calls (the step, and the window kernels of a canvas)."""
    NAMES = (("solver", "solver_step"), ("canvas", "sampler_step_windows"), ("canvas", "window_fuse"), ("canvas", "window_split"))

    def __init__(self):
        from sta import canvas, solver
        self.mods, self.saved, self.pairs = {"solver": solver, "canvas": canvas}, {}, []

    def __enter__(self):
        for mod, name in self.NAMES:
            inner = getattr(self.mods[mod], name)
            self.saved[(mod, name)] = inner

            def timed_call(*a, _inner=inner, **k):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = _inner(*a, **k)
                e.record()
                self.pairs.append((s, e))
                return out
            setattr(self.mods[mod], name, timed_call)
        return self

    def __exit__(self, *exc):
        for (mod, name), inner in self.saved.items():
            setattr(self.mods[mod], name, inner)

    def total_ms(self):
        torch.cuda.synchronize()
        return sum(s.elapsed_time(e) for s, e in self.pairs), len(self.pairs)


def timed(fn, warmup, reps):
    """-> (wall seconds of each of `reps` trajectories, device ms and count of the launches between the UNet calls of one more)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    with LaunchTimer() as tm:
        fn()
        ms, n = tm.total_ms()
    return runs, ms, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "canvas_throughput.json"))
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
    grid = canvas.window_grid(64, 256, s, 32)
    names = ["cat", "dog"]
    uc, c, local = conditionings(model, "a cat left of a dog on a street", names, dt)
    centres = [list(v) for v in DEFAULT_CENTRES[:K]]
    gen = torch.Generator(device=dev).manual_seed(1)
    x_canvas = torch.randn([1, 4, grid.Hc, grid.Wc], generator=gen, device=dev)
    x_batch = torch.randn([grid.T, 4, s, s], generator=gen, device=dev)
    sampler = DDIMSampler(model, opt_epochs=0, use_graph=True, save_images=False)

    def canvas_leg():
        sampler.sample_canvas(S=a.steps, canvas=(grid.Hc, grid.Wc), window=s, stride=grid.stride, conditionings=[c],
                              unconditional_conditionings=uc, bboxs=[centres], object_names=[names], local_conditionings=[local],
                              x_T=x_canvas, unconditional_guidance_scale=7.5, seed=1)

    def batch_leg():
        sampler.sample_batch(S=a.steps, shape=[4, s, s], conditionings=[c] * grid.T, unconditional_conditionings=uc,
                             bboxs=canvas.window_centres(centres, grid), object_names=[names] * grid.T,
                             local_conditionings=[local] * grid.T, x_T=x_batch, unconditional_guidance_scale=7.5, seed=1)

    res = {"run": True, "workload": "DDIM-%d, K=2, fixed weights, synthetic weights, hipGraph, %s; canvas 512x2048 px, windows 512 px, stride 256 px "
                                    "(T=%d) vs sample_batch of %d 512x512 images; latents only" % (a.steps, a.dtype, grid.T, grid.T),
           "reps": a.reps, "warmup": a.warmup, "legs": {}}
    for name, fn, fused in (("sample_batch_7x512", batch_leg, True), ("canvas_fused_step", canvas_leg, True), ("canvas_three_launches", canvas_leg, False)):
        sampler.canvas_fused_step = fused
        runs, ms, n = timed(fn, a.warmup, a.reps)
        res["legs"][name] = {"s_per_trajectory": [round(r, 4) for r in runs], "best_s": round(min(runs), 4),
                             "ms_per_call": round(1e3 * min(runs) / a.steps, 3), "launches_between_unet_calls": n,
                             "their_device_us_per_call": round(1e3 * ms / a.steps, 2)}
        print("[%s] %s" % (name, res["legs"][name]), file=sys.stderr, flush=True)
    base = res["legs"]["sample_batch_7x512"]["best_s"]
    for name in ("canvas_fused_step", "canvas_three_launches"):
        res["legs"][name]["vs_sample_batch"] = round(res["legs"][name]["best_s"] / base, 4)
        res["legs"][name]["window_work_ms_per_call"] = round(1e3 * (res["legs"][name]["best_s"] - base) / a.steps, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
