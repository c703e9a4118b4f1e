"""What the inpainting blend costs on a canvas: one 512 x 2048 canvas (stride 256: T = 7 windows) with its left 512 x 512 kept, DDIM,
50 steps, K = 2, fixed blend weights, synthetic weights, hipGraph replay. Three legs on the same box in one run:
  masked_fused            inpaint_canvas: sta_window_blend, then one sta_sampler_step_windows_masked launch per call;
  masked_three_launches   the same with `canvas_fused_step = False` (sta_window_fuse + sta_sampler_step_masked + sta_window_split per call);
  unmasked                sample_canvas: one sta_sampler_step_windows launch per call.
All three run the same UNet batch of 14 rows per call; the masked launch reads three more canvas-sized fp32 streams (x0, keep over the
channels, the blend noise) than the unmasked one. Besides the wall time of whole trajectories, one more trajectory per leg runs with HIP
events around every launch between the UNet calls (event-timed launches have a floor of some 15 us each); the step launches of a call
are reported per leg and as ratios against the unmasked leg and against the three-launch form. The blend draws are made once, before
the legs (`mask_noise` as a list): a torch.randn right in front of a timed launch would be counted into its event pair. The latent is
timed (no decode).

    python tools/canvas_inpaint_throughput.py [--steps 50] [--reps 3] [--warmup 1] [--dtype fp16] [--out profiles/canvas_inpaint_throughput.json]
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from canvas_throughput import REPO, LaunchTimer  # noqa: E402  (imports bench.py: environment and sys.path of the bench run)

import torch  # noqa: E402


class StepTimer(LaunchTimer):
    """LaunchTimer over the masked entry points as well, with the device time kept per entry point."""
    NAMES = LaunchTimer.NAMES + (("canvas", "sampler_step_windows_masked"), ("canvas", "window_blend"), ("solver", "solver_step_masked"),
                                 ("solver", "latent_blend"))

    def __enter__(self):
        self.by_name = {}
        for mod, name in self.NAMES:
            inner = getattr(self.mods[mod], name)
            self.saved[(mod, name)] = inner

            def timed_call(*a, _inner=inner, _name=name, **k):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = _inner(*a, **k)
                e.record()
                self.by_name.setdefault(_name, []).append((s, e))
                return out
            setattr(self.mods[mod], name, timed_call)
        return self

    def per_name(self):
        torch.cuda.synchronize()
        return {name: (sum(s.elapsed_time(e) for s, e in pairs), len(pairs)) for name, pairs in self.by_name.items()}


def timed(fn, warmup, reps):
    """-> (wall seconds of each of `reps` trajectories, {entry point: (device ms, launches)} of one more)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    with StepTimer() as tm:
        fn()
        return runs, tm.per_name()


# the launches that make up the step after a UNet call, per leg
STEP = {"masked_fused": ("sampler_step_windows_masked", "sampler_step_windows"),
        "masked_three_launches": ("window_fuse", "solver_step_masked", "solver_step", "window_split"),
        "unmasked": ("sampler_step_windows",)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "canvas_inpaint_throughput.json"))
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
    shape = [1, 4, grid.Hc, grid.Wc]
    x_T = torch.randn(shape, generator=gen, device=dev)
    x0 = torch.randn(shape, generator=gen, device=dev)
    keep = torch.zeros(1, 1, grid.Hc, grid.Wc, device=dev)
    keep[..., :s] = 1.0                                      # the left 512 x 512 pixels are kept
    draws = [torch.randn(shape, generator=gen, device=dev) for _ in range(a.steps)]
    sampler = DDIMSampler(model, opt_epochs=0, use_graph=True, save_images=False, mask_noise=draws)
    kw = dict(S=a.steps, canvas=(grid.Hc, grid.Wc), window=s, stride=grid.stride, conditionings=[c], unconditional_conditionings=uc,
              bboxs=[centres], object_names=[names], local_conditionings=[local], x_T=x_T, unconditional_guidance_scale=7.5, seed=1)

    def masked_leg():
        sampler.inpaint_canvas(mask=keep, x0=x0, **kw)

    def unmasked_leg():
        sampler.sample_canvas(**kw)

    res = {"run": True, "workload": "DDIM-%d, K=2, fixed weights, synthetic weights, hipGraph, %s; canvas 512x2048 px, windows 512 px, stride 256 px "
                                    "(T=%d), the left 512x512 kept; latents only" % (a.steps, a.dtype, grid.T),
           "reps": a.reps, "warmup": a.warmup, "legs": {}}
    for name, fn, fused in (("unmasked", unmasked_leg, True), ("masked_fused", masked_leg, True), ("masked_three_launches", masked_leg, False)):
        sampler.canvas_fused_step = fused
        runs, per = timed(fn, a.warmup, a.reps)
        step_ms = sum(per[n][0] for n in STEP[name] if n in per)
        step_n = sum(per[n][1] for n in STEP[name] if n in per)
        res["legs"][name] = {"s_per_trajectory": [round(r, 4) for r in runs], "best_s": round(min(runs), 4),
                             "ms_per_call": round(1e3 * min(runs) / a.steps, 3),
                             "launches": {n: {"count": cnt, "device_us_each": round(1e3 * ms / cnt, 2)} for n, (ms, cnt) in sorted(per.items())},
                             "step_launches_per_call": round(step_n / a.steps, 2), "step_device_us_per_call": round(1e3 * step_ms / a.steps, 2)}
        print("[%s] %s" % (name, res["legs"][name]), file=sys.stderr, flush=True)
    sampler.canvas_fused_step = True
    legs = res["legs"]
    fused_us = legs["masked_fused"]["step_device_us_per_call"]
    res["masked_fused_step_vs_unmasked"] = round(fused_us / legs["unmasked"]["step_device_us_per_call"], 3)
    res["masked_fused_step_vs_three_launches"] = round(fused_us / legs["masked_three_launches"]["step_device_us_per_call"], 3)
    res["masked_fused_trajectory_vs_unmasked"] = round(legs["masked_fused"]["best_s"] / legs["unmasked"]["best_s"], 4)
    res["masked_fused_trajectory_vs_three_launches"] = round(legs["masked_fused"]["best_s"] / legs["masked_three_launches"]["best_s"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
