"""What the layout-guided hi-res fix costs, at the settings of tools/canvas_img2img_throughput.py — DDIM, 50 steps, t_start = 25, K = 2, fixed
blend weights, synthetic weights, hipGraph replay, latents only.

Two figures, both from this one run.
(a) The entry launch, timed with HIP events around it: the fused sta_latent_upscale_step_windows against the sequence it replaces
    (the torch restatement of the upscale and the noising, then sta_window_split) issued back to back, the two forms alternating, for
    512^2 -> 1024^2 and 512x2048 -> 1024x4096 pixels (windows 512, stride 256), clamped and wrapped along x. Median and quartiles: the
    quartiles are the run's own spread. Every event-timed launch sits on a floor of several us, which the fused form pays once and the
    sequence once per launch in it; the bytes the fused form moves are counted from the shapes. The two forms round the noising
    differently (one fused multiply-add against a product and a sum), so their x differ in the last bit here and there and a few of
    the 16-bit window inputs with them: both are counted.
(b) Seconds per two-pass trajectory (`sample` of a 512^2 image, then `hires_canvas` to 1024^2: 25 UNet calls of 2 T window rows, T = 9)
    against the first pass alone plus `decode_batch` of T 512^2 images at the same t_start, which runs the same UNet batches: the
    difference is the cost of the upscale and the window work. --wide adds the same for a 512x2048 canvas closed along x refined at
    1024x4096 (T = 48).

    python tools/hires_throughput.py [--steps 50] [--t_start 25] [--reps 3] [--warmup 1] [--dtype fp16] [--wide] [--out profiles/hires_throughput.json]
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from canvas_throughput import timed  # noqa: E402  (imports bench.py for the environment and sys.path of the bench run)

import torch  # noqa: E402


def event_us(fns, warmup=20, reps=200):
    """Per callable (median, lower quartile, upper quartile) device microseconds, HIP events around one issue of it, the callables
    alternating."""
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
    out = []
    for p in pairs:
        us = sorted(1e3 * a.elapsed_time(b) for a, b in p)
        q = statistics.quantiles(us, n=4)
        out.append([round(statistics.median(us), 2), round(q[0], 2), round(q[2], 2)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--t_start", type=int, default=25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    ap.add_argument("--wide", action="store_true", help="also time the two-pass trajectory 512x2048 -> 1024x4096, wrapped along x")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hires_throughput.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("a GPU is required: nothing here is a measurement without one")
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta import canvas, lib
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, use_shipped_miopen_db
    dev = torch.device("cuda", 0)
    lib.load()
    use_shipped_miopen_db(0)
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    model = build_sd_v1(dev, dt, init_weights=True, seed=0, channels_last=True)
    K, s, stride = 2, 64, 32
    names = ["cat", "dog"]
    uc, c, local = conditionings(model, "a cat left of a dog on a street", names, dt)
    centres = [list(v) for v in DEFAULT_CENTRES[:K]]
    gen = torch.Generator(device=dev).manual_seed(1)
    sampler = DDIMSampler(model, opt_epochs=0, use_graph=True, save_images=False)
    sampler.make_schedule(a.steps, ddim_eta=0.0, verbose=False)
    t_enc = min(a.t_start, a.steps - 1)
    sa, s1m = (float(v[t_enc]) for v in sampler._encode_coefs())
    res = {"run": True, "workload": "DDIM-%d, t_start=%d, K=2, fixed weights, synthetic weights, hipGraph, %s; windows 512 px, stride 256 px; "
                                    "latents only" % (a.steps, a.t_start, a.dtype),
           "note": "every event-timed launch sits on a floor of several us; [median, lower quartile, upper quartile] in us",
           "reps": a.reps, "warmup": a.warmup, "entry_launch": {}, "legs": {}, "trajectory": {}}

    # (a) the entry launch: fused against the sequence it replaces
    for name, (h, w), wrap in (("512x512_to_1024x1024_clamped", (64, 64), ""), ("512x512_to_1024x1024_wrap_x", (64, 64), "x"),
                               ("512x2048_to_1024x4096_clamped", (64, 256), ""), ("512x2048_to_1024x4096_wrap_x", (64, 256), "x")):
        grid = canvas.window_grid(2 * h, 2 * w, s, stride, wrap)
        z = torch.randn([1, 4, h, w], generator=gen, device=dev)
        noise = torch.randn([1, 4, grid.Hc, grid.Wc], generator=gen, device=dev)
        one = lambda: canvas.upscale_step_windows(z, noise, sa, s1m, grid, dt)
        two = lambda: canvas.window_split(canvas.upscale_step_windows_reference(z, noise, sa, s1m, grid, want_xin=False)[0], grid, dt)
        a_out, b_out = one(), two()
        differ = (a_out[0] - canvas.upscale_step_windows_reference(z, noise, sa, s1m, grid, want_xin=False)[0]).abs().max().item()
        assert differ <= 32 * 2.0 ** -24 * (abs(sa) * z.abs().max().item() + abs(s1m) * noise.abs().max().item()), differ
        (f_us, f_lo, f_hi), (u_us, u_lo, u_hi) = event_us([one, two])
        px = grid.Hc * grid.Wc
        res["entry_launch"][name] = {"T": grid.T, "fused_us": [f_us, f_lo, f_hi], "restatement_plus_split_us": [u_us, u_lo, u_hi],
                                     "fused_over_sequence": round(f_us / u_us, 3), "max_abs_difference_of_x": differ,
                                     "fused_bytes": 4 * 4 * (h * w + 2 * px) + 2 * grid.T * 4 * s * s * 2,
                                     "xin_elements_that_differ": int((a_out[2] != b_out).sum())}
        print("[entry %s] %s" % (name, res["entry_launch"][name]), file=sys.stderr, flush=True)

    # (b) two passes against the first pass alone + decode_batch of T windows; latents only: no decode is part of the comparison
    vae, model.first_stage_model = model.first_stage_model, None
    try:
        cases = [("512x512_to_1024x1024_clamped", None, canvas.window_grid(128, 128, s, stride))]
        if a.wide:
            cases.append(("512x2048_to_1024x4096_wrap_x", canvas.window_grid(64, 256, s, stride, "x"), canvas.window_grid(128, 512, s, stride, "x")))
        for name, g1, g2 in cases:
            kw = dict(conditionings=[c], unconditional_conditionings=uc, bboxs=[centres], object_names=[names], local_conditionings=[local],
                      unconditional_guidance_scale=7.5, seed=1)
            x_T = torch.randn([1, 4, 64, 64] if g1 is None else [1, 4, g1.Hc, g1.Wc], generator=gen, device=dev)

            def first():
                if g1 is None:
                    sampler.sample(S=a.steps, conditioning=c, batch_size=1, shape=[4, 64, 64], verbose=False, unconditional_guidance_scale=7.5,
                                   unconditional_conditioning=uc, eta=0.0, x_T=x_T, text_index=0, curr_text="x", bboxs_curr=centres, seed=1,
                                   prompt_idx=0, object_names=names, local_conditionings=local)
                else:
                    sampler.sample_canvas(S=a.steps, canvas=(g1.Hc, g1.Wc), window=s, stride=stride, x_T=x_T, eta=0.0, wrap=g1.wrap, **kw)
                return sampler.last_result["x0"]

            def two_pass():
                sampler.hires_canvas(first(), (g2.Hc, g2.Wc), s, stride, t_start=a.t_start, wrap=g2.wrap, **kw)
            x_batch = torch.randn([g2.T, 4, s, s], generator=gen, device=dev)

            def baseline():
                first()
                sampler.decode_batch(x_batch, [c] * g2.T, uc, canvas.window_centres(centres, g2), [names] * g2.T, [local] * g2.T, a.t_start,
                                     unconditional_guidance_scale=7.5, seed=1)
            for leg, fn in (("first_pass_plus_decode_batch_%dx512_%s" % (g2.T, name), baseline), ("two_pass_" + name, two_pass)):
                runs, ms, n = timed(fn, a.warmup, a.reps)
                res["legs"][leg] = {"s_per_trajectory": [round(r, 4) for r in runs], "best_s": round(min(runs), 4),
                                    "launches_between_unet_calls": n, "their_device_ms": round(ms, 3)}
                print("[%s] %s" % (leg, res["legs"][leg]), file=sys.stderr, flush=True)
            base = res["legs"]["first_pass_plus_decode_batch_%dx512_%s" % (g2.T, name)]["best_s"]
            two = res["legs"]["two_pass_" + name]["best_s"]
            res["trajectory"][name] = {"T": g2.T, "two_pass_vs_first_pass_plus_decode_batch": round(two / base, 4),
                                       "upscale_and_window_work_ms_per_refine_call": round(1e3 * (two - base) / a.t_start, 3)}
    finally:
        model.first_stage_model = vae
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
