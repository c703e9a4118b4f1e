"""What attention-guided sampling costs: python tools/attn_guidance_bench.py [--out profiles/attn_guidance.md] [--images 16]

1. The update launch sta_latent_guide (xin and stats written, no mask) at the bench shape (16 images of 4 x 64 x 64) and at a shape large
   enough to show bandwidth, next to sta_latent_blend at the same (b, n) in the same process, in both 16-bit types: HIP events around
   every launch, the two alternating, medians over --launches after --warmup. Bytes = what must cross HBM at least once
   (g, x, x_out, xin: 16 b n; the blend: x, x0, noise, x_out, xin, mask).
2. The flagship shapes (full-width synthetic UNet, NHWC trunk, 512 x 512, K = 2, --images prompts per step), DDIM with --ddim_steps calls:
   unguided, 10 guided calls with blocks="down" and with blocks="all", alternating, host clock around sample_batch ending in a device
   synchronise, medians. One evaluation (forward to the last recording block or the whole UNet, backward to the input pair, the update
   launch) = (guided - unguided) / guided calls; one ordinary call = unguided / calls.
Writes the note given by --out (raw JSON lines go to stdout). Needs a GPU: a timing from anywhere else says nothing."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))
from sta import guidance, solver  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_guidance.md"))
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--ddim_steps", type=int, default=50)
ap.add_argument("--guided", type=int, default=10, help="guided calls per trajectory")
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--reps", type=int, default=3, help="timed sample_batch calls per variant")
ap.add_argument("--no-sampler", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("attn_guidance_bench needs a GPU")
dev = torch.device("cuda", 0)
K = 2


def launch_leg(b, side, dtype_name):
    dt = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(b, 4, side, side, generator=gen, device=dev)
    g = (torch.randn(2 * b, 4, side, side, generator=gen, device=dev) * 1e-3).to(dt)
    step = torch.full((b,), 0.05, device=dev)
    bl = solver.Blend(torch.randn_like(x), (torch.rand(b, 1, side, side, generator=gen, device=dev) > 0.5).float(), torch.randn_like(x), 0.8, 0.6)
    variants = {"sta_latent_guide": lambda: guidance.latent_guide(g, x, step, want_xin=True),
                "sta_latent_blend": lambda: solver.latent_blend(x, bl, dtype=dt, want_xin=True)}
    n = x[0].numel()
    nbytes = {"sta_latent_guide": 16 * b * n, "sta_latent_blend": 20 * b * n + 4 * b * side * side}
    times = {k: [] for k in variants}
    for i in range(a.warmup + a.launches):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    rows = []
    for name, t in times.items():
        med = statistics.median(t)
        rec = {"kernel": name, "b": b, "n": n, "dtype": dtype_name, "launches": len(t), "us_median": round(med, 2), "us_min": round(min(t), 2),
               "us_max": round(max(t), 2), "bytes": nbytes[name], "GBs": round(nbytes[name] / med / 1e3, 1), "share_of_8TBs": round(nbytes[name] / med / 1e3 / 8000.0, 4)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def sampler_leg(I, dtype_name):
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts, use_shipped_miopen_db
    dt = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    use_shipped_miopen_db(0)
    model = build_sd_v1(dev, dt, with_vae=False, init_weights=True, seed=0, channels_last=True)
    torch.backends.cudnn.benchmark = False          # immediate-mode library convolutions for conv_in / Downsample / conv_out and their
    #                                                 input gradients: no per-shape solver search inside a timed leg
    unet = model.model.diffusion_model
    prompts = load_prompts(64)
    centres = [list(c) for c in DEFAULT_CENTRES[:K]]
    recs = [prompts[i % len(prompts)] for i in range(I)]
    names = [(r["objects"] + ["object"] * K)[:K] for r in recs]
    conds = [conditionings(model, r["prompt"], nm, dt) for r, nm in zip(recs, names)]
    x_T1 = torch.randn([1, 4, 64, 64], generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    mk = lambda **kw: DDIMSampler(model, opt_epochs=0, use_graph=True, save_images=False,
                                  latent_guidance=guidance.AttnGuidance(unet, resolution=16, scale=0.1, steps=a.guided, **kw) if kw else None)
    samplers = {"unguided": mk(), 'guided, blocks="down"': mk(blocks="down"), 'guided, blocks="all"': mk(blocks="all")}

    def run(s):
        s.sample_batch(S=a.ddim_steps, shape=[4, 64, 64], conditionings=[c[1] for c in conds], unconditional_conditionings=[c[0] for c in conds],
                       bboxs=[centres] * I, object_names=names, local_conditionings=[c[2] for c in conds], curr_texts=[r["prompt"] for r in recs],
                       x_T=x_T1.expand(I, -1, -1, -1), unconditional_guidance_scale=7.5, seed=1)
        torch.cuda.synchronize()
        return s

    times = {n: [] for n in samplers}
    for rep in range(1 + a.reps):                 # first round: warm-up (graph capture, packed weights, library algorithm choice)
        for name, s in samplers.items():          # alternating: every variant sees the same clocks
            t0 = time.perf_counter()
            run(s)
            if rep:
                times[name].append(time.perf_counter() - t0)
    rows = []
    base = statistics.median(times["unguided"])
    for name, t in times.items():
        med = statistics.median(t)
        res = samplers[name].last_guidance
        rec = {"sampler_leg": name, "images": I, "ddim_steps": a.ddim_steps, "guided_calls": 0 if res is None else len(res["calls"]), "dtype": dtype_name,
               "runs": len(t), "s_median": round(med, 4), "s_min": round(min(t), 4), "s_max": round(max(t), 4), "images_per_s": round(I / med, 2),
               "ordinary_call_ms": round(1e3 * base / a.ddim_steps, 2),
               "evaluation_ms": None if res is None else round(1e3 * (med - base) / len(res["calls"]), 2),
               "evaluation_in_ordinary_calls": None if res is None else round((med - base) / len(res["calls"]) / (base / a.ddim_steps), 3),
               "E_first": None if res is None else round(res["energy"][0].mean().item(), 5),
               "E_last": None if res is None else round(res["energy"][-1].mean().item(), 5), "skipped": None if res is None else res["skipped"]}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    del samplers, model
    torch.cuda.empty_cache()
    return rows


launch = []
for dtype_name in ("fp16", "bf16"):
    launch += launch_leg(a.images, 64, dtype_name) + launch_leg(64, 128, dtype_name)
samp = []
if not a.no_sampler:
    for dtype_name in ("fp16", "bf16"):
        samp += sampler_leg(a.images, dtype_name)

md = ["# Attention-guided sampling: what `sta_latent_guide` and a guidance evaluation cost", "",
      "Written by `python tools/attn_guidance_bench.py` on one MI355X (%s); the tables below are from that one run." % torch.cuda.get_device_name(0), "",
      "## The update launch, next to `sta_latent_blend` at the same (b, n)", "",
      "HIP events around each launch, the two kernels alternating in one process, %d launches after %d warm-ups. `sta_latent_guide` writes xin and" % (a.launches, a.warmup),
      "stats and takes no mask; bytes = what must cross HBM at least once (g, x, x_out, xin = 16 b n for the update; x, x0, noise, x_out, xin and the",
      "mask for the blend). The update reads g a second time (and its workgroups each reduce their image's whole g): those reads are served by",
      "L2 / the Infinity Cache and are not counted. At the bench shape both launches move 4 - 5 MB and are bound by launch latency, not bandwidth;",
      "at the large shape the 16 workgroups of an image each read its whole 256 KB gradient for the reduction, which is what the update pays over",
      "the blend there.", "",
      "| b | n | type | kernel | median µs (min … max) | bytes | GB/s | share of 8 TB/s |", "|---|---|---|---|---|---|---|---|"]
for r in launch:
    md.append("| %d | %d | %s | `%s` | %.2f (%.2f … %.2f) | %d | %.0f | %.3f |" % (r["b"], r["n"], r["dtype"], r["kernel"], r["us_median"], r["us_min"], r["us_max"],
                                                                              r["bytes"], r["GBs"], r["share_of_8TBs"]))
md += ["", "Update / blend, median time: " + ", ".join("b = %d, n = %d, %s: %.2f x" % (g["b"], g["n"], g["dtype"], g["us_median"] / bl["us_median"])
                                                       for g, bl in zip(launch[0::2], launch[1::2])) + ".", "",
       "## DDIM with guided calls at the bench shapes", ""]
if samp:
    md += ["Full-width SD-v1 UNet, synthetic weights, NHWC trunk, no VAE, %d prompts per step, K = 2, 512 x 512, DDIM with %d calls, the first %d of them" % (a.images, a.ddim_steps, a.guided),
           "guided (one update each, readouts at 16 x 16, eta = 0.1). Host clock around `sample_batch` ending in a device synchronise, %d timed calls" % a.reps,
           "per variant after one warm-up round, variants alternating; ordinary calls are graph-replayed, evaluations eager. One ordinary call =",
           "unguided / calls (the parent commit's path: nothing of it changed); one evaluation = (guided - unguided) / guided calls: the forward under",
           "autograd (to the last recording encoder block, or the whole UNet), the backward to the input pair and the update launch.", "",
           "| type | variant | median s (min … max) | images/s | ordinary call ms | evaluation ms | evaluation / ordinary call | mean E before first / last update | skipped |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in samp:
        md.append("| %s | %s | %.3f (%.3f … %.3f) | %.2f | %.2f | %s | %s | %s | %s |"
                  % (r["dtype"], r["sampler_leg"], r["s_median"], r["s_min"], r["s_max"], r["images_per_s"], r["ordinary_call_ms"],
                     "–" if r["evaluation_ms"] is None else "%.2f" % r["evaluation_ms"],
                     "–" if r["evaluation_in_ordinary_calls"] is None else "%.2f" % r["evaluation_in_ordinary_calls"],
                     "–" if r["E_first"] is None else "%.4f / %.4f" % (r["E_first"], r["E_last"]), "–" if r["skipped"] is None else r["skipped"]))
    md += ["", "The energies are those of synthetic weights: they say that the update runs and moves the energy, nothing about pictures."]
else:
    md.append("Not measured in this run (`--no-sampler`).")
md.append("")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(md))
print("wrote", a.out)
