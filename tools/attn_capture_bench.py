"""What attention capture costs: python tools/attn_capture_bench.py [--out profiles/attn_capture.md] [--images 64] [--traj-images 8]

1. sta_xattn_token_maps alone at the two shapes a user captures — (I images, K = 2, R = 4, N = 256, C = 1280: the default 16 x 16 level)
   and (N = 4096, C = 320: level 0) — next to the sta_xattn_fwd launch of the same shape in the same process (it does strictly more
   arithmetic: the PV products and the blend on top of the same QK^T and softmax). HIP events around every launch, the two
   alternating, medians over --launches after --warmup.
2. A 50-step PLMS trajectory of the full-width UNet (synthetic weights, no VAE) without capture (hipGraph replay, the product's default),
   eager without capture, and eager with capture at 16 x 16 — capture forces the eager path, so the middle run separates the two costs.
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
from sta import attnmaps, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_capture.md"))
ap.add_argument("--images", type=int, default=64)
ap.add_argument("--traj-images", type=int, default=8)
ap.add_argument("--ddim_steps", type=int, default=50)
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=3, help="timed trajectories per variant")
ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
ap.add_argument("--bench-branch", default=None, help="file with bench.py's JSON line on this branch (recorded in the note)")
ap.add_argument("--bench-parent", default=None, help="the same on the parent commit, same box")
ap.add_argument("--no-trajectory", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("attn_capture_bench needs a GPU")
dev = torch.device("cuda", 0)
dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
K, R, M, heads = 2, 4, 77, 8
SEL = [1, 1, 2, 3]


def kernel_leg(I, N, C):
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(2 * I, N, C, generator=g, device=dev).to(dt)
    k = (torch.randn(I * (K + 2), M, C, generator=g, device=dev) * 0.7).to(dt)
    v = torch.randn(I * (K + 2), M, C, generator=g, device=dev).to(dt)
    packed = ops.pack_kv(k, v, heads, n_img=I)
    side = int(N ** 0.5)
    mask = torch.stack([ops.disc_mask_bits([(0.3, 0.4), (0.7, 0.6)], side)] * I).to(dev)
    coef = torch.full((I * K,), 2.5, device=dev)
    w = torch.zeros(I, R, M, device=dev)
    w[:, :, 2] = 1.0
    out = torch.zeros(I, R, N, device=dev)
    scale = (C // heads) ** -0.5
    variants = {"sta_xattn_token_maps": lambda: attnmaps.token_maps(q, packed, SEL, w, scale, out=out, accumulate=True),
                "sta_xattn_fwd": lambda: ops.xattn_forward(q, packed, mask, coef, scale)}
    times = {n: [] for n in variants}
    for i in range(a.warmup + a.launches):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    d = C // heads
    # what the algorithm needs: QK^T for the contexts attended (token maps: 3 of the 4 here; forward: all 4, plus PV), q read once per context row
    flop_maps = 2.0 * I * heads * N * 80 * d * len(set(SEL))
    flop_fwd = 2.0 * I * heads * N * 80 * d * (K + 2) * 2
    rows = []
    for name, t in times.items():
        med = statistics.median(t)
        rec = {"kernel": name, "I": I, "N": N, "C": C, "K": K, "R": R, "dtype": a.dtype, "launches": len(t), "us_median": round(med, 1),
               "us_min": round(min(t), 1), "us_max": round(max(t), 1),
               "TFLOPs_algorithmic": round((flop_maps if "maps" in name else flop_fwd) / med / 1e6, 1)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def trajectory_leg(I):
    from ldm.models.diffusion.plms import PLMSSampler
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts, use_shipped_miopen_db
    use_shipped_miopen_db(0)
    model = build_sd_v1(dev, dt, with_vae=False, init_weights=True, seed=0, channels_last=True)
    prompts = load_prompts(64)
    centres = [list(c) for c in DEFAULT_CENTRES[:K]]
    recs = [prompts[i % len(prompts)] for i in range(I)]
    names = [(r["objects"] + ["object"] * K)[:K] for r in recs]
    conds = [conditionings(model, r["prompt"], nm, dt) for r, nm in zip(recs, names)]
    x_T = torch.randn([1, 4, 64, 64], generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    cap = attnmaps.AttnCapture(model.model.diffusion_model, resolution=16)
    samplers = {"graph replay, no capture": PLMSSampler(model, opt_epochs=0, use_graph=True, save_images=False),
                "eager, no capture": PLMSSampler(model, opt_epochs=0, use_graph=False, save_images=False),
                "eager, capture at 16 x 16": PLMSSampler(model, opt_epochs=0, use_graph=True, save_images=False, attn_capture=cap)}

    def run(s):
        s.sample_batch(S=a.ddim_steps, shape=[4, 64, 64], conditionings=[c[1] for c in conds], unconditional_conditionings=[c[0] for c in conds],
                       bboxs=[centres] * I, object_names=names, local_conditionings=[c[2] for c in conds], curr_texts=[r["prompt"] for r in recs],
                       x_T=x_T.expand(I, -1, -1, -1), unconditional_guidance_scale=7.5, seed=1)
        torch.cuda.synchronize()

    times = {n: [] for n in samplers}
    for rep in range(1 + a.reps):                 # first round: warm-up (graph capture, library algorithm choice)
        for name, s in samplers.items():          # alternating: every variant sees the same clocks
            t0 = time.perf_counter()
            run(s)
            if rep:
                times[name].append(time.perf_counter() - t0)
    rows = []
    for name, t in times.items():
        rec = {"trajectory": name, "images": I, "ddim_steps": a.ddim_steps, "dtype": a.dtype, "runs": len(t), "s_median": round(statistics.median(t), 3),
               "s_min": round(min(t), 3), "s_max": round(max(t), 3)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    r = samplers["eager, capture at 16 x 16"].last_attn
    rows.append({"block_calls": r.block_calls, "calls": r.calls, "in_disc_mass_image0": [round(float(x), 3) for x in r.in_disc_mass[0]]})
    print(json.dumps(rows[-1]), flush=True)
    return rows


def _line(path):
    if not path or not os.path.exists(path):
        return "not recorded"
    lines = [l.strip() for l in open(path) if l.strip().startswith("{")]
    return "`%s`" % lines[-1][:600] if lines else "not recorded"


kern = kernel_leg(a.images, 256, 1280) + kernel_leg(a.images, 4096, 320)
traj = [] if a.no_trajectory else trajectory_leg(a.traj_images)
md = ["# Attention capture: what `sta_xattn_token_maps` and `--attn_maps` cost", "",
      "Written by `python tools/attn_capture_bench.py` on one MI355X (%s, %s); every figure below is from that one run." % (torch.cuda.get_device_name(0), a.dtype), "",
      "## The launch, next to `sta_xattn_fwd` at the same shape", "",
      "HIP events around each launch, the two kernels alternating in one process, %d launches after %d warm-ups. K = 2, R = 4 readouts" % (a.launches, a.warmup),
      "(two on the global context, one per local context: three contexts attended), I = %d images. `sta_xattn_fwd` does strictly more arithmetic" % a.images,
      "(all four contexts, the PV products and the blend).", "",
      "| shape | kernel | median µs (min … max) | algorithmic TFLOP/s |", "|---|---|---|---|"]
for r in kern:
    md.append("| N = %d, C = %d | `%s` | %.1f (%.1f … %.1f) | %.1f |" % (r["N"], r["C"], r["kernel"], r["us_median"], r["us_min"], r["us_max"], r["TFLOPs_algorithmic"]))
md += ["", "## A %d-step PLMS trajectory with and without capture" % a.ddim_steps, ""]
if traj:
    md += ["Full-width SD-v1 UNet, synthetic weights, no VAE, %d images per CFG batch, 64 x 64 latent; host clock around `sample_batch` ending in a device" % a.traj_images,
           "synchronise, %d timed runs per variant after one warm-up round, variants alternating. Capture runs the kept trajectory eagerly, so the" % a.reps,
           "eager run without capture separates the cost of losing graph replay from the cost of the capture launches.", "",
           "| variant | median s (min … max) |", "|---|---|"]
    for r in traj:
        if "trajectory" in r:
            md.append("| %s | %.3f (%.3f … %.3f) |" % (r["trajectory"], r["s_median"], r["s_min"], r["s_max"]))
    md += ["", "Captured block-calls: %d over %d UNet calls." % (traj[-1]["block_calls"], traj[-1]["calls"])]
else:
    md.append("Not measured in this run (`--no-trajectory`).")
md += ["", "## `bench.py` with capture off: branch against parent, same box", "", "- branch: " + _line(a.bench_branch), "- parent: " + _line(a.bench_parent), ""]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(md))
print("wrote", a.out)
