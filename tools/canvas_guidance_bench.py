"""What attention guidance costs on a canvas: python tools/canvas_guidance_bench.py [--out profiles/canvas_guidance.md]

One 512 x 2048 canvas (latent 64 x 256, windows of 64, stride 32: T = 7 clamped, T = 8 wrapped along x), fp16, K = 2, full-width synthetic
UNet, NHWC trunk, no VAE.
1. The update launch sta_latent_guide_windows (xin and stats written, no mask), HIP events around every launch, in the same process
   and alternating with the unfused sequence it replaces: the adjoint gather in torch (an fp32 sum over the windows, rounded to the 16-bit
   pair), sta_latent_guide on the canvas-shaped pair, sta_window_split. Every event-timed launch sits on a floor of several us.
2. DDIM with --ddim_steps calls on the canvas: unguided `sample_canvas`, `sample_canvas` with --guided guided calls (CanvasGuidance, one
   update each, readouts at 16 x 16, eta = 0.1), and guided `sample_batch` of T 512 x 512 images (AttnGuidance) — the same UNet batch per
   call —, alternating, host clock around each call ending in a device synchronise, medians. One ordinary (graph-replayed) canvas call =
   unguided / calls; one evaluation (forward to the last recording block under autograd, backward to the window pairs, the update launch) =
   (guided - unguided) / guided calls.
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
from sta import canvas, guidance  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "canvas_guidance.md"))
ap.add_argument("--ddim_steps", type=int, default=50)
ap.add_argument("--guided", type=int, default=10, help="guided calls per trajectory")
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=3, help="timed trajectories per variant")
ap.add_argument("--no-sampler", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("canvas_guidance_bench needs a GPU")
dev = torch.device("cuda", 0)
K, S_WIN, DT = 2, 64, torch.float16
GRIDS = {"clamped, T = 7": canvas.window_grid(64, 256, S_WIN, 32), "wrapped along x, T = 8": canvas.window_grid(64, 256, S_WIN, 32, "x")}


def unfused(g, x, step, grid):
    """The sequence the launch replaces: the split's adjoint in torch, sta_latent_guide, sta_window_split."""
    P, C = x.shape[0], x.shape[1]
    gw = g.reshape(P, grid.T, 2, C, grid.s, grid.s)
    acc = torch.zeros((P, 2, C, grid.Hc, grid.Wc), dtype=torch.float32, device=g.device)
    for w, (y0, x0) in enumerate(canvas.windows(grid)):
        acc[(Ellipsis,) + canvas._region(grid, y0, x0, g.device)] += gw[:, w].float()
    x_out, _, rms = guidance.latent_guide(acc.reshape(2 * P, C, grid.Hc, grid.Wc).to(g.dtype), x, step)
    return x_out, canvas.window_split(x_out, grid, g.dtype), rms


def launch_leg(name, grid):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(1, 4, grid.Hc, grid.Wc, generator=gen, device=dev)
    g = (torch.randn(2 * grid.T, 4, S_WIN, S_WIN, generator=gen, device=dev) * 1e-3).to(DT)
    step = torch.full((1,), 0.05, device=dev)
    count = torch.full((1,), float(x.numel()), device=dev)
    variants = {"sta_latent_guide_windows": lambda: canvas.latent_guide_windows(g, x, step, count, grid, want_xin=True),
                "gather (torch) + sta_latent_guide + sta_window_split": lambda: unfused(g, x, step, grid)}
    one, three = (fn() for fn in variants.values())
    torch.cuda.synchronize()
    # the unfused form rounds the summed gradient to 16 bits before the update: the two agree to that rounding, not bit for bit
    rel = ((one[0] - three[0]).abs().max() / (one[0] - x).abs().max()).item()
    times = {k: [] for k in variants}
    for i in range(a.warmup + a.launches):
        for key, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[key].append(e0.elapsed_time(e1) * 1e3)
    rows = []
    for key, t in times.items():
        rec = {"grid": name, "form": key, "launches": len(t), "us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2),
               "us_max": round(max(t), 2), "max_dx_difference_over_max_dx": round(rel, 5)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def sampler_leg():
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, use_shipped_miopen_db
    use_shipped_miopen_db(0)
    model = build_sd_v1(dev, DT, with_vae=False, init_weights=True, seed=0, channels_last=True)
    torch.backends.cudnn.benchmark = False          # immediate-mode library convolutions: no per-shape solver search inside a timed leg
    unet = model.model.diffusion_model
    grid = GRIDS["clamped, T = 7"]
    names = ["cat", "dog"]
    prompt = "a cat left of a dog on a street"
    uc, c, local = conditionings(model, prompt, names, DT)
    centres = [list(v) for v in DEFAULT_CENTRES[:K]]
    gen = torch.Generator(device=dev).manual_seed(1)
    x_canvas = torch.randn([1, 4, grid.Hc, grid.Wc], generator=gen, device=dev)
    x_batch = torch.randn([grid.T, 4, S_WIN, S_WIN], generator=gen, device=dev)
    gkw = dict(resolution=16, scale=0.1, steps=a.guided)
    mk = lambda **kw: DDIMSampler(model, opt_epochs=0, use_graph=True, save_images=False, **kw)
    samplers = {"sample_canvas, unguided": mk(), "sample_canvas, guided": mk(canvas_guidance=guidance.CanvasGuidance(unet, **gkw)),
                "sample_batch of %d 512 x 512, guided" % grid.T: mk(latent_guidance=guidance.AttnGuidance(unet, **gkw))}

    def run(name, s):
        if name.startswith("sample_canvas"):
            s.sample_canvas(S=a.ddim_steps, canvas=(grid.Hc, grid.Wc), window=grid.s, stride=grid.stride, conditionings=[c],
                            unconditional_conditionings=uc, bboxs=[centres], object_names=[names], local_conditionings=[local],
                            curr_texts=[prompt], x_T=x_canvas, unconditional_guidance_scale=7.5, seed=1)
        else:
            s.sample_batch(S=a.ddim_steps, shape=[4, S_WIN, S_WIN], conditionings=[c] * grid.T, unconditional_conditionings=uc,
                           bboxs=canvas.window_centres(centres, grid), object_names=[names] * grid.T, local_conditionings=[local] * grid.T,
                           curr_texts=[prompt] * grid.T, x_T=x_batch, unconditional_guidance_scale=7.5, seed=1)
        torch.cuda.synchronize()

    times = {n: [] for n in samplers}
    for rep in range(1 + a.reps):                 # first round: warm-up (graph capture, packed weights, library algorithm choice)
        for name, s in samplers.items():          # alternating: every variant sees the same clocks
            t0 = time.perf_counter()
            run(name, s)
            if rep:
                times[name].append(time.perf_counter() - t0)
    rows = []
    base = statistics.median(times["sample_canvas, unguided"])
    for name, t in times.items():
        med, res = statistics.median(t), samplers[name].last_guidance
        n = 0 if res is None else len(res["calls"])
        rec = {"sampler_leg": name, "ddim_steps": a.ddim_steps, "guided_calls": n, "runs": len(t), "s_median": round(med, 4),
               "s_min": round(min(t), 4), "s_max": round(max(t), 4), "ordinary_call_ms": round(1e3 * base / a.ddim_steps, 2),
               "evaluation_ms": round(1e3 * (med - base) / n, 2) if n else None,
               "evaluation_in_ordinary_calls": round((med - base) / n / (base / a.ddim_steps), 3) if n else None,
               "E_first": round(res["energy"][0].mean().item(), 5) if n else None, "E_last": round(res["energy"][-1].mean().item(), 5) if n else None,
               "contributing_windows": None if getattr(samplers[name].canvas_guidance, "contributing", None) is None
               else int(samplers[name].canvas_guidance.contributing.sum()), "skipped": res["skipped"] if n else None}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


launch = [r for name, grid in GRIDS.items() for r in launch_leg(name, grid)]
samp = [] if a.no_sampler else sampler_leg()

md = ["# Attention guidance on a canvas: what `sta_latent_guide_windows` and a guidance evaluation cost", "",
      "Written by `python tools/canvas_guidance_bench.py` on one MI355X (%s); the tables below are from that one run." % torch.cuda.get_device_name(0),
      "One 512 x 2048 canvas (latent 64 x 256), windows of 512 px, stride 256 px, fp16, K = 2.", "",
      "## The update launch against the sequence it replaces", "",
      "HIP events around each form, the two alternating in one process, %d issues after %d warm-ups. The launch reads the window pairs' gradient," % (a.launches, a.warmup),
      "forms the split's adjoint (a sum over the covering windows), reduces the canvas's rms in every workgroup of the canvas, updates the state and",
      "writes the next window inputs. The unfused form is a handful of small torch kernels per window for the gather, `sta_latent_guide` and `sta_window_split`; it rounds",
      "the summed gradient to 16 bits on the way, so the two agree to that rounding (last column), not bit for bit. Every event-timed launch sits on",
      "a floor of several µs: the ratio of the launch to the sequence is a count of launches as much as of bytes.", "",
      "| grid | form | median µs (min … max) | max difference of the update / largest update |", "|---|---|---|---|"]
for r in launch:
    md.append("| %s | `%s` | %.2f (%.2f … %.2f) | %.5f |" % (r["grid"], r["form"], r["us_median"], r["us_min"], r["us_max"], r["max_dx_difference_over_max_dx"]))
md += ["", "Launch / sequence, median time: " + ", ".join("%s: %.2f x" % (f["grid"], f["us_median"] / u["us_median"]) for f, u in zip(launch[0::2], launch[1::2])) + ".",
       "", "## DDIM on the canvas with guided calls", ""]
if samp:
    md += ["Full-width SD-v1 UNet, synthetic weights, NHWC trunk, no VAE, DDIM with %d calls, the first %d of them guided (one update each, readouts at" % (a.ddim_steps, a.guided),
           "16 x 16 on the encoder side, eta = 0.1). Host clock around each trajectory ending in a device synchronise, %d timed trajectories per variant" % a.reps,
           "after one warm-up round, variants alternating; ordinary calls are graph-replayed, evaluations eager. One ordinary canvas call = unguided /",
           "calls; one evaluation = (guided - unguided `sample_canvas`) / guided calls: the eager forward of the 2 T window rows to the last recording",
           "block, the backward to the window pairs and the update launch. `sample_batch` of T 512 x 512 images runs the same UNet batch per call and",
           "is guided by `AttnGuidance` (every image moves by the step; on the canvas only the part under a contributing window does).", "",
           "| variant | median s (min … max) | ordinary canvas call ms | evaluation ms | evaluation / ordinary call | E before first / last update | contributing windows | skipped |",
           "|---|---|---|---|---|---|---|---|"]
    for r in samp:
        md.append("| %s | %.3f (%.3f … %.3f) | %.2f | %s | %s | %s | %s | %s |"
                  % (r["sampler_leg"], r["s_median"], r["s_min"], r["s_max"], r["ordinary_call_ms"],
                     "–" if r["evaluation_ms"] is None else "%.2f" % r["evaluation_ms"],
                     "–" if r["evaluation_in_ordinary_calls"] is None else "%.2f" % r["evaluation_in_ordinary_calls"],
                     "–" if r["E_first"] is None else "%.4f / %.4f" % (r["E_first"], r["E_last"]),
                     "–" if r["contributing_windows"] is None else r["contributing_windows"], "–" if r["skipped"] is None else r["skipped"]))
    md += ["", "The energies are those of synthetic weights: they say that the update runs and moves the energy, nothing about pictures."]
else:
    md.append("Not measured in this run (`--no-sampler`).")
md.append("")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(md))
print("wrote", a.out)
