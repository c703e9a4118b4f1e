"""What the attention-layout loss costs: python tools/attn_loss_bench.py [--out profiles/attn_loss.md] [--images 16] [--no-epoch]

1. sta_xattn_token_maps_bwd alone at the two shapes the loss records at — (16 images, K = 2, R = 4, N = 256, C = 1280: the default 16 x 16
   level) and (N = 4096, C = 320: level 0) — next to (a) the forward sta_xattn_token_maps launch and (b) sta_xattn_bwd of the same shape in
   the same process, in both 16-bit types. HIP events around every launch, the three alternating, medians over --launches after --warmup.
2. BASELINE configs[2] as bench.py's side leg runs it (full-width UNet, synthetic weights, VAE, 512 x 512, 50 PLMS steps, --images prompts
   per step, recomputation per UNet call): one tracked epoch + the kept trajectory (opt_epochs = 2) with the attention loss alone and with
   the CLIP stand-in, and the kept trajectory alone (opt_epochs = 0), alternating; a tracked epoch is the difference to the last.
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
from sta import attnloss, attnmaps, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_loss.md"))
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--ddim_steps", type=int, default=50)
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=2, help="timed sample_batch calls per variant")
ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16", help="type of the epoch leg (the kernel leg runs both)")
ap.add_argument("--no-epoch", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("attn_loss_bench needs a GPU")
dev = torch.device("cuda", 0)
K, R, M, heads = 2, 4, 77, 8
SEL = [1, 1, 2, 3]


def kernel_leg(I, N, C, dtype_name):
    dt = torch.float16 if dtype_name == "fp16" else torch.bfloat16
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
    dmaps = torch.randn(I, R, N, generator=g, device=dev)
    dq = torch.empty_like(q)
    dout = torch.randn(2 * I, N, C, generator=g, device=dev).to(dt)
    scale = (C // heads) ** -0.5
    variants = {"sta_xattn_token_maps_bwd": lambda: attnmaps.token_maps_backward(q, packed, SEL, w, dmaps, scale, out=dq),
                "sta_xattn_token_maps": lambda: attnmaps.token_maps(q, packed, SEL, w, scale, out=out),
                "sta_xattn_bwd": lambda: ops.xattn_backward(q, packed, mask, coef, dout, scale)}
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
    n_ctx = len(set(SEL))
    # what the algorithm needs per attended context: QK^T (+ dS K for the readout's backward; + dO V^T and dS K for the blend's backward)
    flop = {"sta_xattn_token_maps_bwd": 2.0 * I * heads * N * 80 * d * n_ctx * 2, "sta_xattn_token_maps": 2.0 * I * heads * N * 80 * d * n_ctx,
            "sta_xattn_bwd": 2.0 * I * heads * N * 80 * d * (K + 2) * 3}
    # bytes that must cross HBM at least once: q (+ dq, dout), the packed operands read, maps / dmaps
    el = 2 * I * N * C * 2
    rows = []
    for name, t in times.items():
        med = statistics.median(t)
        rec = {"kernel": name, "I": I, "N": N, "C": C, "K": K, "R": R, "dtype": dtype_name, "launches": len(t), "us_median": round(med, 1),
               "us_min": round(min(t), 1), "us_max": round(max(t), 1), "TFLOPs_algorithmic": round(flop[name] / med / 1e6, 1),
               "GBs_q_and_dq": round((2 * el if name != "sta_xattn_token_maps" else el) / med / 1e3, 1)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    return rows


def epoch_leg(I, dtype_name):
    from ldm.models.diffusion.plms import DCLIPLoss, PLMSSampler
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts, set_recompute, use_shipped_miopen_db
    from sta.synth import SyntheticCLIP, calibrate_decoder_
    dt = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    use_shipped_miopen_db(0)
    torch.backends.cudnn.benchmark = dtype_name == "fp16"          # the shipped find-db holds the fp16 shapes at 512 x 512 (bench.py)
    model = build_sd_v1(dev, dt, with_vae=True, init_weights=True, seed=0, channels_last=False, use_checkpoint=True)
    mode = set_recompute(model, "call", I)
    prompts = load_prompts(64)
    centres = [list(c) for c in DEFAULT_CENTRES[:K]]
    x_T1 = torch.randn([1, 4, 64, 64], generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    pre = PLMSSampler(model, opt_epochs=0, use_graph=False, save_images=False)
    rec0 = prompts[0]
    nm0 = (rec0["objects"] + ["object"] * K)[:K]
    uc0, c0, l0 = conditionings(model, rec0["prompt"], nm0, dt)
    pre.sample(S=a.ddim_steps, conditioning=c0, batch_size=1, shape=[4, 64, 64], verbose=False, unconditional_guidance_scale=7.5,
               unconditional_conditioning=uc0, eta=0.0, x_T=x_T1, text_index=0, curr_text=rec0["prompt"], bboxs_curr=centres, seed=1,
               prompt_idx=0, object_names=nm0, local_conditionings=l0)
    calibrate_decoder_(model, pre.last_result["x0"])                # as bench.py: the synthetic decoder must not saturate the image clamp
    del pre
    recs = [prompts[i % len(prompts)] for i in range(I)]
    names = [(r["objects"] + ["object"] * K)[:K] for r in recs]
    conds = [conditionings(model, r["prompt"], nm, dt) for r, nm in zip(recs, names)]
    loss = attnloss.AttnLayoutLoss(model.model.diffusion_model, resolution=16)
    attempts = [0]
    real_begin = loss.begin
    loss.begin = lambda *x, **k: (attempts.__setitem__(0, attempts[0] + 1), real_begin(*x, **k))[1]       # one per tracked attempt (loss-scale back-off re-runs)
    clip = DCLIPLoss(SyntheticCLIP().to(dev))
    samplers = {"kept trajectory alone (opt_epochs = 0)": PLMSSampler(model, opt_epochs=0, use_graph=True, save_images=False),
                "attention loss alone (opt_epochs = 2)": PLMSSampler(model, loss_model=None, attn_loss=loss, opt_epochs=2, use_graph=True, save_images=False),
                "CLIP stand-in (opt_epochs = 2)": PLMSSampler(model, loss_model=clip, opt_epochs=2, use_graph=True, save_images=False)}

    def run(s):
        s.sample_batch(S=a.ddim_steps, shape=[4, 64, 64], conditionings=[c[1] for c in conds], unconditional_conditionings=[c[0] for c in conds],
                       bboxs=[centres] * I, object_names=names, local_conditionings=[c[2] for c in conds], curr_texts=[r["prompt"] for r in recs],
                       x_T=x_T1.expand(I, -1, -1, -1), unconditional_guidance_scale=7.5, seed=1)
        torch.cuda.synchronize()
        return s.last_result

    times, last = {n: [] for n in samplers}, {}
    for rep in range(1 + a.reps):                 # first round: warm-up (graph capture, library algorithm choice, one measured kept call)
        for name, s in samplers.items():          # alternating: every variant sees the same clocks
            t0 = time.perf_counter()
            last[name] = run(s)
            if rep:
                times[name].append(time.perf_counter() - t0)
    rows = []
    for name, t in times.items():
        r = last[name]
        rec = {"epoch_leg": name, "images": I, "ddim_steps": a.ddim_steps, "dtype": dtype_name, "recompute": mode, "runs": len(t),
               "s_median": round(statistics.median(t), 3), "s_min": round(min(t), 3), "s_max": round(max(t), 3), "losses": r.get("losses"),
               "W_moved": float((r["W"] - 2.5).abs().max()), "kept_calls": getattr(samplers[name], "last_kept_calls", None)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    rows.append({"tracked_attempts_attention_loss": attempts[0], "sample_batch_calls": 1 + a.reps, "recording_blocks_calls_last_epoch": loss.block_calls})
    print(json.dumps(rows[-1]), flush=True)
    return rows


kern = []
for dtype_name in ("fp16", "bf16"):
    kern += kernel_leg(a.images, 256, 1280, dtype_name) + kernel_leg(a.images, 4096, 320, dtype_name)
ep = [] if a.no_epoch else epoch_leg(a.images, a.dtype)
md = ["# Attention-layout loss: what `sta_xattn_token_maps_bwd` and a tracked epoch with it cost", "",
      "Written by `python tools/attn_loss_bench.py` on one MI355X (%s); the tables below are from that one run." % torch.cuda.get_device_name(0), "",
      "## The backward launch, next to the forward readout and `sta_xattn_bwd` at the same shape", "",
      "HIP events around each launch, the three kernels alternating in one process, %d launches after %d warm-ups. K = 2, R = 4 readouts" % (a.launches, a.warmup),
      "(two on the global context, one per local context: three contexts attended, none on q row 0, whose half of dq the launch zero-fills),",
      "I = %d images. `sta_xattn_bwd` attends all four contexts and has the dO V^T product on top." % a.images, "",
      "| shape | type | kernel | median µs (min … max) | algorithmic TFLOP/s | GB/s on q (+ dq) alone |", "|---|---|---|---|---|---|"]
for r in kern:
    md.append("| N = %d, C = %d | %s | `%s` | %.1f (%.1f … %.1f) | %.1f | %.0f |" % (r["N"], r["C"], r["dtype"], r["kernel"], r["us_median"], r["us_min"], r["us_max"],
                                                                                   r["TFLOPs_algorithmic"], r["GBs_q_and_dq"]))
md += ["", "## A tracked epoch of BASELINE configs[2]: attention loss alone against the CLIP stand-in", ""]
if ep:
    md += ["Full-width SD-v1 UNet and VAE, synthetic weights, calibrated decoder, %d prompts per step, 512 x 512, %d PLMS steps, %s, recomputation per" % (a.images, a.ddim_steps, a.dtype),
           "UNet call; host clock around `sample_batch` ending in a device synchronise, %d timed calls per variant after one warm-up round, variants" % a.reps,
           "alternating. opt_epochs = 2 is one tracked epoch (forward, backward, Adam step) plus the kept trajectory and its decode; the first row is", "that kept trajectory alone.", "",
           "| variant | median s (min … max) | loss of the tracked epoch | max \\|W - W0\\| | kept calls |", "|---|---|---|---|---|"]
    base = None
    for r in ep:
        if "epoch_leg" in r:
            md.append("| %s | %.3f (%.3f … %.3f) | %s | %.4f | %s |" % (r["epoch_leg"], r["s_median"], r["s_min"], r["s_max"],
                                                                    "–" if not r["losses"] else "%.5f" % r["losses"][0], r["W_moved"], r["kept_calls"]))
            base = r["s_median"] if base is None else base
    tr = [r for r in ep if "epoch_leg" in r][1:]
    md += ["", "Tracked epoch = row - first row: " + ", ".join("%s %.3f s" % (r["epoch_leg"].split(" (")[0], r["s_median"] - base) for r in tr) + ".",
           "Tracked attempts with the attention loss: %d over %d `sample_batch` calls (more than one per call = the fp16 loss scale backed off and" % (ep[-1]["tracked_attempts_attention_loss"], ep[-1]["sample_batch_calls"]),
           "the epoch ran again)."]
else:
    md.append("Not measured in this run (`--no-epoch`).")
md.append("")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(md))
print("wrote", a.out)
