"""clip_loss_bench.py — what the built-in CLIP fidelity loss costs on an MI355X (results: profiles/clip_loss.md).

  views  the view construction, forward + backward to the image: sta_clip_views / sta_clip_views_bwd against
         sta.clip.views_reference under autograd on the GPU (upsample x7 + average pool, slice + bilinear resize: what
         DCLIPLoss.forward_2 / forward_3 do), time and peak memory;
  loss   the whole loss, forward + backward to the image: DCLIPLoss.forward_batch against the view-by-view
         PLMSSampler._fidelity_loss loop with the same ClipViTB32 (synthetic weights, 16 bit);
  step   one BASELINE configs[2]-shaped step (16 prompts, 3 epochs, 50 PLMS steps, K = 2; bench.py's weight-optimisation leg is
         the template) with sta.clip.synthetic as the loss model, batched and view by view, and the share of the step the two
         tracked epochs' losses take.
Shapes: 16 images x (1 + 2) views at 512^2 and 4 x (1 + 4) at 768^2. Times are device-synchronised host clocks over `--iters`
iterations after `--warmup`, the two variants alternating; one JSON line per measurement. Needs a GPU: there is no CPU timing.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "diffusion-spacetime-attn_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)
for _k in ("FWD", "BWD", "WRW"):
    os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + _k, "0")

import torch  # noqa: E402

SHAPES = [(16, 2, 512), (4, 4, 768)]          # images, objects, side


def scene(b, K, side, dev):
    from ldm.models.diffusion.plms import object_crop_box
    from sta.pipeline import DEFAULT_CENTRES
    centres = ([list(c) for c in DEFAULT_CENTRES] + [[0.5, 0.5], [0.25, 0.75]])[:K]
    img = torch.rand(b, 3, side, side, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    boxes = []
    for i in range(b):
        boxes.append((i, 0, side, 0, side))
        boxes += [(i,) + tuple(object_crop_box(c, side, side)) for c in centres]
    return img, boxes, centres


def timed(fns, warmup, iters):
    """fns: {name: callable}. Alternates them; -> {name: (ms per call, peak MiB of one call above what was allocated before)}."""
    out = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        out[name] = [0.0, (torch.cuda.max_memory_allocated() - base) / 2 ** 20]
    for _ in range(iters):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[name][0] += 1e3 * (time.perf_counter() - t0) / iters
    return out


def emit(rec, sink):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def part_views(a, dev, sink):
    from sta import clip
    for b, K, side in SHAPES:
        img, boxes, _ = scene(b, K, side, dev)
        dout = torch.randn(len(boxes), 49, 3072, device=dev).to(torch.float16)

        def kernel():
            x = img.clone().requires_grad_(True)
            clip.clip_views(x, boxes, torch.float16).backward(dout)
            return x.grad

        def reference():
            x = img.clone().requires_grad_(True)
            clip.views_reference(x, boxes, torch.float16).backward(dout)
            return x.grad

        g, r = kernel(), reference()
        err = float((g - r).abs().max() / r.abs().max())
        t = timed({"kernel": kernel, "reference": reference}, a.warmup, a.iters)
        mb = (b * 3 * side * side * 4 * 2 + len(boxes) * 49 * 3072 * 2 * 2) / 1e6      # image read + gradient written, rows written + read
        emit({"part": "views", "images": b, "objects": K, "side": side, "views": len(boxes), "kernel_ms": round(t["kernel"][0], 4),
              "reference_ms": round(t["reference"][0], 4), "speedup": round(t["reference"][0] / t["kernel"][0], 1),
              "kernel_peak_mib": round(t["kernel"][1], 1), "reference_peak_mib": round(t["reference"][1], 1), "algorithmic_mb": round(mb, 1),
              "grad_rel_diff": err, "note": "forward + backward incl. the clone of the image and autograd's bookkeeping, fp16 rows"}, sink)


def _loss_fns(lm, img, texts, centres, names):
    from ldm.models.diffusion.plms import PLMSSampler
    sampler = object.__new__(PLMSSampler)
    sampler.clip_loss_model, sampler.local_loss_weight = lm, 5.0
    b = img.shape[0]

    def batched():
        x = img.clone().requires_grad_(True)
        loss = lm.forward_batch(x, texts, [centres] * b, names, 5.0)
        loss.backward()
        return loss.detach(), x.grad

    def view_by_view():
        x = img.clone().requires_grad_(True)
        loss = sum(sampler._fidelity_loss(x[i], texts[i], centres, names[i]) for i in range(b))
        loss.backward()
        return loss.detach(), x.grad

    return batched, view_by_view


def part_loss(a, dev, sink):
    from ldm.models.diffusion.plms import DCLIPLoss
    from sta import clip
    lm = DCLIPLoss(clip.synthetic(dev, dtype=torch.float16))
    out = {}
    for b, K, side in SHAPES:
        if side != 512:
            # the view-by-view path pools the global view by a fixed 16 (a 336^2 image at 768^2, which no ViT-B/32 takes): only the
            # batched loss exists above 512^2
            img, boxes, centres = scene(b, K, side, dev)
            texts, names = ["prompt %d" % i for i in range(b)], [["object %d" % k for k in range(K)]] * b
            batched, _ = _loss_fns(lm, img, texts, centres, names)
            t = timed({"batched": batched}, a.warmup, a.iters)
            emit({"part": "loss", "images": b, "objects": K, "side": side, "batched_ms": round(t["batched"][0], 3),
                  "batched_peak_mib": round(t["batched"][1], 1), "view_by_view_ms": None,
                  "note": "view-by-view: not runnable at this size (forward_2 hands CLIP a 336^2 image)"}, sink)
            continue
        img, boxes, centres = scene(b, K, side, dev)
        texts, names = ["prompt %d" % i for i in range(b)], [["object %d" % k for k in range(K)]] * b
        batched, view_by_view = _loss_fns(lm, img, texts, centres, names)
        (la, ga), (lb, gb) = batched(), view_by_view()
        t = timed({"batched": batched, "view_by_view": view_by_view}, a.warmup, a.iters)
        out[(b, K, side)] = t["batched"][0], t["view_by_view"][0]
        emit({"part": "loss", "images": b, "objects": K, "side": side, "batched_ms": round(t["batched"][0], 3),
              "view_by_view_ms": round(t["view_by_view"][0], 3), "speedup": round(t["view_by_view"][0] / t["batched"][0], 2),
              "batched_peak_mib": round(t["batched"][1], 1), "view_by_view_peak_mib": round(t["view_by_view"][1], 1),
              "loss_batched": float(la), "loss_view_by_view": float(lb), "grad_rel_diff": float((ga - gb).abs().max() / gb.abs().max()),
              "note": "ClipViTB32 synthetic weights fp16; forward + backward to the image; the batched loss caches text features, the view-by-view path encodes the text on every call (as the parent commit does)"}, sink)
    return out


def part_step(a, dev, sink, loss_ms):
    from ldm.models.diffusion.plms import DCLIPLoss, PLMSSampler
    from sta import clip
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts, set_recompute, use_shipped_miopen_db
    from sta.synth import calibrate_decoder_
    images, K, res, S = 16, 2, 512, 50
    dt = torch.float16
    use_shipped_miopen_db(0)
    say = lambda what: print("[step %7.1f s] %s" % (time.perf_counter() - t_start, what), flush=True)
    t_start = time.perf_counter()
    model = build_sd_v1(dev, dt, with_vae=True, init_weights=True, seed=0, channels_last=False, use_checkpoint=True)
    mode = set_recompute(model, "auto", images)
    lm = DCLIPLoss(clip.synthetic(dev, dtype=dt))
    prompts = load_prompts(64)
    lat = res // 8
    centres = [list(c) for c in DEFAULT_CENTRES[:K]]
    x_T1 = torch.randn([1, 4, lat, lat], generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    pre = PLMSSampler(model, opt_epochs=0, use_graph=False, save_images=False)
    rec = prompts[0]
    nm = (rec["objects"] + ["object"] * K)[:K]
    uc0, c0, l0 = conditionings(model, rec["prompt"], nm, dt)
    pre.sample(S=S, conditioning=c0, batch_size=1, shape=[4, lat, lat], verbose=False, unconditional_guidance_scale=7.5,
               unconditional_conditioning=uc0, eta=0.0, x_T=x_T1, text_index=0, curr_text=rec["prompt"], bboxs_curr=centres, seed=1,
               prompt_idx=0, object_names=nm, local_conditionings=l0)
    calibrate_decoder_(model, pre.last_result["x0"])
    del pre
    say("model built, decoder calibrated")
    samplers = {"batched": PLMSSampler(model, opt_epochs=3, loss_model=lm, use_graph=True, save_images=False, batched_loss=True),
                "view_by_view": PLMSSampler(model, opt_epochs=3, loss_model=lm, use_graph=True, save_images=False, batched_loss=False)}

    def step(sampler, j):
        recs = [prompts[(j * images + i) % len(prompts)] for i in range(images)]
        names = [(r["objects"] + ["object"] * K)[:K] for r in recs]
        conds = [conditionings(model, r["prompt"], n, dt) for r, n in zip(recs, names)]
        sampler.sample_batch(S=S, shape=[4, lat, lat], conditionings=[c[1] for c in conds], unconditional_conditionings=[c[0] for c in conds],
                             bboxs=[centres] * images, object_names=names, local_conditionings=[c[2] for c in conds],
                             curr_texts=[r["prompt"] for r in recs], x_T=x_T1.expand(images, -1, -1, -1), unconditional_guidance_scale=7.5, seed=1)
        return sampler.last_result

    step(samplers["batched"], 0)                       # warm-up: solver search, graph capture, activation sizing
    say("warm-up step done")
    res_ms = {k: 0.0 for k in samplers}
    losses = {}
    for j in range(a.steps):
        for name, sampler in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = step(sampler, 1 + j)
            torch.cuda.synchronize()
            res_ms[name] += 1e3 * (time.perf_counter() - t0) / a.steps
            losses[name] = r.get("losses")
            say("%s step %d done" % (name, j))
            assert torch.isfinite(r["x0"]).all() and float((r["W"] - 2.5).abs().max()) > 0
    rec = {"part": "step", "images_per_step": images, "opt_epochs": 3, "ddim_steps": S, "objects": K, "recompute": mode, "dtype": "fp16",
           "loss_model": "sta.clip.synthetic (ViT-B/32 shape)", "timed_steps": a.steps}
    for name in samplers:
        rec[name + "_ms_per_step"] = round(res_ms[name], 1)
        rec[name + "_images_per_s"] = round(images * 1e3 / res_ms[name], 3)
        rec[name + "_losses"] = losses[name]
        if loss_ms:
            rec[name + "_loss_share"] = round(2 * loss_ms[0 if name == "batched" else 1] / res_ms[name], 4)     # two tracked epochs
    emit(rec, sink)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["views", "loss", "step", "all"], default="all")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=1, help="timed configs[2] steps per variant (part step)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_loss_bench.py measures on the GPU; none is visible (there is no CPU timing)")
    dev = torch.device("cuda", 0)
    sink = open(a.out, "a") if a.out else None
    loss_ms = None
    if a.part in ("views", "all"):
        part_views(a, dev, sink)
    if a.part in ("loss", "step", "all"):
        got = part_loss(a, dev, sink)
        loss_ms = got.get((16, 2, 512))
    if a.part in ("step", "all"):
        part_step(a, dev, sink, loss_ms)


if __name__ == "__main__":
    main()
