"""Inpainting on one MI355X: images/s of a masked trajectory next to the unmasked one, same process, same workload.

Imports bench.py (environment, sys.path) like tools/sampler_throughput.py and builds its workload: 512x512, K = 2, 64 prompts per step,
synthetic weights. Two parts, one JSON document (printed, and written to --out):
  * fixed   fixed blend weights, DDIM-50 and DPM-Solver++(2M)-20: sample_batch without a mask against sample_batch with mask= / x0= /
            image= / mask_px= (sta_latent_blend once, sta_sampler_step_masked for S - 1 calls, sta_image_composite once per image batch;
            the blend noise drawn per call with torch.randn on the device), the two alternating for --rounds rounds after a warm-up of each;
            also the device time of the per-call step launch (HIP events around solver_step / solver_step_masked);
  * wopt    3 epochs (2 tracked trajectories + 1, synthetic CLIP loss, per-call recomputation as tools/sampler_throughput.py's wopt line)
            of DPM-Solver++-20 on --wopt-images prompts, masked against unmasked: the tracked epochs differentiate through
            SolverStepMaskedFn and the composite backward.
The mask keeps the left half of every image (a rectangle plus a soft column), so half of the latent is re-noised at every call.

    python tools/inpaint_throughput.py [--dtype fp16] [--images 64] [--rounds 2] [--wopt-images 8] [--out profiles/inpaint_throughput.json]
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

LEGS = {"ddim50": ("DDIMSampler", 50), "dpm20": ("DPMSolverSampler", 20)}


def sampler_cls(name):
    if name == "DPMSolverSampler":
        from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
        return DPMSolverSampler
    from ldm.models.diffusion.ddim import DDIMSampler
    return DDIMSampler


class StepTimer:
    """HIP events around every sta.solver.solver_step / solver_step_masked call."""

    def __init__(self):
        from sta import solver
        self.solver, self.inner, self.pairs = solver, (solver.solver_step, solver.solver_step_masked), []

    def _timed(self, fn):
        def timed(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            self.pairs.append((s, e))
            return out
        return timed

    def __enter__(self):
        self.solver.solver_step, self.solver.solver_step_masked = self._timed(self.inner[0]), self._timed(self.inner[1])
        return self

    def __exit__(self, *exc):
        self.solver.solver_step, self.solver.solver_step_masked = self.inner

    def ms_per_call(self):
        torch.cuda.synchronize()
        return sum(s.elapsed_time(e) for s, e in self.pairs) / max(len(self.pairs), 1)


def inpaint_inputs(n, lat, dev, seed=2):
    """Per-batch inpaint arguments: keep the left half (1), repaint the right half (0), one soft column between them."""
    g = torch.Generator(device=dev).manual_seed(seed)
    keep = torch.zeros(n, 1, lat, lat, device=dev)
    keep[..., : lat // 2] = 1.0
    keep[..., lat // 2] = 0.5
    keep_px = keep.repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)
    x0 = torch.randn(n, 4, lat, lat, device=dev, generator=g)
    image = torch.rand(n, 3, 8 * lat, 8 * lat, device=dev, generator=g)
    return dict(mask=keep, x0=x0, image=image, mask_px=keep_px)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", default=",".join(LEGS))
    ap.add_argument("--wopt-images", type=int, default=8, help="prompts per step of the 3-epoch line (0 = skip)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "inpaint_throughput.json"))
    a = ap.parse_args()
    from sta import lib
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts, use_shipped_miopen_db
    dev = torch.device("cuda", 0)
    lib.load()
    use_shipped_miopen_db(0)
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    K, lat = 2, 64
    model = build_sd_v1(dev, dt, with_vae=True, init_weights=True, seed=0, channels_last=True)
    prompts = load_prompts(64)
    centres = [list(c) for c in DEFAULT_CENTRES[:K]]
    x_T1 = torch.randn([1, 4, lat, lat], generator=torch.Generator(device=dev).manual_seed(1), device=dev)

    def one_step(sampler, S, n, inp):
        recs = [prompts[i % len(prompts)] for i in range(n)]
        names = [(r["objects"] + ["object"] * K)[:K] for r in recs]
        conds = [conditionings(model, r["prompt"], nm, dt) for r, nm in zip(recs, names)]
        sampler.sample_batch(S=S, shape=[4, lat, lat], conditionings=[c[1] for c in conds], unconditional_conditionings=[c[0] for c in conds],
                             bboxs=[centres] * n, object_names=names, local_conditionings=[c[2] for c in conds],
                             curr_texts=[r["prompt"] for r in recs], x_T=x_T1.expand(n, -1, -1, -1), unconditional_guidance_scale=7.5, seed=1,
                             **inp)

    def compare(make_sampler, S, n, rounds, what):
        inp = inpaint_inputs(n, lat, dev)
        sampler = make_sampler()
        for arg in ({}, inp):                              # warm-up of both: graph capture, first-use solver searches
            one_step(sampler, S, n, arg)
        times, step_ms = {"unmasked": [], "masked": []}, {}
        for _ in range(rounds):
            for name, arg in (("unmasked", {}), ("masked", inp)):
                torch.cuda.synchronize()
                with StepTimer() as tm:
                    t0 = time.perf_counter()
                    one_step(sampler, S, n, arg)
                    torch.cuda.synchronize()
                    times[name].append(time.perf_counter() - t0)
                step_ms[name] = round(tm.ms_per_call(), 4) if tm.pairs else None
                print("[%s] %s %.3f s" % (what, name, times[name][-1]), file=sys.stderr, flush=True)
        rec = {k: {"images_per_s": round(n / min(v), 3), "s_per_step": [round(x, 3) for x in v], "step_launch_ms_per_call": step_ms[k]}
               for k, v in times.items()}
        rec["masked_vs_unmasked"] = round(rec["masked"]["images_per_s"] / rec["unmasked"]["images_per_s"], 4)
        rec["images_per_step"], rec["unet_calls_per_image"] = n, S
        return rec

    res = {"workload": "512x512, K=2, %d prompts per step, synthetic weights, hipGraph, %s" % (a.images, a.dtype), "rounds": a.rounds,
           "mask": "left half kept, right half repainted, one soft column; x0, image random", "fixed": {}}
    for leg in [x for x in a.only.split(",") if x]:
        name, S = LEGS[leg]
        res["fixed"][leg] = compare(lambda: sampler_cls(name)(model, opt_epochs=0, use_graph=True, save_images=False), S, a.images, a.rounds, leg)
    if a.wopt_images:
        from ldm.models.diffusion.plms import DCLIPLoss
        from sta.pipeline import set_recompute
        from sta.synth import SyntheticCLIP
        mode = set_recompute(model, "auto", a.wopt_images)
        loss = DCLIPLoss(SyntheticCLIP().to("cuda"))
        rec = compare(lambda: sampler_cls("DPMSolverSampler")(model, opt_epochs=3, loss_model=loss, use_graph=True, save_images=False), 20,
                      a.wopt_images, 1, "wopt_dpm20")
        rec.update(epochs=3, recompute=mode, unet_calls_per_image=60)
        res["wopt_dpm20"] = rec
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
