"""Images/s of the samplers at the bench workload: 512x512, K = 2, 64 prompts per step, fixed blend weights, synthetic weights.

Imports bench.py (environment, sys.path) and builds the model, prompts and centres as its main() does, then times one step of
64 prompts per sampler and 16-bit type: PLMS-50 (bench's default workload), DPM-Solver++(2M) at 20 and 25 steps, DDIM-50.
Also reports the UNet calls per image, the device time of the per-call sampler step (sta_sampler_step, HIP events around each
launch: the time outside the graph replay that the step costs), and a BASELINE configs[2]-shaped weight-optimisation line
(3 epochs, synthetic CLIP loss) for DPM-Solver++ at 20 steps. Prints one JSON line.

    python tools/sampler_throughput.py [--images 64] [--steps 1] [--warmup 1] [--dtypes fp16,bf16] [--only dpm20] [--no-graph]
The profile under profiles/ : rocprofv3 --kernel-trace --stats -- python tools/sampler_throughput.py --only dpm20 --dtypes fp16
    --images 16 --wopt-images 0 --no-graph   (rocprofv3 faults inside hipGraphLaunch: profiles/README.md)
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

LEGS = {"plms50": ("PLMSSampler", 50), "dpm20": ("DPMSolverSampler", 20), "dpm25": ("DPMSolverSampler", 25), "ddim50": ("DDIMSampler", 50)}
CALLS = {"PLMSSampler": lambda S: S + 1, "DPMSolverSampler": lambda S: S, "DDIMSampler": lambda S: S}


def sampler_cls(name):
    if name == "DPMSolverSampler":
        from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
        return DPMSolverSampler
    if name == "DDIMSampler":
        from ldm.models.diffusion.ddim import DDIMSampler
        return DDIMSampler
    from ldm.models.diffusion.plms import PLMSSampler
    return PLMSSampler


class StepTimer:
    """HIP events around every sta.solver.solver_step call (the sampler step of DPM-Solver++ / DDIM)."""

    def __init__(self):
        from sta import solver
        self.solver, self.inner, self.pairs = solver, solver.solver_step, []

    def __enter__(self):
        def timed(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = self.inner(*a, **k)
            e.record()
            self.pairs.append((s, e))
            return out
        self.solver.solver_step = timed
        return self

    def __exit__(self, *exc):
        self.solver.solver_step = self.inner

    def ms_per_call(self):
        torch.cuda.synchronize()
        return sum(s.elapsed_time(e) for s, e in self.pairs) / max(len(self.pairs), 1)


def run_dtype(dtype_name, legs, I, steps, warmup, K=2, res=512, graph=True):
    from sta import lib
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts, use_shipped_miopen_db
    dev = torch.device("cuda", 0)
    lib.load()
    use_shipped_miopen_db(0)
    dt = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    model = build_sd_v1(dev, dt, with_vae=True, init_weights=True, seed=0, channels_last=True)
    prompts = load_prompts(64)
    lat, centres = res // 8, [list(c) for c in DEFAULT_CENTRES[:K]]
    x_T1 = torch.randn([1, 4, lat, lat], generator=torch.Generator(device=dev).manual_seed(1), device=dev)

    def one_step(sampler, S, j, n):
        recs = [prompts[(j * n + i) % len(prompts)] for i in range(n)]
        names = [(r["objects"] + ["object"] * K)[:K] for r in recs]
        conds = [conditionings(model, r["prompt"], nm, dt) for r, nm in zip(recs, names)]
        sampler.sample_batch(S=S, shape=[4, lat, lat], conditionings=[c[1] for c in conds], unconditional_conditionings=[c[0] for c in conds],
                             bboxs=[centres] * n, object_names=names, local_conditionings=[c[2] for c in conds],
                             curr_texts=[r["prompt"] for r in recs], x_T=x_T1.expand(n, -1, -1, -1), unconditional_guidance_scale=7.5, seed=1)

    out = {}
    for leg in legs:
        name, S = LEGS[leg]
        sampler = sampler_cls(name)(model, opt_epochs=0, use_graph=graph, save_images=False)
        for j in range(warmup):
            one_step(sampler, S, j, I)
        torch.cuda.synchronize()
        with StepTimer() as tm:
            t0 = time.perf_counter()
            for j in range(steps):
                one_step(sampler, S, warmup + j, I)
            torch.cuda.synchronize()
            dt_s = time.perf_counter() - t0
        out[leg] = {"images_per_s": round(I * steps / dt_s, 3), "s_per_step": round(dt_s / steps, 3), "unet_calls_per_image": CALLS[name](S),
                    "sampler_step_ms_per_call": round(tm.ms_per_call(), 4) if tm.pairs else None}
        print("[%s %s] %s" % (dtype_name, leg, out[leg]), file=sys.stderr, flush=True)
        del sampler
    return out, model, one_step


def wopt_line(model, one_step, images, epochs=3):
    """BASELINE configs[2] shape (3 epochs: 2 tracked trajectories + 1, synthetic CLIP loss) with DPM-Solver++ at 20 steps."""
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.models.diffusion.plms import DCLIPLoss
    from sta.pipeline import set_recompute
    from sta.synth import SyntheticCLIP
    mode = set_recompute(model, "auto", images)
    sampler = DPMSolverSampler(model, opt_epochs=epochs, loss_model=DCLIPLoss(SyntheticCLIP().to("cuda")), use_graph=True, save_images=False)
    one_step(sampler, 20, 0, images)             # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one_step(sampler, 20, 1, images)
    torch.cuda.synchronize()
    dt_s = time.perf_counter() - t0
    return {"images_per_s": round(images / dt_s, 3), "s_per_step": round(dt_s, 3), "images_per_step": images, "epochs": epochs,
            "recompute": mode, "unet_calls_per_image": 20 * epochs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--only", default=",".join(LEGS))
    ap.add_argument("--wopt-images", type=int, default=8, help="prompts per step of the weight-optimisation line (0 = skip)")
    ap.add_argument("--no-graph", action="store_true", help="issue the UNet calls eagerly (for rocprofv3, which faults inside hipGraphLaunch)")
    a = ap.parse_args()
    legs = [x for x in a.only.split(",") if x]
    res = {"workload": "512x512, K=2, %d prompts per step, fixed weights, synthetic weights, %s" % (a.images, "eager" if a.no_graph else "hipGraph"),
           "steps": a.steps,
           "warmup": a.warmup}
    for dn in a.dtypes.split(","):
        r, model, one_step = run_dtype(dn, legs, a.images, a.steps, a.warmup, graph=not a.no_graph)
        if "plms50" in r:
            for k in r:
                r[k]["vs_plms50"] = round(r[k]["images_per_s"] / r["plms50"]["images_per_s"], 3)
        if a.wopt_images and dn == a.dtypes.split(",")[0]:
            r["wopt_dpm20"] = wopt_line(model, one_step, a.wopt_images)
        res[dn] = r
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
