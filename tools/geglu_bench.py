"""sta_geglu at the FF shapes of the default bench (32 prompts: rows = 64 * N): time, HBM-side GB/s and max error vs fp64.

--C 640: the level-1 GEGLU projection A/B instead — the one pass of csrc/sta_ffgemm.hip (the C = 640 instance) against the pair it replaces
(F.linear + fused.geglu) at R rows (default 131072: the five level-1 blocks of the bench), both 16-bit types, the two variants
alternating launch by launch in one process, one HIP event pair per launch, 20 launches after 3 warm-ups. Every input comes from
HBM: a launch moves > 1 GB, far beyond what the caches keep from the previous one."""
import argparse
import json
import statistics
import sys
import os
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))
from sta import fused, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--C", type=int, default=0, choices=(0, 640))
ap.add_argument("--rows", type=int, default=131072)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()


def level1_ab():
    C, inner, R = 640, 2560, args.rows
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator(device="cuda").manual_seed(1)
        y = torch.randn(R, C, device="cuda", generator=g).to(dtype)
        w = (torch.randn(2 * inner, C, device="cuda", generator=g) / C ** 0.5).to(dtype)
        b = (torch.randn(2 * inner, device="cuda", generator=g) * 0.3).to(dtype)
        yq, wp = ops.to_qfrag(y), fused.pack_geglu_c640_weight(w)
        variants = {"pair": lambda: fused.geglu(torch.nn.functional.linear(y, w, b)),
                    "fused": lambda: fused.ff_geglu_c640_qfrag(yq, wp, b, inner)}
        times = {k: [] for k in variants}
        for i in range(args.warmup + args.launches):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
                del out
        h, h2 = variants["fused"](), variants["pair"]()
        proj = y[:4096].double() @ w.double().t() + b.double()
        ref = proj[:, :inner] * torch.nn.functional.gelu(proj[:, inner:])
        eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
        rec = {"C": C, "inner": inner, "R": R, "dtype": str(dtype).split(".")[-1], "launches": args.launches}
        for name, t in times.items():
            rec[name + "_us"] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
        rec["fused_pflops"] = round(2.0 * R * C * 2 * inner / statistics.median(times["fused"]) / 1e9, 3)
        rec["fused_max_below_pair_min"] = max(times["fused"]) < min(times["pair"])
        rec["fused_err_over_eps"] = float(((h[:4096].double() - ref).abs() / (eps * (1 + ref.abs()))).max())
        rec["pair_err_over_eps"] = float(((h2[:4096].double() - ref).abs() / (eps * (1 + ref.abs()))).max())
        print(json.dumps(rec), flush=True)
        del y, yq, h, h2


if args.C == 640:
    level1_ab()
    sys.exit(0)

for R, D in ((64 * 4096, 1280), (64 * 1024, 2560), (64 * 256, 5120)):
    h = (torch.randn(R, 2 * D, device="cuda") * 2).half()
    y = fused.geglu(h)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fused.geglu(h)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 20
    a, g = h[:4096].double().chunk(2, dim=-1)
    ref = a * torch.nn.functional.gelu(g)
    err = (y[:4096].double() - ref).abs()
    print(json.dumps({"R": R, "D": D, "us": round(us, 1), "GBps": round(R * D * 6 / us / 1e3, 1), "max_err_over_tol": float((err / (2.0 ** -11 * (1 + ref.abs()))).max())}))
