"""sta_ln_qkv alone at the bench shape (level 0, 128 CFG rows x 4096 tokens = 524 288 rows, C = 320) against what it replaces —
sta_add_layernorm + the two library GEMMs (F.linear against [Wq'; Wk], torch.mm(Wv, y^T)) — in one process, alternating, HIP events
around every launch group: python tools/ln_qkv_bench.py [--rows R] [--dtype fp16|bf16] [--launches 20]
Prints one JSON line per variant: median / min / max us, GB/s over the algorithmic 1.34 GB and TFLOP/s over 322 GFLOP (scaled with R)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))
from sta import fused  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=128 * 4096)
ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
R, C = a.rows, 320
dev = torch.device("cuda", 0)
x = (torch.randn(R, C, device=dev) * 1.5 + 0.3).to(dt)
gamma, beta = (1 + 0.1 * torch.randn(C, device=dev)).to(dt), (0.1 * torch.randn(C, device=dev)).to(dt)
wqk, wv = (torch.randn(2 * C, C, device=dev) / C ** 0.5).to(dt), (torch.randn(C, C, device=dev) / C ** 0.5).to(dt)
packed = fused.pack_ln_qkv_weight(wqk, wv)


def parent():
    _, y = fused.add_layernorm(x, None, None, gamma, beta, 1e-5, store_sum=False)
    return F.linear(y, wqk), torch.mm(wv, y.t())


def ours():
    return fused.ln_qkv(x, None, gamma, beta, 1e-5, packed, store_sum=False)[1:]


variants = {"add_layernorm + 2 library GEMMs": parent, "sta_ln_qkv": ours}
times = {k: [] for k in variants}
for i in range(a.warmup + a.launches):
    for name, fn in variants.items():             # alternating: both see the same clocks and cache state
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        if i >= a.warmup:
            times[name].append(e0.elapsed_time(e1) * 1e3)
gbytes = R * C * 2 * 4 / 1e9                      # x in, q|k and V^T out
gflop = 2.0 * R * C * 3 * C / 1e9
for name, t in times.items():
    med = statistics.median(t)
    print(json.dumps({"variant": name, "rows": R, "dtype": a.dtype, "launches": len(t), "us_median": round(med, 1), "us_min": round(min(t), 1),
                      "us_max": round(max(t), 1), "GBps_algorithmic": round(gbytes / med * 1e6, 1), "TFLOPs": round(gflop / med * 1e3, 1)}))
