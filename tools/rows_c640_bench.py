"""sta_rows_c640 (csrc/sta_rows640.hip) against the routes it replaces, at R rows (default 131072: the five level-1 blocks of the bench):

  to_out   K = 640:  F.linear + fused.add_layernorm(qfrag=True)   vs   fused.rows_c640 with the LayerNorm, y in query-fragment order
  ff_out   K = 2560: F.linear + the elementwise add                vs   fused.rows_c640 without

Both 16-bit types, the two variants of a site alternating launch by launch in one process, one HIP event pair per launch (the pair:
around its two launches), 20 launches after 3 warm-ups. Every input comes from HBM: a launch moves 0.7 - 1.2 GB, beyond what the
caches keep from the previous one. One JSON line per (site, dtype)."""
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
ap.add_argument("--rows", type=int, default=131072)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
C, R = 640, args.rows

for site, K in (("to_out", 640), ("ff_out", 2560)):
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator(device="cuda").manual_seed(1)
        a = torch.randn(R, K, device="cuda", generator=g).to(dtype)
        x = torch.randn(R, C, device="cuda", generator=g).to(dtype)
        w = (torch.randn(C, K, device="cuda", generator=g) / K ** 0.5).to(dtype)
        b = (torch.randn(C, device="cuda", generator=g) * 0.3).to(dtype)
        lw = (1.0 + 0.2 * torch.randn(C, device="cuda", generator=g)).to(dtype)
        lb = (0.2 * torch.randn(C, device="cuda", generator=g)).to(dtype)
        wp = fused.pack_rows_c640_weight(w)
        if K == 640:
            variants = {"pair": lambda: fused.add_layernorm(x, F.linear(a, w, b), None, lw, lb, 1e-5, qfrag=True),
                        "fused": lambda: fused.rows_c640(x, a, wp, b, lw, lb, 1e-5, y_qfrag=True)}
        else:
            variants = {"pair": lambda: (F.linear(a, w, b) + x, None),
                        "fused": lambda: fused.rows_c640(x, a, wp, b)}
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
        s1, s2 = variants["fused"]()[0], variants["pair"]()[0]
        ref = x[:4096].double() + a[:4096].double() @ w.double().t() + b.double()
        eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
        rec = {"site": site, "K": K, "R": R, "dtype": str(dtype).split(".")[-1], "launches": args.launches}
        for name, t in times.items():
            rec[name + "_us"] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
        med = statistics.median(times["fused"])
        nbytes = R * 2 * (K + C * (3 if K == 640 else 2))
        rec["fused_tbps"] = round(nbytes / med / 1e6, 3)
        rec["fused_pflops"] = round(2.0 * R * C * K / med / 1e9, 3)
        spread = max(max(t) - min(t) for t in times.values())
        rec["median_gain_us"] = round(statistics.median(times["pair"]) - med, 1)
        rec["gain_exceeds_spreads"] = statistics.median(times["pair"]) - med > spread
        rec["fused_max_below_pair_min"] = max(times["fused"]) < min(times["pair"])
        rec["fused_err_over_eps"] = float(((s1[:4096].double() - ref).abs() / (eps * (1 + ref.abs()))).max())
        rec["pair_err_over_eps"] = float(((s2[:4096].double() - ref).abs() / (eps * (1 + ref.abs()))).max())
        print(json.dumps(rec), flush=True)
        del a, x, s1, s2
