"""sta_ff_tail (csrc/sta_rowstail.hip) against the sequence it replaces, per site at the bench shape (128 rows of 64^2):

  level 0   C = 320, 524288 rows: fused.ff_out_res_hfrag + fused.linear_rows(res, stats) [+ its finalize]   vs   fused.ff_tail(stats)
  level 1   C = 640, 131072 rows: fused.rows_c640 (K = 2560) + fused.linear_rows(res, stats) [+ finalize]    vs   fused.ff_tail(stats)

Both 16-bit types, the two variants of a site alternating launch by launch in one process, one HIP event pair per launch (the
sequence: around all its launches), 20 launches after 3 warm-ups. Every input comes from HBM: a launch moves 1.3 - 2.4 GB, beyond
what the caches keep from the previous one. One JSON line per (site, dtype); `ships_on`: the criterion of profiles/rows_c640.md —
the new pass's median is lower by more than both variants' spreads (max - min)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))
from sta import fused, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=128, help="rows of the UNet call (CFG pairs x 2); level 0 has 4096 pixels each, level 1 1024")
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sites", default="320,640")
args = ap.parse_args()

for C in (int(c) for c in args.sites.split(",")):
    rows_img = 4096 if C == 320 else 1024
    R, inner = args.images * rows_img, 4 * C
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator(device="cuda").manual_seed(1)
        h = torch.randn(R, inner, device="cuda", generator=g).to(dtype)
        x2 = torch.randn(R, C, device="cuda", generator=g).to(dtype)
        x_in = torch.randn(R, C, device="cuda", generator=g).to(dtype)
        net2, proj = torch.nn.Linear(inner, C).to("cuda", dtype), torch.nn.Conv2d(C, C, 1).to("cuda", dtype)
        with torch.no_grad():
            net2.bias.mul_(30.0)
            proj.bias.mul_(30.0)
            w2, wp = net2.weight.detach(), proj.weight.detach().reshape(C, C)
            wt, bt = fused.ff_tail_weights(net2, proj)
            tail_img = fused.pack_ff_tail_weight(torch.cat([wt, wp], dim=1))
            bt = bt.float().contiguous()
            po_img = fused.pack_linear_weight(wp)
            if C == 320:
                hf = ops.to_qfrag(h)
                w2_img = fused.pack_ff_out_weight(w2)
                first = lambda: fused.ff_out_res_hfrag(x2, hf, w2_img, net2.bias)
            else:
                hf = h
                w2_img = fused.pack_rows_c640_weight(w2)
                first = lambda: fused.rows_c640(x2, h, w2_img, net2.bias)[0]
            variants = {"sequence": lambda: fused.linear_rows(first(), po_img, C, bias=proj.bias, res=x_in, stats_rows=rows_img),
                        "fused": lambda: fused.ff_tail(hf, x2, x_in, tail_img, bt, stats_rows=rows_img)}
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
            s1, s2 = variants["fused"](), variants["sequence"]()
            n = 4096
            x3 = x2[:n].double() + h[:n].double() @ w2.double().t() + net2.bias.double()
            ref = x_in[:n].double() + x3 @ wp.double().t() + proj.bias.double()
            S = h[:n].double().abs() @ wt.double().abs().t()
        eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
        rec = {"site": "level %d" % (0 if C == 320 else 1), "C": C, "R": R, "dtype": str(dtype).split(".")[-1], "launches": args.launches}
        for name, t in times.items():
            rec[name + "_us"] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
        med = statistics.median(times["fused"])
        rec["fused_tbps"] = round(R * 2 * (inner + 3 * C) / med / 1e6, 3)
        rec["fused_pflops"] = round(2.0 * R * C * (inner + C) / med / 1e9, 3)
        spread = max(max(t) - min(t) for t in times.values())
        rec["median_gain_us"] = round(statistics.median(times["sequence"]) - med, 1)
        rec["ships_on"] = statistics.median(times["sequence"]) - med > spread
        rec["fused_max_below_sequence_min"] = max(times["fused"]) < min(times["sequence"])
        rec["fused_err_over_bound"] = float(((s1[:n].double() - ref).abs() / (eps * (S + 2 * (1 + ref.abs())))).max())
        rec["sequence_err_over_eps"] = float(((s2[:n].double() - ref).abs() / (eps * (1 + ref.abs()))).max())
        print(json.dumps(rec), flush=True)
        del h, hf, x2, x_in, s1, s2
