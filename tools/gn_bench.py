"""The NHWC GroupNorm (+ pre-add) (+ SiLU) pass of csrc/sta_unet.hip alone, at every GroupNorm shape of a bench UNet call (batch 128,
64 x 64 latents) and at the VAE decoder's shapes (64 images), called through the C entry points.

  python tools/gn_bench.py                                   this tree's library
  python tools/gn_bench.py --lib A.so --lib B.so             several libraries (e.g. the parent commit's, built in its own checkout
                                                             under build/), alternating launch by launch in one process

A shape is (C, HW, Ca of a concatenation or 0, pre-add or not, silu or not, `cstats` (one kernel, per-channel sums given) or `two`
(statistics kernel + apply kernel)). Per shape, dtype and library: median, minimum and maximum of --launches launches after --warmup
warm-ups, one HIP event pair per launch, the bytes a launch has to move (x read once — twice on the two-kernel path — and y written)
and the TB/s of the median. Inputs come from HBM: the launches rotate over enough (x, y) sets that a set has left the 256 MiB
Infinity Cache before it is used again. The shapes of the 16 x 16 and 8 x 8 levels are timed a second time on ONE set, in cache
(`"where": "cache"`). With two libraries a line carries `faster`: the last library's median is lower than the first's by more than
both series' spreads (max - min); `slower`: higher by more than both.

The per-channel sums handed to `cstats` are those of the distribution the inputs are drawn from (sum 0, sum of squares HW), not of
the sample: the time of a launch does not depend on them. The tool reads nothing outside the repository. The driver process does
not touch the GPU: every (group, dtype) runs in a child of its own under `timeout`, and the first failure ends the run."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))

# (C, HW, Ca, add, silu, mode): the GroupNorms of one UNet call of the bench (SD v1 widths 320 / 640 / 1280 / 1280, two ResBlocks per
# level, transformers on the first three levels and in the middle block), each distinct shape once
UNET = [
    (320, 4096, 0, 0, 1, "two"),        # in_layers behind conv_in (library convolution: no producer sums)
    (320, 4096, 0, 0, 1, "cstats"),     # in_layers; the output head
    (320, 4096, 0, 1, 1, "cstats"),     # out_layers (+ time embedding)
    (320, 4096, 0, 0, 0, "cstats"),     # transformer norm
    (960, 4096, 640, 0, 1, "cstats"),   # output blocks, concatenated input
    (640, 4096, 320, 0, 1, "cstats"),
    (320, 1024, 0, 0, 1, "two"),        # behind Downsample
    (640, 1024, 0, 1, 1, "cstats"),
    (640, 1024, 0, 0, 1, "cstats"),
    (640, 1024, 0, 0, 0, "cstats"),
    (1920, 1024, 1280, 0, 1, "cstats"),
    (1280, 1024, 640, 0, 1, "cstats"),
    (960, 1024, 640, 0, 1, "cstats"),
    (640, 256, 0, 0, 1, "two"),
    (1280, 256, 0, 1, 1, "cstats"),
    (1280, 256, 0, 0, 1, "cstats"),
    (1280, 256, 0, 0, 0, "cstats"),
    (2560, 256, 1280, 0, 1, "cstats"),
    (1920, 256, 1280, 0, 1, "cstats"),
    (1280, 64, 0, 0, 1, "two"),
    (1280, 64, 0, 1, 1, "cstats"),
    (1280, 64, 0, 0, 1, "cstats"),
    (1280, 64, 0, 0, 0, "cstats"),
    (2560, 64, 1280, 0, 1, "cstats"),
]
DECODER = [
    (512, 64 * 64, 0, 0, 1, "cstats"),
    (512, 64 * 64, 0, 0, 0, "cstats"),  # the middle attention's norm
    (512, 128 * 128, 0, 0, 1, "cstats"),
    (512, 256 * 256, 0, 0, 1, "cstats"),
    (256, 256 * 256, 0, 0, 1, "cstats"),
    (256, 512 * 512, 0, 0, 1, "cstats"),
    (128, 512 * 512, 0, 0, 1, "cstats"),
]
GROUPS = {"unet": (UNET, 128, "hbm"), "decoder": (DECODER, 64, "hbm"), "cache": ([s for s in UNET if s[1] <= 256], 128, "cache")}
G, GN_EPS = 32, 1e-5


def bytes_moved(B, C, HW, mode):
    return B * HW * C * 2 * (3 if mode == "two" else 2)


def worker(args):
    import torch
    from sta import lib
    names = ("sta_groupnorm_silu_nhwc", "sta_groupnorm_silu_nhwc_cat", "sta_groupnorm_silu_nhwc_cstats", "sta_groupnorm_nhwc_workspace_bytes")
    libs = []
    for path in args.lib or [lib.LIB_PATH]:
        L = ctypes.CDLL(os.path.abspath(path))
        for n in names:
            getattr(L, n).restype, getattr(L, n).argtypes = lib.SYMBOLS[n]
        libs.append((path, L))
    shapes, B, where = GROUPS[args.group]
    B = args.images or B
    dtype = getattr(torch, args.dtype)
    dt = lib.STA_F16 if dtype == torch.float16 else lib.STA_BF16
    st = torch.cuda.current_stream().cuda_stream
    for C, HW, Ca, add, silu, mode in shapes:
        per_set = B * HW * C * 2 * 2
        nset = 1 if where == "cache" else min(48, max(3, -(-(1 << 30) // per_set)))
        while where != "cache" and any(nset % n == 0 for n in range(2, len(libs) + 1)):
            nset += 1       # coprime to the number of libraries: every library visits every set
        g = torch.Generator(device="cuda").manual_seed(1)
        sets = []
        for _ in range(nset):
            xs = [torch.randn(B, HW, c, device="cuda", dtype=dtype, generator=g) for c in ((Ca, C - Ca) if Ca else (C,))]
            sets.append((xs, torch.empty(B, HW, C, device="cuda", dtype=dtype)))
        w = (1.0 + 0.2 * torch.randn(C, device="cuda", generator=g)).to(dtype)
        b = (0.2 * torch.randn(C, device="cuda", generator=g)).to(dtype)
        addt = torch.randn(B, C, device="cuda", generator=g) if add else None
        stats = torch.tensor([0.0, float(HW)], device="cuda").repeat(B, C, 1).contiguous()       # [B][C][2], any leading width
        ws = torch.empty(max(L.sta_groupnorm_nhwc_workspace_bytes(B, HW, G) for _, L in libs) // 4, dtype=torch.float32, device="cuda")
        ap = addt.data_ptr() if add else None

        def call(L, xs, y):
            xa, xb = xs[0].data_ptr(), (xs[1].data_ptr() if Ca else None)
            if mode == "cstats":
                rc = L.sta_groupnorm_silu_nhwc_cstats(xa, xb, Ca or C, stats.data_ptr(), stats.data_ptr() if Ca else None, ap, w.data_ptr(),
                                                      b.data_ptr(), y.data_ptr(), B, C, HW, G, GN_EPS, silu, dt, st)
            elif Ca:
                rc = L.sta_groupnorm_silu_nhwc_cat(xa, xb, Ca, ap, w.data_ptr(), b.data_ptr(), y.data_ptr(), ws.data_ptr(), B, C, HW, G, GN_EPS,
                                                   silu, dt, st)
            else:
                rc = L.sta_groupnorm_silu_nhwc(xa, ap, w.data_ptr(), b.data_ptr(), y.data_ptr(), ws.data_ptr(), B, C, HW, G, GN_EPS, silu, dt, st)
            if rc:
                raise RuntimeError("launch failed (%d) in %s" % (rc, L._name))

        times, k = [[] for _ in libs], 0
        for i in range(args.warmup + args.launches):
            for j, (_, L) in enumerate(libs):
                xs, y = sets[k % nset]
                k += 1
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(L, xs, y)
                e1.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[j].append(e0.elapsed_time(e1) * 1e3)
        nbytes = bytes_moved(B, C, HW, mode)
        rec = {"group": args.group, "where": where, "dtype": args.dtype, "B": B, "C": C, "HW": HW, "Ca": Ca, "add": add, "silu": silu,
               "mode": mode, "bytes": nbytes, "sets": nset, "libs": []}
        for (path, _), t in zip(libs, times):
            med = statistics.median(t)
            rec["libs"].append({"lib": os.path.relpath(os.path.abspath(path), ROOT), "median_us": round(med, 1), "min_us": round(min(t), 1),
                                "max_us": round(max(t), 1), "tbps": round(nbytes / med / 1e6, 3)})
        if len(libs) > 1:
            first, last = times[0], times[-1]
            spread = max(max(first) - min(first), max(last) - min(last))
            gain = statistics.median(first) - statistics.median(last)
            rec.update(median_gain_us=round(gain, 1), spread_us=round(spread, 1), faster=gain > spread, slower=-gain > spread)
        print(json.dumps(rec), flush=True)
        del sets, xs, y


ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append", help="library to time (repeat to alternate several; default: this tree's)")
ap.add_argument("--groups", default="unet,decoder,cache")
ap.add_argument("--dtypes", default="float16,bfloat16")
ap.add_argument("--images", type=int, default=0, help="batch of every shape (default: 128 UNet rows, 64 decoder images)")
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--timeout", type=int, default=240, help="seconds a (group, dtype) child may take")
ap.add_argument("--group", help=argparse.SUPPRESS)
ap.add_argument("--dtype", help=argparse.SUPPRESS)
args = ap.parse_args()
if args.group:
    worker(args)
else:
    for group in args.groups.split(","):
        for dtype in args.dtypes.split(","):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--group", group, "--dtype", dtype,
                   "--images", str(args.images), "--launches", str(args.launches), "--warmup", str(args.warmup)]
            for path in args.lib or []:
                cmd += ["--lib", path]
            rc = subprocess.run(cmd).returncode
            if rc:
                sys.exit("gn_bench: %s / %s ended with status %d; nothing further was started" % (group, dtype, rc))
