"""The HIP 3x3 convolution (csrc/sta_conv.hip) against the library convolution at the UNet's shapes (64 = 2 x 32 images, NHWC):
max error against an fp32 convolution of the same 16-bit operands, and microseconds per call of both.
usage: python tools/conv_bench.py [--dtype fp16|bf16] [--batch 64] [--only 320x320@64,...] [--iters 20]

--up2-ab: the Upsample convolutions instead — the four 2x2 sub-pixel passes (sta_conv3x3_up2_nhwc) against the 3x3 `up2` kernel they
replace, at the three UNet shapes (128 rows of the bench) and the three VAE decoder shapes (64 images; --batch / --vae-batch), the two
variants alternating launch by launch in one process, one HIP event pair per launch, 20 launches after 3 warm-ups; median (min .. max)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "diffusion-spacetime-attn_amd"))
for _k in ("FWD", "BWD", "WRW"):
    os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + _k, "0")
import torch
import torch.nn.functional as F

from sta import fused
from sta.pipeline import use_shipped_miopen_db

use_shipped_miopen_db()

# (Cin, Cout, H = W, up2, how many per UNet call) — the 3x3 stride-1 convolutions of SD-v1's UNet at 512^2 the kernel takes
SHAPES = [(320, 320, 64, 0, 7), (640, 320, 64, 0, 2), (960, 320, 64, 0, 1), (640, 640, 64, 1, 1),
          (320, 640, 32, 0, 1), (640, 640, 32, 0, 6), (960, 640, 32, 0, 1), (1280, 640, 32, 0, 1), (1920, 640, 32, 0, 1), (1280, 1280, 32, 1, 1),
          (640, 1280, 16, 0, 1), (1280, 1280, 16, 0, 6), (1920, 1280, 16, 0, 1), (2560, 1280, 16, 0, 2), (1280, 1280, 16, 1, 1),
          (1280, 1280, 8, 0, 11), (2560, 1280, 8, 0, 3)]


# (Cin = Cout, output H = W, which model) — Upsample.conv of SD-v1's UNet at 512^2 and of its VAE decoder
UP2_SHAPES = [(1280, 16, "unet"), (1280, 32, "unet"), (640, 64, "unet"), (512, 128, "vae"), (512, 256, "vae"), (256, 512, "vae")]


def up2_ab(a, dt, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    eps = 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8
    for c, hw, model in UP2_SHAPES:
        name = "%dx%d@%dup" % (c, c, hw)
        if a.only and name not in a.only.split(","):
            continue
        B, Hs = (a.up2_batch if model == "unet" else a.vae_batch), hw // 2
        x = torch.randn(B, c, Hs, Hs, generator=g).to(dt).to(dev).contiguous(memory_format=torch.channels_last)
        w = (torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5).to(dt).to(dev).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            assert fused.conv3x3_supported(x, w, up2=True) and fused.conv3x3_up2_subpixel_supported(x, w), name
            wp3, wp2 = fused.pack_conv3x3_weight(w), fused.pack_conv3x3_up2_weight(w)
            variants = {"up2_3x3": lambda: fused.conv3x3_nhwc(x, wp3, c, up2=True),
                        "subpixel": lambda: fused.conv3x3_nhwc(x, wp2, c, up2=True, subpixel=True)}
            times = {k: [] for k in variants}
            for i in range(a.warmup + a.launches):
                for k, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        times[k].append(e0.elapsed_time(e1) * 1e3)
                    del out
            rec = {"shape": name, "model": model, "batch": B, "dtype": a.dtype, "launches": a.launches}
            for k, t in times.items():
                rec[k + "_us"] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
            flop = 2.0 * B * hw * hw * c * c
            rec["up2_3x3_tflops"] = round(9 * flop / statistics.median(times["up2_3x3"]) / 1e6, 1)
            rec["subpixel_tflops"] = round(4 * flop / statistics.median(times["subpixel"]) / 1e6, 1)      # the flops it does: 4/9
            rec["subpixel_max_below_3x3_min"] = max(times["subpixel"]) < min(times["up2_3x3"])
            if not a.no_check:
                nb = min(B, 2)
                ref = F.conv2d(F.interpolate(x[:nb], scale_factor=2.0, mode="nearest").float().contiguous(), w.float().contiguous(), None, 1, 1)
                for k, fn in variants.items():
                    rec[k + "_err_over_eps"] = round(((fn()[:nb].float() - ref).abs() / (eps * (1 + ref.abs()))).max().item(), 3)
        print(json.dumps(rec), flush=True)
        del x, w, wp3, wp2


def timed(fn, iters):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-lib", action="store_true", help="skip the library convolution (its solver search takes minutes on a fresh box)")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--up2-ab", action="store_true", help="the Upsample shapes: sub-pixel passes against the 3x3 up2 kernel")
    ap.add_argument("--up2-batch", type=int, default=128)
    ap.add_argument("--vae-batch", type=int, default=64)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[a.dtype]
    dev = torch.device("cuda:0")
    if a.up2_ab:
        return up2_ab(a, dt, dev)
    torch.backends.cudnn.benchmark = True
    g = torch.Generator(device="cpu").manual_seed(0)
    tot = {"hip": 0.0, "lib": 0.0, "tflop": 0.0}
    for cin, cout, hw, up2, cnt in SHAPES:
        name = "%dx%d@%d%s" % (cin, cout, hw, "up" if up2 else "")
        if a.only and name not in a.only.split(","):
            continue
        B, Hs = a.batch, hw >> up2
        x = torch.randn(B, cin, Hs, Hs, generator=g).to(dt).to(dev).contiguous(memory_format=torch.channels_last)
        w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(dt).to(dev).contiguous(memory_format=torch.channels_last)
        wp = fused.pack_conv3x3_weight(w)
        with torch.no_grad():
            assert fused.conv3x3_supported(x, w, up2=bool(up2)), name
            ours = lambda: fused.conv3x3_nhwc(x, wp, cout, up2=bool(up2))
            def lib_conv():
                xi = F.interpolate(x, scale_factor=2.0, mode="nearest") if up2 else x
                return F.conv2d(xi, w, None, 1, 1)
            rec = {"shape": name, "per_call": cnt}
            if not a.no_check:
                nb = min(B, 8)
                xi = F.interpolate(x[:nb], scale_factor=2.0, mode="nearest") if up2 else x[:nb]
                ref = F.conv2d(xi.float().contiguous(), w.float().contiguous(), None, 1, 1)
                got = ours()[:nb].float()
                rec["max_err"] = round((got - ref).abs().max().item(), 5)
                rec["max_ref"] = round(ref.abs().max().item(), 3)
            flop = 2.0 * B * hw * hw * 9 * cin * cout
            rec["hip_us"] = round(timed(ours, a.iters), 1)
            rec["hip_tflops"] = round(flop / rec["hip_us"] / 1e6, 1)
            if not a.no_lib:
                rec["lib_us"] = round(timed(lib_conv, a.iters), 1)
                rec["lib_tflops"] = round(flop / rec["lib_us"] / 1e6, 1)
                tot["lib"] += cnt * rec["lib_us"]
            tot["hip"] += cnt * rec["hip_us"]
            tot["tflop"] += cnt * flop / 1e12
        print(json.dumps(rec), flush=True)
    print(json.dumps({"per_unet_call_ms": {k_: round(v / 1e3, 2) for k_, v in tot.items() if k_ != "tflop"}, "tflop": round(tot["tflop"], 2)}))


if __name__ == "__main__":
    main()
