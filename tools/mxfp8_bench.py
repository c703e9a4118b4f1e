"""MXFP8 Linears (sta.mxfp8, csrc/sta_mxfp8.hip) against the other paths of the transformer-block Linears, on one GPU.

Part 1, per GEMM shape: every transformer Linear of SD-v1 at 512x512 (64 images) and at 768x768 (BASELINE configs[4]'s sizes: 4 images,
K = 4 objects; rows = CFG batch 2 x images x tokens of the level). For each: the MX kernel (sta_mx8_gemm, with and without the activation
quantiser sta_mx8_quant_rows in front), hipBLASLt's row-scaled e4m3 GEMM (torch._scaled_mm, the --fp8 path, without its quantiser) and
16-bit F.linear; the GEGLU projection as the MX GEGLU-epilogue GEMM (16-bit and MXFP8 output) vs F.linear + the fused geglu pass and,
at level 0, the 16-bit fused sta_ffgemm passes. TFLOP/s and the fraction of the MX-fp8 dense peak (5.0 PF).

Part 2 (--e2e): images/s of configs[4] (768x768, K = 4, 4 images per step, fixed weights, hipGraph replay) with 16-bit, --fp8 and
--mxfp8 Linears; the model is built as bench.py's side runs build it.

    python tools/mxfp8_bench.py [--dtype fp16] [--e2e] [--ddim_steps 50] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))
import __graft_entry__  # noqa: E402,F401  (paths and environment defaults)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MX_PEAK = 5.0e15


def timed(fn, reps=20, warm=3):
    """median µs of `reps` back-to-back launches, each bracketed by events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def shapes():
    """(label, rows, K, N, kind) for every transformer Linear; kind 'geglu' is the projection C -> 8C followed by GEGLU."""
    out = []
    for res, images in ((512, 64), (768, 4)):
        lat = res // 8
        for lvl, C in enumerate((320, 640, 1280)):
            R = 2 * images * (lat >> lvl) ** 2
            tag = "%d^2 L%d" % (res, lvl)
            out += [(tag + " attn1 [Wq;Wk]", R, C, 2 * C, "plain"), (tag + " attn1 to_v", R, C, C, "plain"),
                    (tag + " to_out", R, C, C, "plain"), (tag + " ff GEGLU proj", R, C, 8 * C, "geglu"),
                    (tag + " ff out", R, 4 * C, C, "plain")]
    return out


def gemm_table(dt):
    from sta import fp8, fused, mxfp8
    dev = "cuda"
    rows = []
    for label, R, K, N, kind in shapes():
        g = torch.Generator(device=dev).manual_seed(R + K + N)
        x = torch.randn(R, K, device=dev, generator=g).to(dt)
        lin = torch.nn.Linear(K, N).to(dev, dt)
        flop = 2.0 * R * K * N
        r = {"shape": label, "rows": R, "K": K, "N": N}
        with torch.no_grad():
            mx = mxfp8.MxFp8Linear.from_linear(lin)
            xq = mxfp8.quant_rows_mx(x)
            r["mx_quant_us"] = timed(lambda: mxfp8.quant_rows_mx(x))
            f8 = fp8.Fp8Linear.from_linear(lin)
            x8, sx = fp8.quant_rows(x)
            r["rowscaled_fp8_gemm_us"] = timed(lambda: fp8.scaled_mm(x8, f8.weight_q.t(), sx, f8.weight_scale, f8.bias, dt))
            r["f16_linear_us"] = timed(lambda: F.linear(x, lin.weight, lin.bias))
            if kind == "plain":
                r["mx_gemm_us"] = timed(lambda: mx(xq, out_dtype=dt))
            else:
                r["mx_gemm_us"] = timed(lambda: mx.forward_geglu(xq, out_dtype=dt))
                r["mx_geglu_mxout_us"] = timed(lambda: mx.forward_geglu(xq, mx_out=True, out_dtype=dt))
                r["f16_linear_plus_geglu_us"] = timed(lambda: fused.geglu(F.linear(x, lin.weight, lin.bias)))
                if K == 320 and fused.ff_geglu_supported(K, N // 2):
                    w1 = fused.pack_geglu_weight(lin.weight)
                    lin2 = torch.nn.Linear(N // 2, K).to(dev, dt)
                    w2 = fused.pack_ff_out_weight(lin2.weight)
                    try:
                        h = fused.ff_geglu_qfrag(x, w1, lin.bias, N // 2, h_frag=True)
                        r["f16_ffgemm_geglu_us"] = timed(lambda: fused.ff_geglu_qfrag(x, w1, lin.bias, N // 2, h_frag=True))
                        r["f16_ffgemm_out_us"] = timed(lambda: fused.ff_out_res_hfrag(x, h, w2, lin2.bias))
                    except RuntimeError as e:             # rows beyond what one launch of the fused pass addresses
                        r["f16_ffgemm_note"] = str(e)[:120]
                    mx2 = mxfp8.MxFp8Linear.from_linear(lin2)
                    hq = mx.forward_geglu(xq, mx_out=True, out_dtype=dt)
                    r["mx_ff_out_from_mx_h_us"] = timed(lambda: mx2(hq, out_dtype=dt))
        r["mx_tflops"] = flop / r["mx_gemm_us"] / 1e6
        r["mx_frac_of_peak"] = flop / (r["mx_gemm_us"] * 1e-6) / MX_PEAK
        r["rowscaled_fp8_tflops"] = flop / r["rowscaled_fp8_gemm_us"] / 1e6
        r["f16_tflops"] = flop / r["f16_linear_us"] / 1e6
        rows.append({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()})
        print(json.dumps(rows[-1]), flush=True)
        del x, lin, mx, xq, f8, x8
        torch.cuda.empty_cache()
    return rows


def e2e(dtype_name, linears, steps, warmup, ddim_steps, res=768, K=4, images=4):
    """bench.py's side_run for configs[4] (fixed weights, hipGraph replay), with the transformer Linears as `linears`."""
    from ldm.models.diffusion.plms import PLMSSampler
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts
    dev = torch.device("cuda", 0)
    dt = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    model = build_sd_v1(dev, dt, with_vae=True, init_weights=True, seed=0, channels_last=True, use_checkpoint=False)
    torch.backends.cudnn.benchmark = False
    if linears == "fp8":
        from sta import fp8
        fp8.convert_transformer_linears_(model.model.diffusion_model)
    elif linears == "mxfp8":
        from sta import mxfp8
        mxfp8.convert_transformer_linears_mx_(model.model.diffusion_model)
    sampler = PLMSSampler(model, opt_epochs=0, use_graph=True, save_images=False)
    prompts = load_prompts(64)
    lat = res // 8
    centres = [list(c) for c in DEFAULT_CENTRES[:K]]
    x_T1 = torch.randn([1, 4, lat, lat], generator=torch.Generator(device=dev).manual_seed(1), device=dev)

    def step(j):
        recs = [prompts[(j * images + i) % len(prompts)] for i in range(images)]
        names = [(r["objects"] + ["object"] * K)[:K] for r in recs]
        conds = [conditionings(model, r["prompt"], nm, dt) for r, nm in zip(recs, names)]
        sampler.sample_batch(S=ddim_steps, shape=[4, lat, lat], conditionings=[c[1] for c in conds],
                             unconditional_conditionings=[c[0] for c in conds], bboxs=[centres] * images, object_names=names,
                             local_conditionings=[c[2] for c in conds], curr_texts=[r["prompt"] for r in recs],
                             x_T=x_T1.expand(images, -1, -1, -1), unconditional_guidance_scale=7.5, seed=1)
        return sampler.last_result

    for j in range(warmup):
        step(j)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(steps):
        r = step(warmup + j)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    assert torch.isfinite(r["x0"]).all()
    out = {"linears": linears, "images_per_s": round(steps * images / el, 3), "dtype": dtype_name, "res": res, "K": K,
           "images_per_step": images, "steps": steps, "warmup": warmup, "ddim_steps": ddim_steps}
    print(json.dumps(out), flush=True)
    del model, sampler
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    ap.add_argument("--no-gemm", action="store_true", help="skip the per-shape table")
    ap.add_argument("--e2e", action="store_true", help="also the configs[4] images/s of 16 bit, --fp8 and --mxfp8")
    ap.add_argument("--legs", default="f16,fp8,mxfp8")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ddim_steps", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from sta import lib
    lib.load()
    dt = torch.float16 if a.dtype == "fp16" else torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0), "dtype": a.dtype}
    if not a.no_gemm:
        res["gemm"] = gemm_table(dt)
    if a.e2e:
        res["e2e"] = [e2e(a.dtype, leg, a.steps, a.warmup, a.ddim_steps) for leg in a.legs.split(",")]
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
