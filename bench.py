"""bench.py — images/sec at 512x512, 50 PLMS steps, 2 objects (BASELINE.json metric) on N MI355X.

One "step" = one image = one pass of the hot path over one prompt: 50 PLMS steps = 51 classifier-
free-guidance UNet calls (batch 2: uncond | cond) of the SD-v1 UNet with the fused spatial-temporal
cross-attention in its 16 transformer blocks, then the VAE decode and clamp (the PNG encode on the
host is not timed). Workload = BASELINE.json configs[1]: fixed blend weights W = 5/K, 16-bit (fp16 default, --dtype bf16), synthetic
weights of the SD-v1-4 architecture and synthetic text embeddings (no checkpoints / network here).

Multi-GPU: one process per GPU (torch.distributed.run), prompts sharded round-robin, the frozen
weights broadcast once from rank 0 over RCCL before the timed region; no communication inside it.

Prints ONE JSON line on rank 0 (see the task contract). A plain run sets up, warms up, times --steps steps and reports
the headline (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step` = milliseconds of one timed step);
--dump-outputs DIR also writes what the last timed step computed (dump_outputs). --full adds, after the headline run,
  roofline     — the dominant cross-attention forward kernel: algorithmic bytes and flops / per-launch
                 time measured here with HIP events on the launch stream, against the 8 TB/s HBM3E and 2.5 PFLOP/s
                 dense 16-bit MFMA peaks (the binding one is `bound`), and the hostile_logits leg beside it;
  side runs    — the other 16-bit type, BASELINE configs[3]'s per-GPU shard, configs[4] at 768x768, configs[2] (weight
                 optimisation);
  cpu_baseline — the same workload through the CPU oracle (fp32 torch), on a bounded sample.
The --no-* switches thin out what --full adds.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, "diffusion-spacetime-attn_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


# MIOpen benchmarks every applicable convolution solver the first time it sees a shape; its naive reference
# solvers (50-400 ms per run at these sizes) make that 200 s of warm-up on a fresh box. Excluding only those
# keeps the real solver search: warm-up 11 s, same steady state (3.2-3.4 images/s either way). NOTE:
# MIOPEN_FIND_MODE=FAST is NOT an option — on a cold find-db it falls back to CK kernels that are 5x slower.
for _k in ("FWD", "BWD", "WRW"):
    os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + _k, "0")

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable
MFMA_PEAK_TFLOPS = 2500.0      # dense bf16 / fp16 MFMA peak
M_KEYS = 77


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="after the headline run, also measure everything beside it: the roofline and hostile-logits legs, the side runs "
                         "and the CPU baseline (each can be left out with its --no-* switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy in float32 (see dump_outputs), for an output-by-output "
                         "comparison of two builds; the inputs are seeded, identical from run to run for the same arguments")
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--ddim_steps", type=int, default=50)
    ap.add_argument("--objects", type=int, default=2)
    ap.add_argument("--images-per-step", type=int, default=None,
                    help="independent prompts sampled together per step (one CFG batch of 2I per UNet call); default 64 for "
                         "fixed weights at 512^2 (one step = the 64 prompts of BASELINE configs[3]; +2.3 %% images/s over 32 same box; 4 above "
                         "512^2), 1 with --opt-epochs > 0")
    ap.add_argument("--no-graph", action="store_true", help="issue the UNet eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--channels-last", action="store_true", help="(default when --opt-epochs 0) NHWC UNet trunk")
    ap.add_argument("--checkpoint", choices=["auto", "all", "res", "none", "call"], default="auto",
                    help="weight optimisation: which blocks recompute their forward in backward. all = ResBlocks and "
                         "transformer blocks (the reference); res = ResBlocks only; none = keep every activation of the 51 "
                         "UNet calls (79.5 GiB per prompt at 512x512 — 288 GB of HBM hold two prompts); call = per UNet CALL behind "
                         "the fixed-weight forward (16 KB kept per call and image). auto = none for <= 2 prompts per step, call "
                         "above (sta.pipeline.set_recompute)")
    ap.add_argument("--nchw", action="store_true", help="keep the UNet trunk in NCHW (2.6%% slower at 8 prompts per step)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-hostile", action="store_true", help="skip the hostile_logits leg (tools/profile_bench.sh: its ~700 launches of the dominant "
                    "kernel on other operands would be averaged into the committed trace's figure for that kernel)")
    ap.add_argument("--no-side-runs", action="store_true", help="skip the bounded side measurement after the headline run "
                                                                 "(3-epoch weight optimisation = BASELINE configs[2])")
    ap.add_argument("--no-config5", action="store_true", help="skip the 768x768 / 4-object side leg (BASELINE configs[4] on one GPU)")
    ap.add_argument("--no-other-dtype", action="store_true", help="skip the side leg that times one step in the other 16-bit type "
                                                                   "(bf16 when the headline runs fp16; its convolution solvers are in the shipped MIOpen find-db)")
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16",
                    help="16-bit type of weights and activations. fp16 is the reference's own compute type (CUDA autocast) and the "
                         "one that meets north_star's 1e-3 attention-map tolerance; bf16 runs at the same MFMA rate but rounding "
                         "the block input alone to 8 mantissa bits moves the maps by 2e-3 (DESIGN.md section 2)")
    ap.add_argument("--fp8", action="store_true", help="e4m3 Linear weights in the transformer blocks (BASELINE configs[4]; sta.fp8)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak (default): every rank samples --images-per-step prompts per step, whatever the world size. strong: a step "
                         "is the 64-prompt batch of BASELINE configs[3] split 64/world per rank (8 prompts per GPU per UNet call at 8 GPUs)")
    ap.add_argument("--cpu-calls", type=int, default=3, help="timed full-width CPU UNet calls of the baseline sample (median)")
    ap.add_argument("--dry-launch", action="store_true",
                    help="start the ranks, form the process group (RCCL on GPUs, gloo without), broadcast the frozen weights, check every "
                         "rank holds rank 0's bytes, and stop BEFORE the first kernel of the sampler: the multi-rank plumbing of --gpus N, "
                         "runnable on a CPU-only host (a reduced-width UNet there)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="TEST MODE for one-GPU boxes: all --gpus N ranks run on GPU 0 and gloo carries the collectives (RCCL refuses duplicate "
                         "devices in one communicator). Everything else of the N > 1 path is the real thing: own ranks, per-rank MIOpen db copies, "
                         "the bucketed weight transfer, hipGraph capture in N processes, barrier + max over ranks. Not a throughput figure")
    ap.add_argument("--opt-epochs", type=int, default=0,
                    help="weight-optimisation epochs (0 = fixed weights = BASELINE configs[1], the headline; 3 = configs[2] "
                         "with a CLIP stand-in loss, reported as a side measurement)")
    a = ap.parse_args()
    if a.steps < 1:
        raise SystemExit("--steps must be at least 1 (the timed region is --steps steps)")
    if a.scaling == "strong":
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if 64 % world:
            raise SystemExit("--scaling strong splits the 64 prompts of BASELINE configs[3]: the world size must divide 64")
        a.images_per_step = 64 // world
    if a.images_per_step is None:
        a.images_per_step = (64 if a.res <= 512 else 4) if a.opt_epochs == 0 else 1
    return a


def launch_units(kind, n_img, N, C, K):
    """Algorithmic work of ONE forward launch (16-bit activations, M = 77 keys):
      attention       F = 4*M*C*N*(K+2) flop per image;  Bt = 8*N*C (q or y in, out) + 4*(K+2)*M*C (K,V) + K*N (mask) bytes
      + projection    the to_q GEMM inside the kernel (sta_xattn_fwd_proj): + 2*2*N*C*C flop per image, + 2*C*C bytes (Wq) once."""
    flops = 4.0 * M_KEYS * C * N * (K + 2) * n_img
    byts = (8.0 * N * C + 4.0 * (K + 2) * M_KEYS * C + K * N) * n_img
    if kind == "bwd":
        # backward unit: F_bwd = 2 F (S = Q K^T, dP = dO V^T, dQ = dS K and the P V-sized products behind dcoef —
        # the kernel gets those from sum_key P dP and issues THREE phases; the dense definition stays 2 F); bytes = 12 N C (read q and
        # dO, write dq) + K, V once + the mask bytes + K floats
        return 2.0 * flops, (12.0 * N * C + 4.0 * (K + 2) * M_KEYS * C + K * N) * n_img
    if kind == "proj":
        flops += 4.0 * N * C * C * n_img
        byts += 2.0 * C * C
    return flops, byts


def measure_xattn(run_eager_call, n_calls=4, reps=20):
    """Per-launch duration of every cross-attention forward launch of a UNet call, two ways:
      in situ  — `n_calls` real CFG UNet calls are issued eagerly while sta.ops brackets every launch with its own
                 HIP-event pair on the launch stream (torch's current stream IS the stream the C-ABI call is given).
                 RAW event times, nothing subtracted: an empty event pair alone measures ~4.6 us on this stack, so
                 these sit that much ABOVE rocprofv3's kernel durations (profiles/ holds the trace of the same command);
      warm     — each recorded launch re-issued `reps` times back to back between ONE event pair (inputs resident in
                 L2 / Infinity Cache, no neighbours): what the kernel does when its operands are on chip."""
    from sta import ops
    run_eager_call()                                     # warm the eager path (first launches, allocator)
    ops.LAUNCH_LOG = []
    try:
        for _ in range(n_calls):
            run_eager_call()
        torch.cuda.synchronize()
        log = ops.LAUNCH_LOG
    finally:
        ops.LAUNCH_LOG = None
    per_call = len(log) // n_calls
    rows = []
    for j in range(per_call):
        kind, n_img, N, C, K = log[j][:5]
        us = [log[j + c * per_call][5].elapsed_time(log[j + c * per_call][6]) * 1e3 for c in range(n_calls)]
        relaunch = log[j][7]
        for _ in range(3):
            relaunch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            relaunch()
        e1.record()
        torch.cuda.synchronize()
        flops, byts = launch_units(kind, n_img, N, C, K)
        rows.append(dict(kind=kind, N=N, C=C, us=sum(us) / len(us), warm_us=e0.elapsed_time(e1) * 1e3 / reps, flops=flops, bytes=byts))
    return rows


LEVELS = [("L0", 4096, 320), ("L1", 1024, 640), ("L2", 256, 1280), ("mid", 64, 1280)]      # SD-v1 at 512^2: (N, C) per UNet level, 8 heads


def cpu_baseline(res, ddim_steps, K, n_calls):
    """The reference's CPU path restated ("Timing the reference CPU path"): fp32 torch modules with the
    ORACLE's fused op on this box's host cores (oracle/ is the checker; here it is the thing timed, as the contract allows).
      per_level_us  the fused op alone (K + 2 attentions + disc masks + blend, oracle.fused_xattn) at the four (N, C) level shapes
                    of a 512x512 UNet call, one image: median of 5 runs after 1 warm-up — the CPU figure beside `roofline`'s kernel;
      config1_s     BASELINE configs[0] END TO END, really run: one prompt, 64x64 latent, S = 10 PLMS steps (11 CFG UNet calls),
                    K = 1 object, fixed weights, + the VAE decode, through the product's own sampler with the oracle op — on the
                    REDUCED-WIDTH UNet of the golden fixtures (model_channels 64, same topology; the full-width run is ~2 min);
      value         images/s of the bench workload (512x512, 50 steps, K objects, FULL width), EXTRAPOLATED from the median of
                    `n_calls` full-width CFG UNet calls and one VAE decode to 51 calls + 1 decode."""
    import statistics
    from ldm.models.diffusion.plms import PLMSSampler
    from oracle import xattn_oracle as orc
    from sta import prompt_state
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings
    from tests.cpu_backend import oracle_ops
    torch.manual_seed(0)
    cores = torch.get_num_threads()
    # (1) the fused op per level. These are small problems (4096 x 77 scores per head at level 0): on all cores of a 128-thread
    # box the per-call thread hand-off dominates and the median of 5 does not reproduce (4.4 ms on one box, 38.7 ms on another);
    # 16 threads — one CCD's worth — and the median of 9 after 2 warm-ups do
    per_level, runs, level_threads = {}, 9, min(cores, 16)
    torch.set_num_threads(level_threads)
    try:
        with torch.no_grad():
            for name, N, C in LEVELS:
                dim = int(N ** 0.5)
                q = torch.randn(2, N, C)
                k, v = torch.randn(K + 2, M_KEYS, C) * 0.78, torch.randn(K + 2, M_KEYS, C)
                mask = orc.disc_masks([list(cc) for cc in DEFAULT_CENTRES[:K]], dim).reshape(K, N) if K else torch.zeros(0, N, dtype=torch.bool)
                coef = torch.full((K,), 5.0 / max(K, 1))
                ts = []
                for r in range(runs + 2):
                    t0 = time.perf_counter()
                    orc.fused_xattn(q, k, v, mask, coef, 8, (C // 8) ** -0.5)
                    ts.append(time.perf_counter() - t0)
                per_level["%s_N%d_C%d" % (name, N, C)] = round(statistics.median(ts[2:]) * 1e6, 1)
    finally:
        torch.set_num_threads(cores)
    # (2) configs[0] end to end on the reduced-width UNet
    small = build_sd_v1("cpu", torch.float32, with_vae=True, init_weights=False, unet_overrides=dict(model_channels=64))
    for p in small.parameters():
        torch.nn.init.normal_(p, std=0.02)
    uc, c, local = conditionings(small, "a bench prompt", ["obj0"])
    x_T = torch.randn(1, 4, 64, 64)
    sampler = PLMSSampler(small, opt_epochs=0, use_graph=False, save_images=False)
    with oracle_ops(), torch.no_grad():
        t0 = time.perf_counter()
        sampler.sample(S=10, conditioning=c, batch_size=1, shape=[4, 64, 64], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=uc, eta=0.0, x_T=x_T, text_index=0, curr_text="a bench prompt",
                       bboxs_curr=[list(DEFAULT_CENTRES[0])], seed=1, prompt_idx=0, object_names=["obj0"], local_conditionings=local)
        config1_s = time.perf_counter() - t0
    assert torch.isfinite(sampler.last_result["x0"]).all()
    del small, sampler
    # (3) the bench workload at full width: a bounded sample, extrapolated
    model = build_sd_v1("cpu", torch.float32, with_vae=True, init_weights=False)
    for p in model.parameters():          # cheap init (values do not change the timing)
        torch.nn.init.normal_(p, std=0.02)
    uc, c, local = conditionings(model, "a bench prompt", ["obj%d" % i for i in range(K)])
    lat = res // 8
    x = torch.randn(2, 4, lat, lat)
    t = torch.tensor([981, 981])
    coef = torch.full((K,), 5.0 / max(K, 1))
    centres = [list(cc) for cc in DEFAULT_CENTRES[:K]]
    with oracle_ops(), torch.no_grad():
        prompt_state.begin_prompt(local, first_timestep=981)
        c_in = torch.cat([uc, c])
        model.apply_model_extra(x, 0, t, c_in, coef=coef, bboxs_curr=centres)           # warm-up (allocator, oneDNN)
        calls = []
        for _ in range(n_calls):
            t0 = time.perf_counter()
            model.apply_model_extra(x, 0, t, c_in, coef=coef, bboxs_curr=centres)
            calls.append(time.perf_counter() - t0)
        t_call = statistics.median(calls)
        t0 = time.perf_counter()
        model.decode_first_stage(x[:1])
        t_dec = time.perf_counter() - t0
    n_unet = ddim_steps + 1
    return dict(value=1.0 / (n_unet * t_call + t_dec), unit="images/s", cores=cores, kind="port", extrapolated=True,
                sample="median of %d full-width CFG UNet calls (%.2f s) + 1 VAE decode (%.2f s) at %dx%d, fp32 torch + oracle op, after 1 "
                       "warm-up call; EXTRAPOLATED to %d calls + 1 decode per image" % (n_calls, t_call, t_dec, res, res, n_unet),
                unet_call_s=[round(x_, 3) for x_ in calls], vae_decode_s=round(t_dec, 3),
                per_level_us=per_level, per_level_what="oracle fused op (K = %d: %d attentions + disc masks + blend), one image, fp32, median of %d "
                                                       "runs after 2 warm-ups on %d threads" % (K, K + 2, runs, level_threads), runs=runs,
                per_level_threads=level_threads,
                config1_s=round(config1_s, 2),
                config1_what="BASELINE configs[0] end to end, really run: 1 prompt, 64x64 latent, S = 10 PLMS steps (11 CFG UNet calls), K = 1, "
                             "fixed weights, + full VAE decode; REDUCED-width UNet (model_channels 64, the golden fixtures' topology), fp32")


def source_sha(names=("sta_xattn_proj3.hip", "sta_xattn_proj3.h", "sta_xattn_dev.h", "sta_xattn_proj.hip", "sta_xattn.hip")):
    """sha256 over the kernel sources a committed counter measurement belongs to (profiles/xattn_fwd_hbm_traffic.json keeps the
    hash it was taken at; a measurement of an older kernel is refused instead of being reported as this one's)."""
    import hashlib
    h = hashlib.sha256()
    for n in names:
        with open(os.path.join(PKG, "csrc", n), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _selfattn_optimistic_state():
    """What the level-0 self-attention calls of the timed region left in their flags buffers (sta.ops._SA_FLAGS: one per shape): the calls the
    optimistic loop still sits out, and how many workgroups the LAST call handed to the repair launch of the standard loop — the timed
    rate belongs to the optimistic loop only if both are 0."""
    from sta import ops
    res = []
    for (d_, _stream_, nbytes), f in ops._SA_FLAGS.items():
        w = f.view(torch.int32).cpu()
        res.append({"workgroups": (nbytes // 4) - 32, "sitting_out_calls": int(w[0]), "flagged_last_call": int(w[32:].sum())})
    return {"enabled": bool(ops.SELFATTN_OPTIMISTIC), "buffers": res}


def _trunk_kernels(a):
    """Which of the trunk's operations run on own HIP kernels in this run (sta.fused switches; the tracked epochs keep the library's
    differentiable convolutions / GEMMs)."""
    from sta import fused
    nhwc = (a.channels_last or a.opt_epochs == 0) and not a.nchw
    return {"conv3x3": "csrc/sta_conv.hip" if fused.CONV3X3 and nhwc else "MIOpen",
            "proj_out+residual, skip 1x1 over cat": "csrc/sta_gemm.hip" if fused.LINEAR_ROWS and nhwc else "hipBLASLt / MIOpen",
            "cat([h, skip]) of the output blocks": "read in place" if fused.CAT_IN_PLACE and fused.LINEAR_ROWS and nhwc else "torch.cat"}


def roofline_leg(model, dev, dt, dtype_name, I, K, lat, rec, centres):
    """`roofline` of the JSON line: per-launch times of the cross-attention forward kernels on the tensors of real CFG UNet
    calls of `model` (measure_xattn), the dominant launch against the HBM and MFMA peaks, the 16-launch aggregate beside it."""
    from sta import prompt_state
    from sta.pipeline import conditionings
    names = (rec["objects"] + ["object"] * K)[:K]
    uc, c, local_c = conditionings(model, rec["prompt"], names, dt)
    pair = lambda u, v: torch.stack([u, v], dim=1).reshape(2 * I, *u.shape[1:])
    c_in = pair(uc.expand(I, -1, -1), c.expand(I, -1, -1)).contiguous()
    x_in = torch.randn(2 * I, 4, lat, lat, device=dev)
    t_in = torch.full((2 * I,), 981, device=dev, dtype=torch.long)
    coef = torch.full((I, K), 5.0 / max(K, 1), device=dev) if I > 1 else torch.full((K,), 5.0 / max(K, 1), device=dev)
    boxes = [centres] * I if I > 1 else centres
    prompt_state.begin_prompt([local_c] * I if I > 1 else local_c, first_timestep=981)

    def run_eager_call():
        with torch.no_grad():
            model.apply_model_extra(x_in, 0, t_in, c_in, coef=coef, bboxs_curr=boxes)

    rows = measure_xattn(run_eager_call)
    by_shape = {}
    for r in rows:
        by_shape.setdefault((r["kind"], r["N"], r["C"]), []).append(r)
    # the dominant kernel = the launch shape with the largest share of the cross-attention time of a UNet call
    dom = max(by_shape, key=lambda k_: sum(r["us"] for r in by_shape[k_]))
    d_us = sum(r["us"] for r in by_shape[dom]) / len(by_shape[dom])
    d_flops, d_bytes = by_shape[dom][0]["flops"], by_shape[dom][0]["bytes"]
    t_hbm, t_mfma = d_bytes / (HBM_PEAK_GBS * 1e3), d_flops / (MFMA_PEAK_TFLOPS * 1e6)      # us at either peak
    all_us, all_bytes, all_flops = (sum(r[k_] for r in rows) for k_ in ("us", "bytes", "flops"))
    # which projection-fused kernel the library dispatches (csrc/sta_xattn_proj.hip): a head pair per workgroup when two
    # heads' compact operand images fit one CU's LDS (d = 40, K <= 2) and the launch has >= 256 pair workgroups; it then reads
    # norm2's output in query-fragment order (sta_add_layernorm_qfrag -> sta_xattn_fwd_proj_qfrag)
    pair_k = dom[2] == 320 and K <= 2 and (dom[1] // 128) * 4 * I >= 256
    # HBM-side traffic: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (tools/pmc_traffic_kernel.py), committed per kernel, shape,
    # images per launch AND the hash of the kernel sources they were taken at — a measurement of an older kernel is not reported
    traffic, traffic_note = None, "no committed PMC measurement for this launch"
    pmc = os.path.join(REPO, "profiles", "xattn_fwd_hbm_traffic.json")
    if os.path.exists(pmc):
        ent = json.load(open(pmc)).get("by_kernel", {}).get("%s_N%d_C%d_I%d" % (dom + (I,)) + ("" if dtype_name == "fp16" else "_" + dtype_name))
        if ent and ent.get("source_sha") == source_sha() and ent.get("dtype", "fp16") == dtype_name:
            traffic, traffic_note = ent["bytes_per_launch"], "rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + WRITE_SIZE, separate passes, kernel sources %s" % ent["source_sha"]
        elif ent:
            traffic_note = "the committed PMC measurement belongs to other kernel sources / dtype (%s, %s): refused as stale" % (ent.get("source_sha"), ent.get("dtype", "fp16"))
    kname = {"proj": ("xattn_fwd_proj_p3_kernel (to_q GEMM + QK^T + softmax + disc mask + blend + PV in one launch, a head pair per workgroup, y in query-fragment order)" if pair_k else
                      "xattn_fwd_proj_kernel (to_q GEMM + QK^T + softmax + disc mask + blend + PV in one launch, one head per workgroup)"),
             "attn": "xattn_fwd{,_staged}_kernel (QK^T + softmax + disc mask + blend + PV)"}[dom[0]]
    bound = "hbm" if t_hbm >= t_mfma else "mfma"
    roof = {
        "bound": bound,
        "achieved": d_bytes / d_us / 1e3 if bound == "hbm" else d_flops / d_us / 1e6,
        "peak": HBM_PEAK_GBS if bound == "hbm" else MFMA_PEAK_TFLOPS, "unit": "GB/s" if bound == "hbm" else "TFLOP/s",
        "frac": max(t_hbm, t_mfma) / d_us, "traffic": traffic, "traffic_note": traffic_note, "dtype": dtype_name,
        "kernel": "%s, N=%d C=%d, %d image(s) per launch, %d of the %d launches of a UNet call (%.0f %% of their time)"
                  % (kname, dom[1], dom[2], I, len(by_shape[dom]), len(rows), 100.0 * d_us * len(by_shape[dom]) / all_us),
        "bytes_per_launch": d_bytes, "flops_per_launch": d_flops, "avg_launch_us": d_us,
        # the samples behind the average (it is a plain mean: one stalled launch among them would show here, not be dropped)
        "launch_us_samples": {"n": len(by_shape[dom]), "min": round(min(r["us"] for r in by_shape[dom]), 2),
                              "median": round(sorted(r["us"] for r in by_shape[dom])[len(by_shape[dom]) // 2], 2),
                              "max": round(max(r["us"] for r in by_shape[dom]), 2)},
        "flop_per_byte": d_flops / d_bytes, "ridge_flop_per_byte": MFMA_PEAK_TFLOPS * 1e3 / HBM_PEAK_GBS,
        "hbm_gbps": d_bytes / d_us / 1e3, "hbm_frac": t_hbm / d_us, "mfma_tflops": d_flops / d_us / 1e6, "mfma_frac": t_mfma / d_us,
        "peak_note": "the MFMA peak (%.0f TFLOP/s dense) is the 2.4 GHz figure; under the level-0 launch the chip sustains 1.95 - 1.97 GHz in fp16 and "
                     "2.06 GHz in bf16 with identical busy cycles (tools/p3_clock.py, profiles/r06_p3_clock.json)" % MFMA_PEAK_TFLOPS,
        "how": "in situ: 4 real eager CFG UNet calls, one HIP-event pair per launch on the launch stream, RAW event times "
               "(an empty pair measures ~4.6 us here; nothing subtracted)",
        "warm_launch_us": sum(r["warm_us"] for r in by_shape[dom]) / len(by_shape[dom]),
        "warm_how": "the same launches re-issued 20x back to back between one event pair. NOT comparable with `in situ` below level 0: a level-1 "
                    "launch touches 168 MB (q + out), which stays resident in the 256 MiB Infinity Cache between repetitions, so warm times are "
                    "cache-resident times; in situ the same bytes come from HBM behind the to_q GEMM (profiles/r04_insitu_vs_warm.md)",
        "all_launches": {"n": len(rows), "sum_us": all_us, "hbm_gbps": all_bytes / all_us / 1e3, "hbm_frac": all_bytes / all_us / 1e3 / HBM_PEAK_GBS,
                         "mfma_tflops": all_flops / all_us / 1e6, "mfma_frac": all_flops / all_us / 1e6 / MFMA_PEAK_TFLOPS},
        "per_shape_us": {"%s_N%d_C%d" % k_: round(sum(r["us"] for r in v) / len(v), 2) for k_, v in sorted(by_shape.items(), key=lambda kv: -kv[0][1])},
        "per_shape_warm_us": {"%s_N%d_C%d" % k_: round(sum(r["warm_us"] for r in v) / len(v), 2) for k_, v in sorted(by_shape.items(), key=lambda kv: -kv[0][1])}}
    prof = os.path.join(REPO, "profiles", "r06_bench_kernel_stats.csv")
    if os.path.exists(prof) and dtype_name == "fp16":      # rocprofv3 --kernel-trace summary of this command, committed: the cross-check
        import csv
        want = "xattn_fwd_proj" if dom[0] == "proj" else "xattn_fwd_staged"      # xattn_fwd_proj_p3_kernel / xattn_fwd_proj_kernel
        hit = [r for r in csv.DictReader(open(prof)) if want in r["kernel"]]
        if hit:
            best = max(hit, key=lambda r: float(r["total_ns"]))
            roof["rocprof_avg_us_committed"] = float(best["avg_ns"]) / 1e3
    return roof


def roofline_bwd_leg(model, dev, dt, dtype_name, I, K, lat, rec, centres, n_calls=3, reps=20):
    """`roofline_bwd` of the weight-optimisation leg: every sta_xattn_bwd launch (dq, dcoef of the fused op) of a TRACKED CFG UNet
    call — forward under autograd exactly as the tracked epochs run it (sta.fused.tracked, the model's recomputation policy), then
    backward of a scalar of its output — bracketed in situ by its own HIP-event pair on the launch stream, and re-issued warm.
    Units: launch_units("bwd"). The forward launches of the same call (sta_xattn_fwd: the tracked path keeps q) are timed beside it."""
    from sta import fused, ops, prompt_state
    from sta.pipeline import conditionings
    names = (rec["objects"] + ["object"] * K)[:K]
    uc, c, local_c = conditionings(model, rec["prompt"], names, dt)
    pair = lambda u, v: torch.stack([u, v], dim=1).reshape(2 * I, *u.shape[1:])
    c_in = pair(uc.expand(I, -1, -1), c.expand(I, -1, -1)).contiguous()
    t_in = torch.full((2 * I,), 981, device=dev, dtype=torch.long)
    boxes = [centres] * I if I > 1 else centres
    prompt_state.begin_prompt([local_c] * I if I > 1 else local_c, first_timestep=981)
    by_call = bool(getattr(model, "sta_call_recompute", False))

    def call():
        x = torch.randn(I, 4, lat, lat, device=dev, requires_grad=True)
        coef = (torch.full((I, K), 5.0 / max(K, 1), device=dev) if I > 1 else torch.full((K,), 5.0 / max(K, 1), device=dev)).requires_grad_(True)
        with torch.enable_grad(), fused.tracked(by_call):
            out = model.apply_model_extra(pair(x, x), 0, t_in, c_in, coef=coef, bboxs_curr=boxes)
            out.float().square().mean().backward()

    call()
    ops.LAUNCH_LOG = []
    try:
        for _ in range(n_calls):
            call()
        torch.cuda.synchronize()
        log = ops.LAUNCH_LOG
    finally:
        ops.LAUNCH_LOG = None
    shapes = {}
    for kind, n_img, N, C, K_, e0, e1, relaunch in log:
        s = shapes.setdefault((kind, N, C), dict(us=[], relaunch=relaunch, n_img=n_img, K=K_))
        s["us"].append(e0.elapsed_time(e1) * 1e3)
    rows = {}
    for (kind, N, C), s in shapes.items():
        for _ in range(3):
            s["relaunch"]()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            s["relaunch"]()
        e1.record()
        torch.cuda.synchronize()
        flops, byts = launch_units(kind, s["n_img"], N, C, s["K"])
        us = sum(s["us"]) / len(s["us"])
        rows[(kind, N, C)] = dict(us=us, warm_us=e0.elapsed_time(e1) * 1e3 / reps, launches_per_call=len(s["us"]) // n_calls, flops=flops, bytes=byts)
    bwd = {k_: v for k_, v in rows.items() if k_[0] == "bwd"}
    if not bwd:
        return {"error": "no sta_xattn_bwd launch was recorded in a tracked UNet call"}
    dom = max(bwd, key=lambda k_: bwd[k_]["us"] * bwd[k_]["launches_per_call"])
    d = bwd[dom]
    traffic, traffic_note = None, "no committed PMC measurement for this launch"
    pmc = os.path.join(REPO, "profiles", "xattn_bwd_hbm_traffic.json")
    sha = source_sha(("sta_xattn_bwd.hip", "sta_xattn_dev.h"))
    if os.path.exists(pmc):
        ent = json.load(open(pmc)).get("by_kernel", {}).get("bwd_N%d_C%d_I%d" % (dom[1], dom[2], I) + ("" if dtype_name == "fp16" else "_" + dtype_name))
        if ent and ent.get("source_sha") == sha:
            traffic, traffic_note = ent["bytes_per_launch"], "rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + WRITE_SIZE, separate passes, kernel sources %s" % sha
        elif ent:
            traffic_note = "the committed PMC measurement belongs to other kernel sources (%s): refused as stale" % ent.get("source_sha")
    t_hbm, t_mfma = d["bytes"] / (HBM_PEAK_GBS * 1e3), d["flops"] / (MFMA_PEAK_TFLOPS * 1e6)
    table = {}
    for (kind, N, C), v in sorted(bwd.items(), key=lambda kv: -kv[0][1]):
        f = rows.get(("attn", N, C))
        table["N%d_C%d" % (N, C)] = {"bwd_us": round(v["us"], 2), "bwd_warm_us": round(v["warm_us"], 2), "launches_per_call": v["launches_per_call"],
                                     "hbm_frac": round(v["bytes"] / v["us"] / 1e3 / HBM_PEAK_GBS, 4), "mfma_frac": round(v["flops"] / v["us"] / 1e6 / MFMA_PEAK_TFLOPS, 4),
                                     "fwd_us": round(f["us"], 2) if f else None, "fwd_warm_us": round(f["warm_us"], 2) if f else None,
                                     "bwd_over_fwd": round(v["us"] / f["us"], 2) if f else None, "bwd_over_fwd_warm": round(v["warm_us"] / f["warm_us"], 2) if f else None}
    all_us = sum(v["us"] * v["launches_per_call"] for v in bwd.values())
    all_b = sum(v["bytes"] * v["launches_per_call"] for v in bwd.values())
    all_f = sum(v["flops"] * v["launches_per_call"] for v in bwd.values())
    bound = "hbm" if t_hbm >= t_mfma else "mfma"
    return {"bound": bound, "achieved": d["bytes"] / d["us"] / 1e3 if bound == "hbm" else d["flops"] / d["us"] / 1e6,
            "peak": HBM_PEAK_GBS if bound == "hbm" else MFMA_PEAK_TFLOPS, "unit": "GB/s" if bound == "hbm" else "TFLOP/s",
            "frac": max(t_hbm, t_mfma) / d["us"], "traffic": traffic, "traffic_note": traffic_note, "dtype": dtype_name,
            "kernel": "xattn_bwd_res_kernel + dcoef_reduce_kernel (sta_xattn_bwd: dq and dcoef of the fused op; S^T, dP^T, dQ^T per context, no attention "
                      "outputs formed), N=%d C=%d, %d image(s) per launch, %d of the %d backward launches of a tracked UNet call"
                      % (dom[1], dom[2], I, d["launches_per_call"], sum(v["launches_per_call"] for v in bwd.values())),
            "bytes_per_launch": d["bytes"], "flops_per_launch": d["flops"], "avg_launch_us": d["us"], "warm_launch_us": d["warm_us"],
            "hbm_gbps": d["bytes"] / d["us"] / 1e3, "hbm_frac": t_hbm / d["us"], "mfma_tflops": d["flops"] / d["us"] / 1e6, "mfma_frac": t_mfma / d["us"],
            "how": "in situ: %d tracked CFG UNet calls (forward under autograd with the leg's recomputation policy, then backward), one HIP-event pair per "
                   "sta_xattn_bwd call on the launch stream — the pair covers the backward kernel AND its dcoef reduction launch, RAW event times (an empty "
                   "pair measures ~4.6 us here; nothing subtracted); warm: the same call re-issued %dx back to back" % (n_calls, reps),
            "per_level": table,
            "all_launches": {"n": sum(v["launches_per_call"] for v in bwd.values()), "sum_us": all_us, "hbm_frac": all_b / all_us / 1e3 / HBM_PEAK_GBS,
                             "mfma_frac": all_f / all_us / 1e6 / MFMA_PEAK_TFLOPS}}


def hostile_logits_leg(dev, dtype_name, I, K, lat):
    """How much does the level-0 roofline figure depend on friendly logits? The bench's weights are synthetic (std 0.02): every context's
    largest score lies inside the optimistic softmax's window. Real SD-v1 cross-attention is known for a dominant BOS-token logit, so
    this leg re-issues the dominant launch (the head-pair kernel at the bench's batch, stand-alone, warm) on operands in which key 0 of
    every context leads by ~ +16 nats: `friendly` (the bench's regime), `hostile_first` (the first launch after the statistics words were
    zeroed: optimistic attempt + fall-back per context), `hostile_steady` (the launches after it: the device-side switch has sat the
    optimistic path out, every context takes the standard softmax) and `standard_build`-equivalent = hostile_steady on friendly operands."""
    from sta import lib, ops
    dt = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    N, C, heads = lat * lat, 320, 8
    g = torch.Generator(device="cpu").manual_seed(0)
    y = torch.randn(2 * I, N, C, generator=g).to(dt).to(dev)
    wq = (torch.randn(C, C, generator=g) / C ** 0.5).to(dt).to(dev)
    k = (torch.randn(I * (K + 2), M_KEYS, C, generator=g) * 0.78)
    v = torch.randn(I * (K + 2), M_KEYS, C, generator=g).to(dt).to(dev)
    mask = ops.disc_mask_bits([(0.30, 0.40), (0.70, 0.60), (0.5, 0.2), (0.25, 0.75)][:K], lat).to(dev).repeat(I, 1)
    coef = torch.full((I, K), 5.0 / max(K, 1), device=dev)
    scale = (C // heads) ** -0.5
    if not ops.proj_qfrag_supported(C, heads, M_KEYS, K, N, I):
        return {"skipped": "the launch does not take the head-pair kernel at this size"}
    wqf, yq = ops.pack_wq(wq, heads), ops.to_qfrag(y)
    q = (y[:2].float() @ wq.float().t()).view(2, N, heads, C // heads)
    qm = q.mean((0, 1)); qm = qm / qm.norm(dim=-1, keepdim=True)
    lead = 16.0 / scale / (q * qm).sum(-1).abs().mean().item()
    kh = k.clone(); kh[:, 0] = (qm * lead).reshape(C).cpu()
    out = {}

    def timed(kvp, stats, reps=20, rounds=3):
        # the smallest of `rounds` event-pair averages: a box now and then stalls one launch of a back-to-back series by ~1 ms (seen as
        # 302 against 255 us for the same binary and operands on two boxes), which a single average of 20 carries as +50 us
        best = None
        for _ in range(rounds if reps > 1 else 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.xattn_forward_proj(yq, wqf, kvp, mask, coef, scale, qfrag=True, ofrag=True, stats=stats)
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) * 1e3 / reps
            best = t if best is None else min(best, t)
        return best

    for name, kk in (("friendly", k), ("hostile", kh)):
        kvp = ops.pack_kv_proj(kk.to(dt).to(dev), v, heads, n_img=I)
        stats = torch.zeros(lib.P3_STATS_WORDS, dtype=torch.int32, device=dev)
        for _ in range(200):     # ~50 ms: the chip's clocks settle (the first series behind 3 launches read 10 % slower than the ones after it)
            ops.xattn_forward_proj(yq, wqf, kvp, mask, coef, scale, qfrag=True, ofrag=True, stats=None)      # warm, no switch: always optimistic
        out[name + "_always_optimistic_us"] = round(timed(kvp, None), 2)
        first = timed(kvp, stats, reps=1)
        s1 = stats.cpu().tolist()
        steady = timed(kvp, stats)
        s2 = stats.cpu().tolist()
        out[name] = {"first_launch_us": round(first, 2), "steady_us": round(steady, 2), "fallback_rate_first_launch": round(s1[5] / max(s1[4], 1), 4),
                     "sitting_out_after_first": s1[0], "launches_sat_out_of_61": s2[7]}
        if name == "friendly":      # the standard softmax alone on the friendly operands: force the switch
            stats[0] = 1 << 20
            out["friendly_standard_softmax_us"] = round(timed(kvp, stats), 2)
    out["what"] = ("head-pair kernel (to_q + attention + blend, query fragments in, out fragments out), N=%d C=%d K=%d, %d images, %s, warm back-to-back launches; "
                   "hostile = key 0 of every context leads by ~ +16 nats; steady = the smallest 20-launch average of three series behind the first launch (the switch engaged where the "
                   "fall-back rate was above 1/8: it holds for 64 launches and is renewed by the first optimistic launch after them)" % (N, C, K, I, dtype_name))
    out["worst_case_over_standard"] = round(out["hostile"]["steady_us"] / out["friendly_standard_softmax_us"], 4)
    return out


def side_run(dev, dtype_name, opt_epochs, images, steps, warmup, res, ddim_steps, K, checkpoint="auto", find=True, roofline=False, roofline_bwd=False,
             fp8_linears=False):
    """A bounded side measurement on rank 0 after the headline run: the same workload with another 16-bit type, or
    BASELINE configs[2] (3 weight-optimisation epochs: two tracked trajectories with backward + one fixed-weight one).
    Builds its own model, reports images/s over `steps` timed steps after `warmup` untimed ones."""
    from ldm.models.diffusion.plms import DCLIPLoss, PLMSSampler
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts, set_recompute
    from sta.synth import SyntheticCLIP
    dt = torch.float16 if dtype_name == "fp16" else torch.bfloat16
    model = build_sd_v1(dev, dt, with_vae=True, init_weights=True, seed=0, channels_last=opt_epochs == 0, use_checkpoint=opt_epochs > 1)
    torch.backends.cudnn.benchmark = bool(find)
    if fp8_linears:          # BASELINE configs[4]: e4m3 Linear weights in the transformer blocks (sta.fp8: a memory option, torch._scaled_mm)
        from sta import fp8
        fp8.convert_transformer_linears_(model.model.diffusion_model)
    mode = set_recompute(model, checkpoint, images) if opt_epochs > 1 else None
    loss_model = DCLIPLoss(SyntheticCLIP().to(dev)) if opt_epochs > 0 else None
    sampler = PLMSSampler(model, opt_epochs=opt_epochs, loss_model=loss_model, use_graph=True, save_images=False)
    prompts = load_prompts(64)
    lat = res // 8
    centres = [list(c) for c in DEFAULT_CENTRES[:K]]
    x_T1 = torch.randn([1, 4, lat, lat], generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    calib = None
    if opt_epochs > 1:
        # synthetic VAE weights saturate the image clamp (zero loss gradient): rescale the decoder's last convolution on one
        # fixed-weight sample so that the tracked epochs optimise something (sta.synth.calibrate_decoder_)
        from sta.synth import calibrate_decoder_
        pre = PLMSSampler(model, opt_epochs=0, use_graph=False, save_images=False)
        rec = prompts[0]
        nm = (rec["objects"] + ["object"] * K)[:K]
        uc0, c0, l0 = conditionings(model, rec["prompt"], nm, dt)
        pre.sample(S=ddim_steps, conditioning=c0, batch_size=1, shape=[4, lat, lat], verbose=False, unconditional_guidance_scale=7.5,
                   unconditional_conditioning=uc0, eta=0.0, x_T=x_T1, text_index=0, curr_text=rec["prompt"], bboxs_curr=centres, seed=1,
                   prompt_idx=0, object_names=nm, local_conditionings=l0)
        calib = calibrate_decoder_(model, pre.last_result["x0"])
        del pre

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
    out = {"value": steps * images / el, "unit": "images/s", "dtype": dtype_name, "images_per_step": images, "steps": steps,
           "warmup": warmup, "ms_per_step": 1e3 * el / steps}
    if roofline:
        out["roofline"] = roofline_leg(model, dev, dt, dtype_name, images, K, lat, prompts[0], centres)
    if roofline_bwd and opt_epochs > 1 and K > 0:
        out["roofline_bwd"] = roofline_bwd_leg(model, dev, dt, dtype_name, images, K, lat, prompts[0], centres)
    if opt_epochs:
        w0 = sampler.weight_init / max(K, 1)
        moved = float((r["W"] - w0).abs().max()) if K else 0.0
        assert K == 0 or opt_epochs < 2 or moved > 0.0, "the tracked epochs did not move the blend weights (zero gradient)"
        out.update(W_moved=moved, decoder_calibration={"mean_before": calib[0], "std_before": calib[1], "std_after": 0.25} if calib else None)
        if mode == "call":
            out.update(kept_calls=getattr(sampler, "last_kept_calls", None),
                       call_activation_gib_per_image=round(getattr(sampler, "_call_bytes_per_image", 0) / 2 ** 30, 2))
        out.update(opt_epochs=opt_epochs, recompute=mode, miopen_find=bool(find), loss="CLIP stand-in (sta.synth.SyntheticCLIP): real front-end, VAE decode "
                   "and backward through 2 x 51 UNet calls; the third epoch runs the fixed-weight path", losses=r.get("losses"))
    del sampler, model
    torch.cuda.empty_cache()
    return out


DUMP_SAMPLE = 4 << 20      # elements kept of an output larger than this (16 MB in float32; the bench's image is 50 M values)


def dump_outputs(path, result):
    """--dump-outputs: what a caller of the timed path receives from its last step (sampler.last_result of rank 0) as
    <path>/<name>.npy in float32: `x0` (the final latents, full), `W` (the blend weights, full), `losses` (weight optimisation
    only) and `image_sample` — the decoded, clamped images are larger than DUMP_SAMPLE, so they are stored as a fixed sample:
    the values at DUMP_SAMPLE indices of the flattened [I, 3, H, W] array drawn (sorted, with repetition) from a CPU generator
    seeded with 0, the same indices in every run with the same arguments. The inputs are seeded too, but the sampling path is not
    bitwise deterministic: two runs of one build on one MI355X agreed in W exactly and in x0 to 2.5e-3 of max|x0| (1.9e-3 in the
    mean), so two builds compare within such a tolerance. -> {file name: shape}"""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    written = {}
    for name in ("x0", "W", "image", "losses"):
        val = result.get(name)
        if val is None:
            continue
        t = torch.as_tensor(val).detach()
        if t.numel() > DUMP_SAMPLE:
            idx = torch.randint(t.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
            t, name = t.reshape(-1)[idx.to(t.device)], name + "_sample"
        arr = t.float().cpu().numpy()
        np.save(os.path.join(path, name + ".npy"), arr)
        written[name + ".npy"] = list(arr.shape)
    return written


_T0 = time.perf_counter()


def _phase(name):
    """Wall-clock log of the bench's phases on stderr (the JSON line on stdout stays alone)."""
    print("[bench %7.1f s] %s" % (time.perf_counter() - _T0, name), file=sys.stderr, flush=True)


def self_launch(n_ranks):
    """`python bench.py --gpus N` without a torch.distributed environment: start the N ranks here, one process per GPU, exactly as
    the documented launch line does (torch.distributed.run, rendezvous on 127.0.0.1, a free port). The ranks inherit stdout, so the
    ONE JSON line of rank 0 is this process's output; the exit code is non-zero if any rank failed (torchrun tears the others down)."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: what RCCL needs on this driver stack
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // n_ranks)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def dry_launch(a, rank, world, local):
    """--dry-launch: everything a multi-rank run does before its first sampler kernel — process group, model skeleton on every rank,
    weights on rank 0 only, the bucketed scatter + all-gather transfer, a checksum of what arrived, barrier, max-over-ranks — then
    the JSON line and out. On a GPU box it moves the real SD-v1 weights over RCCL; without GPUs (the CPU test suite) a
    reduced-width UNet over gloo."""
    import torch.distributed as dist
    from sta import parallel
    from sta.pipeline import build_sd_v1
    on_gpu = torch.cuda.is_available()
    dev = torch.device("cuda", 0 if a.share_gpu else local) if on_gpu else torch.device("cpu")
    dt = (torch.float16 if a.dtype == "fp16" else torch.bfloat16) if on_gpu else torch.float32
    over = None if on_gpu else dict(model_channels=32, num_heads=2, context_dim=64)
    model = build_sd_v1(dev, dt, with_vae=on_gpu, init_weights=(rank == 0), seed=0, unet_overrides=over,
                        channels_last=on_gpu and not a.nchw)
    if rank != 0:                                   # whatever to_empty left behind: make "nothing arrived" visible
        for t in model.state_dict().values():
            if torch.is_tensor(t) and t.is_floating_point():
                t.fill_(-7.0)
    t0 = time.perf_counter()
    nbytes = parallel.broadcast_module_(model, bucket_bytes=(512 << 20) if on_gpu else (1 << 20))
    if on_gpu:
        torch.cuda.synchronize()
    t_bcast = time.perf_counter() - t0
    # every rank must hold rank 0's bytes: compare a checksum of the whole state with rank 0's
    cks = torch.stack([t.double().sum() for _, t in sorted(model.state_dict().items()) if torch.is_tensor(t)]).sum().reshape(1).to(dev)
    mine = cks.clone()
    if world > 1:
        dist.broadcast(cks, src=0)
    ok = bool(torch.isfinite(mine).all()) and bool((mine == cks).all())
    oks = torch.tensor([1.0 if ok else 0.0], device=dev)
    if world > 1:
        dist.all_reduce(oks, op=dist.ReduceOp.MIN)
    parallel.barrier()
    el = parallel.max_over_ranks(time.perf_counter() - t0, dev)
    I = a.images_per_step
    shard = [((0 * world + r) * I + i) % 64 for r in range(world) for i in range(min(I, 2))]
    # what every rank would do next, gathered: the prompts of its step 0 (main()'s `mine(0)`), its MIOpen user-db copy, its device, the
    # rendezvous it saw — the first 8-GPU run of the driver must not be the first execution of any of this
    from sta.pipeline import use_shipped_miopen_db
    db = use_shipped_miopen_db(local)
    mine0 = [((0 * world + rank) * I + i) % 64 for i in range(I)]
    info = {"rank": rank, "local_rank": local, "device": str(dev), "prompts_step0": mine0, "miopen_user_db": db,
            "master": "%s:%s" % (os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT")), "pid": os.getpid()}
    infos = [info]
    if world > 1:
        infos = [None] * world
        dist.all_gather_object(infos, info)
    if rank == 0:
        print(json.dumps({"dry_launch": True, "n_gpus": world, "backend": dist.get_backend() if world > 1 else None, "scaling": a.scaling,
                          "images_per_step": I, "global_batch": world * I, "weights_identical_on_every_rank": bool(oks.item() == 1.0),
                          "weight_broadcast_bytes": nbytes, "weight_broadcast_s": round(t_bcast, 3), "elapsed_max_over_ranks_s": round(el, 3),
                          "first_prompts_of_step0": shard, "device": str(dev.type), "ranks": infos}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    if not bool(oks.item() == 1.0):
        raise SystemExit("dry launch: a rank does not hold rank 0's weights after the broadcast")


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        raise SystemExit(self_launch(a.gpus))
    from sta import parallel
    rank, world, local = parallel.init_from_env(backend="gloo" if a.share_gpu else None)
    if world != a.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d (run `python bench.py --gpus %d`, which starts its own ranks, or "
                         "torch.distributed.run --nproc-per-node %d)" % (a.gpus, world, a.gpus, a.gpus))
    if a.dry_launch:
        return dry_launch(a, rank, world, local)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    db_slot = local
    if a.share_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    from ldm.models.diffusion.plms import PLMSSampler
    from sta import lib
    from sta.pipeline import DEFAULT_CENTRES, build_sd_v1, conditionings, load_prompts, set_recompute, use_shipped_miopen_db
    lib.load()
    use_shipped_miopen_db(db_slot)      # per-rank copy of the shipped MIOpen find-db (before the first convolution)

    K, dt = a.objects, (torch.float16 if a.dtype == "fp16" else torch.bfloat16)
    ckpt_mode = None
    # rank 0 creates the (synthetic) frozen weights; everyone else receives them over RCCL/xGMI
    model = build_sd_v1(dev, dt, with_vae=True, init_weights=(rank == 0), seed=0, channels_last=(a.channels_last or a.opt_epochs == 0) and not a.nchw,
                        use_checkpoint=a.opt_epochs > 1)
    if a.opt_epochs > 1:
        ckpt_mode = set_recompute(model, a.checkpoint, a.images_per_step)
    t0 = time.perf_counter()
    nbytes = parallel.broadcast_module_(model)
    torch.cuda.synchronize()
    t_bcast = time.perf_counter() - t0

    if a.fp8:
        from sta import fp8
        fp8.convert_transformer_linears_(model.model.diffusion_model)
    prompts = load_prompts(64)
    I = a.images_per_step
    # Step j of rank r samples prompts (j * world + r) * I ... + I - 1 (mod 64): the I prompts of one UNet call are distinct and
    # the ranks of a step take disjoint slices of the list. --scaling strong: I = 64 / world, a step is exactly the 64-prompt batch
    # of BASELINE configs[3], rank r holding prompts r * I .. (the reference loops over them one by one, txt2img-gpt.py:305-341).
    mine = lambda j: [((j * world + rank) * I + i) % len(prompts) for i in range(I)]
    lat = a.res // 8
    centres = [list(c) for c in DEFAULT_CENTRES[:K]]
    loss_model = None
    if a.opt_epochs > 0:
        from ldm.models.diffusion.plms import DCLIPLoss
        from sta.synth import SyntheticCLIP
        loss_model = DCLIPLoss(SyntheticCLIP().to(dev))
    sampler = PLMSSampler(model, opt_epochs=a.opt_epochs, loss_model=loss_model, use_graph=not a.no_graph, save_images=False)

    g = torch.Generator(device=dev).manual_seed(1)                          # seed = 1 for every prompt (txt2img-gpt.py:304)
    x_T1 = torch.randn([1, 4, lat, lat], generator=g, device=dev)

    def one_step(j):
        """One step = I independent prompts of this rank's shard sampled together (I = 1: the reference's loop body)."""
        recs = [prompts[i] for i in mine(j)]
        names = [(r["objects"] + ["object"] * K)[:K] for r in recs]
        conds = [conditionings(model, r["prompt"], nm, dt) for r, nm in zip(recs, names)]
        if I == 1:
            uc, c, local_c = conds[0]
            sampler.sample(S=a.ddim_steps, conditioning=c, batch_size=1, shape=[4, lat, lat], verbose=False,
                           unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0, x_T=x_T1, text_index=0,
                           curr_text=recs[0]["prompt"], bboxs_curr=centres, seed=1, prompt_idx=0, object_names=names[0],
                           local_conditionings=local_c)
        else:
            sampler.sample_batch(S=a.ddim_steps, shape=[4, lat, lat], conditionings=[c[1] for c in conds],
                                 unconditional_conditionings=[c[0] for c in conds], bboxs=[centres] * I, object_names=names,
                                 local_conditionings=[c[2] for c in conds], curr_texts=[r["prompt"] for r in recs],
                                 x_T=x_T1.expand(I, -1, -1, -1), unconditional_guidance_scale=7.5, seed=1)
        return sampler.last_result

    _phase("model built")
    for j in range(a.warmup):
        one_step(j)
    _phase("warm-up done (MIOpen solver search, graph capture)")
    parallel.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(a.steps):
        r = one_step(a.warmup + j)
    torch.cuda.synchronize()
    parallel.barrier()
    elapsed = time.perf_counter() - t0
    elapsed = parallel.max_over_ranks(elapsed, dev)
    assert torch.isfinite(r["x0"]).all() and r["image"] is not None and r["x0"].shape[0] == I

    _phase("timed region done")
    peak_gb = torch.cuda.max_memory_allocated() / 2 ** 30
    if rank != 0:
        return
    if a.dump_outputs:
        _phase("outputs of the last timed step written: %s" % dump_outputs(a.dump_outputs, r))
    out = {
        "metric": "images/sec at 512x512, 50 PLMS steps, 2 objects", "value": world * a.steps * I / elapsed, "unit": "images/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * elapsed / a.steps,
        "higher_is_better": True, "scaling": a.scaling, "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": "SD-v1-4 UNet+VAE (synthetic weights), %dx%d, %d PLMS steps (%d CFG UNet calls), %d objects, "
                               "%s" % (a.res, a.res, a.ddim_steps, a.ddim_steps + 1, K,
                                       "fixed blend weights (BASELINE configs[1])" if a.opt_epochs == 0 else
                                       "%d weight-optimisation epochs, CLIP stand-in loss (BASELINE configs[2])" % a.opt_epochs),
                   "global_batch": world * I, "images_per_step": I, "prompts": "first 64 of datasets/mscoco.txt; step j of rank r takes prompts ((j * %d + r) * %d + i) %% 64" % (world, I),
                   "parallelism": "prompt-parallel dp%d" % world + (" (TEST MODE: all ranks on GPU 0, collectives over gloo)" if a.share_gpu else ""), "hipgraph": not a.no_graph,
                   "linear_weights": "e4m3 (sta.fp8)" if a.fp8 else a.dtype, "trunk_layout": "NHWC" if (a.channels_last or a.opt_epochs == 0) and not a.nchw else "NCHW",
                   "trunk_kernels": _trunk_kernels(a),
                   "weight_broadcast_s": round(t_bcast, 3), "weight_broadcast_bytes": nbytes,
                   "peak_hbm_gib": round(peak_gb, 1), **({"recompute": ckpt_mode} if a.opt_epochs > 1 else {})},
    }
    out["config"]["selfattn_optimistic"] = _selfattn_optimistic_state()
    from sta import ops as _ops
    # the cross-attention head-pair kernel's optimistic softmax over the whole run: wave-level context evaluations, how many fell back
    # to the standard softmax, launches that sat the optimistic path out — the level-0 roofline figure belongs to the optimistic path
    # only if fallbacks and launches_sat_out are (near) 0; `hostile_logits` beside `roofline` shows the other regime
    out["config"]["xattn_optimistic"] = _ops.proj_stats_summary()
    if not a.full:          # a plain run ends with the headline line: what follows is measured under --full only
        print(json.dumps(out))
        return
    if not a.no_roofline:
        out["roofline"] = roofline_leg(model, dev, dt, a.dtype, I, K, lat, prompts[mine(0)[0]], centres)
    if not a.no_roofline and a.opt_epochs > 1 and K > 0:
        out["roofline_bwd"] = roofline_bwd_leg(model, dev, dt, a.dtype, I, K, lat, prompts[mine(0)[0]], centres)
    if not a.no_roofline and not a.no_hostile and a.opt_epochs == 0 and a.res == 512:
        try:
            out["hostile_logits"] = hostile_logits_leg(dev, a.dtype, I, K, lat)
        except Exception as e:          # noqa: BLE001
            out["hostile_logits"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
    _phase("roofline leg done")
    if world == 1 and not a.no_side_runs and a.opt_epochs == 0:
        # reported beside the headline, never part of `value`: the other 16-bit type, and BASELINE configs[2]
        def guarded(fn):      # a side leg that fails (e.g. out of memory on a smaller box) is reported, it does not take the headline line with it
            try:
                return fn()
            except Exception as e:          # noqa: BLE001
                torch.cuda.empty_cache()
                return {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        if not a.no_other_dtype:
            # the same workload in the other 16-bit type on an equal footing: the headline's steps and warm-up, its own roofline block
            out["other_dtype"] = guarded(lambda: side_run(dev, "bf16" if a.dtype == "fp16" else "fp16", 0, I, a.steps, a.warmup, a.res, a.ddim_steps, K,
                                                          roofline=not a.no_roofline))
        # MIOpen's per-shape solver search for the backward convolutions of the UNet and the VAE decoder costs ~10 min on a
        # fresh box; the shipped user find-db (sta/data/miopen_userdb) holds them for fp16 at 512^2, other cases run in
        # immediate mode (no search, slower solvers)
        find = a.dtype == "fp16" and a.res == 512
        torch.backends.cudnn.benchmark = find
        if a.res == 512:
            # BASELINE configs[3] at ITS OWN per-GPU size: 64 prompts over 8 GPUs = 8 prompts per UNet call on this GPU (what
            # `--gpus 8 --scaling strong` gives every rank), same steps / warm-up as the headline, with the per-launch table at that
            # size — the N = 1 anchor of the strong-scaling line beside the weak one (scripts/txt2img-gpt.py:305-341 is the loop sharded)
            out["config3_shard"] = guarded(lambda: side_run(dev, a.dtype, 0, 8, a.steps, a.warmup, a.res, a.ddim_steps, K, roofline=not a.no_roofline))
            out["config3_shard"]["config"] = ("BASELINE configs[3] per-GPU shard: 64 mscoco prompts / 8 GPUs = 8 prompts per step on this GPU "
                                              "(--scaling strong at world 8), %d PLMS steps, %d objects, fixed weights" % (a.ddim_steps, K))
        if a.res == 512 and not a.no_config5:
            # BASELINE configs[4] on ONE GPU (the per-GPU work of its 8-GPU line): VSR-style prompts at 768x768, 4 object boxes, 50 steps, in 16 bit
            # and with e4m3 Linear weights; 4 prompts per step, 2 timed steps after 1 warm-up, MIOpen in immediate mode (no find-db for these
            # shapes), each with its own cross-attention launch table (`roofline`). K = 4: level 0 takes the one-head-per-workgroup
            # projection-fused kernel (the head-pair kernel holds K <= 2), level 1 the locals-from-L2 kernel.
            torch.backends.cudnn.benchmark = False
            out["config5"] = {"config": "BASELINE configs[4] on one GPU: 768x768, %d PLMS steps, 4 objects, fixed weights, 4 prompts per step" % a.ddim_steps,
                              a.dtype: guarded(lambda: side_run(dev, a.dtype, 0, 4, 2, 1, 768, a.ddim_steps, 4, find=False, roofline=not a.no_roofline)),
                              "fp8_linear_weights": guarded(lambda: side_run(dev, a.dtype, 0, 4, 2, 1, 768, a.ddim_steps, 4, find=False, fp8_linears=True))}
            torch.backends.cudnn.benchmark = find
        out["weight_optimisation"] = guarded(lambda: side_run(dev, a.dtype, 3, 16 if a.res <= 512 else 2, 3, 1, a.res, a.ddim_steps, K, find=find,
                                                              roofline_bwd=not a.no_roofline))
        out["weight_optimisation"]["config"] = "BASELINE configs[2]: %dx%d, %d PLMS steps, %d objects, 3 epochs of per-step blend-weight optimisation" % (
            a.res, a.res, a.ddim_steps, K)
    _phase("side runs done")
    if not a.no_cpu_baseline and world == 1:
        out["cpu_baseline"] = cpu_baseline(a.res, a.ddim_steps, K, a.cpu_calls)
    _phase("cpu baseline done")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
