"""img2img on the MI355X: the encoder's stride-2 Downsample kernel and the fused encode step (csrc/sta_encode.hip) against fp32 /
float64 restatements, the full-width encoder on the HIP path against the same module in fp32 and against the reference's golden, and
the DDIM decode's graph replay and prompt batching."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402

G = gi.GOLDEN
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# the SD-v1 encoder's three Downsample inputs (H = W, C) at 512^2 and 768^2, and at the golden's 128^2
S2_SHAPES = [(512, 128), (256, 256), (128, 512), (768, 128), (384, 256), (192, 512), (128, 128), (64, 256), (32, 512)]


def _close(got, ref, dtype, k=2.0):
    err = (got.float().cpu() - ref.float().cpu()).abs()
    tol = k * EPS[dtype] * (1.0 + ref.float().cpu().abs())
    assert (err <= tol).all(), "max err %.4g at tol %.4g" % (err.max().item(), tol.max().item())


@pytest.mark.parametrize("HW,C", S2_SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_conv3x3_s2_nhwc_vs_fp32(HW, C, dtype):
    """sta_conv3x3_s2_nhwc against an fp32 F.pad + conv2d(stride 2) of the same 16-bit operands, B in {1, 2, 3}, with and without bias;
    fp32 accumulation: the error is the 16-bit rounding of the result (the stride-1 kernel's bound). The epilogue statistics equal
    the fp32 per-channel sums of the stored values."""
    from sta import fused, lib
    for B in (1, 2, 3):
        g = torch.Generator().manual_seed(HW + C + B)
        x = torch.randn(B, C, HW, HW, generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
        w = (torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(dtype).cuda()
        bias = (0.5 * torch.randn(C, generator=g)).to(dtype).cuda()
        assert lib.load().sta_conv3x3_s2_nhwc_supported(B, HW, HW, C, C) == 1
        with torch.no_grad():
            wp = fused.pack_conv3x3_weight(w)
            for bb in (None, bias):
                ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), None if bb is None else bb.float(), stride=2)
                got = fused.conv3x3_s2_nhwc(x, wp, C, bias=bb, stats=bb is not None)
                torch.cuda.synchronize()
                assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
                _close(got, ref, dtype)
                if bb is not None:
                    st = fused._producer_stats(got)
                    yf = got.float()
                    want = torch.stack([yf.sum(dim=(2, 3)), (yf * yf).sum(dim=(2, 3))], dim=-1)
                    torch.testing.assert_close(st, want, rtol=1e-4, atol=1e-2)
        del x, w, ref, got
        torch.cuda.empty_cache()


def test_conv3x3_s2_unsupported_shapes_go_to_the_fallback():
    """Shapes outside the supported set are refused by the C-ABI; the Downsample module then runs F.pad + the library convolution."""
    from ldm.models.autoencoder import Downsample
    from sta import fused, lib
    L = lib.load()
    for H, W, Cin, Cout in [(48, 48, 128, 128), (64, 64, 96, 128), (64, 64, 128, 160), (64, 64, 320, 320), (30, 64, 128, 128)]:
        assert L.sta_conv3x3_s2_nhwc_supported(2, H, W, Cin, Cout) == 0
    x = torch.zeros(1, 128, 64, 64, dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
    rc = L.sta_conv3x3_s2_nhwc(x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, x.data_ptr(), 0, 1, 48, 48, 128, 128, lib.STA_F16, 0)
    assert rc != 0 and b"unsupported" in L.sta_last_error()
    m = Downsample(96).half().cuda().to(memory_format=torch.channels_last)
    xi = torch.randn(2, 96, 64, 64, device="cuda").half().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        assert not fused.conv3x3_s2_supported(xi, m.conv.weight)
        torch.testing.assert_close(m(xi), m.conv(F.pad(xi, (0, 1, 0, 1))), rtol=0, atol=0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_vae_encode_step_vs_float64(dtype):
    """sta_vae_encode_step against a float64 restatement of quant_conv + posterior sample + stochastic_encode, with logvar pushed
    beyond both clamp limits; xin is bitwise the 16-bit CFG pair of x (sta.solver._pair(x).to(dtype))."""
    from sta import fused, solver
    g = torch.Generator().manual_seed(3)
    B, hh = 3, 24
    h = torch.randn(B, 8, hh, hh, generator=g).to(dtype)
    h[:, 4:, :4] = 40.0            # logvar above 20 ...
    h[:, 4:, 4:8] = -40.0          # ... and below -30 (through an identity-ish quant_conv)
    qw = (torch.eye(8) + 0.01 * torch.randn(8, 8, generator=g)).reshape(8, 8, 1, 1)
    qb = 0.1 * torch.randn(8, generator=g)
    n_post, n_enc = torch.randn(B, 4, hh, hh, generator=g), torch.randn(B, 4, hh, hh, generator=g)
    sf, sa, s1m = 0.18215, 0.5, 0.8660254
    hd = h.cuda().contiguous(memory_format=torch.channels_last)
    x, z0, xin = fused.vae_encode_step(hd, qw.cuda(), qb.cuda(), n_post.cuda(), n_enc.cuda(), sf, sa, s1m, want_z0=True)
    torch.cuda.synchronize()
    m = torch.einsum("oi,bihw->bohw", qw.reshape(8, 8).double(), h.double()) + qb.double()[None, :, None, None]
    lv = m[:, 4:].clamp(-30.0, 20.0)
    assert (m[:, 4:] > 20).any() and (m[:, 4:] < -30).any()
    z_ref = sf * (m[:, :4] + torch.exp(0.5 * lv) * n_post.double())
    x_ref = np.float32(sa) * z_ref + np.float32(s1m) * n_enc.double()
    for got, ref in ((z0, z_ref), (x, x_ref)):
        err = (got.cpu().double() - ref).abs()
        assert (err <= 1e-5 * (1.0 + ref.abs())).all(), err.max().item()
    assert torch.equal(xin, solver._pair(x).to(dtype))


def _encoder(dtype, seed=5):
    from ldm.models.autoencoder import AutoencoderKL
    from sta import pipeline, synth
    vae = AutoencoderKL().add_encoder()
    part = pipeline.encoder_part(vae)
    synth.seeded_fill_(part, seed)
    return vae


def _count_hip(monkeypatch):
    from sta import fused
    calls = {"s1": 0, "s2": 0}
    f1, f2 = fused.conv3x3_nhwc, fused.conv3x3_s2_nhwc

    def c1(*a, **k):
        calls["s1"] += 1
        return f1(*a, **k)

    def c2(*a, **k):
        calls["s2"] += 1
        return f2(*a, **k)
    monkeypatch.setattr(fused, "conv3x3_nhwc", c1)
    monkeypatch.setattr(fused, "conv3x3_s2_nhwc", c2)
    return calls


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_full_width_encoder_hip_path_vs_fp32(dtype, monkeypatch):
    """The SD-v1 encoder (synthetic weights) at 512^2, B = 2, NHWC 16-bit on the HIP path against the same module in fp32; every
    stride-1 3x3 convolution of the trunk and all three Downsample convolutions took the HIP kernels."""
    calls = _count_hip(monkeypatch)
    vae = _encoder(dtype)
    g = torch.Generator().manual_seed(1)
    img = (torch.rand(2, 3, 512, 512, generator=g) * 2 - 1)
    with torch.no_grad():
        ref = vae.float().cuda().encode_moments_input(img.cuda()).float().cpu()
        vh = vae.to(dtype).to(memory_format=torch.channels_last)
        got = vh.encode_moments_input(img.cuda()).float().cpu()
    assert calls == {"s1": 20, "s2": 3}, calls          # 2 x 2 per level x 4 levels + 2 x 2 in the middle; conv_in / conv_out: library
    err = (got - ref).abs()
    # 16-bit activations through ~26 layers: relative to the tensor's scale
    assert err.max().item() <= 64 * EPS[dtype] * ref.abs().max().item(), (err.max().item(), ref.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_encoder_vs_reference_golden_with_gates_lowered(dtype, monkeypatch):
    """The encoder + posterior at the golden's 128^2 x 2 geometry (tools/gen_img2img_golden.py): with the work-item gates lowered every
    convolution the kernels support takes the HIP path; h, the moments and z against the reference's fp32 values."""
    from sta import fused
    monkeypatch.setattr(fused, "CONV_MIN_ITEMS", 1)
    monkeypatch.setattr(fused, "CONV_S2_MIN_ITEMS", 1)
    calls = _count_hip(monkeypatch)
    gz = np.load(os.path.join(G, "vae_encoder.npz"))
    vae = _encoder(dtype, int(gz["seed"])).to(dtype).cuda().to(memory_format=torch.channels_last)
    x = torch.from_numpy(gz["image_u8"]).float() / 255.0 * 2.0 - 1.0
    with torch.no_grad():
        post = vae.encode(x.cuda())
        z = post.sample(noise=torch.from_numpy(gz["n_post"]))
    assert calls == {"s1": 20, "s2": 3}, calls
    for got, key in ((post.parameters, "moments"), (z, "z")):
        ref = torch.from_numpy(gz[key])
        err = (got.float().cpu() - ref).abs()
        assert err.max().item() <= 64 * EPS[dtype] * ref.abs().max().item(), (key, err.max().item(), ref.abs().max().item())


def _small_model(dtype):
    from sta.pipeline import build_sd_v1
    return build_sd_v1("cuda", dtype, with_vae=False, unet_overrides=dict(model_channels=64))


@pytest.mark.parametrize("dtype", [torch.float16])
def test_decode_graph_replay_equals_eager_and_batch_equals_single(dtype):
    """A fixed-weight DDIM decode (S = 10, t_start = 6, K = 2) replayed from the captured hipGraph against the eager decode (the
    samplers' graph bound), a given first-call xin (what the fused encode step writes) against the pair built from x, and
    decode_batch of two prompts against each decoded alone."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta.pipeline import conditionings
    model = _small_model(dtype)
    centres, names = [[0.3, 0.4], [0.7, 0.6]], ["cat", "dog"]
    prompts = ["a cat left of a dog", "a dog right of a cat"]
    conds = [conditionings(model, p, names, dtype) for p in prompts]
    g = torch.Generator().manual_seed(7)
    lat = [torch.randn(1, 4, 32, 32, generator=g).cuda() for _ in prompts]
    outs = {}
    for graph in (False, True):
        s = DDIMSampler(model, opt_epochs=0, save_images=False, use_graph=graph)
        s.make_schedule(10, ddim_eta=0.0, verbose=False)
        uc, c, local = conds[0]
        outs[graph] = s.decode(lat[0], c, 6, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, bboxs_curr=centres,
                               object_names=names, local_conditionings=local, curr_text=prompts[0]).clone()
    a, b = outs[False].float(), outs[True].float()
    assert (a - b).abs().max() <= 0.02 * a.abs().max(), ((a - b).abs().max(), a.abs().max())     # test_solver_gpu's graph bound
    s = DDIMSampler(model, opt_epochs=0, save_images=False, use_graph=True)
    s.make_schedule(10, ddim_eta=0.0, verbose=False)
    uc, c, local = conds[0]
    xin = torch.stack([lat[0], lat[0]], 1).reshape(2, 4, 32, 32).to(dtype)
    got = s.decode(lat[0], c, 6, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, bboxs_curr=centres, object_names=names,
                   local_conditionings=local, curr_text=prompts[0], xin=xin)
    assert (got.float() - b).abs().max() <= 0.02 * b.abs().max()
    # the first call follows the given xin, not a pair rebuilt from x: a different xin moves the result well beyond that bound
    other = torch.randn(1, 4, 32, 32, generator=g).cuda()
    alt = s.decode(lat[0], c, 6, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, bboxs_curr=centres, object_names=names,
                   local_conditionings=local, curr_text=prompts[0], xin=torch.stack([other, other], 1).reshape(2, 4, 32, 32).to(dtype))
    assert (alt.float() - b).abs().max() > 0.1 * b.abs().max()
    single = []
    for (uc, c, local), x in zip(conds, lat):
        single.append(s.decode(x, c, 6, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, bboxs_curr=centres,
                               object_names=names, local_conditionings=local).clone())
    batch = s.decode_batch(torch.cat(lat), [c for _, c, _ in conds], [uc for uc, _, _ in conds], [centres] * 2, [names] * 2,
                           [local for _, _, local in conds], 6, curr_texts=prompts)
    for i in range(2):
        err = (batch[i] - single[i][0]).abs().max().item()
        assert err <= 2e-2 * single[i].abs().max().item(), (i, err)


def test_encode_step_then_decode_equals_stochastic_encode_then_decode():
    """DDIMSampler.encode_step (one sta_vae_encode_step from the encoder output) + decode(xin=...) against the unfused chain:
    quant_conv -> posterior sample -> get_first_stage_encoding -> stochastic_encode -> decode, with the same noises."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta import solver
    from sta.pipeline import build_sd_v1, conditionings
    dtype = torch.float16
    model = build_sd_v1("cuda", dtype, unet_overrides=dict(model_channels=64), with_encoder=True)
    vae = model.first_stage_model
    vae.encoder.to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(11)
    img = (torch.rand(1, 3, 256, 256, generator=g) * 2 - 1).cuda()
    n_post, n_enc = torch.randn(1, 4, 32, 32, generator=g), torch.randn(1, 4, 32, 32, generator=g).cuda()
    s = DDIMSampler(model, opt_epochs=0, save_images=False, use_graph=True)
    s.make_schedule(10, ddim_eta=0.0, verbose=False)
    t_enc = 6
    with torch.no_grad():
        h = vae.encode_moments_input(img)
        x, z0, xin = s.encode_step(h, vae, t_enc, n_post, n_enc, want_z0=True)
        post = vae.encode(img)
        z_ref = model.scale_factor * post.sample(noise=n_post).float()
        x_ref = s.stochastic_encode(z_ref, torch.tensor([t_enc]), noise=n_enc)
    for got, ref in ((z0, z_ref), (x, x_ref)):
        err = (got - ref).abs().max().item()
        assert err <= 4 * 2.0 ** -11 * (1.0 + ref.abs().max().item()), err       # quant_conv in fp32 here, in fp16 on the unfused side
    assert torch.equal(xin, solver._pair(x).to(dtype))
    uc, c, local = conditionings(model, "a cat left of a dog", ["cat", "dog"], dtype)
    kw = dict(unconditional_guidance_scale=7.5, unconditional_conditioning=uc, bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], object_names=["cat", "dog"],
              local_conditionings=local)
    a = s.decode(x, c, t_enc, xin=xin, **kw).clone()
    b = s.decode(x_ref, c, t_enc, **kw).clone()
    assert (a - b).abs().max() <= 0.02 * b.abs().max()


@pytest.mark.parametrize("dtype,tol_max,tol_mean", [(torch.float16, 0.01, 0.005), (torch.bfloat16, 0.03, 0.02)])
@pytest.mark.parametrize("tag", ["eta0", "eta05"])
def test_img2img_ddim_trajectory_vs_reference_golden(tag, dtype, tol_max, tol_mean):
    """The reference's img2img DDIM (tests/golden/ddim_img2img.npz) on the GPU with the fused kernels: the final x within the DDIM GPU
    bounds of tests/test_solver_gpu.py (fp16 max 1 % / mean 0.5 %, bf16 3 % / 2 % of max|x| / mean|x|)."""
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from tests.test_img2img_cpu import _golden_model, run_img2img_golden
    g = np.load(os.path.join(G, "ddim_img2img.npz"), allow_pickle=False)
    model, _ = _golden_model()
    model = LatentDiffusion(unet_config=model.model.diffusion_model.to("cuda", dtype)).cuda()
    for p in model.parameters():
        p.requires_grad_(False)
    z, x, _, _ = run_img2img_golden(model, g, tag, "cuda")
    np.testing.assert_array_equal(z.cpu().numpy(), g[tag + "_z_enc"])
    ref = g[tag + "_x"]
    err = np.abs(x.float().cpu().numpy() - ref)
    assert err.max() <= tol_max * np.abs(ref).max(), (err.max(), np.abs(ref).max())
    assert err.mean() <= tol_mean * np.abs(ref).mean(), (err.mean(), np.abs(ref).mean())


@pytest.mark.parametrize("form", ["file", "dir"])
def test_img2img_script_synthetic_end_to_end(form, tmp_path):
    """scripts/img2img.py --synthetic: 10 DDIM steps, strength 0.5, K = 2 from a --layout, fixed weights, a generated 256^2 PNG as one
    --init-img file or a directory with one image per prompt; writes one image per prompt of the input's size, named as txt2img names them."""
    import json as _json
    import subprocess
    import sys
    from PIL import Image
    rng = np.random.default_rng(0)
    if form == "file":
        init = str(tmp_path / "in.png")
        Image.fromarray(rng.integers(0, 255, (256, 256, 3), dtype=np.uint8)).save(init)
    else:
        init = str(tmp_path / "imgs")
        os.makedirs(init)
        for i in range(2):
            Image.fromarray(rng.integers(0, 255, (256, 256, 3), dtype=np.uint8)).save(os.path.join(init, "%d.png" % i))
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("a cat left of a dog\na dog right of a cat\n")
    layout = tmp_path / "layout.json"
    layout.write_text(_json.dumps({"0": {"cat": [0.3, 0.4], "dog": [0.7, 0.6]}, "1": {"dog": [0.3, 0.4], "cat": [0.7, 0.6]}}))
    out = tmp_path / "out"
    root = os.path.dirname(G.rstrip("/")).rsplit("/tests", 1)[0]
    script = os.path.join(root, "diffusion-spacetime-attn_amd", "scripts", "img2img.py")
    env = dict(os.environ, STA_CONV_FIND="0")
    r = subprocess.run([sys.executable, script, "--synthetic", "--init-img", init, "--from-file", str(prompts), "--layout", str(layout),
                        "--ddim_steps", "10", "--strength", "0.5", "--opt_epochs", "0", "--outdir", str(out), "--batch_prompts", "2"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for i in range(2):
        path = out / ("final0_s42_index_%d.png" % i)
        assert path.exists(), sorted(os.listdir(out))
        assert Image.open(path).size == (256, 256)
