"""sta_xattn_token_maps on the GPU: against the float64 oracle's attention maps, its structural guarantees (bit-reproducible,
image-count independent, exact accumulation, bounds), the capturing block against the reference's own maps, and the samplers."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from oracle import xattn_oracle as orc  # noqa: E402
from sta.synth import seeded_fill_  # noqa: E402

G = gi.GOLDEN
M = 77


def _qk(N, C, K, dtype, I=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(2 * I, N, C, generator=g).to(dtype)
    k = (torch.randn(I * (K + 2), M, C, generator=g) * 0.7).to(dtype)
    v = torch.randn(I * (K + 2), M, C, generator=g).to(dtype)
    return q, k, v


def _readouts(K, R, seed=1):
    """The row mix of the issue: one-hot at token 0, at token 76 (the last key before the padding) and in the middle, a uniform
    1/77 row, a random signed row, an all-ones row; contexts so that several readouts share one and every context kind occurs.
    Further rows (up to R) are random signed rows walking over all contexts."""
    g = torch.Generator().manual_seed(seed)
    last = K + 1
    sel = [0, 1, 1, min(2, last), last, 1]
    w = torch.zeros(6, M)
    w[0, 0] = 1.0
    w[1, M - 1] = 1.0
    w[2, M // 2] = 1.0
    w[3] = 1.0 / M
    w[4] = torch.randn(M, generator=g)
    w[5] = 1.0
    while len(sel) < R:
        sel.append(len(sel) % (K + 2))
        w = torch.cat([w, torch.randn(1, M, generator=g)])
    return sel, w


def _expected(q, k, v, sel, w, heads, K, I=1):
    """einsum(maps.mean(heads), w) with the oracle's maps in float64 on the 16-bit-rounded inputs -> [I, R, N]."""
    N, C = q.shape[1], q.shape[2]
    scale = (C // heads) ** -0.5
    w = (w if w.dim() == 3 else w.unsqueeze(0).expand(I, -1, -1)).double()
    out = []
    for i in range(I):
        s = slice(i * (K + 2), (i + 1) * (K + 2))
        _, maps = orc.fused_xattn(q[2 * i:2 * i + 2].double(), k[s].double(), v[s].double(), torch.zeros(K, N, dtype=torch.bool),
                                  torch.zeros(K, dtype=torch.float64), heads, scale, want_maps=True)
        out.append(torch.einsum("rnm,rm->rn", maps.mean(1)[sel], w[i]))
    return torch.stack(out)


def _launch(q, k, v, sel, w, heads, I=1, **kw):
    from sta import attnmaps, ops
    packed = ops.pack_kv(k.cuda(), v.cuda(), heads, n_img=I)
    out = attnmaps.token_maps(q.cuda(), packed, sel, w.cuda(), (q.shape[2] // heads) ** -0.5, **kw)
    torch.cuda.synchronize()
    return out


SHAPES = [
    # N, C, heads, K, R
    (64, 64, 8, 1, 6),       # d = 8
    (256, 320, 8, 2, 6),     # d = 40
    (64, 640, 8, 2, 6),      # d = 80
    (256, 1280, 8, 2, 6),    # the default capture shape, d = 160
    (100, 128, 4, 3, 6),     # ragged N, d = 32
    (256, 192, 8, 0, 6),     # no objects: contexts 0 and 1 only
    (64, 320, 8, 8, 16),     # R = 16 (five readouts on context 1: two work groups of one context)
]


@pytest.mark.parametrize("N,C,heads,K,R", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_token_maps_match_oracle(N, C, heads, K, R, dtype):
    """Tolerance 1e-4 max(1, sum |w|) absolute: the bound tests/test_kernel_gpu.py holds the same softmax's maps to, which a head
    mean cannot exceed. The all-ones row must give 1 at every pixel within it (the padded keys 77..79 are excluded)."""
    q, k, v = _qk(N, C, K, dtype)
    sel, w = _readouts(K, R)
    assert len(sel) == R
    got = _launch(q, k, v, sel, w, heads).cpu().double()
    ref = _expected(q, k, v, sel, w, heads, K)
    assert got.shape == ref.shape == (1, R, N)
    tol = 1e-4 * torch.clamp(w.abs().sum(1).double(), min=1.0)
    err = (got - ref).abs().amax(dim=(0, 2))
    print("N=%d C=%d K=%d %s: max err / tol per readout %s" % (N, C, K, dtype, (err / tol).tolist()))
    assert (err <= tol).all(), (err, tol)
    assert ((got[0, 5] - 1.0).abs() <= 1e-4 * M).all(), (got[0, 5] - 1.0).abs().max()


def test_images_are_independent_and_launches_reproducible():
    """n_img = 3 equals three one-image launches bitwise (per-image weights), and two identical launches are bit-identical."""
    N, C, heads, K, I = 100, 128, 4, 3, 3
    q, k, v = _qk(N, C, K, torch.float16, I=I, seed=2)
    sel, w0 = _readouts(K, 8)
    w = torch.stack([w0, w0.flip(0), 0.5 * w0])
    three = _launch(q, k, v, sel, w, heads, I=I)
    again = _launch(q, k, v, sel, w, heads, I=I)
    assert torch.equal(three, again)
    for i in range(I):
        s = slice(i * (K + 2), (i + 1) * (K + 2))
        one = _launch(q[2 * i:2 * i + 2], k[s], v[s], sel, w[i], heads)
        assert torch.equal(one[0], three[i]), i
    err = (three.cpu().double() - _expected(q, k, v, sel, w, heads, K, I)).abs().max()
    assert err <= 1e-4 * w.abs().sum(-1).max().clamp(min=1.0), err


@pytest.mark.parametrize("N,C,heads,K", [(100, 128, 4, 3), (256, 1280, 8, 2)])
def test_accumulate_is_old_plus_fresh_and_nothing_outside_out_is_touched(N, C, heads, K):
    """accumulate = 1 on a filled buffer equals old + fresh bitwise; every pixel of the ragged tail is written; a guard band of a
    known pattern on both sides of `out` stays as it was."""
    from sta import attnmaps, ops
    q, k, v = _qk(N, C, K, torch.bfloat16, seed=3)
    sel, w = _readouts(K, 6)
    R, guard = len(sel), 4096
    packed = ops.pack_kv(k.cuda(), v.cuda(), heads)
    scale = (C // heads) ** -0.5
    flat = torch.full((guard + R * N + guard,), -12345.0, device="cuda")
    out = flat[guard:guard + R * N].view(1, R, N)
    attnmaps.token_maps(q.cuda(), packed, sel, w.cuda(), scale, out=out)
    fresh = out.clone()
    assert (fresh != -12345.0).all()                                            # written everywhere, the tail tile included
    assert (flat[:guard] == -12345.0).all() and (flat[guard + R * N:] == -12345.0).all()
    old = torch.randn(1, R, N, device="cuda")
    out.copy_(old)
    attnmaps.token_maps(q.cuda(), packed, sel, w.cuda(), scale, out=out, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(out, old + fresh)
    assert (flat[:guard] == -12345.0).all() and (flat[guard + R * N:] == -12345.0).all()


# ---------------------------------------------------------------------------------------------------
# the capturing block against the reference's own maps
# ---------------------------------------------------------------------------------------------------
def _block(name, dtype):
    from ldm.modules.attention import BasicTransformerBlock
    g = np.load(os.path.join(G, "block_%s.npz" % name), allow_pickle=False)
    dim, C, heads, K, seed = (int(g[k]) for k in ("dim", "C", "heads", "K", "seed"))
    x, context, local_ctx = gi.block_inputs(dim, C, K, seed, gi.load_uncond())
    blk = BasicTransformerBlock(C, heads, C // heads, context_dim=768, checkpoint=False)
    seeded_fill_(blk, seed)
    blk = blk.to("cuda", dtype)
    for p in blk.parameters():
        p.requires_grad_(False)
    centres = [list(c) for c in g["centres"]]

    def run(b=blk):
        with torch.no_grad():
            return b(x.cuda().to(dtype), context=context.cuda().to(dtype), time=torch.tensor(981),
                     coef=torch.from_numpy(g["coef"]).cuda(), bboxs_curr=centres)
    return g, blk, [c.cuda() for c in local_ctx], centres, dim, K, run


def _block_readouts(K):
    """Per context a one-hot row (a different token each) and a uniform row: R = 2 (K + 2) <= 12."""
    sel = [c for c in range(K + 2)] * 2
    w = torch.zeros(len(sel), M)
    for c in range(K + 2):
        w[c, (5 * c) % M] = 1.0
        w[K + 2 + c] = 1.0 / M
    return sel, w


@pytest.mark.parametrize("name", ["d40", "d80", "d160", "d8k4"])
@pytest.mark.parametrize("dtype,tol", [(torch.float16, 1e-3), (torch.bfloat16, 8e-3)])
def test_block_capture_vs_reference_maps(name, dtype, tol, monkeypatch):
    """The readouts a capturing PRODUCT block records (16-bit end to end) against the head mean of the reference's fp32 maps at the
    fixture's 32 pixels, within the project's stated map bounds (fp16 1e-3, bf16 8e-3; the rows weigh sum |w| = 1).
    d160: the block output with capture is bit-identical to the output without (q exists anyway). d40: the capturing block leaves
    the projection-fused launch for the to_q GEMM + blend path and stays inside the golden bound of its file, while a second block
    that does not capture still takes the projection-fused launch."""
    from sta import attnmaps, ops, prompt_state
    if name == "d40":
        monkeypatch.setattr(ops, "PROJ_MIN_WORKGROUPS", 0)                      # the fused launch at this small N, as the existing test forces it
    calls = []
    real = ops.xattn_forward_proj
    monkeypatch.setattr(ops, "xattn_forward_proj", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g, blk, local_ctx, centres, dim, K, run = _block(name, dtype)
    sel, w = _block_readouts(K)
    prompt_state.begin_prompt(local_ctx, first_timestep=981)
    plain = run()
    assert len(calls) == (1 if name == "d40" else 0)
    cap = attnmaps.AttnCapture(blk, resolution=dim)
    cap.set_readouts(sel, w)
    cap.begin([centres])
    with cap:
        out = run()
    assert len(calls) == (1 if name == "d40" else 0), "a capturing block must not run to_q inside the attention kernel"
    r = cap.result()
    assert r.block_calls == 1 and r.maps.shape == (1, len(sel), dim, dim)
    pix = torch.from_numpy(g["map_pixels"])
    got = r.maps.reshape(len(sel), -1)[:, pix.cuda()].cpu().double()
    want = torch.einsum("rnm,rm->rn", torch.from_numpy(g["maps"]).double().mean(1)[sel], w.double())
    err = (got - want).abs().max().item()
    print("block %s %s: max |readout - reference| = %.3g (bound %.3g)" % (name, dtype, err, tol))
    assert err < tol, (name, dtype, err)
    if name == "d160":
        assert torch.equal(out, plain)
    if name == "d40":
        ref = g["out"]
        eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
        e = np.abs(out.float().cpu().numpy() - ref)
        assert e.max() <= 8 * eps * np.abs(ref).max() and e.mean() <= 4 * eps * np.abs(ref).mean(), (e.max(), e.mean())
        # a second block of the same shape, no capture attached: still the projection-fused launch, while the first one captures
        _, other, _, _, _, _, run_other = _block(name, dtype)
        cap.begin([centres])
        with cap:
            run()
            n = len(calls)
            run_other()
        assert len(calls) == n + 1 and cap.result().block_calls == 1


# ---------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------
def _golden_unet(dtype, **over):
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    meta = json.load(open(os.path.join(G, "unet_state_dict_keys.json")))
    unet = UNetModel(**dict(meta["cfg"], **over)).eval()
    seeded_fill_(unet, 21)
    for p in unet.parameters():
        p.requires_grad_(False)
    return unet.to("cuda", dtype)


def _sample_batch(sampler, S=4, I=2, K=2):
    cs, locs, xts = [], [], []
    for i in range(I):
        c, local_ctx, x_T = gi.unet_inputs(K, 50 + i)
        cs.append(c.cuda()), locs.append([l.cuda() for l in local_ctx]), xts.append(x_T.cuda())
    boxes = [[[0.3 + 0.1 * i, 0.4], [0.7, 0.6 - 0.1 * i]] for i in range(I)]
    sampler.sample_batch(S=S, shape=[4, 32, 32], conditionings=cs, unconditional_conditionings=gi.load_uncond().cuda(), bboxs=boxes,
                         object_names=[["cat", "dog"]] * I, local_conditionings=locs, curr_texts=["a cat left of a dog"] * I,
                         x_T=torch.cat(xts), seed=1)
    torch.cuda.synchronize()
    return sampler.last_result["x0"].clone()


@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_sampler_capture(kind, monkeypatch):
    """The golden reduced-width UNet (32 x 32 latent: transformer levels 32, 16, 8 and the 4 x 4 middle), 4 steps, K = 2, two images,
    eager. Captured at the deepest level (8 x 8, the one whose blocks have q in HBM anyway, like C = 1280 of SD-v1): x0 is
    bit-identical with and without capture; block-calls = blocks x UNet calls (PLMS: S + 1, DDIM: S); per_call slices average to
    maps; in_disc_mass lies in [0, 1].
    Two eager runs of the SAME model are not bit-identical by default here (the convolution library picks kernels with atomics:
    0.19 - 0.22 max |dx0| between identical runs, measured); with its deterministic kernels requested they are, which is the setting
    in which "capture changes nothing" can be asked bit for bit (NCHW trunk: the library has no deterministic NHWC kernel)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.plms import PLMSSampler
    from ldm.modules.attention import BasicTransformerBlock
    from sta import attnmaps
    cls = PLMSSampler if kind == "plms" else DDIMSampler
    S, res, I = 4, 8, 2
    model = LatentDiffusion(unet_config=_golden_unet(torch.float16)).cuda()
    plain = _sample_batch(cls(model, opt_epochs=0, use_graph=False, save_images=False), S, I)
    cap = attnmaps.AttnCapture(model.model.diffusion_model, resolution=res, per_call=True)
    sampler = cls(model, opt_epochs=0, use_graph=False, save_images=False, attn_capture=cap)
    assert torch.equal(_sample_batch(sampler, S, I), plain)
    blocks = [b for b in model.modules() if isinstance(b, BasicTransformerBlock)]
    n_res = sum(b._last_n == res * res for b in blocks)
    calls = S + 1 if kind == "plms" else S
    r = sampler.last_attn
    assert n_res == 5 and r.calls == calls and r.block_calls == n_res * calls
    assert r.maps.shape == (I, 4, res, res) and r.maps.is_cuda and r.per_call.shape == (calls, I, 4, res, res)
    assert torch.isfinite(r.maps).all() and (r.maps >= 0).all() and (r.maps <= 1 + 1e-5).all()
    assert torch.allclose(r.per_call.mean(0), r.maps, atol=1e-6)
    assert r.in_disc_mass.shape == (I, 4) and ((r.in_disc_mass >= 0) & (r.in_disc_mass <= 1)).all()
    # with graph replay requested, the captured trajectory still runs eagerly and records the same number of block-calls
    graphed = cls(model, opt_epochs=0, use_graph=True, save_images=False, attn_capture=cap)
    _sample_batch(graphed, S, I)
    assert graphed.last_attn.block_calls == n_res * calls


def test_tracked_epoch_records_nothing():
    """opt_epochs = 2 (DPM-Solver++, S = 4 calls): the tracked first epoch records nothing, the kept trajectory records blocks x S."""
    from ldm.models.autoencoder import AutoencoderKL
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from sta import attnmaps
    from sta.pipeline import set_recompute

    class Loss(torch.nn.Module):
        def forward_2(self, image, text):
            return image.float().mean().reshape(1)

        def forward_3(self, image, text):
            return (image.float() ** 2).mean().reshape(1)

    vae = AutoencoderKL(ddconfig=dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32,
                                      ch_mult=[1, 2, 4, 4], num_res_blocks=1, attn_resolutions=[], dropout=0.0))
    seeded_fill_(vae, 3)
    model = LatentDiffusion(unet_config=_golden_unet(torch.bfloat16, use_checkpoint=False), first_stage_config=vae.to(torch.bfloat16)).cuda()
    for p in model.parameters():
        p.requires_grad_(False)
    set_recompute(model, "none")
    cap = attnmaps.AttnCapture(model.model.diffusion_model, resolution=8)
    sampler = DPMSolverSampler(model, loss_model=Loss(), opt_epochs=2, use_graph=False, save_images=False, attn_capture=cap)
    c, local_ctx, x_T = gi.unet_inputs(2, 6)
    sampler.sample(S=4, conditioning=c.cuda(), batch_size=1, shape=[4, 32, 32], verbose=False, unconditional_guidance_scale=7.5,
                   unconditional_conditioning=gi.load_uncond().cuda(), x_T=x_T.cuda(), text_index=0, curr_text="a cat left of a dog",
                   bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], seed=1, prompt_idx=0, object_names=["cat", "dog"],
                   local_conditionings=[l.cuda() for l in local_ctx])
    assert len(sampler.last_result["losses"]) == 1
    assert sampler.last_attn.calls == 4 and sampler.last_attn.block_calls == 5 * 4
