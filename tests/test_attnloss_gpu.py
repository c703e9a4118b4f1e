"""sta_xattn_token_maps_bwd and the attention-layout loss on the GPU: the kernel against float64 autograd of the readout formula,
its structural guarantees (bit-reproducible, image-count independent, dq overwritten completely, bounds), the autograd Function, a
miniature weight optimisation with the attention loss alone under every recomputation policy against the fp32 host chain, the
fp16 loss scale on the per-call terms, both losses together, and the off path."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from oracle import xattn_oracle as orc  # noqa: E402
from sta.synth import seeded_fill_  # noqa: E402

G = gi.GOLDEN
M = 77
CENTRES = [[0.3, 0.4], [0.7, 0.6]]
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _qk(N, C, K, dtype, I=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(2 * I, N, C, generator=g).to(dtype)
    k = (torch.randn(I * (K + 2), M, C, generator=g) * 0.7).to(dtype)
    v = torch.randn(I * (K + 2), M, C, generator=g).to(dtype)
    return q, k, v


def _readouts(K, R, seed=1):
    """The row mix of tests/test_attnmaps_gpu.py: one-hot at token 0, at token 76 (the last key before the padding) and in the
    middle, a uniform 1/77 row, a random signed row, an all-ones row; contexts so that several readouts share one and every context
    kind occurs. Further rows (up to R) are random signed rows walking over all contexts."""
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


def _oracle(q, k, sel, w, heads, dmaps):
    """(maps, dq) in float64: autograd through token_maps_reference on the 16-bit-rounded inputs, upstream dmaps (None: maps only)."""
    from sta import attnmaps
    q64 = q.double().requires_grad_(dmaps is not None)
    maps = attnmaps.token_maps_reference(q64, k.double(), sel, w.double(), heads, (q.shape[2] // heads) ** -0.5)
    if dmaps is None:
        return maps, None
    (maps * dmaps.double()).sum().backward()
    return maps.detach(), q64.grad


def _layout_dmaps(maps, N, R):
    """The gradient of layout_energy on `maps` [I, R, N] with discs at (0.3, 0.4) / (0.7, 0.6), readout r against object r % 2."""
    from sta import ops
    from sta.attnloss import layout_energy
    disc = ops.disc_masks(CENTRES, math.isqrt(N)).float()[[r % 2 for r in range(R)]].unsqueeze(0).expand(maps.shape[0], -1, -1)
    m = maps.float().clone().requires_grad_(True)
    layout_energy(m, disc, torch.ones(maps.shape[0], R, dtype=torch.bool)).sum().backward()
    return m.grad


def _launch(q, k, v, sel, w, heads, dmaps, I=1, out=None):
    from sta import attnmaps, ops
    packed = ops.pack_kv(k.cuda(), v.cuda(), heads, n_img=I)
    dq = attnmaps.token_maps_backward(q.cuda(), packed, sel, w.cuda(), dmaps.cuda(), (q.shape[2] // heads) ** -0.5, out=out)
    torch.cuda.synchronize()
    return dq


SHAPES = [
    # N, C, heads, K, R
    (64, 64, 8, 1, 6),       # d = 8
    (256, 320, 8, 2, 6),     # d = 40
    (64, 640, 8, 2, 6),      # d = 80
    (256, 1280, 8, 2, 6),    # the default recording shape, d = 160
    (100, 128, 4, 3, 6),     # ragged N, 4 heads
    (256, 192, 8, 0, 6),     # contexts 0 and 1 only
    (64, 320, 8, 8, 16),     # a context read by five readouts: several register groups of one context summed into one dq
]


@pytest.mark.parametrize("N,C,heads,K,R", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_bwd_matches_oracle(N, C, heads, K, R, dtype):
    """max |dq - dq_ref| <= 6 eps max |dq_ref| + 1e-6 (eps = 2^-8 bf16, 2^-11 fp16): the bound test_bwd_matches_oracle holds
    sta_xattn_bwd's dq to, which has the same rounding (dS to 16 bits before the dS . K product). Upstream once standard normal
    and once the actual gradient of layout_energy."""
    q, k, v = _qk(N, C, K, dtype)
    sel, w = _readouts(K, R)
    assert len(sel) == R
    g = torch.Generator().manual_seed(7)
    maps_ref, _ = _oracle(q, k, sel, w, heads, None)
    for kind, dmaps in (("normal", torch.randn(1, R, N, generator=g)), ("layout", _layout_dmaps(maps_ref, N, R))):
        _, ref = _oracle(q, k, sel, w, heads, dmaps)
        got = _launch(q, k, v, sel, w, heads, dmaps).cpu().double()
        err, top = (got - ref).abs().max().item(), ref.abs().max().item()
        bound = 6 * EPS[dtype] * top + 1e-6
        print("N=%d C=%d heads=%d K=%d R=%d %s %s: max |dq - ref| / bound = %.3f (max |ref| %.3g)" % (N, C, heads, K, R, dtype, kind, err / bound, top))
        assert top > 0 and err <= bound, (kind, err, bound)


def test_launches_reproducible_and_images_independent():
    """Two launches on the same inputs are bit-identical, and n_img = 3 equals the three one-image launches bit for bit."""
    N, C, heads, K, I = 100, 128, 4, 3, 3
    q, k, v = _qk(N, C, K, torch.float16, I=I, seed=2)
    sel, w0 = _readouts(K, 8)
    w = torch.stack([w0, w0.flip(0), 0.5 * w0])
    dmaps = torch.randn(I, len(sel), N, generator=torch.Generator().manual_seed(3))
    three = _launch(q, k, v, sel, w, heads, dmaps, I=I)
    assert torch.equal(three, _launch(q, k, v, sel, w, heads, dmaps, I=I))
    for i in range(I):
        s = slice(i * (K + 2), (i + 1) * (K + 2))
        one = _launch(q[2 * i:2 * i + 2], k[s], v[s], sel, w[i], heads, dmaps[i:i + 1])
        assert torch.equal(one, three[2 * i:2 * i + 2]), i
    assert three.float().abs().max() > 0


@pytest.mark.parametrize("N,C,heads,K", [(100, 128, 4, 3), (256, 1280, 8, 2)])
def test_dq_is_overwritten_completely_and_nothing_else_is_touched(N, C, heads, K):
    """A dq buffer full of NaN comes back finite everywhere, row 0 is exactly zero when no readout names context 0, and guard bands
    of a known pattern around dq and around dmaps stay as they were."""
    from sta import attnmaps, ops
    dtype = torch.bfloat16
    q, k, v = _qk(N, C, K, dtype, seed=3)
    sel = [1, K + 1, 1]                                                         # context 0 is not selected
    w = torch.randn(3, M, generator=torch.Generator().manual_seed(5))
    guard, n_dq, n_dm = 4096, 2 * N * C, 3 * N
    flat = torch.full((guard + n_dq + guard,), 7.0, device="cuda", dtype=dtype)
    dq = flat[guard:guard + n_dq].view(2, N, C)
    dq.fill_(float("nan"))
    flat_dm = torch.full((guard + n_dm + guard,), -12345.0, device="cuda")
    dm = torch.randn(1, 3, N, generator=torch.Generator().manual_seed(6))
    flat_dm[guard:guard + n_dm].copy_(dm.reshape(-1))
    packed = ops.pack_kv(k.cuda(), v.cuda(), heads)
    attnmaps.token_maps_backward(q.cuda(), packed, sel, w.cuda(), flat_dm[guard:guard + n_dm].view(1, 3, N), (C // heads) ** -0.5, out=dq)
    torch.cuda.synchronize()
    assert torch.isfinite(dq).all()
    assert (dq[0] == 0).all() and dq[1].float().abs().max() > 0
    assert (flat[:guard] == 7.0).all() and (flat[guard + n_dq:] == 7.0).all()
    assert (flat_dm[:guard] == -12345.0).all() and (flat_dm[guard + n_dm:] == -12345.0).all()
    assert torch.equal(flat_dm[guard:guard + n_dm].cpu(), dm.reshape(-1))
    _, ref = _oracle(q, k, sel, w, heads, dm)
    assert (dq.cpu().double() - ref).abs().max() <= 6 * EPS[dtype] * ref.abs().max() + 1e-6


# ---------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------
def test_autograd_function_equals_the_binding_and_gradients_add_up():
    """TokenMapsFn through torch.autograd.grad is the direct binding call, bit for bit; a q that feeds both ops.xattn_blend and
    token_maps_tracked receives the sum of both gradients, held to the dq bound applied to the float64 sum."""
    from sta import attnmaps, ops
    dtype, eps = torch.float16, EPS[torch.float16]
    N, C, heads, K = 256, 320, 8, 2
    q, k, v = _qk(N, C, K, dtype, seed=4)
    sel, w = [1, 1, 2, 3], torch.rand(4, M, generator=torch.Generator().manual_seed(8))
    scale = (C // heads) ** -0.5
    packed = ops.pack_kv(k.cuda(), v.cuda(), heads)
    up = torch.randn(1, 4, N, generator=torch.Generator().manual_seed(9))
    qd = q.cuda().requires_grad_(True)
    maps = attnmaps.token_maps_tracked(qd, packed, sel, w.cuda(), scale)
    assert torch.equal(maps.detach(), attnmaps.token_maps(q.cuda(), packed, sel, w.cuda(), scale))
    (got,) = torch.autograd.grad(maps, qd, up.cuda())
    assert torch.equal(got, attnmaps.token_maps_backward(q.cuda(), packed, sel, w.cuda(), up.cuda(), scale))
    # the same q into the blend as well
    mask = ops.disc_masks(CENTRES, 16)
    coef = torch.tensor([2.5, 2.5])
    go = torch.randn(2, N, C, generator=torch.Generator().manual_seed(10)).to(dtype)
    qd = q.cuda().requires_grad_(True)
    out = ops.xattn_blend(qd, coef.cuda(), packed, ops.mask_bits(mask).cuda(), scale)
    maps = attnmaps.token_maps_tracked(qd, packed, sel, w.cuda(), scale)
    torch.autograd.backward([out, maps], [go.cuda(), up.cuda()])
    q64 = q.double().requires_grad_(True)
    ref_out = orc.fused_xattn(q64, k.double(), v.double(), mask.bool(), coef.double(), heads, scale)
    ref_maps = attnmaps.token_maps_reference(q64, k.double(), sel, w.double(), heads, scale)
    torch.autograd.backward([ref_out, ref_maps], [go.double(), up.double()])
    err, top = (qd.grad.cpu().double() - q64.grad).abs().max().item(), q64.grad.abs().max().item()
    print("blend + readout on one q: max |dq - ref| / bound = %.3f" % (err / (6 * eps * top + 1e-6)))
    assert err <= 6 * eps * top + 1e-6, (err, top)


# ---------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------
RES, S, K = 8, 4, 2
VAE_CFG = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4, 4], num_res_blocks=1,
               attn_resolutions=[], dropout=0.0)


def _model(dtype, device="cuda", vae=True):
    from ldm.models.autoencoder import AutoencoderKL
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    meta = json.load(open(os.path.join(G, "unet_state_dict_keys.json")))
    unet = UNetModel(**dict(meta["cfg"], use_checkpoint=True)).eval()
    seeded_fill_(unet, 21)
    first = None
    if vae:
        first = AutoencoderKL(ddconfig=VAE_CFG)
        seeded_fill_(first, 3)
        first = first.to(dtype)
    model = LatentDiffusion(unet_config=unet.to(dtype), first_stage_config=first).to(device)
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def _epoch(sampler, device="cuda"):
    """opt_epochs = 2 on the miniature (32 x 32 latent, K = 2, "a cat left of a dog": every name token is found, so all 2 K
    readouts count) -> (last_result, dLoss/dW of the tracked epoch [K, S])."""
    grads = []
    orig_step = torch.optim.Adam.step
    torch.optim.Adam.step = lambda self, *a, **k: (grads.append(self.param_groups[0]["params"][0].grad.clone()), orig_step(self, *a, **k))[1]
    c, local_ctx, x_T = gi.unet_inputs(K, 6)
    try:
        sampler.sample(S=S, conditioning=c.to(device), batch_size=1, shape=[4, 32, 32], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond().to(device), x_T=x_T.to(device), text_index=0,
                       curr_text="a cat left of a dog", bboxs_curr=CENTRES, seed=1, prompt_idx=0, object_names=["cat", "dog"],
                       local_conditionings=[l.to(device) for l in local_ctx])
    finally:
        torch.optim.Adam.step = orig_step
    if device == "cuda":
        torch.cuda.synchronize()
    return sampler.last_result, grads[0].float().cpu().reshape(K, -1)


_HOST, _LOSSES = {}, {}


def _host_reference():
    """The same tracked epoch in fp32 on the host with the oracle's differentiable fused op (tests/cpu_backend.py) and the torch
    readout under autograd: loss, dLoss/dW, W after one Adam step."""
    if not _HOST:
        from ldm.models.diffusion.plms import PLMSSampler
        from sta.attnloss import AttnLayoutLoss
        from sta.pipeline import set_recompute
        from tests.cpu_backend import oracle_ops
        model = _model(torch.float32, "cpu", vae=False)
        set_recompute(model, "none")
        loss = AttnLayoutLoss(model.model.diffusion_model, resolution=RES)
        sampler = PLMSSampler(model, loss_model=None, opt_epochs=2, use_graph=False, save_images=False, attn_loss=loss)
        with oracle_ops():
            r, grad = _epoch(sampler, "cpu")
        _HOST.update(loss=r["losses"][0], W=r["W"].clone(), grad=grad)
    return _HOST


@pytest.mark.parametrize("recompute", ["none", "res", "all", "call"])
def test_weight_optimisation_with_the_attention_loss_alone(recompute):
    """BASELINE configs[2] in miniature without CLIP: bf16, PLMS, S = 4, the loss recorded at 8 x 8, a VAE attached only to count
    decodes (the tracked epoch must not decode). Bounds: the project's own for this chain at this size
    (test_weight_optimisation_on_gpu) — loss within 1 % of the fp32 host chain, max |dW - dW_ref| / max |dW_ref| <= 0.15, sign
    agreement >= 95 % on the entries above 5 % of the largest reference gradient (which are > 30 % of all), the losses of the four
    policies within 2 % + 1e-3 of each other, and >= 80 % of the W entries move by lr."""
    from ldm.models.diffusion.plms import PLMSSampler
    from ldm.modules.attention import BasicTransformerBlock
    from sta.attnloss import AttnLayoutLoss
    from sta.pipeline import set_recompute
    model = _model(torch.bfloat16)
    assert set_recompute(model, recompute) == recompute
    decodes = []
    real_decode = model.decode_first_stage
    model.decode_first_stage = lambda z: (decodes.append(1), real_decode(z))[1]
    loss = AttnLayoutLoss(model.model.diffusion_model, resolution=RES)
    sampler = PLMSSampler(model, loss_model=None, opt_epochs=2, save_images=False, attn_loss=loss)
    r, grad = _epoch(sampler)
    assert len(r["losses"]) == 1 and torch.isfinite(r["x0"]).all() and len(decodes) == 1
    assert all(b._attn_loss is None for b in model.modules() if isinstance(b, BasicTransformerBlock))
    if recompute == "call":
        assert sampler.last_kept_calls >= 1
    step = (r["W"] - 2.5).abs()
    assert (step <= 0.005 + 1e-5).all() and (step > 0.0049).float().mean() >= 0.8, step
    ref = _host_reference()
    _LOSSES[recompute] = r["losses"][0]
    e_loss = abs(r["losses"][0] - ref["loss"]) / abs(ref["loss"])
    e_max = ((grad - ref["grad"]).abs().max() / ref["grad"].abs().max()).item()
    strong = ref["grad"].abs() > 0.05 * ref["grad"].abs().max()
    agree = (torch.sign(grad[strong]) == torch.sign(ref["grad"][strong])).float().mean().item()
    print("recompute=%s: loss %.6f (host %.6f, rel %.4f), max |dW - dW_ref| / max |dW_ref| = %.3f, strong %.2f of all, sign agreement %.3f"
          % (recompute, r["losses"][0], ref["loss"], e_loss, e_max, strong.float().mean().item(), agree))
    if len(_LOSSES) == 4:
        vals = list(_LOSSES.values())
        assert max(vals) - min(vals) <= 0.02 * abs(vals[0]) + 1e-3, _LOSSES
    assert e_loss <= 0.01, (r["losses"][0], ref["loss"])
    assert e_max <= 0.15, e_max
    assert strong.float().mean() > 0.3 and agree >= 0.95, (strong.float().mean(), agree)


def test_fp16_call_mode_dpm_solver_scales_the_injected_terms():
    """fp16, per-call recomputation, DPM-Solver++ with S = 4 calls: the loss scale reaches the terms differentiated inside the
    recomputed calls (finite loss and gradient, W moves)."""
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from sta.attnloss import AttnLayoutLoss
    from sta.pipeline import set_recompute
    model = _model(torch.float16, vae=False)
    set_recompute(model, "call")
    loss = AttnLayoutLoss(model.model.diffusion_model, resolution=RES)
    sampler = DPMSolverSampler(model, loss_model=None, opt_epochs=2, save_images=False, attn_loss=loss)
    r, grad = _epoch(sampler)
    print("fp16 call dpm: loss %.6f, max |dW| %.3g, kept calls %d" % (r["losses"][0], grad.abs().max().item(), sampler.last_kept_calls))
    assert len(r["losses"]) == 1 and math.isfinite(r["losses"][0]) and r["losses"][0] > 0
    assert torch.isfinite(grad).all() and grad.abs().max() > 0 and torch.isfinite(r["x0"]).all()
    assert ((r["W"] - 2.5).abs() > 0.0049).any()


def test_both_losses_add_up():
    """CLIP stand-in + 2 x the attention loss: the first epoch's recorded loss is the CLIP-only epoch's plus 2 x the attention-only
    epoch's (same first epoch, same initial W), within 1 %. Mode `call`: the per-call terms ride on a backward the image loss roots."""
    from ldm.models.diffusion.plms import DCLIPLoss, PLMSSampler
    from sta.attnloss import AttnLayoutLoss
    from sta.pipeline import set_recompute
    from sta.synth import SyntheticCLIP
    model = _model(torch.bfloat16)
    set_recompute(model, "call")
    clip = DCLIPLoss(SyntheticCLIP().cuda())
    loss = AttnLayoutLoss(model.model.diffusion_model, resolution=RES)
    vals = {}
    for name, kw in (("clip", dict(loss_model=clip)), ("attn", dict(loss_model=None, attn_loss=loss)),
                     ("both", dict(loss_model=clip, attn_loss=loss, attn_loss_weight=2.0))):
        r, grad = _epoch(PLMSSampler(model, opt_epochs=2, save_images=False, **kw))
        assert torch.isfinite(grad).all() and grad.abs().max() > 0
        vals[name] = r["losses"][0]
    want = vals["clip"] + 2.0 * vals["attn"]
    print("both losses: clip %.5f attn %.6f both %.5f (clip + 2 attn = %.5f)" % (vals["clip"], vals["attn"], vals["both"], want))
    assert abs(vals["both"] - want) <= 0.01 * abs(want), vals


def test_off_path_is_untouched(monkeypatch):
    """attn_loss=None is today's sampler: x0 bit-identical to a sampler that was never given the keyword (deterministic convolution
    kernels requested, as test_sampler_capture does, NCHW trunk); and after a trajectory with a loss attached no block keeps it."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    from ldm.models.diffusion.plms import PLMSSampler
    from ldm.modules.attention import BasicTransformerBlock
    from sta.attnloss import AttnLayoutLoss
    model = _model(torch.float16, vae=False)

    def x0(sampler):
        c, local_ctx, x_T = gi.unet_inputs(K, 6)
        sampler.sample(S=S, conditioning=c.cuda(), batch_size=1, shape=[4, 32, 32], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond().cuda(), x_T=x_T.cuda(), text_index=0, curr_text="a cat left of a dog",
                       bboxs_curr=CENTRES, seed=1, prompt_idx=0, object_names=["cat", "dog"], local_conditionings=[l.cuda() for l in local_ctx])
        torch.cuda.synchronize()
        return sampler.last_result["x0"].clone()

    plain = x0(PLMSSampler(model, opt_epochs=0, use_graph=False, save_images=False))
    assert torch.equal(x0(PLMSSampler(model, opt_epochs=0, use_graph=False, save_images=False, attn_loss=None)), plain)
    # a loss that is given but never used (no tracked epoch): still the same image, and nothing stays attached
    loss = AttnLayoutLoss(model.model.diffusion_model, resolution=RES)
    assert torch.equal(x0(PLMSSampler(model, opt_epochs=0, use_graph=False, save_images=False, attn_loss=loss)), plain)
    assert loss.block_calls == 0
    assert all(b._attn_loss is None for b in model.modules() if isinstance(b, BasicTransformerBlock))
