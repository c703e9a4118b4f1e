"""sta_latent_guide and attention-guided sampling on the GPU: the kernel against guide_reference in float64, the guarantees of its
launch (bit-reproducible, images independent, outputs overwritten completely and nothing else touched, skipped images bit-equal),
the gradient that reaches the latent on the miniature against the fp32 host chain, the three samplers end to end, and the off path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from tests.test_attnloss_gpu import CENTRES, K, RES, S, _model  # noqa: E402

SHAPES = [(1, 256, 64), (3, 4096, 1024), (2, 36864, 9216)]        # (b, n, hw): one partial block; 2 workgroups per image; 16 with a ragged slice
DTYPES = [torch.bfloat16, torch.float16]


def _inputs(b, n, hw, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    side = int(round(hw ** 0.5))
    x = torch.randn(b, n // hw, side, side, generator=g)
    gp = (torch.randn(2 * b, n // hw, side, side, generator=g) * 3e-3).to(dtype)
    keep = (torch.rand(b, 1, side, side, generator=g) > 0.6).float()
    keep[:, :, 0, :3] = 0.25                                                    # a soft edge as well
    step = torch.rand(b, generator=g) * 0.2 + 0.01
    return x, gp, keep, step


def _raw(gp, x, keep, step, x_out, xin, stats, normalize=True, inv_scale=1.0):
    """The binding itself on caller-owned buffers (views into guarded allocations)."""
    from sta import lib
    b, n, hw = x.shape[0], x[0].numel(), x.shape[-2] * x.shape[-1]
    ptr = lambda t: 0 if t is None else t.data_ptr()
    lib.check(lib.load().sta_latent_guide(gp.data_ptr(), x.data_ptr(), ptr(keep), step.data_ptr(), x_out.data_ptr(), ptr(xin), ptr(stats), b, n, hw,
                                          int(normalize), float(inv_scale), lib.STA_BF16 if gp.dtype == torch.bfloat16 else lib.STA_F16,
                                          torch.cuda.current_stream().cuda_stream), "sta_latent_guide")
    torch.cuda.synchronize()


@pytest.mark.parametrize("b,n,hw", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_matches_the_float64_reference(b, n, hw, dtype):
    """rms within 1e-5 relative (fp32 accumulation over <= 36 864 terms), x_out within 1e-5 (|x| + |s d|) elementwise, xin bit-equal to
    x_out.to(dtype) in both rows; keep on / off, normalize on / off, xin and stats written / NULL."""
    from sta.guidance import guide_reference, latent_guide
    x, gp, keep, step = _inputs(b, n, hw, dtype)
    worst_rms = worst_x = 0.0
    for kp in (None, keep):
        for normalize in (True, False):
            inv = 1.0 if normalize else 16.0
            ref, rms_ref = guide_reference(gp, x.double(), step.double(), keep=kp, normalize=normalize, inv_scale=inv)
            moved = (ref - x.double()).abs()                                    # |s d|
            assert moved.max() > 1e-3
            for want_xin in (True, False):
                for want_stats in (True, False):
                    out, xin, rms = latent_guide(gp.cuda(), x.cuda(), step.cuda(), keep=None if kp is None else kp.cuda(), normalize=normalize,
                                                 inv_scale=inv, want_xin=want_xin, want_stats=want_stats)
                    torch.cuda.synchronize()
                    assert (xin is None) == (not want_xin) and (rms is None) == (not want_stats)
                    err = ((out.cpu().double() - ref).abs() / (x.double().abs() + moved)).max().item()
                    worst_x = max(worst_x, err)
                    assert err <= 1e-5, (kp is not None, normalize, err)
                    if want_stats:
                        e = ((rms.cpu().double() - rms_ref).abs() / rms_ref).max().item()
                        worst_rms = max(worst_rms, e)
                        assert e <= 1e-5, (kp is not None, normalize, e)
                    if want_xin:
                        assert xin.dtype == dtype and torch.equal(xin[0::2], out.to(dtype)) and torch.equal(xin[1::2], out.to(dtype))
    print("b=%d n=%d hw=%d %s: worst rms rel err %.2e, worst x_out err / (|x| + |s d|) %.2e" % (b, n, hw, dtype, worst_rms, worst_x))


def test_launches_reproducible_and_images_independent():
    from sta.guidance import latent_guide
    b, n, hw = 3, 4096, 1024
    x, gp, keep, step = (t.cuda() for t in _inputs(b, n, hw, torch.float16, seed=1))
    one = latent_guide(gp, x, step, keep=keep, want_xin=True)
    two = latent_guide(gp, x, step, keep=keep, want_xin=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(one, two))
    gp2 = gp.clone()
    gp2[2:4] = gp2[2:4] * 2.0 + 1.0                                             # image 1's gradient changes
    other = latent_guide(gp2, x, step, keep=keep, want_xin=True)
    torch.cuda.synchronize()
    for a, c, rows in zip(one, other, (1, 2, 1)):
        assert torch.equal(a[:rows], c[:rows]) and torch.equal(a[2 * rows:], c[2 * rows:]) and not torch.equal(a[rows:2 * rows], c[rows:2 * rows])
    # an image alone equals the same image inside the batch
    alone = latent_guide(gp[4:6], x[2:3], step[2:3], keep=keep[2:3], want_xin=True)
    torch.cuda.synchronize()
    assert torch.equal(alone[0], one[0][2:3]) and torch.equal(alone[1], one[1][4:6]) and torch.equal(alone[2], one[2][2:3])


@pytest.mark.parametrize("b,n,hw", [(3, 4096, 1024), (2, 36864, 9216)])
def test_outputs_are_overwritten_completely_and_nothing_else_is_touched(b, n, hw):
    """x_out, xin and stats full of NaN come back finite everywhere and right; guard bands of a known pattern around all three stay
    as they were, and the inputs are unchanged."""
    from sta.guidance import guide_reference
    dtype = torch.bfloat16
    x, gp, keep, step = _inputs(b, n, hw, dtype, seed=2)
    guard = 4096
    flat_x = torch.full((guard + b * n + guard,), 7.0, device="cuda")
    flat_in = torch.full((guard + 2 * b * n + guard,), 5.0, device="cuda", dtype=dtype)
    flat_st = torch.full((guard + b + guard,), -3.0, device="cuda")
    x_out = flat_x[guard:guard + b * n].view_as(x)
    xin = flat_in[guard:guard + 2 * b * n].view_as(gp)
    stats = flat_st[guard:guard + b]
    for t in (x_out, xin, stats):
        t.fill_(float("nan"))
    xd, gd, kd, sd = x.cuda(), gp.cuda(), keep.cuda(), step.cuda()
    _raw(gd, xd, kd, sd, x_out, xin, stats)
    assert torch.isfinite(x_out).all() and torch.isfinite(xin).all() and torch.isfinite(stats).all()
    assert (flat_x[:guard] == 7.0).all() and (flat_x[guard + b * n:] == 7.0).all()
    assert (flat_in[:guard] == 5.0).all() and (flat_in[guard + 2 * b * n:] == 5.0).all()
    assert (flat_st[:guard] == -3.0).all() and (flat_st[guard + b:] == -3.0).all()
    assert torch.equal(xd.cpu(), x) and torch.equal(gd.cpu(), gp) and torch.equal(kd.cpu(), keep) and torch.equal(sd.cpu(), step)
    ref, rms_ref = guide_reference(gp, x.double(), step.double(), keep=keep)
    assert ((x_out.cpu().double() - ref).abs() <= 1e-5 * (x.double().abs() + (ref - x.double()).abs())).all()
    assert ((stats.cpu().double() - rms_ref).abs() <= 1e-5 * rms_ref).all()
    assert torch.equal(xin[0::2], x_out.to(dtype)) and torch.equal(xin[1::2], x_out.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("normalize", [True, False])
def test_zero_and_non_finite_gradient_rows_leave_x_bit_equal(dtype, normalize):
    from sta.guidance import latent_guide
    b, n, hw = 4, 4096, 1024
    x, gp, keep, step = _inputs(b, n, hw, dtype, seed=3)
    x[0, 0, 0, 0] = -0.0                                                        # signed zeros survive a skip too
    gp[0:2] = 0.0                                                               # image 0: zero gradient
    gp[3, 2, 5, 7] = float("inf")                                               # image 1: Inf in the last slice of the image
    gp[4, 0, 0, 0] = float("nan")                                               # image 2: NaN in the first
    out, xin, rms = latent_guide(gp.cuda(), x.cuda(), step.cuda(), normalize=normalize, inv_scale=4.0, want_xin=True)
    torch.cuda.synchronize()
    out, xin, rms = out.cpu(), xin.cpu(), rms.cpu()
    assert torch.equal(out[:3].view(torch.int32), x[:3].view(torch.int32))
    assert rms[0].item() == 0.0 and not torch.isfinite(rms[1]) and not torch.isfinite(rms[2]) and torch.isfinite(rms[3]) and rms[3] > 0
    assert not torch.equal(out[3], x[3]) and torch.isfinite(out).all()
    assert torch.equal(xin[0::2], out.to(dtype)) and torch.equal(xin[1::2], out.to(dtype))


# ---------------------------------------------------------------------------------------------------
# the miniature: 32 x 32 latent, K = 2, "a cat left of a dog", readouts at 8 x 8, S = 4
# ---------------------------------------------------------------------------------------------------
def _sample(model, kind, guidance, device="cuda", use_graph=True, mask=None, x0=None, **kw):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    cls = dict(ddim=DDIMSampler, plms=PLMSSampler, dpm=DPMSolverSampler)[kind]
    sampler = cls(model, loss_model=None, opt_epochs=0, use_graph=use_graph, save_images=False, latent_guidance=guidance, **kw)
    c, local_ctx, x_T = gi.unet_inputs(K, 6)
    extra = {} if mask is None else dict(mask=mask.to(device), x0=x0.to(device))
    sampler.sample(S=S, conditioning=c.to(device), batch_size=1, shape=[4, 32, 32], verbose=False, unconditional_guidance_scale=7.5,
                   unconditional_conditioning=gi.load_uncond().to(device), eta=0.0, x_T=x_T.to(device), text_index=0,
                   curr_text="a cat left of a dog", bboxs_curr=CENTRES, seed=1, prompt_idx=0, object_names=["cat", "dog"],
                   local_conditionings=[l.to(device) for l in local_ctx], **extra)
    if device == "cuda":
        torch.cuda.synchronize()
    return sampler


class _Tap:
    """Records what every latent_guide call of a run was given and returned."""

    def __init__(self, monkeypatch):
        from sta import guidance
        self.calls = []
        real = guidance.latent_guide

        def tapped(g, x, step, **kw):
            out = real(g, x, step, **kw)
            self.calls.append(dict(g=g.detach().float().cpu(), x=x.detach().cpu(), x_out=out[0].detach().cpu(), kw=kw))
            return out
        monkeypatch.setattr(guidance, "latent_guide", tapped)


_HOST = {}


def _host_d(blocks, monkeypatch):
    """d = g_u + g_c of the first update on the fp32 host chain (oracle-backed blocks), and its energy drop at eta = 0.1."""
    if blocks not in _HOST:
        from sta.guidance import AttnGuidance
        from tests.cpu_backend import oracle_ops
        model = _model(torch.float32, "cpu", vae=False)
        tap = _Tap(monkeypatch)
        with oracle_ops():
            s = _sample(model, "ddim", AttnGuidance(model.model.diffusion_model, resolution=RES, scale=0.1, steps=1, iters=2, blocks=blocks),
                        device="cpu", use_graph=False)
        g = tap.calls[0]["g"]
        e = s.last_guidance["energy"]
        _HOST[blocks] = dict(d=g[0] + g[1], e0=e[0, 0].item(), drop=(e[0, 0] - e[1, 0]).item())
    return _HOST[blocks]


@pytest.mark.parametrize("blocks", ["down", "all"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_reaches_the_latent(blocks, dtype, monkeypatch):
    """d = g_u + g_c of the first update against the fp32 host chain. Bounds: the project's own for this chain at this size
    (test_weight_optimisation_with_the_attention_loss_alone): max |d - d_ref| / max |d_ref| <= 0.15, sign agreement >= 95 % on the
    entries above 5 % of the largest. fp16: the gradient arrives scaled by the loss scale (non-zero: without it |d| ~ 1e-4 loses its
    small entries to fp16's subnormals) and meets the same bounds once unscaled. Measured on the first run (profiles/attn_guidance.md): 0.021 /
    0.024 (bf16, down / all) and 0.004 / 0.004 (fp16) of max |d_ref|, sign agreement 100 % — the bounds stand as they are."""
    from sta.guidance import AttnGuidance
    ref = _host_d(blocks, monkeypatch)
    model = _model(dtype, vae=False)
    tap = _Tap(monkeypatch)
    s = _sample(model, "ddim", AttnGuidance(model.model.diffusion_model, resolution=RES, scale=0.1, steps=1, iters=1, blocks=blocks))
    call = tap.calls[0]
    inv = call["kw"]["inv_scale"]
    assert call["g"].dtype == torch.float32 and (inv < 1.0) == (dtype == torch.float16)
    d = (call["g"][0] + call["g"][1]) * inv
    e_max = ((d - ref["d"]).abs().max() / ref["d"].abs().max()).item()
    strong = ref["d"].abs() > 0.05 * ref["d"].abs().max()
    agree = (torch.sign(d[strong]) == torch.sign(ref["d"][strong])).float().mean().item()
    res = s.last_guidance
    print("blocks=%s %s: E0 %.5f (host %.5f), loss scale %g, max |d - d_ref| / max |d_ref| = %.4f, strong %.3f of all, sign agreement %.4f, rms %.3e"
          % (blocks, dtype, res["energy"][0, 0].item(), ref["e0"], 1.0 / inv, e_max, strong.float().mean().item(), agree, res["rms"][0, 0].item()))
    assert torch.isfinite(d).all() and d.abs().max() > 0 and res["skipped"] == 0
    assert not torch.equal(call["x_out"], call["x"])                           # the update is not zero
    assert abs(res["energy"][0, 0].item() - ref["e0"]) <= 0.01 * ref["e0"]
    assert e_max <= 0.15, e_max
    assert agree >= 0.95, agree


@pytest.mark.parametrize("kind,dtype", [("ddim", torch.bfloat16), ("dpm", torch.bfloat16), ("plms", torch.float16)])
def test_guided_sampling_end_to_end(kind, dtype):
    """eta = 0.1, steps = 2, iters = 2 (ordinary calls graph-replayed, evaluations eager): E falls across the first update by at
    least half the host chain's drop (>= 0.014), x0 is finite and differs from the unguided x0."""
    from ldm.modules.attention import BasicTransformerBlock
    from sta.guidance import AttnGuidance
    model = _model(dtype, vae=False)
    plain = _sample(model, kind, None).last_result["x0"]
    s = _sample(model, kind, AttnGuidance(model.model.diffusion_model, resolution=RES, scale=0.1, steps=2, iters=2))
    res, x0 = s.last_guidance, s.last_result["x0"]
    e = res["energy"][:, 0].tolist()
    print("%s %s: E before the updates %s, rms %s" % (kind, dtype, ["%.5f" % v for v in e], ["%.3e" % v for v in res["rms"][:, 0].tolist()]))
    assert res["calls"] == [(0, 0), (0, 1), (1, 0), (1, 1)] and res["skipped"] == 0
    assert e[0] - e[1] >= 0.014, e
    assert torch.isfinite(x0).all() and not torch.equal(x0, plain)
    assert all(b._attn_loss is None for b in model.modules() if isinstance(b, BasicTransformerBlock))


def test_masked_run_does_not_guide_the_kept_region(monkeypatch):
    from sta.guidance import AttnGuidance
    model = _model(torch.bfloat16, vae=False)
    g = torch.Generator().manual_seed(11)
    keep = torch.zeros(1, 1, 32, 32)
    keep[:, :, :, :12] = 1.0
    keep[:, :, 20:, 12:16] = 0.5
    z0 = torch.randn(1, 4, 32, 32, generator=g)
    tap = _Tap(monkeypatch)
    s = _sample(model, "ddim", AttnGuidance(model.model.diffusion_model, resolution=RES, scale=0.1, steps=2, iters=1), mask=keep, x0=z0)
    assert len(tap.calls) == 2 and torch.isfinite(s.last_result["x0"]).all()
    kept = (keep == 1.0).expand(1, 4, 32, 32)
    for call in tap.calls:
        assert call["kw"]["keep"] is not None
        delta = call["x_out"] - call["x"]
        assert (delta[kept] == 0).all() and torch.equal(call["x_out"][kept].view(torch.int32), call["x"][kept].view(torch.int32))
        assert delta[~kept].abs().max() > 0 and delta[(keep == 0.5).expand(1, 4, 32, 32)].abs().max() > 0


def test_off_path_is_untouched(monkeypatch):
    """latent_guidance=None: latent_guide is never reached and x0 is bit-equal from run to run (deterministic convolution kernels
    requested, as tests/test_attnloss_gpu.py does)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    from sta import guidance
    monkeypatch.setattr(guidance, "latent_guide", lambda *a, **k: pytest.fail("latent_guide was called"))
    model = _model(torch.float16, vae=False)
    a = _sample(model, "ddim", None, use_graph=False)
    assert a.last_guidance is None
    assert torch.equal(a.last_result["x0"], _sample(model, "ddim", None, use_graph=False).last_result["x0"])
    # a guidance that is given but switched off (steps = 0): the same image, nothing evaluated
    off = guidance.AttnGuidance(model.model.diffusion_model, resolution=RES, scale=0.1, steps=0)
    assert torch.equal(a.last_result["x0"], _sample(model, "ddim", off, use_graph=False).last_result["x0"]) and off.loss.block_calls == 0
