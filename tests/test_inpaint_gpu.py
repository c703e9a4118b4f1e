"""Layout-guided inpainting on the MI355X: the kernels of csrc/sta_inpaint.hip against float64 restatements, and the masked samplers:
the reference's golden trajectory, graph replay, prompt batching with per-image masks, DPM-Solver++ with a mask, a tracked epoch through
SolverStepMaskedFn and the composite backward, and scripts/inpaint.py end to end on synthetic weights."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from tests.test_solver_gpu import _case, _golden_unet, _step64, _wopt_model  # noqa: E402

G = gi.GOLDEN
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
LATENTS = [(4, 8, 8), (4, 2, 12), (4, 64, 64)]        # (4, 2, 12): hw = 24, a lane's 8 elements cross rows but never channels
Q_A, Q_B = 0.8253, 0.5647


def _keep(b, h, w, gen, device="cuda"):
    """Exact 0, exact 1 and fractional cells."""
    r = torch.rand(b, 1, h, w, generator=gen)
    keep = torch.where(r < 0.3, torch.zeros_like(r), torch.where(r > 0.7, torch.ones_like(r), r))
    keep.view(-1)[0], keep.view(-1)[-1] = 0.0, 1.0
    return keep.to(device)


def _blend64(xn, axn, x0, keep, n, q_a=Q_A, q_b=Q_B):
    """float64 restatement of the blend and the sum of its absolute terms: keep (|q_a x0| + |q_b n|) + (1 - keep) |x_next terms|."""
    k = keep.double()
    q_a, q_b = float(np.float32(q_a)), float(np.float32(q_b))          # the kernel takes them as float32
    out = k * (q_a * x0.double() + q_b * n.double()) + (1.0 - k) * xn
    mag = k * ((q_a * x0.double()).abs() + (q_b * n.double()).abs()) + (1.0 - k) * axn
    return out, mag


def _inputs(b, lat, c, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    shape = (b,) + lat
    r = lambda *s: torch.randn(*s, generator=gen).cuda()
    eps = r(2 * b, *lat).to(dtype)
    x = r(*shape) * 3
    m_prev = r(*shape) if c.c_p else None
    noise = r(*shape) if c.c_n else None
    x0, qn = r(*shape), r(*shape)
    return eps, x, m_prev, noise, x0, qn, _keep(b, lat[1], lat[2], gen)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("lat", LATENTS)
@pytest.mark.parametrize("mode", ["first", "second", "noise"])
def test_masked_step_kernel_vs_fp64(dtype, b, lat, mode):
    """sta_sampler_step_masked against test_solver_gpu._step64 followed by the float64 blend, err <= 1e-6 (1 + sum of |terms|); m is the
    unmasked step's; xin is bitwise pair(x_next).to(dtype); where keep == 0 the state is bitwise sta_sampler_step's; the backward
    (sta_sampler_step_masked_bwd) against float64 autograd with test_solver_gpu's bounds."""
    from sta import solver
    c = _case(mode)
    eps, x, m_prev, noise, x0, qn, keep = _inputs(b, lat, c, dtype, b * 100 + lat[2])
    bl = solver.Blend(x0, keep, qn, Q_A, Q_B)
    xn, m, xin = solver.solver_step_masked(eps, x, m_prev, noise, c, bl, want_xin=True)
    rx, rm, ax, am = _step64(eps, x, m_prev, noise, c, magnitudes=True)
    rb, ab = _blend64(rx, ax, x0, keep, qn)
    for got, ref, mag in ((xn, rb, ab), (m, rm, am)):
        err = (got.double() - ref).abs()
        print("%s %s b=%d %s: max err / (1 + mag) = %.3g" % (mode, dtype, b, lat, (err / (1 + mag)).max().item()))
        assert (err <= 1e-6 * (1 + mag)).all(), (err / (1 + mag)).max().item()
    assert torch.equal(xin, solver._pair(xn).to(dtype))
    plain, pm, _ = solver.solver_step(eps, x, m_prev, noise, c)
    zero = (keep == 0).expand_as(xn)
    assert zero.any() and (keep == 1).any() and ((keep > 0) & (keep < 1)).any()
    assert torch.equal(xn[zero], plain[zero]) and torch.equal(m, pm)
    # the CPU restatement agrees with the kernel
    cpu = lambda t: None if t is None else t.cpu()
    cx, cm, _ = solver.solver_step_masked(eps.cpu().float(), x.cpu(), cpu(m_prev), cpu(noise), c, solver.Blend(x0.cpu(), keep.cpu(), qn.cpu(), Q_A, Q_B))
    assert ((cx.double() - xn.cpu().double()).abs() <= 2e-6 * (1 + ab.cpu())).all()
    # backward
    shape = x.shape
    gen = torch.Generator().manual_seed(7)
    gx, gm = torch.randn(shape, generator=gen).cuda(), torch.randn(shape, generator=gen).cuda()
    e_ = eps.float().requires_grad_(True)
    x_ = x.clone().requires_grad_(True)
    mp_ = None if m_prev is None else m_prev.clone().requires_grad_(True)
    a, bm, _ = solver.solver_step_masked(e_, x_, mp_, noise, c, bl, dtype=dtype)
    torch.autograd.backward([a, bm], [gx, gm])
    e64 = eps.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    mp64 = None if m_prev is None else m_prev.double().requires_grad_(True)
    ra, rbm = _step64(e64, x64, mp64, noise, c)
    ra = keep.double() * (Q_A * x0.double() + Q_B * qn.double()) + (1.0 - keep.double()) * ra
    torch.autograd.backward([ra, rbm], [gx.double(), gm.double()])
    gk = (1.0 - keep.double()) * gx.double().abs()
    gmag = gk * abs(c.c_x) + (gm.double().abs() + abs(c.c_m) * gk) / abs(c.alpha_t)
    assert ((x_.grad.double() - x64.grad).abs() <= 1e-6 * (1 + gmag)).all()
    assert ((e_.grad.double() - e64.grad).abs() <= ULP[dtype] * e64.grad.abs() + 1e-6).all()
    if mp_ is not None:
        assert torch.allclose(mp_.grad.double(), mp64.grad, rtol=1e-6, atol=1e-6)
        one = (keep == 1).expand_as(xn)
        assert (mp_.grad[one] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("lat", LATENTS)
def test_latent_blend_kernel_vs_fp64(dtype, b, lat):
    from sta import solver
    _, x, _, _, x0, qn, keep = _inputs(b, lat, _case("first"), dtype, b * 10 + lat[2])
    bl = solver.Blend(x0, keep, qn, Q_A, Q_B)
    xb, xin = solver.latent_blend(x, bl, dtype=dtype, want_xin=True)
    ref, mag = _blend64(x.double(), x.double().abs(), x0, keep, qn)
    err = (xb.double() - ref).abs()
    assert (err <= 1e-6 * (1 + mag)).all(), (err / (1 + mag)).max().item()
    assert torch.equal(xin, solver._pair(xb).to(dtype))
    zero, one = (keep == 0).expand_as(x), (keep == 1).expand_as(x)
    assert torch.equal(xb[zero], x[zero])
    q = np.float32(Q_A) * x0 + np.float32(Q_B) * qn
    assert ((xb - q).abs()[one] <= 1e-6 * (1 + q.abs()[one])).all()
    xb2, none = solver.latent_blend(x, bl, dtype=dtype, want_xin=False)
    assert none is None and torch.equal(xb2, xb)
    cb, _ = solver.latent_blend(x.cpu(), solver.Blend(x0.cpu(), keep.cpu(), qn.cpu(), Q_A, Q_B))
    assert ((cb.double() - xb.cpu().double()).abs() <= 2e-6 * (1 + mag.cpu())).all()


def test_masked_step_grid_stride_case():
    """b = 5, (4, 1024, 1024), fp16: 2 621 440 lanes, more than the grid cap of 8192 blocks x 256 lanes, so lanes take a second element; compared on
    the device in float64 with the kernel bound."""
    from sta import solver
    c = _case("noise")
    b, lat = 5, (4, 1024, 1024)
    assert b * 4 * 1024 * 1024 // 8 > 8192 * 256
    gen = torch.Generator(device="cuda").manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=gen, device="cuda")
    eps = r(2 * b, *lat).half()
    x, noise, x0, qn = r(b, *lat) * 3, r(b, *lat), r(b, *lat), r(b, *lat)
    u = torch.rand(b, 1, 1024, 1024, generator=gen, device="cuda")
    keep = torch.where(u < 0.3, torch.zeros_like(u), torch.where(u > 0.7, torch.ones_like(u), u))
    xn, m, xin = solver.solver_step_masked(eps, x, None, noise, c, solver.Blend(x0, keep, qn, Q_A, Q_B), want_xin=True)
    assert torch.equal(xin.view(b, 2, *lat)[:, 0], xn.half()) and torch.equal(xin.view(b, 2, *lat)[:, 1], xn.half())
    for i in range(b):           # image by image: the float64 temporaries stay small
        s = slice(i, i + 1)
        rx, rm, ax, am = _step64(eps[2 * i:2 * i + 2], x[s], None, noise[s], c, magnitudes=True)
        rb, ab = _blend64(rx, ax, x0[s], keep[s], qn[s])
        assert ((xn[s].double() - rb).abs() <= 1e-6 * (1 + ab)).all(), i
        assert ((m[s].double() - rm).abs() <= 1e-6 * (1 + am)).all(), i
        del rx, rm, ax, am, rb, ab


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("with_gm", [True, False])
@pytest.mark.parametrize("with_gmprev", [True, False])
def test_masked_bwd_with_keep_zero_is_the_unmasked_bwd_bit_for_bit(dtype, with_gm, with_gmprev):
    """keep == 0 everywhere: g_x, g_eps and g_mprev of sta_sampler_step_masked_bwd carry the bits of sta_sampler_step_bwd's (both run the
    one step1_bwd of csrc/sta_step_dev.h; (1 - 0) g is g). b = 2, latent [4, 8, 8]: 32 lanes per image, so one wavefront spans both
    images, and hw = 64 wraps inside a row."""
    from sta import lib
    from sta.solver import _DT, StepCoef
    L = lib.load()
    b, lat = 2, (4, 8, 8)
    n, hw = 4 * 8 * 8, 8 * 8
    c = StepCoef(7.5, 0.95, 0.31, 0.997, 0.0417, -0.0133, 0.35, 0.0)        # every coefficient of the backward non-zero
    gen = torch.Generator().manual_seed(11)
    g_xn, g_m = torch.randn(b, *lat, generator=gen).cuda(), torch.randn(b, *lat, generator=gen).cuda()
    keep = torch.zeros(b, 1, 8, 8, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else 0
    st = torch.cuda.current_stream().cuda_stream

    def outs():
        return (torch.full((b, *lat), float("nan"), device="cuda"), torch.full((2 * b, *lat), float("nan"), dtype=dtype, device="cuda"),
                torch.full((b, *lat), float("nan"), device="cuda") if with_gmprev else None)

    px, pe, pp = outs()
    lib.check(L.sta_sampler_step_bwd(ptr(g_xn), ptr(g_m if with_gm else None), ptr(px), ptr(pe), ptr(pp), b, n, *c[:7], _DT[dtype], st),
              "sta_sampler_step_bwd")
    mx, me, mp = outs()
    lib.check(L.sta_sampler_step_masked_bwd(ptr(g_xn), ptr(g_m if with_gm else None), ptr(keep), ptr(mx), ptr(me), ptr(mp), b, n, hw, *c[:7],
                                            _DT[dtype], st), "sta_sampler_step_masked_bwd")
    torch.cuda.synchronize()
    assert not torch.isnan(px).any() and not torch.isnan(pe.float()).any() and px.abs().max() > 0 and pe.float().abs().max() > 0
    assert torch.equal(mx.view(torch.int32), px.view(torch.int32))
    assert torch.equal(me.view(torch.int16), pe.view(torch.int16))
    if with_gmprev:
        assert not torch.isnan(pp).any() and torch.equal(mp.view(torch.int32), pp.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 3, 16, 24), (1, 3, 64, 64)])
def test_image_composite_vs_torch_autograd(dtype, shape):
    """sta_image_composite / _bwd against torch autograd in float64: dec with values below -1, above 1 and exactly +-1 (the clamp's
    gradient is inclusive at the bounds); forward within 1 ulp of the output dtype; the backward's zero pattern equals autograd's."""
    from sta import solver
    gen = torch.Generator().manual_seed(shape[-1])
    b, _, hgt, wid = shape
    dec = (1.5 * torch.randn(shape, generator=gen)).to(dtype)
    flat = dec.view(-1)
    flat[0], flat[1], flat[2], flat[3] = 1.0, -1.0, 3.0, -3.0
    assert (dec < -1).any() and (dec > 1).any()
    orig = torch.rand(shape, generator=gen)
    keep_px = _keep(b, hgt, wid, gen, "cpu")
    keep_px.view(-1)[:4] = 0.25                           # the +-1 and out-of-range probes sit on a fractional cell
    g = torch.randn(shape, generator=gen).to(dtype)
    d_ = dec.cuda().requires_grad_(True)
    out = solver.image_composite(d_, orig.cuda(), keep_px.cuda())
    assert out.dtype == dtype
    out.backward(g.cuda())
    d64 = dec.double().requires_grad_(True)
    ref = solver.image_composite_reference(d64, orig.double(), keep_px.double())
    ref.backward(g.double())
    err = (out.detach().cpu().double() - ref.detach()).abs()
    assert (err <= ULP[dtype] * ref.detach().abs() + 1e-7).all(), err.max().item()
    got = d_.grad.cpu().double()
    assert torch.equal(got == 0, d64.grad == 0)
    assert d64.grad.view(-1)[0] != 0 and d64.grad.view(-1)[1] != 0 and d64.grad.view(-1)[2] == 0 and d64.grad.view(-1)[3] == 0
    assert ((got - d64.grad).abs() <= ULP[dtype] * d64.grad.abs() + 1e-7).all()
    kept = (keep_px == 1).expand(shape)
    assert (out.detach().cpu()[kept].double() - orig[kept].double()).abs().max() <= ULP[dtype]
    assert (got[kept] == 0).all()


def test_inpaint_kernels_refuse_misuse_without_launching():
    """A misaligned pointer, hw % 8 != 0, n not a multiple of hw, a null x0 with a mask: STA_E_ARG with a text, nothing launched."""
    from sta import lib
    L = lib.load()
    new = lambda n, dt=torch.float32: torch.zeros(n + 8, device="cuda", dtype=dt)
    fin, o1, o2 = new(256), new(256), new(256)                    # inputs never alias outputs, every launch below stays inside them
    hin, hout = new(512, torch.float16), new(512, torch.float16)
    p, q1, q2, hp, hq, st = fin.data_ptr(), o1.data_ptr(), o2.data_ptr(), hin.data_ptr(), hout.data_ptr(), 0
    coefs = (7.5, 0.6, 0.8, 0.0, 0.9, 0.0, 0.35, 0.0, 0.8, 0.6)
    E_ARG = -1

    def step(x0=p, keep=p, x=p, hw=64, n=256):
        return L.sta_sampler_step_masked(hp, x, 0, 0, x0, keep, p, q1, q2, hq, 1, n, hw, *coefs, lib.STA_F16, st)
    assert step() == 0
    for kw, text in ((dict(x0=0), b"null"), (dict(keep=0), b"null"), (dict(x=p + 4), b"aligned"), (dict(keep=p + 8), b"aligned"),
                     (dict(hw=60, n=240), b"hw"), (dict(hw=64, n=264), b"hw")):
        assert step(**kw) == E_ARG and text in L.sta_last_error(), (kw, L.sta_last_error())
    bwd = lambda keep=p, g=p, hw=64: L.sta_sampler_step_masked_bwd(g, 0, keep, q1, hq, 0, 1, 256, hw, *coefs[:7], lib.STA_F16, st)
    assert bwd() == 0
    assert bwd(keep=0) == E_ARG and b"null" in L.sta_last_error()
    assert bwd(g=p + 4) == E_ARG and b"aligned" in L.sta_last_error()
    assert bwd(hw=12) == E_ARG and b"hw" in L.sta_last_error()
    blend = lambda x0=p, x=p, hw=64, n=256: L.sta_latent_blend(x, x0, p, p, q1, hq, 1, n, hw, 0.8, 0.6, lib.STA_F16, st)
    assert blend() == 0
    assert blend(x0=0) == E_ARG and b"null" in L.sta_last_error()
    assert blend(x=p + 4) == E_ARG and b"aligned" in L.sta_last_error()
    assert blend(hw=20, n=80) == E_ARG and b"hw" in L.sta_last_error()
    comp = lambda orig=p, dec=hp, hw=64: L.sta_image_composite(dec, orig, p, hq, 1, hw, lib.STA_F16, st)      # 3 x 64 elements
    assert comp() == 0
    assert comp(orig=0) == E_ARG and b"null" in L.sta_last_error()
    assert comp(dec=hp + 2) == E_ARG and b"aligned" in L.sta_last_error()
    assert comp(hw=36) == E_ARG and b"hw" in L.sta_last_error()
    cbwd = lambda kp=p, hw=64: L.sta_image_composite_bwd(hp, hp, kp, hq, 1, hw, lib.STA_F16, st)
    assert cbwd() == 0
    assert cbwd(kp=0) == E_ARG and cbwd(kp=p + 4) == E_ARG and cbwd(hw=36) == E_ARG
    torch.cuda.synchronize()
    assert (o1 == 0).all() and (hout == 0).all()                  # zeros in, zeros out: the refused calls wrote nothing else


# ---- the samplers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol_max,tol_mean", [(torch.float16, 0.01, 0.005), (torch.bfloat16, 0.03, 0.02)])
@pytest.mark.parametrize("tag", ["eta0", "eta05"])
def test_inpaint_ddim_trajectory_vs_reference_golden(tag, dtype, tol_max, tol_mean):
    """The reference's masked DDIM (tests/golden/ddim_inpaint.npz) on the fused kernels (sta_latent_blend, sta_sampler_step_masked with
    the 16-bit xin): the final x within the DDIM GPU bounds of tests/test_solver_gpu.py."""
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from tests.test_img2img_cpu import _golden_model
    from tests.test_inpaint_cpu import run_inpaint_golden
    g = np.load(os.path.join(G, "ddim_inpaint.npz"), allow_pickle=False)
    model, _ = _golden_model()
    model = LatentDiffusion(unet_config=model.model.diffusion_model.to("cuda", dtype)).cuda()
    for p in model.parameters():
        p.requires_grad_(False)
    x, seen, _ = run_inpaint_golden(model, g, tag, "cuda")
    assert len(seen) == int(g["S"])
    ref = g[tag + "_x"]
    err = np.abs(x.float().cpu().numpy() - ref)
    print("inpaint ddim %s %s: max %.3f %%, mean %.3f %%" % (tag, dtype, 100 * err.max() / np.abs(ref).max(), 100 * err.mean() / np.abs(ref).mean()))
    assert err.max() <= tol_max * np.abs(ref).max(), (err.max(), np.abs(ref).max())
    assert err.mean() <= tol_mean * np.abs(ref).mean(), (err.mean(), np.abs(ref).mean())


def _rect_keep(side, device="cuda"):
    keep = torch.zeros(1, 1, side, side)
    keep[:, :, side // 4:3 * side // 4, side // 8:5 * side // 8] = 1.0
    keep[:, :, 1, 1:4] = 0.25
    keep[:, :, side - 2, side - 5:side - 2] = 0.5
    return keep.to(device)


def _masked_sample(sampler, S, c, x_T, local_ctx, keep, x0, device="cuda", eta=0.0):
    d = lambda t: t.to(device)
    sampler.sample(S=S, conditioning=d(c), batch_size=1, shape=[4, 32, 32], verbose=False, unconditional_guidance_scale=7.5,
                   unconditional_conditioning=d(gi.load_uncond()), eta=eta, x_T=d(x_T), text_index=0, curr_text="x",
                   bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], seed=1, prompt_idx=0, object_names=["a", "b"],
                   local_conditionings=[d(l) for l in local_ctx], mask=d(keep), x0=d(x0))
    return sampler.last_result["x0"].clone()


def _draws(S, seed, shape=(1, 4, 32, 32)):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=gen) for _ in range(S)]


def test_masked_graph_replay_matches_eager():
    """hipGraph replay == eager launches for masked DDIM (eta 0.5) and masked DPM-Solver++, test_solver_gpu's graph bound (2 % of max)."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    S = 10
    c, local_ctx, x_T = gi.unet_inputs(2, 41)
    model = LatentDiffusion(unet_config=_golden_unet(torch.float16)).cuda()
    x0, keep = _draws(1, 5)[0], _rect_keep(32)
    for cls, kw in ((DDIMSampler, dict(noise=[n.cuda() for n in _draws(S, 6)])), (DPMSolverSampler, {})):
        res = {}
        for graph in (False, True):
            s = cls(model, opt_epochs=0, use_graph=graph, save_images=False, mask_noise=_draws(S, 7), **kw)
            res[graph] = _masked_sample(s, S, c, x_T, local_ctx, keep, x0, eta=0.5).float()
        a, b = res[False], res[True]
        assert (a - b).abs().max() <= 0.02 * a.abs().max(), (cls.__name__, (a - b).abs().max(), a.abs().max())
        s = cls(model, opt_epochs=0, use_graph=True, save_images=False, mask_noise=_draws(S, 7), **kw)
        s.sample(S=S, conditioning=c.cuda(), batch_size=1, shape=[4, 32, 32], verbose=False, unconditional_guidance_scale=7.5,
                 unconditional_conditioning=gi.load_uncond().cuda(), eta=0.5, x_T=x_T.cuda(), text_index=0, curr_text="x",
                 bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], seed=1, prompt_idx=0, object_names=["a", "b"],
                 local_conditionings=[l.cuda() for l in local_ctx])
        plain = s.last_result["x0"].float()
        assert (plain - b).abs().max() > 0.05 * b.abs().max()           # the mask does something


def test_dpm_solver_with_a_mask_agrees_with_its_cpu_restatement():
    """Masked DPM-Solver++(2M), S = 10, K = 2, fp16 on the fused kernels against the same sampler in fp32 on the CPU (oracle ops,
    step_reference_masked), to the graph bound (2 % of max). No reference exists for this combination: the reference's DPM-Solver
    wrapper has no mask path; the blend is the reference's DDIM blend at the solver's own marginal (alpha(t_i), sigma(t_i))."""
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from tests.cpu_backend import oracle_ops
    from tests.test_img2img_cpu import _golden_model
    S = 10
    c, local_ctx, x_T = gi.unet_inputs(2, 41)
    x0, keep = _draws(1, 5)[0], _rect_keep(32, "cpu")
    cpu_model, _ = _golden_model()
    with oracle_ops():
        ref = _masked_sample(DPMSolverSampler(cpu_model, opt_epochs=0, use_graph=False, save_images=False, mask_noise=_draws(S, 7)),
                             S, c, x_T, local_ctx, keep, x0, device="cpu")
    model = LatentDiffusion(unet_config=_golden_unet(torch.float16)).cuda()
    got = _masked_sample(DPMSolverSampler(model, opt_epochs=0, use_graph=True, save_images=False, mask_noise=_draws(S, 7)),
                         S, c, x_T, local_ctx, keep, x0).float().cpu()
    err = (got - ref).abs().max().item()
    print("masked dpm: max err %.3f %% of max" % (100 * err / ref.abs().max().item()))
    assert err <= 0.02 * ref.abs().max().item(), (err, ref.abs().max().item())


def test_batched_masks_equal_one_by_one():
    """decode_batch and sample_batch of two prompts with their own masks and latents against each prompt alone: within 2e-2 of its max,
    test_img2img_gpu's batched bound."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta.pipeline import conditionings
    from tests.test_img2img_gpu import _small_model
    dtype = torch.float16
    model = _small_model(dtype)
    centres, names = [[0.3, 0.4], [0.7, 0.6]], ["cat", "dog"]
    prompts = ["a cat left of a dog", "a dog right of a cat"]
    conds = [conditionings(model, p, names, dtype) for p in prompts]
    S, t_start = 10, 6
    gen = torch.Generator().manual_seed(7)
    lat = [torch.randn(1, 4, 32, 32, generator=gen).cuda() for _ in prompts]
    x0 = [torch.randn(1, 4, 32, 32, generator=gen).cuda() for _ in prompts]
    masks = [_rect_keep(32), 1.0 - _rect_keep(32)]
    qn = _draws(S, 9, (2, 4, 32, 32))
    s = DDIMSampler(model, opt_epochs=0, save_images=False, use_graph=True)
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    single_d, single_s = [], []
    for i, ((uc, c, local), x) in enumerate(zip(conds, lat)):
        s.mask_noise = [n[i:i + 1] for n in qn]
        kw = dict(unconditional_guidance_scale=7.5, unconditional_conditioning=uc, bboxs_curr=centres, object_names=names,
                  local_conditionings=local, mask=masks[i], x0=x0[i])
        single_d.append(s.decode(x, c, t_start, **kw).clone())
        s.sample(S=S, conditioning=c, batch_size=1, shape=[4, 32, 32], verbose=False, eta=0.0, x_T=x, text_index=0, curr_text="x", seed=1,
                 prompt_idx=i, **kw)
        single_s.append(s.last_result["x0"].clone())
    s.mask_noise = qn
    args = ([c for _, c, _ in conds], [uc for uc, _, _ in conds], [centres] * 2, [names] * 2, [local for _, _, local in conds])
    batch_d = s.decode_batch(torch.cat(lat), *args, t_start, curr_texts=prompts, mask=masks, x0=x0).clone()
    s.sample_batch(S, [4, 32, 32], *args, x_T=torch.cat(lat), mask=masks, x0=x0)
    batch_s = s.last_result["x0"].clone()
    assert s._inpaint is None
    for i in range(2):
        for what, batch, single in (("decode", batch_d, single_d), ("sample", batch_s, single_s)):
            err = (batch[i] - single[i][0]).abs().max().item()
            assert err <= 2e-2 * single[i].abs().max().item(), (what, i, err)
    assert (single_d[0] - single_d[1]).abs().max() > 0.05 * single_d[0].abs().max()


def _masked_wopt_epoch(model, loss_model, device, keep, keep_px):
    """Two epochs x 4 masked DPM-Solver++ calls with the pixel-space paste; returns (sampler, dLoss/dW of the tracked epoch)."""
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    c, local_ctx, x_T = gi.unet_inputs(2, 6)
    gen = torch.Generator().manual_seed(12)
    x0 = torch.randn(1, 4, 32, 32, generator=gen)
    orig = torch.rand(1, 3, 256, 256, generator=gen)
    sampler = DPMSolverSampler(model, loss_model=loss_model, opt_epochs=2, save_images=False, use_graph=device != "cpu",
                               mask_noise=_draws(4, 13))
    grads = []
    orig_step = torch.optim.Adam.step
    torch.optim.Adam.step = lambda self, *a, **k: (grads.append(self.param_groups[0]["params"][0].grad.clone()), orig_step(self, *a, **k))[1]
    try:
        sampler.sample(S=4, conditioning=c.to(device), batch_size=1, shape=[4, 32, 32], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond().to(device), x_T=x_T.to(device), text_index=0, curr_text="two things",
                       bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], seed=1, prompt_idx=0, object_names=["The cat", "dog"],
                       local_conditionings=[l.to(device) for l in local_ctx], mask=keep, x0=x0, image=orig, mask_px=keep_px)
    finally:
        torch.optim.Adam.step = orig_step
    return sampler, grads[0][0].float().cpu()


def _wopt_masks():
    keep = torch.zeros(1, 1, 32, 32)
    keep[:, :, :, :12] = 1.0                # the left strip is kept; both object centres (x = 0.3: half in, x = 0.7) are repainted
    keep[:, :, 5, 12:15] = 0.5
    keep_px = keep.repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1)
    return keep, keep_px


_REF = {}


@pytest.mark.parametrize("recompute", ["call", "none"])
def test_masked_tracked_epoch_gradient(recompute):
    """A tracked masked epoch (S = 4, K = 2, bf16, reduced golden UNet) through SolverStepMaskedFn (sta_sampler_step_masked_bwd) and the
    composite backward (sta_image_composite_bwd): dLoss/dW against the fp32 host chain through step_reference_masked and torch ops,
    with the bound of test_solver_gpu's tracked-epoch test (loss within 1 %, max |dW - dW_ref| <= 0.15 max |dW_ref|); every column gets a
    non-zero gradient; a keep == 1 mask over the whole image gives dW == 0 exactly."""
    from ldm.models.diffusion.plms import DCLIPLoss
    from sta.pipeline import set_recompute
    from sta.synth import SyntheticCLIP
    from tests.cpu_backend import oracle_ops
    keep, keep_px = _wopt_masks()
    if not _REF:
        with oracle_ops():
            s, g = _masked_wopt_epoch(_wopt_model(torch.float32, "cpu"), DCLIPLoss(SyntheticCLIP()), "cpu", keep, keep_px)
        _REF.update(grad=g, loss=s.last_result["losses"][0])
    model = _wopt_model(torch.bfloat16, "cuda")
    assert set_recompute(model, recompute) == recompute
    loss_model = DCLIPLoss(SyntheticCLIP().cuda())
    sampler, g = _masked_wopt_epoch(model, loss_model, "cuda", keep, keep_px)
    r = sampler.last_result
    ref = _REF["grad"]
    assert (ref != 0).all() and (g != 0).all(), (ref, g)
    assert abs(r["losses"][0] - _REF["loss"]) <= 0.01 * abs(_REF["loss"]), (r["losses"][0], _REF["loss"])
    e_max = ((g - ref).abs().max() / ref.abs().max()).item()
    print("masked dpm recompute=%s: max |dW - dW_ref| / max |dW_ref| = %.3f" % (recompute, e_max))
    assert e_max <= 0.15, e_max
    img = r["image"].float().cpu()
    kept = (keep_px == 1).expand_as(img)
    assert kept.any() and not kept.all()
    _, g1 = _masked_wopt_epoch(model, loss_model, "cuda", torch.ones(1, 1, 32, 32), torch.ones(1, 1, 256, 256))
    assert (g1 == 0).all(), g1


@pytest.mark.parametrize("form", ["mask", "layout"])
def test_inpaint_script_synthetic_end_to_end(form, tmp_path):
    """scripts/inpaint.py --synthetic --opt_epochs 0 on a generated 256^2 PNG, K = 2 from a --layout: with a --mask file at strength 0.5
    (DDIM decode), and with --mask_from_layout at strength 1 (DPM-Solver++ from noise). The saved image is byte-equal to the input
    outside the mask and differs from it inside."""
    import subprocess
    import sys
    from PIL import Image
    rng = np.random.default_rng(0)
    src = rng.integers(0, 255, (256, 256, 3), dtype=np.uint8)
    init = str(tmp_path / "in.png")
    Image.fromarray(src).save(init)
    layout = tmp_path / "layout.json"
    layout.write_text(json.dumps({"0": {"cat": [0.3, 0.4], "dog": [0.7, 0.6]}}))
    out = tmp_path / "out"
    root = os.path.dirname(G.rstrip("/")).rsplit("/tests", 1)[0]
    script = os.path.join(root, "diffusion-spacetime-attn_amd", "scripts", "inpaint.py")
    if form == "mask":
        repaint = np.zeros((256, 256), dtype=bool)
        repaint[64:200, 40:131] = True                    # not aligned to the 8 x 8 latent cells
        mpath = str(tmp_path / "mask.png")
        Image.fromarray((repaint * 255).astype(np.uint8)).save(mpath)
        extra = ["--mask", mpath, "--strength", "0.5"]
    else:
        from sta import ops
        m = ops.disc_masks([(0.3, 0.4), (0.7, 0.6)], 32, radius_sq=0.2 * 0.2).reshape(2, 32, 32).amax(0).numpy().astype(bool)
        repaint = np.repeat(np.repeat(m, 8, axis=0), 8, axis=1)
        extra = ["--mask_from_layout", "0.2", "--strength", "1.0", "--dpm_solver"]
    env = dict(os.environ, STA_CONV_FIND="0")
    r = subprocess.run([sys.executable, script, "--synthetic", "--init-img", init, "--prompt", "a cat left of a dog", "--layout", str(layout),
                        "--ddim_steps", "10", "--opt_epochs", "0", "--outdir", str(out)] + extra,
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    path = out / "final0_s42_index_0.png"
    assert path.exists(), sorted(os.listdir(out))
    got = np.array(Image.open(path).convert("RGB"))
    assert got.shape == src.shape
    assert repaint.any() and not repaint.all()
    assert (got[~repaint] == src[~repaint]).all()
    assert (got[repaint] != src[repaint]).mean() > 0.5
