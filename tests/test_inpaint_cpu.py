"""Layout-guided inpainting on CPU: the new C-ABI symbols, the samplers' mask= / x0= surface, the masked DDIM trajectory against the
reference's own ddim_sampling(mask=, x0=) (tests/golden/ddim_inpaint.npz, tools/gen_inpaint_golden.py), restatement identities of the
blend on a stub sampler (keep == 0, keep == 1, decode(t_start = S) == sample, the draw order), and scripts/inpaint.py's refusals and
mask construction."""
import os

import numpy as np
import pytest
import torch

from oracle import golden_inputs as gi
from tests.test_img2img_cpu import _decode, _golden_model, _png, _stub_sampler

G = gi.GOLDEN
SHAPE = (1, 4, 8, 8)


def test_inpaint_c_abi_symbols_are_exported():
    from sta import lib
    L = lib.load()
    for name in ("sta_sampler_step_masked", "sta_sampler_step_masked_bwd", "sta_latent_blend", "sta_image_composite",
                 "sta_image_composite_bwd"):
        assert name in lib.SYMBOLS and getattr(L, name) is not None
    assert any(os.path.basename(s) == "sta_inpaint.hip" for s in lib.SOURCES)


def _sample(s, x_T, S, eta=0.0, **kw):
    cond = torch.zeros(1, 77, 8)
    s.sample(S=S, conditioning=cond, batch_size=1, shape=list(x_T.shape[1:]), verbose=False, unconditional_guidance_scale=7.5,
             unconditional_conditioning=cond, eta=eta, x_T=x_T, seed=0, prompt_idx=0, bboxs_curr=[[0.3, 0.4], [0.7, 0.6]],
             object_names=["cat", "dog"], **kw)
    return s.last_result["x0"].clone()


def _spy(s):
    """Records the state (first row of the CFG pair) every UNet call of the stub sampler is fed."""
    seen, inner = [], s.model.apply_model_extra

    def spy(x_in, *a, **k):
        seen.append(x_in[:1].float().clone())
        return inner(x_in, *a, **k)
    s.model.apply_model_extra = spy
    return seen


def _soft_mask(h=8, w=8):
    m = torch.zeros(1, 1, h, w)
    m[:, :, 2:6, 1:5] = 1.0
    m[:, :, 0, :3] = 0.25
    m[:, :, 7, 5] = 0.5
    return m


def test_ddim_accepts_a_mask_and_plms_still_refuses():
    from ldm.models.diffusion.plms import PLMSSampler
    s, calls = _stub_sampler(S=4)
    x = _sample(s, torch.randn(SHAPE), 4, mask=_soft_mask(), x0=torch.randn(SHAPE))
    assert len(calls) == 4 and torch.isfinite(x).all() and s._inpaint is None
    p = PLMSSampler(s.model, opt_epochs=0, save_images=False, use_graph=False)
    with pytest.raises(NotImplementedError, match="inpainting / quantisation / score correction are not on this path"):
        _sample(p, torch.randn(SHAPE), 4, mask=_soft_mask())
    with pytest.raises(ValueError, match="both mask= and x0="):
        _sample(s, torch.randn(SHAPE), 4, mask=_soft_mask())
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        _sample(s, torch.randn(SHAPE), 4, mask=2.0 * _soft_mask(), x0=torch.randn(SHAPE))
    assert s._inpaint is None                                   # cleared in `finally`, also after a refusal


def test_dpm_solver_accepts_a_mask():
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    s, _ = _stub_sampler(S=4)
    d = DPMSolverSampler(s.model, opt_epochs=0, save_images=False, use_graph=False)
    seen = _spy(d)
    x0, n = torch.randn(SHAPE), [torch.randn(SHAPE) for _ in range(4)]
    d.mask_noise = n
    _sample(d, torch.randn(SHAPE), 4, mask=torch.ones(1, 1, 8, 8), x0=x0)
    for i in range(4):          # keep == 1: every call sees the marginal of its own continuous time
        a, b = np.float32(d.tables["alpha_t"][i]), np.float32(d.tables["sigma_t"][i])
        assert torch.equal(seen[i], float(a) * x0 + float(b) * n[i])


# ---- the reference's masked DDIM (tests/golden/ddim_inpaint.npz) ---------------------------------------------------------------------
def run_inpaint_golden(model, g, tag, device, graph=False):
    """The masked S-call trajectory with the golden's W, x_T, x0, mask and recorded draws; returns (x, the state of every call, the
    timesteps)."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta import prompt_state
    S = int(g["S"])
    c, local_ctx, _ = gi.unet_inputs(int(g["K"]), int(g["input_seed"]))
    noise = [torch.from_numpy(n).to(device) for n in g[tag + "_noise"]] if tag + "_noise" in g else None
    qnoise = [torch.from_numpy(n).to(device) for n in g[tag + "_qnoise"]]
    s = DDIMSampler(model, opt_epochs=0, use_graph=graph, save_images=False, noise=noise, mask_noise=qnoise)
    s.make_schedule(S, ddim_eta=float(g[tag + "_eta"]), verbose=False)
    seen, inner = [], model.apply_model_extra

    def spy(x_in, *a, **k):
        seen.append(x_in[:1].float().clone())
        return inner(x_in, *a, **k)
    model.apply_model_extra = spy
    tr = s._time_range()
    try:
        s._set_inpaint(torch.from_numpy(g["mask"]), torch.from_numpy(g["x0"]))
        with torch.no_grad():
            prompt_state.begin_prompt([l.to(device) for l in local_ctx], first_timestep=int(tr[0]))
            x = s._trajectory(torch.from_numpy(g["x_T"]).to(device), c.to(device), gi.load_uncond().to(device), float(g["scale"]), tr,
                              torch.from_numpy(g["W"]).to(device), [list(cc) for cc in g["centres"]], 0, graph=graph)
    finally:
        s._inpaint = None
        del model.apply_model_extra
    return x, seen, [int(t) for t in tr]


@pytest.mark.parametrize("tag", ["eta0", "eta05"])
def test_inpaint_ddim_matches_reference(tag):
    """The input of every call and the final x of the masked DDIM trajectory against the reference's ddim_sampling(mask=, x0=) with
    the per-call weight columns, within the DDIM CPU bound of test_img2img_cpu (relative max error < 2e-3)."""
    from tests.cpu_backend import oracle_ops
    g = np.load(os.path.join(G, "ddim_inpaint.npz"), allow_pickle=False)
    model, checksum = _golden_model()
    assert abs(checksum - float(g["checksum"])) <= 1e-6 * abs(float(g["checksum"]))
    with oracle_ops():
        x, seen, ts = run_inpaint_golden(model, g, tag, "cpu")
    assert ts == [int(t) for t in g[tag + "_timesteps"]]
    assert len(seen) == int(g["S"])
    for i, ref in enumerate(g[tag + "_xs"]):
        err = np.abs(seen[i].numpy() - ref).max() / max(1.0, np.abs(ref).max())
        assert err < 2e-3, (tag, i, err)
    ref = g[tag + "_x"]
    err = np.abs(x.numpy() - ref).max() / np.abs(ref).max()
    assert err < 2e-3, (tag, err)


# ---- restatement identities on the stub sampler --------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_keep_zero_everywhere_is_the_unmasked_trajectory(eta):
    S = 6
    x_T, x0 = torch.randn(SHAPE), torch.randn(SHAPE)
    noise = [torch.randn(SHAPE) for _ in range(S)]
    s, _ = _stub_sampler(S=S, eta=eta)
    s.noise = noise
    a = _sample(s, x_T, S, eta=eta)
    s2, _ = _stub_sampler(S=S, eta=eta)
    s2.noise, s2.mask_noise = noise, [torch.randn(SHAPE) for _ in range(S)]
    b = _sample(s2, x_T, S, eta=eta, mask=torch.zeros(1, 1, 8, 8), x0=x0)
    assert torch.equal(a, b)


def test_keep_one_everywhere_feeds_q_sample_of_x0_to_every_call():
    from sta import solver
    S = 6
    x0 = torch.randn(SHAPE)
    n = [torch.randn(SHAPE) for _ in range(S)]
    s, _ = _stub_sampler(S=S, eta=0.5)
    s.mask_noise = n
    seen = _spy(s)
    _sample(s, torch.randn(SHAPE), S, eta=0.5, mask=torch.ones(1, 1, 8, 8), x0=x0)
    acp = s.model.alphas_cumprod
    assert len(seen) == S
    for i in range(S):
        t = int(s.tables["t_in"][i])
        want = s.stochastic_encode(x0, torch.tensor([t]), use_original_steps=True, noise=n[i])       # q_sample(x0, t_i, n_i)
        assert torch.equal(seen[i], want), i
        q_a, q_b = solver.blend_coefs(acp, t)
        assert q_a == float(torch.sqrt(acp[t])) and q_b == float(torch.sqrt(1.0 - acp[t]))


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_masked_decode_with_t_start_s_equals_masked_sample(eta):
    S = 6
    x, x0, mask = torch.randn(SHAPE), torch.randn(SHAPE), _soft_mask()
    noise, qn = [torch.randn(SHAPE) for _ in range(S)], [torch.randn(SHAPE) for _ in range(S)]
    s, _ = _stub_sampler(S=S, eta=eta)
    s.noise, s.mask_noise = noise, qn
    a = _decode(s, x, S, mask=mask, x0=x0).clone()
    assert s._inpaint is None and s._start == 0
    s2, _ = _stub_sampler(S=S, eta=eta)
    s2.noise, s2.mask_noise = noise, qn
    b = _sample(s2, x, S, eta=eta, mask=mask, x0=x0)
    assert torch.equal(a, b)
    s3, _ = _stub_sampler(S=S, eta=eta)
    s3.noise, s3.mask_noise = noise, qn
    assert not torch.equal(b, _sample(s3, x, S, eta=eta))       # the mask does something


def test_blend_and_eta_draws_interleave_in_the_reference_order():
    """blend draw of call i, eta draw of call i, blend draw of call i + 1, ...: S blend draws and S eta draws, none after the last step."""
    S, t_start = 5, 3
    order = []
    s, _ = _stub_sampler(S=S, eta=0.5)
    s.mask_noise = lambda i, shape, device: (order.append(("blend", i)), torch.zeros(shape))[1]
    s.noise = lambda i, shape, device: (order.append(("eta", i)), torch.zeros(shape))[1]
    _sample(s, torch.randn(SHAPE), S, eta=0.5, mask=_soft_mask(), x0=torch.randn(SHAPE))
    assert order == [(k, i) for i in range(S) for k in ("blend", "eta")]
    del order[:]
    _decode(s, torch.randn(SHAPE), t_start, mask=_soft_mask(), x0=torch.randn(SHAPE))
    assert order == [(k, i) for i in range(t_start) for k in ("blend", "eta")]     # indexed by the call of the decode, as `noise=`


def test_only_one_minus_keep_of_the_gradient_flows_through_a_blend():
    from sta import solver
    c = solver.StepCoef(5.0, 0.6, 0.8, 0.0, 0.9, 0.0, 0.35, 0.22)
    keep = _soft_mask()
    bl = solver.Blend(torch.randn(SHAPE), keep, torch.randn(SHAPE), 0.7, 0.714)
    eps = torch.randn(2, 4, 8, 8)
    x = torch.randn(SHAPE, requires_grad=True)
    xr = x.detach().clone().requires_grad_(True)
    noise = torch.randn(SHAPE)
    g = torch.randn(SHAPE)
    xn, _, _ = solver.solver_step_masked(eps, x, None, noise, c, bl)
    xn.backward(g)
    rn, _, _ = solver.solver_step(eps, xr, None, noise, c)
    rn.backward((1.0 - keep) * g)
    assert torch.allclose(x.grad, xr.grad, rtol=1e-6, atol=1e-7)
    assert (x.grad[:, :, 2:6, 1:5] == 0).all()


def test_per_image_arguments_may_be_lists():
    """mask= / x0= as per-image lists (the batched forms' convention) mean the same as the stacked tensors."""
    S = 4
    x_T, x0, mask = torch.randn(SHAPE), torch.randn(SHAPE), _soft_mask()
    qn = [torch.randn(SHAPE) for _ in range(S)]
    s1, _ = _stub_sampler(S=S)
    s1.mask_noise = qn
    one = _sample(s1, x_T, S, mask=mask, x0=x0)
    s2, _ = _stub_sampler(S=S)
    s2.mask_noise = qn
    assert torch.equal(one, _sample(s2, x_T, S, mask=[mask], x0=[x0]))
    with pytest.raises(ValueError, match="batch of 1"):
        _sample(s2, x_T, S, mask=[mask, mask], x0=[x0, x0])


def test_pixel_space_paste_forms_the_result_and_the_saved_pixels():
    """image= / mask_px=: last_result["image"] is the composite; the saved 8-bit pixels are the original's where keep_px == 1."""
    from sta import solver
    S = 4
    s, _ = _stub_sampler(S=S)
    orig_u8 = torch.randint(0, 256, (1, 3, 64, 64), dtype=torch.uint8)
    orig = orig_u8.float() / 255.0
    keep_px = torch.ones(1, 1, 64, 64)
    keep_px[:, :, 16:48, 8:40] = 0.0
    keep = 1.0 - torch.nn.functional.max_pool2d(1.0 - keep_px, 8)
    _sample(s, torch.randn(SHAPE), S, mask=keep, x0=torch.randn(SHAPE), image=orig, mask_px=keep_px)
    img = s.last_result["image"]
    dec = s.model.decode_first_stage(s.last_result["x0"])
    assert torch.equal(img, solver.image_composite_reference(dec, orig, keep_px))
    kept = keep_px.expand(1, 3, 64, 64) == 1
    assert torch.equal(img[kept], orig[kept]) and not torch.equal(img[~kept], orig[~kept])
    s._set_inpaint(keep, torch.randn(SHAPE), orig, keep_px)
    try:
        arr = s._to_u8(img[0].half(), 0)                      # a 16-bit composite does not round-trip k / 255; the paste is exact
    finally:
        s._inpaint = None
    want = orig_u8[0].permute(1, 2, 0).numpy()
    k2 = (keep_px[0, 0] == 1).numpy()
    assert (arr[k2] == want[k2]).all()


# ---- scripts/inpaint.py -------------------------------------------------------------------------------------------------------------
def _script():
    import importlib.util
    import sys
    path = os.path.join(os.path.dirname(G.rstrip("/")).rsplit("/tests", 1)[0], "diffusion-spacetime-attn_amd", "scripts", "inpaint.py")
    spec = importlib.util.spec_from_file_location("inpaint_script", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules.pop("img2img", None)          # the script's sibling import: keep it out of other tests' namespace
    return mod


def _mask_png(path, arr):
    from PIL import Image
    Image.fromarray(arr.astype(np.uint8)).save(path)
    return path


@pytest.mark.parametrize("args,what", [
    (["--mask_from_layout", "0.2", "--layout", "x.json", "--plms"], "PLMS"),
    (["--mask_from_layout", "0.2", "--layout", "x.json", "--dpm_solver", "--strength", "0.5"], "DDIM"),
    (["--mask_from_layout", "0.2", "--layout", "x.json", "--n_samples", "2"], "n_samples"),
    (["--mask_from_layout", "0.2", "--layout", "x.json", "--strength", "0.0"], "strength"),
    (["--mask_from_layout", "0.2", "--layout", "x.json", "--strength", "1.5"], "strength"),
    (["--mask_from_layout", "0.2", "--layout", "x.json", "--strength", "0.05", "--ddim_steps", "10"], "t_enc"),
    ([], "exactly one"),
    (["--mask", "m.png", "--mask_from_layout", "0.2", "--layout", "x.json"], "exactly one"),
    (["--mask_from_layout", "0.2"], "--layout"),
])
def test_inpaint_cli_refusals(args, what, tmp_path, monkeypatch):
    mod = _script()
    built = []
    monkeypatch.setattr("sta.pipeline.build_sd_v1", lambda *a, **k: built.append(1))
    img = _png(str(tmp_path / "a.png"), 64, 64)
    with pytest.raises(SystemExit) as e:
        mod.main(["--init-img", img, "--synthetic"] + args)
    assert what in str(e.value) and not built


def test_inpaint_cli_refuses_masks(tmp_path, monkeypatch):
    """A mask of another size than the image, a mask that repaints nothing, a prompt without layout objects."""
    import json
    mod = _script()
    built = []
    monkeypatch.setattr("sta.pipeline.build_sd_v1", lambda *a, **k: built.append(1))
    img = _png(str(tmp_path / "a.png"), 64, 64)
    small = _mask_png(str(tmp_path / "small.png"), np.full((32, 32), 255))
    black = _mask_png(str(tmp_path / "black.png"), np.zeros((64, 64)))
    layout = tmp_path / "l.json"
    layout.write_text(json.dumps({"1": {"cat": [0.5, 0.5]}}))
    for args, what in ((["--mask", small], "32 x 32"), (["--mask", black], "repaints nothing"),
                       (["--mask_from_layout", "0.2", "--layout", str(layout)], "no layout objects")):
        with pytest.raises(SystemExit) as e:
            mod.main(["--init-img", img, "--synthetic", "--prompt", "a cat"] + args)
        assert what in str(e.value) and not built, (what, str(e.value))


def test_inpaint_allows_dpm_solver_at_strength_one():
    mod = _script()
    opt = mod.build_parser().parse_args(["--init-img", "a.png", "--mask", "m.png", "--dpm_solver", "--strength", "1.0", "--ddim_steps", "20",
                                         "--opt_epochs", "0"])
    assert mod.check_options(opt) == 20
    opt = mod.build_parser().parse_args(["--init-img", "a.png", "--mask", "m.png", "--strength", "0.5", "--ddim_steps", "20", "--opt_epochs", "0"])
    assert mod.check_options(opt) == 10


def test_mask_polarity_and_max_pool(tmp_path):
    """White = repaint (the CompVis convention), binarised at 0.5; a latent cell is repainted if any of its 8 x 8 pixels is; the sampler
    gets keep = 1 - repaint (1 = keep the original, the reference's ddim.py convention)."""
    mod = _script()
    px = np.zeros((16, 16))
    px[3, 12] = 255            # one white pixel in the top-right cell
    px[8:16, 0:8] = 127        # just below 0.5: black
    px[15, 15] = 128           # just above 0.5: white
    path = _mask_png(str(tmp_path / "m.png"), px)
    repaint_px = mod.load_mask(path, 16)
    assert repaint_px.shape == (1, 1, 16, 16) and repaint_px.sum() == 2 and repaint_px[0, 0, 3, 12] == 1 and repaint_px[0, 0, 15, 15] == 1
    assert torch.equal(mod.latent_repaint(repaint_px), torch.tensor([[[[0.0, 1.0], [0.0, 1.0]]]]))
    opt = mod.build_parser().parse_args(["--init-img", "a.png", "--mask", path])
    keep, keep_px = mod.masks_for(opt, 0, {}, path, 16)
    assert torch.equal(keep, torch.tensor([[[[1.0, 0.0], [1.0, 0.0]]]]))
    assert torch.equal(keep_px, 1.0 - repaint_px)


def test_mask_from_layout_is_the_union_of_the_blocks_discs():
    mod = _script()
    g = np.load(os.path.join(G, "masks.npz"), allow_pickle=False)
    centres = [tuple(c) for c in g["centres"]]
    for dim in g["dims"]:
        dim = int(dim)
        ref = np.unpackbits(g["mask_%d" % dim], axis=1)[:, : dim * dim].reshape(len(centres), dim, dim)
        union = ref.max(0).astype(np.float32)
        got = mod.layout_repaint(centres, dim, 0.2)
        assert got.shape == (1, 1, dim, dim) and (got[0, 0].numpy() == union).all(), dim
    opt = mod.build_parser().parse_args(["--init-img", "a.png", "--mask_from_layout", "0.2", "--layout", "l.json"])
    keep, keep_px = mod.masks_for(opt, 0, {"a": list(centres[0]), "b": list(centres[1])}, None, 256)
    want = 1.0 - mod.layout_repaint(centres[:2], 32, 0.2)
    assert torch.equal(keep, want) and keep_px.shape == (1, 1, 256, 256)
    assert torch.equal(torch.nn.functional.max_pool2d(keep_px, 8), keep) and torch.equal(-torch.nn.functional.max_pool2d(-keep_px, 8), keep)
