"""img2img on CPU: the VAE encoder + posterior against the reference's own (tests/golden/vae_encoder*.{npz,json},
tools/gen_img2img_golden.py), build_sd_v1(with_encoder=True) leaving the default build's weights alone, DDIM's stochastic_encode and
decode (the timestep-tied weight columns, the columns a decode never calls), and the new C-ABI symbols."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import golden_inputs as gi

G = gi.GOLDEN


def _vae_with_encoder(seed):
    from ldm.models.autoencoder import AutoencoderKL
    from sta import pipeline, synth
    vae = AutoencoderKL().add_encoder().eval()
    synth.seeded_fill_(pipeline.encoder_part(vae), seed)
    return vae


def test_encoder_state_dict_names_and_shapes_match_reference():
    from ldm.models.autoencoder import AutoencoderKL
    from sta import pipeline
    ref = json.load(open(os.path.join(G, "vae_encoder_state_dict.json")))
    got = [[k, list(v.shape)] for k, v in pipeline.encoder_part(AutoencoderKL().add_encoder()).state_dict().items()]
    assert got == ref["names"]


def test_encoder_and_posterior_match_reference_golden():
    """Eager fp32 encoder + quant_conv + DiagonalGaussianDistribution against the reference's modules with the same seeded weights."""
    gz = np.load(os.path.join(G, "vae_encoder.npz"))
    vae = _vae_with_encoder(int(gz["seed"]))
    x = torch.from_numpy(gz["image_u8"]).float() / 255.0 * 2.0 - 1.0
    with torch.no_grad():
        h = vae.encode_moments_input(x)
        post = vae.encode(x)
        z = post.sample(noise=torch.from_numpy(gz["n_post"]))
    for got, key in ((h, "h"), (post.parameters, "moments"), (z, "z")):
        ref = torch.from_numpy(gz[key])
        err = (got - ref).abs().max().item()
        assert err <= 1e-5 * ref.abs().max().item(), (key, err)


def test_posterior_sample_draws_cpu_randn_as_the_reference():
    from ldm.models.autoencoder import DiagonalGaussianDistribution
    from ldm.models.diffusion.ddpm import LatentDiffusion
    moments = torch.randn(2, 8, 4, 4)
    post = DiagonalGaussianDistribution(moments)
    torch.manual_seed(42)
    got = post.sample()
    torch.manual_seed(42)
    want = post.mean + post.std * torch.randn(post.mean.shape)
    assert torch.equal(got, want)
    ld = LatentDiffusion(unet_config=torch.nn.Identity())
    torch.manual_seed(42)
    assert torch.equal(ld.get_first_stage_encoding(post), ld.scale_factor * want)
    assert torch.equal(ld.get_first_stage_encoding(moments), ld.scale_factor * moments)


def test_build_with_encoder_keeps_the_default_weights():
    """build_sd_v1(with_encoder=True): same UNet and decoder parameters (names, order, values) as the default build, plus the encoder."""
    from sta.pipeline import build_sd_v1
    kw = dict(device="cpu", dtype=torch.float32, unet_overrides=dict(model_channels=32), real_text_encoder=False)
    a = build_sd_v1(**kw)
    b = build_sd_v1(with_encoder=True, **kw)
    pa, pb = list(a.named_parameters()), list(b.named_parameters())
    assert [n for n, _ in pa] == [n for n, _ in pb][:len(pa)]
    assert all(n.startswith(("first_stage_model.encoder.", "first_stage_model.quant_conv.")) for n, _ in pb[len(pa):])
    assert len(pb) > len(pa)
    for (n, x), (_, y) in zip(pa, pb):
        assert torch.equal(x, y), n
    assert not a.first_stage_model.has_encoder and b.first_stage_model.has_encoder


def _stub_sampler(S=10, eta=0.0, opt_epochs=0):
    """DDIMSampler around a LatentDiffusion whose UNet call is a stub that records (timestep, weight column, announced first
    timestep) and returns eps = x * 0.1 + sum(coef) / 100: differentiable in the column it was handed."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from sta import prompt_state
    model = LatentDiffusion(unet_config=torch.nn.Conv2d(4, 4, 1))
    calls = []

    def apply_model_extra(x, text_index, t, cond, coef=None, bboxs_curr=None, **kw):
        calls.append((int(t[0]), coef.detach().clone(), prompt_state.first_timestep()))
        return 0.1 * x + 0.01 * coef.sum()
    model.apply_model_extra = apply_model_extra

    class _FirstStage(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1), requires_grad=False)

        def decode(self, z):
            return torch.nn.functional.interpolate(z[:, :3], scale_factor=8.0)

    class _Loss:
        def forward_2(self, image, text):
            return image.mean()

        def forward_3(self, image, text):
            return image.mean()
    model.first_stage_model = _FirstStage()
    s = DDIMSampler(model, opt_epochs=opt_epochs, save_images=False, use_graph=False, loss_model=_Loss())
    s.make_schedule(S, ddim_eta=eta, verbose=False)
    return s, calls


def _decode(s, x, t_start, **kw):
    cond = torch.zeros(1, 77, 8)
    return s.decode(x, cond, t_start, unconditional_guidance_scale=7.5, unconditional_conditioning=cond,
                    bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], object_names=["cat", "dog"], **kw)


def test_stochastic_encode_indexes_the_ddim_tables():
    s, _ = _stub_sampler(S=10)
    x0 = torch.randn(2, 4, 8, 8)
    n = torch.randn(2, 4, 8, 8)
    a = torch.tensor(s.tables["a"], dtype=torch.float32)
    for t in (1, 6, 9):
        got = s.stochastic_encode(x0, torch.tensor([t, t]), noise=n)
        want = torch.sqrt(a[t]) * x0 + torch.sqrt(1.0 - a[t]) * n
        assert torch.equal(got, want)
    acp = s.model.alphas_cumprod
    got = s.stochastic_encode(x0, torch.tensor([500, 500]), use_original_steps=True, noise=n)
    assert torch.equal(got, torch.sqrt(acp[500]) * x0 + torch.sqrt(1.0 - acp[500]) * n)


def test_decode_runs_the_last_t_start_timesteps_with_tied_columns():
    """Call j of a t_start-call decode runs at the timestep of call S - t_start + j of a full trajectory and uses column S - t_start + j;
    the blocks are told the decode's first timestep. The reference's off-by-one: noised to index t_enc, first call at index t_enc - 1."""
    S, t_enc = 10, 6
    s, calls = _stub_sampler(S=S)
    _decode(s, torch.randn(1, 4, 8, 8), t_enc)
    ts = [c[0] for c in calls]
    assert ts == [int(v) for v in s.tables["t_in"][S - t_enc:]]
    assert ts[0] == int(s.ddim_timesteps[t_enc - 1])
    assert all(c[2] == ts[0] for c in calls)
    W = s.last_result["W"]
    assert len(calls) == t_enc
    # a fixed W holds 5 / K everywhere: identify the column by handing out a W whose columns differ
    s2, calls2 = _stub_sampler(S=S)
    s2.weight_init = 5.0
    orig = torch.full
    cols = torch.arange(S, dtype=torch.float32)

    def full(size, fill, **kw):
        t = orig(size, fill, **kw)
        if isinstance(size, tuple) and len(size) == 3 and size[-1] == S:
            t = t + cols
        return t
    torch.full = full
    try:
        _decode(s2, torch.randn(1, 4, 8, 8), t_enc)
    finally:
        torch.full = orig
    used = [round(float(c[1][0] - 2.5), 4) for c in calls2]
    assert used == [float(v) for v in range(S - t_enc, S)]
    assert W.shape == (2, S)


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_decode_with_t_start_s_equals_sample_from_the_same_latent(eta):
    """decode(x, t_start = S) is the whole DDIM trajectory from x, as sample(x_T = x) runs it (same calls, same noise)."""
    S = 6
    x = torch.randn(1, 4, 8, 8)
    noise = [torch.randn(1, 4, 8, 8) for _ in range(S)]
    s, _ = _stub_sampler(S=S, eta=eta)
    s.noise = noise
    a = _decode(s, x, S).clone()
    s2, _ = _stub_sampler(S=S, eta=eta)
    s2.noise = noise
    cond = torch.zeros(1, 77, 8)
    s2.sample(S=S, conditioning=cond, batch_size=1, shape=[4, 8, 8], verbose=False, unconditional_guidance_scale=7.5,
              unconditional_conditioning=cond, eta=eta, x_T=x, seed=0, prompt_idx=0, bboxs_curr=[[0.3, 0.4], [0.7, 0.6]],
              object_names=["cat", "dog"])
    assert torch.equal(a, s2.last_result["x0"])


def test_decode_opt_epochs_leave_uncalled_columns_at_their_initial_value():
    S, t_enc = 10, 4
    s, _ = _stub_sampler(S=S, opt_epochs=3)
    _decode(s, 0.01 * torch.randn(1, 4, 8, 8), t_enc, curr_text="a cat")
    W = s.last_result["W"]
    init = torch.full((2, S), 5.0 / 2)
    assert torch.equal(W[:, :S - t_enc], init[:, :S - t_enc])
    assert (W[:, S - t_enc:] != init[:, S - t_enc:]).all()
    assert len(s.last_result["losses"]) == 2


def test_decode_refuses_original_steps_and_bad_t_start():
    s, _ = _stub_sampler(S=10)
    with pytest.raises(NotImplementedError):
        _decode(s, torch.randn(1, 4, 8, 8), 5, use_original_steps=True)
    for t in (0, 11):
        with pytest.raises(ValueError):
            _decode(s, torch.randn(1, 4, 8, 8), t)


def test_new_c_abi_symbols_are_exported():
    from sta import lib
    L = lib.load()
    for name in ("sta_conv3x3_s2_nhwc_supported", "sta_conv3x3_s2_stats_slots", "sta_conv3x3_s2_nhwc", "sta_vae_encode_step"):
        assert name in lib.SYMBOLS and getattr(L, name) is not None
    assert L.sta_conv3x3_s2_nhwc_supported(2, 512, 512, 128, 128) == 1
    assert L.sta_conv3x3_s2_nhwc_supported(2, 80, 80, 128, 128) == 0
    assert L.sta_conv3x3_s2_stats_slots(128, 128) == 2 * 8 * 4


# ---- the reference's img2img DDIM (tests/golden/ddim_img2img.npz, tools/gen_img2img_golden.py) -------------------------------------
def _golden_model():
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from sta.synth import seeded_fill_
    meta = json.load(open(os.path.join(G, "unet_state_dict_keys.json")))
    unet = UNetModel(**meta["cfg"]).eval()
    checksum = seeded_fill_(unet, 21)
    return LatentDiffusion(unet_config=unet), checksum


def run_img2img_golden(model, g, tag, device, graph=False):
    """stochastic_encode + the decode trajectory with the golden's W (its column S - t_enc + j at decode call j); returns
    (z_enc, x, the state x of every call)."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta import prompt_state
    S, t_enc = int(g["S"]), int(g["t_enc"])
    c, local_ctx, _ = gi.unet_inputs(int(g["K"]), int(g["input_seed"]))
    noise = [torch.from_numpy(n).to(device) for n in g[tag + "_noise"]] if tag + "_noise" in g else None
    s = DDIMSampler(model, opt_epochs=0, use_graph=graph, save_images=False, noise=noise)
    s.make_schedule(S, ddim_eta=float(g[tag + "_eta"]), verbose=False)
    z = s.stochastic_encode(torch.from_numpy(g["x0"]).to(device), torch.tensor([t_enc]), noise=torch.from_numpy(g["n_enc"]).to(device))
    seen, inner = [], model.apply_model_extra

    def spy(x_in, *a, **k):
        seen.append(x_in[:1].float().clone())
        return inner(x_in, *a, **k)
    model.apply_model_extra = spy
    tr = s._time_range()
    s._start = S - t_enc
    try:
        with torch.no_grad():
            prompt_state.begin_prompt([l.to(device) for l in local_ctx], first_timestep=int(tr[s._start]))
            x = s._trajectory(z.clone(), c.to(device), gi.load_uncond().to(device), float(g["scale"]), tr,
                              torch.from_numpy(g["W"]).to(device), [list(cc) for cc in g["centres"]], 0, graph=graph)
    finally:
        s._start = 0
        del model.apply_model_extra
    return z, x, seen, [int(t) for t in tr[S - t_enc:]]


@pytest.mark.parametrize("tag", ["eta0", "eta05"])
def test_img2img_ddim_matches_reference(tag):
    """stochastic_encode (bitwise: the same float32 tables) and the t_enc-call decode trajectory against the reference's own img2img
    sampling with the timestep-tied weight columns, within the DDIM CPU bound (2e-3 of max |x|)."""
    from tests.cpu_backend import oracle_ops
    g = np.load(os.path.join(G, "ddim_img2img.npz"), allow_pickle=False)
    model, checksum = _golden_model()
    assert abs(checksum - float(g["checksum"])) <= 1e-6 * abs(float(g["checksum"]))
    with oracle_ops():
        z, x, seen, ts = run_img2img_golden(model, g, tag, "cpu")
    np.testing.assert_array_equal(z.numpy(), g[tag + "_z_enc"])
    assert ts == [int(t) for t in g[tag + "_timesteps"]]
    assert len(seen) == int(g["t_enc"])
    for i, ref in enumerate(g[tag + "_xs"]):
        err = np.abs(seen[i].numpy() - ref).max() / max(1.0, np.abs(ref).max())
        assert err < 2e-3, (tag, i, err)
    ref = g[tag + "_x"]
    err = np.abs(x.numpy() - ref).max() / np.abs(ref).max()
    assert err < 2e-3, (tag, err)


# ---- scripts/img2img.py: refusals, --init-img forms, seed / draw order --------------------------------------------------------------
def _script():
    import importlib.util
    path = os.path.join(os.path.dirname(G.rstrip("/")).rsplit("/tests", 1)[0], "diffusion-spacetime-attn_amd", "scripts", "img2img.py")
    spec = importlib.util.spec_from_file_location("img2img_script", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _png(path, w, h, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    Image.fromarray(rng.integers(0, 255, size=(h, w, 3), dtype=np.uint8)).save(path)
    return path


@pytest.mark.parametrize("args,what", [
    (["--plms"], "PLMS"),
    (["--dpm_solver"], "DDIM"),
    (["--n_samples", "2"], "n_samples"),
    (["--strength", "1.0", "--ddim_steps", "10"], "t_enc"),
    (["--strength", "0.05", "--ddim_steps", "10"], "t_enc"),
])
def test_img2img_cli_refusals(args, what, tmp_path, monkeypatch):
    mod = _script()
    built = []
    monkeypatch.setattr("sta.pipeline.build_sd_v1", lambda *a, **k: built.append(1))
    img = _png(str(tmp_path / "a.png"), 64, 64)
    with pytest.raises(SystemExit) as e:
        mod.main(["--init-img", img, "--synthetic"] + args)
    assert what in str(e.value) and not built


@pytest.mark.parametrize("sizes,what", [([(96, 64)], "not square"), ([(96, 96)], "multiple of 64"), ([(64, 64), (128, 128)], "mixed")])
def test_img2img_cli_refuses_images(sizes, what, tmp_path, monkeypatch):
    mod = _script()
    built = []
    monkeypatch.setattr("sta.pipeline.build_sd_v1", lambda *a, **k: built.append(1))
    for i, (w, h) in enumerate(sizes):
        _png(str(tmp_path / ("%d.png" % i)), w, h, i)
    prompts = tmp_path / "p.txt"
    prompts.write_text("\n".join("prompt %d" % i for i in range(len(sizes))))
    with pytest.raises(SystemExit) as e:
        mod.main(["--init-img", str(tmp_path), "--from-file", str(prompts), "--synthetic", "--strength", "0.5"])
    assert what in str(e.value) and not built


def test_img2img_init_img_file_and_directory_forms(tmp_path):
    """One file: every prompt starts from it. A directory: prompt i from <dir>/<i>.png|jpg; a missing one is refused. load_img rounds
    the sides down to a multiple of 32 and scales to [-1, 1]."""
    mod = _script()
    f = _png(str(tmp_path / "one.png"), 100, 70)
    assert mod.image_paths(f, 3) == [f, f, f]
    im = mod.load_img(f)
    assert im.shape == (1, 3, 64, 96) and float(im.min()) >= -1.0 and float(im.max()) <= 1.0
    d = tmp_path / "dir"
    d.mkdir()
    _png(str(d / "0.png"), 64, 64)
    _png(str(d / "1.jpg"), 64, 64)
    assert mod.image_paths(str(d), 2) == [str(d / "0.png"), str(d / "1.jpg")]
    with pytest.raises(SystemExit):
        mod.image_paths(str(d), 3)


def test_img2img_seed_and_draw_order():
    """Draw 1: the posterior noise is seeded with --seed right before each image's draw on the CPU default generator (what
    DiagonalGaussianDistribution.sample draws right after torch.manual_seed(seed)); draw 2: the encode noise is seeded again right before
    each prompt's draw. Neither depends on what was drawn before."""
    from ldm.models.autoencoder import DiagonalGaussianDistribution
    mod = _script()
    shape = (1, 4, 8, 8)
    a = mod.posterior_noise(42, shape)
    torch.randn(100)
    b = mod.posterior_noise(42, shape)
    assert torch.equal(a, b)
    post = DiagonalGaussianDistribution(torch.zeros(1, 8, 8, 8))
    torch.manual_seed(42)
    assert torch.equal(post.sample(), post.mean + post.std * a)
    e1 = mod.encode_noise(42, shape, "cpu")
    torch.randn(7)
    assert torch.equal(e1, mod.encode_noise(42, shape, "cpu"))
