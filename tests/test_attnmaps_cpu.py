"""Attention heat maps without a GPU: the torch reference of the token maps against the oracle's attention maps, the token
weights, AttnCapture over a trajectory with the oracle-backed blocks (tests/cpu_backend.py), the CLI flags, and the refusals of
sta_xattn_token_maps (fake pointers: none of these calls may reach a launch). The kernel is checked in test_attnmaps_gpu.py."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import golden_inputs as gi
from oracle import xattn_oracle as orc
from sta.synth import seeded_fill_
from tests.cpu_backend import oracle_ops

G = gi.GOLDEN
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------
# the reference formula
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,heads,K", [(64, 64, 8, 1), (100, 128, 4, 3), (48, 192, 8, 0)])
def test_reference_matches_oracle_maps(N, C, heads, K):
    from sta import attnmaps
    g = torch.Generator().manual_seed(3)
    I, M = 2, 77
    q = torch.randn(2 * I, N, C, generator=g, dtype=torch.float64)
    k = torch.randn(I * (K + 2), M, C, generator=g, dtype=torch.float64) * 0.7
    sel = [1, 0, 1] + [2 + i for i in range(K)]
    w = torch.randn(I, len(sel), M, generator=g, dtype=torch.float64)
    got = attnmaps.token_maps_reference(q, k, sel, w, heads, (C // heads) ** -0.5)
    assert got.dtype == torch.float64 and got.shape == (I, len(sel), N)
    for i in range(I):
        ki = k[i * (K + 2):(i + 1) * (K + 2)]
        _, maps = orc.fused_xattn(q[2 * i:2 * i + 2], ki, ki, torch.zeros(K, N, dtype=torch.bool), torch.zeros(K, dtype=torch.float64),
                                  heads, (C // heads) ** -0.5, want_maps=True)                          # [K+2, heads, N, M]
        for r, c in enumerate(sel):
            want = torch.einsum("nm,m->n", maps[c].mean(0), w[i, r])
            assert (got[i, r] - want).abs().max() < 1e-12
    # float32 inputs stay float32; a [R, M] weight is shared by the images
    got32 = attnmaps.token_maps_reference(q.float(), k.float(), sel, w[0].float(), heads, (C // heads) ** -0.5)
    assert got32.dtype == torch.float32 and (got32[0].double() - got[0]).abs().max() < 1e-5


def test_token_maps_on_cpu_needs_the_stand_in_and_accumulates():
    from sta import attnmaps
    from tests.cpu_backend import CpuPacked
    g = torch.Generator().manual_seed(4)
    q, k = torch.randn(2, 32, 64, generator=g), torch.randn(3, 77, 64, generator=g)
    packed = CpuPacked(k, k, 8, 1)
    w = torch.rand(2, 77, generator=g)
    a = attnmaps.token_maps(q, packed, [1, 2], w, 8 ** -0.5)
    assert torch.equal(a, attnmaps.token_maps_reference(q, k, [1, 2], w, 8, 8 ** -0.5))
    buf = torch.full((1, 2, 32), 0.5)
    attnmaps.token_maps(q, packed, [1, 2], w, 8 ** -0.5, out=buf, accumulate=True)
    assert torch.equal(buf, 0.5 + a)
    with pytest.raises(ValueError):
        attnmaps.token_maps(q, packed, [3], w[:1], 8 ** -0.5)                 # context 3 of 3
    with pytest.raises(ValueError):
        attnmaps.token_maps(q, packed, [1] * 17, w[:1].expand(17, -1), 8 ** -0.5)
    with pytest.raises(ValueError):
        attnmaps.token_maps(q, packed, [1, 2], w, 8 ** -0.5, accumulate=True)  # nothing to add to

    class NoKeys:                                                               # a real packed image has no CPU reader
        n_img, n_ctx, heads, M, C, dtype = 1, 3, 8, 77, 64, torch.float32
    with pytest.raises(RuntimeError, match="no CPU path"):
        attnmaps.token_maps(q, NoKeys(), [1, 2], w, 8 ** -0.5)


# ---------------------------------------------------------------------------------------------------
# token weights
# ---------------------------------------------------------------------------------------------------
VOCAB = {}


def _fake_tokenize(text):
    """Content ids only; 'skateboard' splits into two sub-word tokens, as a BPE vocabulary would."""
    out = []
    for word in text.lower().replace(",", " ").split():
        for piece in (["skate", "board"] if word == "skateboard" else [word]):
            out.append(VOCAB.setdefault(piece, 1000 + len(VOCAB)))
    return out


def test_token_weights_found_not_found_repeated_multi_token():
    from sta import attnmaps
    prompt = "a dog on a skateboard next to a dog"
    names = ["dog", "skateboard", "zebra"]
    local = ["a photo of " + n for n in names]
    sel, w, found = attnmaps.token_weights(_fake_tokenize, prompt, names, local)
    assert sel == [1, 1, 1, 2, 3, 4] and w.shape == (6, 77) and w.dtype == torch.float32
    assert found.tolist() == [True, True, False, True, True, True]
    # "dog" is content token 1 and 9: the FIRST occurrence, key 0 being the begin token
    assert w[0].nonzero().flatten().tolist() == [2] and w[0, 2] == 1.0
    # a two-token name: content tokens 4, 5 -> keys 5, 6, half each
    assert w[1].nonzero().flatten().tolist() == [5, 6] and torch.allclose(w[1, 5:7], torch.tensor([0.5, 0.5]))
    assert not w[2].any()                                                      # not found: a zero row, nothing raised
    # local prompts "a photo of X": X starts at content token 3 -> key 4
    assert w[3].nonzero().flatten().tolist() == [4] and w[4].nonzero().flatten().tolist() == [4, 5]
    assert w[5].nonzero().flatten().tolist() == [4]                            # the local prompt of the zebra does name it
    assert torch.allclose(w.sum(1), found.float())


def test_token_weights_without_tokenizer_is_the_word_index_stand_in():
    from sta import attnmaps
    sel, w, found = attnmaps.token_weights(None, "A cat, left of the Dog.", ["cat", "the dog", "bird"], ["a photo of cat", "a photo of the dog", "x"])
    assert sel == [1, 1, 1, 2, 3, 4]
    assert w[0].nonzero().flatten().tolist() == [2]                            # word 1 -> key 2
    assert w[1].nonzero().flatten().tolist() == [5, 6]
    assert found.tolist() == [True, True, False, True, True, False]
    # a name beyond the 77-key window is not found either (key 76 is the end token of a truncated prompt)
    long_prompt = " ".join(["w%d" % i for i in range(80)]) + " cat"
    assert not attnmaps.token_weights(None, long_prompt, ["cat"], ["a photo of cat"])[2][0]
    with pytest.raises(ValueError):
        attnmaps.token_weights(None, "a cat", ["cat"], [])


# ---------------------------------------------------------------------------------------------------
# AttnCapture over a trajectory (oracle-backed blocks)
# ---------------------------------------------------------------------------------------------------
def _model():
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    meta = json.load(open(os.path.join(G, "unet_state_dict_keys.json")))
    unet = UNetModel(**meta["cfg"]).eval()
    seeded_fill_(unet, 21)
    for p in unet.parameters():
        p.requires_grad_(False)
    return LatentDiffusion(unet_config=unet)


def _sample(sampler, S=3, lat=16, K=2):
    c, local_ctx, x_T = gi.unet_inputs(K, 5)
    with oracle_ops():
        sampler.sample(S=S, conditioning=c, batch_size=1, shape=[4, lat, lat], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond(), eta=0.0, x_T=x_T[:, :, :lat, :lat], text_index=0,
                       curr_text="a cat left of a dog", bboxs_curr=[[0.3, 0.4], [0.7, 0.6]], seed=1, prompt_idx=0,
                       object_names=["cat", "dog"], local_conditionings=local_ctx)
    return sampler.last_result["x0"]


@pytest.mark.parametrize("kind,S", [("plms", 4), ("ddim", 4), ("dpm", 3)])      # PLMS / DDIM steps divide the 1000 timesteps
def test_capture_over_a_trajectory_and_off_path_is_untouched(kind, S):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    from ldm.modules.attention import BasicTransformerBlock
    from sta import attnmaps
    cls = dict(plms=PLMSSampler, ddim=DDIMSampler, dpm=DPMSolverSampler)[kind]
    res = 4                                                                      # 16 x 16 latent: levels 16, 8, 4 and the 2 x 2 middle
    model = _model()
    plain = _sample(cls(model, opt_epochs=0, use_graph=False, save_images=False), S)      # no capture ever constructed
    cap = attnmaps.AttnCapture(model.model.diffusion_model, resolution=res, per_call=True)
    sampler = cls(model, opt_epochs=0, use_graph=False, save_images=False, attn_capture=cap)
    assert torch.equal(_sample(sampler, S), plain)
    blocks = [b for b in model.modules() if isinstance(b, BasicTransformerBlock)]
    assert all(b._attn_capture is None for b in blocks)                         # detached again
    n_res = sum(b._last_n == res * res for b in blocks)
    calls = S + 1 if kind == "plms" else S
    r = sampler.last_attn
    assert n_res == 5 and r.calls == calls and r.block_calls == n_res * calls
    assert r.maps.shape == (1, 4, res, res) and r.per_call.shape == (calls, 1, 4, res, res)
    assert r.sel_ctx == [1, 1, 2, 3] and r.found.tolist() == [[True, True, True, True]]
    assert torch.allclose(r.per_call.mean(0), r.maps, atol=1e-6)
    assert ((r.in_disc_mass >= 0) & (r.in_disc_mass <= 1)).all()
    # a one-hot / averaged softmax mass: every pixel in [0, 1]
    assert (r.maps >= 0).all() and (r.maps <= 1 + 1e-6).all()
    # the capture exists but this sampler was not given it: the run where none was ever constructed, bit for bit
    again = cls(model, opt_epochs=0, use_graph=False, save_images=False)
    assert torch.equal(_sample(again, S), plain) and again.last_attn is None


def test_capture_matches_the_reference_formula_on_one_block():
    """One block call on CPU: what AttnCapture records is token_maps_reference on that block's own q and keys."""
    from ldm.modules.attention import BasicTransformerBlock
    from sta import attnmaps, prompt_state
    g = np.load(os.path.join(G, "block_d8k4.npz"), allow_pickle=False)
    dim, C, heads, K, seed = (int(g[k]) for k in ("dim", "C", "heads", "K", "seed"))
    x, context, local_ctx = gi.block_inputs(dim, C, K, seed, gi.load_uncond())
    blk = BasicTransformerBlock(C, heads, C // heads, context_dim=768, checkpoint=False)
    seeded_fill_(blk, seed)
    pix = torch.from_numpy(g["map_pixels"])
    sel = [0, 1] + [2 + i for i in range(K)] + [1]
    w = torch.zeros(len(sel), 77)
    for r in range(len(sel) - 1):
        w[r, 3 * r] = 1.0
    w[-1] = 1.0 / 77
    cap = attnmaps.AttnCapture(blk, resolution=dim)
    cap.set_readouts(sel, w)
    centres = [list(c) for c in g["centres"]]
    with oracle_ops(), torch.no_grad():
        prompt_state.begin_prompt(local_ctx, first_timestep=981)
        plain = blk(x, context=context, time=torch.tensor(981), coef=torch.from_numpy(g["coef"]), bboxs_curr=centres)
        cap.begin([centres])
        with cap:
            out = blk(x, context=context, time=torch.tensor(981), coef=torch.from_numpy(g["coef"]), bboxs_curr=centres)
        with cap, torch.enable_grad():                                          # under autograd nothing is recorded
            blk(x, context=context, time=torch.tensor(981), coef=torch.from_numpy(g["coef"]), bboxs_curr=centres)
    assert torch.equal(out, plain)
    r = cap.result()
    assert r.block_calls == 1 and r.calls == 1 and r.per_call is None
    got = r.maps.reshape(len(sel), -1)[:, pix].double()
    want = torch.einsum("rnm,rm->rn", torch.from_numpy(g["maps"]).double().mean(1)[sel], w.double())
    assert (got - want).abs().max() < 1e-5                                      # the reference's own fp32 maps
    assert torch.isnan(r.in_disc_mass[0, :2]).all() and torch.isnan(r.in_disc_mass[0, -1])     # contexts 0 / 1: no object
    assert ((r.in_disc_mass[0, 2:-1] >= 0) & (r.in_disc_mass[0, 2:-1] <= 1)).all()


def test_tracked_epoch_records_nothing():
    """opt_epochs = 2: the first epoch is tracked (autograd) and records nothing; only the kept trajectory is captured."""
    from ldm.models.autoencoder import AutoencoderKL
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from sta import attnmaps

    class Loss(torch.nn.Module):
        def forward_2(self, image, text):
            return image.mean().reshape(1)

        def forward_3(self, image, text):
            return (image ** 2).mean().reshape(1)

    unet = _model().model.diffusion_model
    vae = AutoencoderKL(ddconfig=dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32,
                                      ch_mult=[1, 2], num_res_blocks=1, attn_resolutions=[], dropout=0.0))
    seeded_fill_(vae, 3)
    for p in vae.parameters():
        p.requires_grad_(False)
    model = LatentDiffusion(unet_config=unet, first_stage_config=vae)
    cap = attnmaps.AttnCapture(unet, resolution=2)                              # 8 x 8 latent: levels 8, 4, 2 and the 1 x 1 middle
    sampler = DPMSolverSampler(model, loss_model=Loss(), opt_epochs=2, use_graph=False, save_images=False, attn_capture=cap)
    _sample(sampler, S=3, lat=8)
    assert len(sampler.last_result["losses"]) == 1
    assert sampler.last_attn.calls == 3 and sampler.last_attn.block_calls == 5 * 3


def test_save_result_writes_npz_and_overlays(tmp_path):
    from sta import attnmaps
    maps = torch.rand(1, 4, 8, 8)
    r = attnmaps.AttnResult(maps, None, torch.tensor([[0.5, 0.25, 0.75, 1.0]]), 10, 2, [1, 1, 2, 3], torch.tensor([[True, False, True, True]]))
    lines = attnmaps.save_result(str(tmp_path), 7, ["cat", "big dog"], [[0.3, 0.4], [0.7, 0.6]], r, image=torch.rand(3, 64, 64))
    assert len(lines) == 4 and "cat" in lines[0] and "0.500" in lines[0] and "not found" in lines[1]
    z = np.load(tmp_path / "attn" / "7.npz")
    assert z["maps"].shape == (4, 8, 8) and list(z["names"]) == ["cat", "big dog"] and z["centres"].shape == (2, 2)
    assert z["found"].tolist() == [True, False, True, True] and np.allclose(z["in_disc_mass"], [0.5, 0.25, 0.75, 1.0])
    assert sorted(p.name for p in (tmp_path / "attn").glob("*.png")) == ["7_big_dog_ctx1.png", "7_big_dog_ctx3.png", "7_cat_ctx1.png", "7_cat_ctx2.png"]
    img = attnmaps.overlay(np.zeros((64, 64, 3), np.uint8), np.eye(8), (0.5, 0.5))
    assert img.shape == (64, 64, 3) and img.dtype == np.uint8 and (img == 255).all(-1).any()      # the disc outline


# ---------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------
def _cli():
    sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts"))
    import _txt2img_common as c
    return c


def test_cli_flags_parse_and_refuse():
    c = _cli()
    p = c.build_parser("x.json")
    opt = p.parse_args(["--opt_epochs", "0"])
    assert opt.attn_maps is False and opt.attn_res == 16
    c.check_options(opt)
    opt = p.parse_args(["--opt_epochs", "0", "--attn_maps", "--attn_res", "32"])
    assert opt.attn_maps and opt.attn_res == 32
    c.check_options(opt)
    with pytest.raises(SystemExit):
        p.parse_args(["--attn_res", "12"])
    with pytest.raises(SystemExit, match="no transformer level"):                # a 256 x 256 image has levels 32, 16, 8, 4
        c.check_options(p.parse_args(["--opt_epochs", "0", "--attn_maps", "--attn_res", "64", "--H", "256", "--W", "256"]))
    with pytest.raises(SystemExit, match="square"):
        c.check_options(p.parse_args(["--opt_epochs", "0", "--attn_maps", "--H", "512", "--W", "768"]))
    c.check_options(p.parse_args(["--opt_epochs", "0", "--attn_res", "64", "--H", "256", "--W", "256"]))    # not asked for: not checked


# ---------------------------------------------------------------------------------------------------
# C-ABI refusals
# ---------------------------------------------------------------------------------------------------
STA_E_ARG, STA_E_UNSUP = -1, -2
P = 0x10000                                            # a fake device pointer: non-null, 16-byte aligned, never read


def _sel(*v):
    arr = (ctypes.c_int32 * max(len(v), 1))(*v)
    return arr, ctypes.cast(arr, ctypes.c_void_p).value


def _call(L, q=P, packed=P, sel=(1, 2), w=P, out=P, n_img=1, N=256, C=320, heads=8, M=77, K=2, R=None, scale=0.158, accumulate=0,
          dtype=0, sel_ptr=None):
    arr, ptr = _sel(*sel)
    rc = L.sta_xattn_token_maps(q, packed, ptr if sel_ptr is None else sel_ptr, w, out, n_img, N, C, heads, M, K,
                                len(sel) if R is None else R, scale, accumulate, dtype, None)
    return rc, L.sta_last_error().decode()


def test_abi_refusals_reach_no_launch():
    from sta import lib
    L = lib.load()
    assert len(lib.SYMBOLS["sta_xattn_token_maps"][1]) == 16 and lib.MAX_READOUTS == 16
    cases = [
        (dict(R=0), STA_E_ARG, "R=0"),
        (dict(sel=(1,) * 17), STA_E_ARG, "R=17"),
        (dict(sel=(1, 4)), STA_E_ARG, "sel_ctx[1]=4"),
        (dict(sel=(-1, 1)), STA_E_ARG, "sel_ctx[0]=-1"),
        (dict(sel=(2,), K=0), STA_E_ARG, "sel_ctx[0]=2"),
        (dict(q=0), STA_E_ARG, "null pointer"),
        (dict(packed=0), STA_E_ARG, "null pointer"),
        (dict(sel_ptr=0), STA_E_ARG, "null pointer"),
        (dict(w=0), STA_E_ARG, "null pointer"),
        (dict(out=0), STA_E_ARG, "null pointer"),
        (dict(q=P + 8), STA_E_ARG, "misaligned"),
        (dict(out=P + 2), STA_E_ARG, "misaligned"),
        (dict(n_img=0), STA_E_ARG, "n_img=0"),
        (dict(N=0), STA_E_ARG, "non-positive"),
        (dict(accumulate=2), STA_E_ARG, "accumulate=2"),
        (dict(M=81), STA_E_UNSUP, "M=81"),
        (dict(C=324), STA_E_ARG, "not divisible"),
        (dict(C=8 * 168), STA_E_UNSUP, "head dim 168"),
        (dict(K=9, sel=(1,)), STA_E_UNSUP, "K=9"),
        (dict(dtype=7), STA_E_UNSUP, "dtype 7"),
    ]
    for kw, code, text in cases:
        rc, err = _call(L, **kw)
        assert rc == code and text in err, (kw, rc, err)
    assert _call(L, dtype=7)[1] == "dtype 7"                                   # the same text every entry point gives
