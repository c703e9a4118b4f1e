"""The attention-layout loss without a GPU: layout_energy, the tracked readout on the host stand-in, the refusals of
sta_xattn_token_maps_bwd (fake pointers: none of these calls may reach a launch), a miniature weight optimisation with the loss
alone through the oracle-backed blocks (tests/cpu_backend.py), and the CLI flag. The kernel is checked in test_attnloss_gpu.py."""
import ctypes
import json
import os
import sys

import pytest
import torch

from oracle import golden_inputs as gi
from sta.synth import seeded_fill_
from tests.cpu_backend import CpuPacked, oracle_ops

G = gi.GOLDEN
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------
# layout_energy
# ---------------------------------------------------------------------------------------------------
def test_layout_energy_by_hand():
    from sta.attnloss import layout_energy
    maps = torch.tensor([[[1.0, 1.0, 2.0, 0.0], [3.0, 1.0, 0.0, 0.0], [5.0, 5.0, 5.0, 5.0]]])
    disc = torch.tensor([[[1, 0, 1, 0], [0, 1, 0, 0], [1, 1, 1, 1]]], dtype=torch.uint8)
    # shares 3/4, 1/4 and 1 -> energies 1/16, 9/16 and 0
    e = layout_energy(maps, disc, torch.tensor([[True, True, True]]))
    assert e.shape == (1,) and abs(e.item() - (1 / 16 + 9 / 16 + 0) / 3) < 1e-7
    # invalid readouts are excluded from the sum AND from the count
    e = layout_energy(maps, disc, torch.tensor([[True, False, True]]))
    assert abs(e.item() - (1 / 16) / 2) < 1e-7
    e = layout_energy(maps, disc, torch.tensor([[False, True, False]]))
    assert abs(e.item() - 9 / 16) < 1e-7


def test_layout_energy_without_valid_readouts_is_exactly_zero_with_zero_gradient():
    from sta.attnloss import layout_energy
    g = torch.Generator().manual_seed(0)
    maps = torch.rand(2, 3, 16, generator=g).requires_grad_(True)
    maps.data[1, 2] = 0.0                                                       # an all-zero (name not found) map must not give 0 / 0
    disc = (torch.rand(2, 3, 16, generator=g) > 0.5).float()
    valid = torch.tensor([[True, True, False], [False, False, False]])
    e = layout_energy(maps, disc, valid)
    assert e[1].item() == 0.0 and e[0].item() > 0
    e.sum().backward()
    assert torch.isfinite(maps.grad).all()
    assert (maps.grad[1] == 0).all() and (maps.grad[0, 2] == 0).all() and maps.grad[0, :2].abs().max() > 0


def test_layout_energy_gradcheck():
    from sta.attnloss import layout_energy
    g = torch.Generator().manual_seed(1)
    maps = (torch.rand(2, 4, 9, generator=g, dtype=torch.float64) + 0.1).requires_grad_(True)
    disc = (torch.rand(2, 4, 9, generator=g) > 0.5).double()
    valid = torch.tensor([[True, True, False, True], [True, False, True, True]])
    assert torch.autograd.gradcheck(lambda m: layout_energy(m, disc, valid), (maps,))


# ---------------------------------------------------------------------------------------------------
# the tracked readout on the host stand-in
# ---------------------------------------------------------------------------------------------------
def test_token_maps_tracked_on_the_stand_in():
    from sta import attnmaps
    g = torch.Generator().manual_seed(4)
    I, N, C, heads, K = 2, 32, 64, 8, 1
    q = torch.randn(2 * I, N, C, generator=g)
    k = torch.randn(I * (K + 2), 77, C, generator=g) * 0.7
    w = torch.randn(I, 4, 77, generator=g)
    sel = [1, 0, 2, 1]
    packed = CpuPacked(k, k, heads, I)
    up = torch.randn(I, 4, N, generator=g)
    q1 = q.clone().requires_grad_(True)
    got = attnmaps.token_maps_tracked(q1, packed, sel, w, heads ** -0.5)
    assert got.dtype == torch.float32 and torch.equal(got.detach(), attnmaps.token_maps_reference(q, k, sel, w, heads, heads ** -0.5))
    (got * up).sum().backward()
    q64 = q.double().requires_grad_(True)
    (attnmaps.token_maps_reference(q64, k.double(), sel, w.double(), heads, heads ** -0.5) * up.double()).sum().backward()
    assert q1.grad is not None and (q1.grad.double() - q64.grad).abs().max() <= 1e-5 * q64.grad.abs().max()
    assert q64.grad[0::2].abs().max() > 0 and q64.grad[1::2].abs().max() > 0    # both q rows are read (contexts 0 and 1, 2)

    class NoKeys:                                                               # a real packed image has no CPU reader
        n_img, n_ctx, heads, M, C, dtype = 2, 3, 8, 77, 64, torch.float32
    with pytest.raises(RuntimeError, match="no CPU path"):
        attnmaps.token_maps_tracked(q1, NoKeys(), sel, w, heads ** -0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        attnmaps.token_maps_backward(q, NoKeys(), sel, w, up, heads ** -0.5)


# ---------------------------------------------------------------------------------------------------
# C-ABI refusals
# ---------------------------------------------------------------------------------------------------
STA_E_ARG, STA_E_UNSUP = -1, -2
P = 0x10000                                            # a fake device pointer: non-null, 16-byte aligned, never read


def _call(L, q=P, packed=P, sel=(1, 2), w=P, dmaps=P, dq=P, n_img=1, N=256, C=320, heads=8, M=77, K=2, R=None, scale=0.158, dtype=0,
          sel_ptr=None):
    arr = (ctypes.c_int32 * max(len(sel), 1))(*sel)
    ptr = ctypes.cast(arr, ctypes.c_void_p).value
    rc = L.sta_xattn_token_maps_bwd(q, packed, ptr if sel_ptr is None else sel_ptr, w, dmaps, dq, n_img, N, C, heads, M, K,
                                    len(sel) if R is None else R, scale, dtype, None)
    return rc, L.sta_last_error().decode()


def test_abi_symbol_and_refusals_reach_no_launch():
    from sta import lib
    L = lib.load()
    res, args = lib.SYMBOLS["sta_xattn_token_maps_bwd"]
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert res is i and args == [vp] * 6 + [i] * 7 + [f, i, vp]                 # the declaration of include/sta_xattn.h
    header = open(os.path.join(ROOT, "include", "sta_xattn.h")).read()
    assert "int sta_xattn_token_maps_bwd(const void* q, const void* packed, const int32_t* sel_ctx, const float* w," in header
    # the kernel's file is built as part of the cross-attention backward's translation unit, with that unit's flags
    host = lib.INCLUDED_SOURCES["sta_xattn_maps_bwd.hip"]
    assert host in [os.path.basename(s) for s in lib.SOURCES] and "-ffinite-math-only" in lib.PER_SOURCE_FLAGS[host]
    assert '#include "sta_xattn_maps_bwd.hip"' in open(os.path.join(lib.CSRC, host)).read()
    assert os.path.isfile(os.path.join(lib.CSRC, "sta_xattn_maps_bwd.hip"))
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
        (dict(dmaps=0), STA_E_ARG, "null pointer"),
        (dict(dq=0), STA_E_ARG, "null pointer"),
        (dict(q=P + 8), STA_E_ARG, "misaligned"),
        (dict(dq=P + 8), STA_E_ARG, "misaligned"),
        (dict(dmaps=P + 2), STA_E_ARG, "misaligned"),
        (dict(n_img=0), STA_E_ARG, "n_img=0"),
        (dict(N=0), STA_E_ARG, "non-positive"),
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


# ---------------------------------------------------------------------------------------------------
# miniature weight optimisation with the attention loss alone (oracle-backed blocks, fp32)
# ---------------------------------------------------------------------------------------------------
RES, LAT, S, K = 8, 32, 4, 2
CENTRES = [[0.3, 0.4], [0.7, 0.6]]


def _model():
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    meta = json.load(open(os.path.join(G, "unet_state_dict_keys.json")))
    unet = UNetModel(**dict(meta["cfg"], use_checkpoint=True)).eval()
    seeded_fill_(unet, 21)
    for p in unet.parameters():
        p.requires_grad_(False)
    return LatentDiffusion(unet_config=unet)


_RUNS = {}


def _run(kind, recompute):
    """One sample() with opt_epochs = 2 and the attention loss alone; Adam's step is observed and then UNDONE, so that the kept
    (second) trajectory runs with the weights of the tracked one and its captured maps are the maps the loss saw."""
    if (kind, recompute) in _RUNS:
        return _RUNS[(kind, recompute)]
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.plms import PLMSSampler
    from ldm.modules.attention import BasicTransformerBlock
    from sta import attnloss, attnmaps
    from sta.pipeline import set_recompute
    model = _model()
    assert set_recompute(model, recompute) == recompute
    unet = model.model.diffusion_model
    loss = attnloss.AttnLayoutLoss(unet, resolution=RES)
    cap = attnmaps.AttnCapture(unet, resolution=RES, per_call=True)
    sampler = (PLMSSampler if kind == "plms" else DDIMSampler)(model, loss_model=None, opt_epochs=2, use_graph=False, save_images=False,
                                                               attn_loss=loss, attn_capture=cap)
    seen = {}
    orig_step = torch.optim.Adam.step

    def step(self, *a, **k):
        W = self.param_groups[0]["params"][0]
        before = W.detach().clone()
        seen["grad"] = W.grad.clone()
        out = orig_step(self, *a, **k)
        seen["moved"] = (W.detach() - before).clone()
        W.data.copy_(before)
        return out

    torch.optim.Adam.step = step
    decodes = []
    model.decode_first_stage = lambda z: decodes.append(1)                      # there is no VAE: nothing may ask for one
    c, local_ctx, x_T = gi.unet_inputs(K, 5)
    try:
        with oracle_ops():
            sampler.sample(S=S, conditioning=c, batch_size=1, shape=[4, LAT, LAT], verbose=False, unconditional_guidance_scale=7.5,
                           unconditional_conditioning=gi.load_uncond(), eta=0.0, x_T=x_T[:, :, :LAT, :LAT], text_index=0,
                           curr_text="a cat left of a dog", bboxs_curr=CENTRES, seed=1, prompt_idx=0, object_names=["cat", "dog"],
                           local_conditionings=local_ctx)
    finally:
        torch.optim.Adam.step = orig_step
    blocks = [b for b in model.modules() if isinstance(b, BasicTransformerBlock)]
    assert all(b._attn_loss is None and b._attn_capture is None for b in blocks) and not decodes
    _RUNS[(kind, recompute)] = dict(result=sampler.last_result, attn=sampler.last_attn, loss=loss, **seen)
    return _RUNS[(kind, recompute)]


@pytest.mark.parametrize("kind", ["plms", "ddim"])
def test_miniature_weight_optimisation_with_the_attention_loss_alone(kind):
    from sta import ops
    from sta.attnloss import layout_energy
    r = _run(kind, "none")
    calls = S + 1 if kind == "plms" else S
    losses = r["result"]["losses"]
    assert len(losses) == 1 and 0 < losses[0] <= 1.0 and torch.isfinite(r["result"]["x0"]).all()
    assert r["loss"].calls == calls and r["loss"].block_calls == 5 * calls      # five blocks at 8 x 8, every tracked call
    # Adam's first step is lr g / (|g| + 1e-8): lr wherever the gradient is not ~0
    grad, moved = r["grad"], r["moved"]
    assert grad.shape == (1, K, S) and torch.isfinite(grad).all()
    live = grad.abs() > 1e-6 * grad.abs().max()
    assert live.float().mean() > 0.5 and ((moved[live].abs() - 0.005).abs() < 1e-5).all(), (grad, moved)
    assert (torch.sign(moved[live]) == -torch.sign(grad[live])).all()
    # the recorded loss is layout_energy on the per-call maps the capture saw on the kept trajectory (same W, same fp32 path)
    a = r["attn"]
    assert a.calls == calls and a.per_call.shape == (calls, 1, 2 * K, RES, RES) and a.found.all()
    disc = ops.disc_masks(CENTRES, RES).float()[[0, 1, 0, 1]].unsqueeze(0)      # readout r measures object r % K
    valid = torch.ones(1, 2 * K, dtype=torch.bool)
    want = sum(layout_energy(a.per_call[k].reshape(1, 2 * K, -1), disc, valid).sum() for k in range(calls)).item() / calls
    assert abs(losses[0] - want) <= 1e-5 * abs(want), (losses[0], want)


def test_modes_none_and_all_agree_on_the_host():
    """Mode `all` checkpoints every transformer block; the recording blocks leave their checkpoint while the loss is attached, so
    the side value exists and the loss and dLoss/dW are those of mode `none`."""
    a, b = _run("plms", "none"), _run("plms", "all")
    la, lb = a["result"]["losses"][0], b["result"]["losses"][0]
    assert abs(la - lb) <= 1e-5 * abs(la), (la, lb)
    assert (a["grad"] - b["grad"]).abs().max() <= 1e-5 * a["grad"].abs().max(), (a["grad"], b["grad"])


def test_no_loss_at_all_still_raises_before_the_first_trajectory():
    from ldm.models.diffusion.plms import PLMSSampler
    model = _model()
    calls = []
    model.apply_model_extra = lambda *a, **k: calls.append(1)
    sampler = PLMSSampler(model, loss_model=None, opt_epochs=2, use_graph=False, save_images=False)
    c, local_ctx, x_T = gi.unet_inputs(K, 5)
    with pytest.raises(RuntimeError, match="loss_model"), oracle_ops():
        sampler.sample(S=S, conditioning=c, batch_size=1, shape=[4, LAT, LAT], verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning=gi.load_uncond(), eta=0.0, x_T=x_T[:, :, :LAT, :LAT], text_index=0,
                       curr_text="a cat left of a dog", bboxs_curr=CENTRES, seed=1, prompt_idx=0, object_names=["cat", "dog"],
                       local_conditionings=local_ctx)
    assert not calls


# ---------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------
def _cli():
    sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts"))
    import _txt2img_common as c
    return c


def test_cli_attn_loss_parses_and_refuses(monkeypatch):
    c = _cli()
    p = c.build_parser("x.json")
    assert p.parse_args(["--opt_epochs", "0"]).attn_loss is None
    opt = p.parse_args(["--opt_epochs", "3", "--attn_loss", "0.5"])
    assert opt.attn_loss == 0.5 and opt.attn_res == 16 and opt.clip is None
    c.check_options(opt)                                                        # no --clip: accepted with the attention loss
    for bad in ("0", "-1", "nan"):
        with pytest.raises(SystemExit):
            p.parse_args(["--attn_loss", bad])
    with pytest.raises(SystemExit, match="nothing would be optimised"):
        c.check_options(p.parse_args(["--opt_epochs", "1", "--attn_loss", "1.0"]))
    with pytest.raises(SystemExit, match="no transformer level"):                # a 256 x 256 image has levels 32, 16, 8, 4
        c.check_options(p.parse_args(["--opt_epochs", "3", "--attn_loss", "1.0", "--attn_res", "64", "--H", "256", "--W", "256"]))
    # without --clip and without the attention loss nothing could be optimised (the default loss model is a package that is absent)
    monkeypatch.setattr(c.importlib.util, "find_spec", lambda name: None)
    with pytest.raises(SystemExit, match="needs a loss"):
        c.check_options(p.parse_args(["--opt_epochs", "3"]))
    c.check_options(p.parse_args(["--opt_epochs", "3", "--attn_loss", "1.0"]))
