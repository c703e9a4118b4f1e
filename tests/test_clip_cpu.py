"""sta.clip on the host: the built-in CLIP ViT-B/32 against an independent implementation (transformers.CLIPModel with
shared random weights), its state_dict contract and loaders, the view rules against the reference's fixture, and
DCLIPLoss.forward_batch against the view-by-view path."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import golden_inputs as gi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SCRIPTS = os.path.join(REPO, "diffusion-spacetime-attn_amd", "scripts")

# Measured on the host: largest |difference| over the largest |feature| between ClipViTB32 and transformers.CLIPModel, both
# fp32 with the same weights (summation order is all that differs): 4.5e-7 image, 5.8e-7 text.
# The bound is ten times the larger, and below the 1e-4 cap.
FP32_PARITY = 5.8e-6
assert FP32_PARITY <= 1e-4

NARROW = dict(embed_dim=32, image_resolution=224, vision_layers=2, vision_width=64, vision_patch_size=32, vision_heads=4,
              transformer_width=48, transformer_heads=4, transformer_layers=2)


def _hf_model(narrow, dtype):
    from transformers import CLIPConfig, CLIPModel
    if narrow:
        text = dict(hidden_size=48, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4)
        vision = dict(hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4)
        proj = 32
    else:
        text = dict(hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8)
        vision = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12)
        proj = 512
    text.update(vocab_size=49408, max_position_embeddings=77, hidden_act="quick_gelu", eos_token_id=49407, bos_token_id=49406,
                pad_token_id=1, layer_norm_eps=1e-5)
    vision.update(image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    torch.manual_seed(0)
    hf = CLIPModel(CLIPConfig(text_config=text, vision_config=vision, projection_dim=proj)).eval().to(dtype)
    with torch.no_grad():        # HF initialises biases and LayerNorms to 0 / 1: a swapped pair would go unseen
        g = torch.Generator().manual_seed(1)
        for name, p in hf.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g, dtype=torch.float32).to(dtype))
    return hf


def _features(out):
    return out if torch.is_tensor(out) else out.pooler_output


def _tokens():
    rows = torch.zeros(2, 77, dtype=torch.long)
    g = torch.Generator().manual_seed(2)
    for r, n in enumerate((7, 20)):
        rows[r, 0] = 49406
        rows[r, 1:1 + n] = torch.randint(1, 49405, (n,), generator=g)
        rows[r, 1 + n] = 49407
    return rows


def _parity(narrow, dtype):
    from sta import clip
    hf = _hf_model(narrow, dtype)
    model = clip.ClipViTB32(**(NARROW if narrow else {})).to(dtype).eval()
    sd = clip.from_hf_state_dict(hf.state_dict())
    clip.check_state_dict(model, sd)
    model.load_state_dict(sd, strict=True)
    img = torch.rand(3, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(dtype)
    tok = _tokens()
    with torch.no_grad():
        fi, ft = model.encode_image(img), model.encode_text(tok)
        ri = _features(hf.get_image_features(pixel_values=img))
        rt = _features(hf.get_text_features(input_ids=tok))
        padded = torch.where(tok == 0, torch.full_like(tok, 49407), tok)          # 49407 padding pools the same position
        assert torch.allclose(model.encode_text(padded), ft, rtol=0, atol=1e-6 * float(ft.abs().max()))
    ei = float((fi - ri).abs().max() / ri.abs().max())
    et = float((ft - rt).abs().max() / rt.abs().max())
    print("ClipViTB32 vs transformers.CLIPModel (%s, %s): image %.3g, text %.3g of the largest feature"
          % ("narrow" if narrow else "ViT-B/32", dtype, ei, et))
    return ei, et


def test_towers_match_transformers_clip_fp32():
    """Test 1: ViT-B/32 sizes, fp32 on both sides, weights through from_hf_state_dict with strict=True."""
    ei, et = _parity(False, torch.float32)
    assert ei <= FP32_PARITY and et <= FP32_PARITY, (ei, et)


def test_towers_match_transformers_clip_float64_narrow():
    """A narrow 2-layer configuration in float64: a wrong formula cannot hide inside the fp32 tolerance."""
    ei, et = _parity(True, torch.float64)
    assert ei <= 1e-10 and et <= 1e-10, (ei, et)


def _expected_names():
    names = {"visual.conv1.weight": (768, 3, 32, 32), "visual.class_embedding": (768,), "visual.positional_embedding": (50, 768),
             "visual.proj": (768, 512), "visual.ln_pre.weight": (768,), "visual.ln_pre.bias": (768,), "visual.ln_post.weight": (768,),
             "visual.ln_post.bias": (768,), "token_embedding.weight": (49408, 512), "positional_embedding": (77, 512),
             "ln_final.weight": (512,), "ln_final.bias": (512,), "text_projection": (512, 512), "logit_scale": ()}
    for prefix, w in (("visual.transformer.resblocks.", 768), ("transformer.resblocks.", 512)):
        for i in range(12):
            b = "%s%d." % (prefix, i)
            names.update({b + "ln_1.weight": (w,), b + "ln_1.bias": (w,), b + "ln_2.weight": (w,), b + "ln_2.bias": (w,),
                          b + "attn.in_proj_weight": (3 * w, w), b + "attn.in_proj_bias": (3 * w,), b + "attn.out_proj.weight": (w, w),
                          b + "attn.out_proj.bias": (w,), b + "mlp.c_fc.weight": (4 * w, w), b + "mlp.c_fc.bias": (4 * w,),
                          b + "mlp.c_proj.weight": (w, 4 * w), b + "mlp.c_proj.bias": (w,)})
    return names


def test_state_dict_names_and_loaders(tmp_path):
    """Test 2: the OpenAI names and shapes exactly; a missing key / a wrong shape is refused by name; the three file kinds load.
    The TorchScript route is a real archive, nothing mocked: torch.jit.script of a holder module tree that carries the narrow
    model's tensors under their dotted names plus the official archive's three extra entries, saved and read back."""
    from sta import clip
    model = clip.ClipViTB32()
    want = _expected_names()
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == want
    sd = model.state_dict()
    short = dict(sd)
    del short["visual.ln_post.bias"]
    with pytest.raises(ValueError, match="visual.ln_post.bias"):
        clip.check_state_dict(model, short)
    off = dict(sd)
    off["visual.proj"] = torch.zeros(512, 768)
    with pytest.raises(ValueError, match="visual.proj"):
        clip.check_state_dict(model, off)

    # plain state_dict file and Hugging Face state_dict file, narrow sizes through read_state_dict
    small = clip.ClipViTB32(**NARROW)
    plain = tmp_path / "plain.pt"
    torch.save(small.state_dict(), plain)
    back = clip.read_state_dict(str(plain))
    assert set(back) == set(small.state_dict()) and all(torch.equal(back[k], v) for k, v in small.state_dict().items())
    hf = _hf_model(True, torch.float32)
    hf_file = tmp_path / "hf.pt"
    torch.save(hf.state_dict(), hf_file)
    conv = clip.read_state_dict(str(hf_file))
    clip.check_state_dict(small, conv)

    class Node(torch.nn.Module):
        pass

    root = Node()
    extras = dict(input_resolution=torch.tensor(224), context_length=torch.tensor(77), vocab_size=torch.tensor(49408))
    for key, val in list(small.state_dict().items()) + list(extras.items()):
        mod, parts = root, key.split(".")
        for part in parts[:-1]:
            if not hasattr(mod, part):
                mod.add_module(part, Node())
            mod = getattr(mod, part)
        if val.is_floating_point():
            mod.register_parameter(parts[-1], torch.nn.Parameter(val.clone(), requires_grad=False))
        else:
            mod.register_buffer(parts[-1], val.clone())
    archive = tmp_path / "archive.pt"
    torch.jit.script(root).save(str(archive))
    assert "vocab_size" in torch.jit.load(str(archive), map_location="cpu").state_dict()
    scripted = clip.read_state_dict(str(archive))
    assert set(scripted) == set(small.state_dict()) and all(torch.equal(scripted[k], v) for k, v in small.state_dict().items())
    with pytest.raises(FileNotFoundError):
        clip.load(str(tmp_path / "missing.pt"), "cpu", torch.float32)
    with pytest.raises(ValueError, match="missing"):          # narrow weights into the ViT-B/32 default: refused by name
        clip.load(str(plain), "cpu", torch.float32)


def _cases():
    from oracle.gen_golden import LOSS_CASES
    return LOSS_CASES


def _case_boxes(objs, image=0, side=512):
    from ldm.models.diffusion.plms import object_crop_box
    return [(image, 0, side, 0, side)] + [(image,) + tuple(object_crop_box(c, side, side)) for _, c in objs]


def test_views_reference_matches_reference_fixture():
    """Test 3: the patch rows of views_reference, un-patchified, are the 224^2 images the REFERENCE's DCLIPLoss hands to CLIP
    (tests/golden/loss_frontend.npz; case 1 has border-clipped, non-square crops). Bounds of the existing front-end test."""
    from sta import clip
    g = np.load(os.path.join(GOLDEN, "loss_frontend.npz"))
    for n, (seed, text, objs) in enumerate(_cases()):
        img = gi.loss_image(seed)
        rows = clip.views_reference(img.unsqueeze(0), _case_boxes(objs))
        assert rows.shape == (1 + len(objs), 49, 3072) and rows.dtype == torch.float32
        fed = clip.unpatchify(rows, 32)
        assert np.abs(fed[:, :, ::7, ::7].numpy() - g["case%d_fed" % n]).max() < 1e-6
        assert np.allclose([float(f.double().sum()) for f in fed], g["case%d_fed_sum" % n], rtol=1e-6)
    assert torch.equal(clip.patchify(fed, 32), rows)


def test_view_shape_rules():
    from sta import clip
    for H, W in ((224, 224), (512, 768), (520, 520), (1056, 1056)):
        with pytest.raises(ValueError):
            clip.check_view_shapes(H, W)
    clip.check_view_shapes(768, 768, [(0, 0, 768, 0, 768), (1, 3, 5, 0, 768)], 2)
    for bad in ([(0, 0, 513, 0, 512)], [(0, 4, 5, 0, 512)], [(2, 0, 512, 0, 512)], [(1, 0, 512, 0, 512), (0, 0, 512, 0, 512)]):
        with pytest.raises(ValueError):
            clip.check_view_shapes(512, 512, bad, 2)


def test_c_abi_refuses_bad_shapes_with_text():
    """The shape rules are checked on the host copy of the box table before any launch: no GPU needed to be refused."""
    from sta import lib
    L = lib.load()
    fake = 4096          # never dereferenced: every call below is refused before the launch
    for fn in (L.sta_clip_views, L.sta_clip_views_bwd):
        for H, W, box, text in ((224, 224, [0, 0, 224, 0, 224], "256 <= H <= 1024"), (512, 768, [0, 0, 512, 0, 768], "H == W"),
                                (520, 520, [0, 0, 520, 0, 520], "multiple of 32"), (512, 512, [0, 0, 513, 0, 512], "inside 512x512"),
                                (512, 512, [0, 9, 10, 0, 512], "2x2"), (512, 512, [3, 0, 512, 0, 512], "image 3 of 2")):
            host = torch.tensor([box], dtype=torch.int32)
            assert fn(fake, fake, host.data_ptr(), fake, 2, H, W, 1, lib.STA_F16, None) != 0
            assert text in lib.last_error(), lib.last_error()
    host = torch.tensor([[1, 0, 512, 0, 512], [0, 0, 512, 0, 512]], dtype=torch.int32)
    assert L.sta_clip_views_bwd(fake, fake, host.data_ptr(), fake, 2, 512, 512, 2, lib.STA_F16, None) != 0
    assert "grouped by image" in lib.last_error()
    host = torch.tensor([[0, 0, 512, 0, 512]], dtype=torch.int32)
    assert L.sta_clip_views(fake, fake, host.data_ptr(), fake, 1, 512, 512, 1, 7, None) != 0 and "dtype" in lib.last_error()


def test_forward_batch_equals_view_by_view():
    """Test 4: one batch of the three fixture cases (K = 2, 3, 0) through forward_batch against the sum of
    PLMSSampler._fidelity_loss, value and image gradient; the text cache."""
    from ldm.models.diffusion.plms import DCLIPLoss, PLMSSampler
    from sta import clip
    model = clip.synthetic("cpu", seed=5, dtype=torch.float32, **NARROW)
    calls = []
    enc = model.encode_text
    model.encode_text = lambda tok: (calls.append(1), enc(tok))[1]
    lm = DCLIPLoss(model)
    assert lm.tokenize is clip.hash_tokenize
    sampler = object.__new__(PLMSSampler)
    sampler.clip_loss_model, sampler.local_loss_weight = lm, 5.0
    cases = _cases()
    imgs = torch.stack([gi.loss_image(seed) for seed, _, _ in cases])
    texts = [t for _, t, _ in cases]
    boxes = [[c for _, c in objs] for _, _, objs in cases]
    names = [[nm for nm, _ in objs] for _, _, objs in cases]

    a = imgs.clone().requires_grad_(True)
    ref = sum(sampler._fidelity_loss(a[i], texts[i], boxes[i], names[i]) for i in range(len(cases)))
    ref.backward()
    b = imgs.clone().requires_grad_(True)
    del calls[:]
    got = lm.forward_batch(b, texts, boxes, names, 5.0)
    got.backward()
    print("forward_batch %.8f view-by-view %.8f" % (float(got), float(ref)))
    assert abs(float(got) - float(ref)) <= 1e-5
    assert float((a.grad - b.grad).abs().max()) <= 1e-5 * float(a.grad.abs().max())
    assert not lm.batch_ready(imgs)                       # CPU tensors: the sampler keeps the view-by-view path

    distinct = len(set(s for t, nm in zip(texts, names) for s in clip.loss_strings(t, nm)))
    assert len(calls) == distinct == len(lm._text_cache) == 8
    f1 = lm.text_feature(texts[0], imgs.device)
    again = lm.forward_batch(imgs, texts, boxes, names, 5.0)
    assert len(calls) == distinct and lm.text_feature(texts[0], imgs.device) is f1
    assert abs(float(again) - float(got)) <= 1e-6


class _StubTokenizer:
    """The call interface of transformers.CLIPTokenizer that sta.clip.ClipTokenize uses: one id per word."""

    def __call__(self, text, add_special_tokens=True, **kw):
        assert add_special_tokens is False
        return {"input_ids": [100 + len(w) for w in text.split()]}


def test_tokenizer_adapter():
    from sta import clip
    tok = clip.ClipTokenize(_StubTokenizer())
    out = tok(["a cat", "one two three"])
    assert out.shape == (2, 77) and out.dtype == torch.int64
    assert out[0].tolist()[:5] == [49406, 101, 103, 49407, 0] and int(out[1, 4]) == 49407 and int(out[:, 5:].sum()) == 0
    assert tok("a cat").shape == (1, 77)
    tok([" ".join(["w"] * 75)])
    with pytest.raises(RuntimeError, match="too long"):
        tok([" ".join(["w"] * 76)])
    assert clip.hash_tokenize(["A Cat", "a cat"])[0].tolist() == clip.hash_tokenize(["A Cat", "a cat"])[1].tolist()
    with pytest.raises(RuntimeError, match="too long"):
        clip.hash_tokenize([" ".join(["w"] * 76)])


def _script(name):
    if SCRIPTS not in sys.path:
        sys.path.insert(0, SCRIPTS)
    import importlib
    return importlib.import_module(name)


def test_cli_refuses_before_any_model_is_built(tmp_path, monkeypatch):
    """Test 5: --clip builtin:/no/such/file and an over-long prompt stop the entry points before a model exists."""
    common = _script("_txt2img_common")
    opt = common.build_parser("gpt").parse_args(["--clip", "builtin:/no/such/file", "--clip_tokenizer", str(tmp_path)])
    with pytest.raises(SystemExit, match="no such weights file"):
        common.check_options(opt)
    opt = common.build_parser("gpt").parse_args(["--clip", "builtin:" + __file__])
    with pytest.raises(SystemExit, match="clip_tokenizer"):
        common.check_options(opt)
    opt = common.build_parser("gpt").parse_args(["--clip", "builtin:synthetic", "--H", "520", "--W", "520"])
    with pytest.raises(SystemExit, match="multiple of 32"):
        common.check_options(opt)
    common.check_options(common.build_parser("gpt").parse_args(["--clip", "builtin:/no/such/file", "--opt_epochs", "0"]))
    common.check_options(common.build_parser("gpt").parse_args(["--clip", "builtin:synthetic"]))
    from sta import clip
    with pytest.raises(SystemExit, match="too long"):
        common.check_loss_texts(clip.ClipTokenize(_StubTokenizer()), [("a cat", ["cat"]), ("short", [" ".join(["w"] * 80)])])
    common.check_loss_texts(clip.ClipTokenize(_StubTokenizer()), [("a cat", ["The cat", "dog"])])

    from ldm.models.diffusion.plms import load_clip_model
    with pytest.raises(FileNotFoundError):
        load_clip_model("builtin:/no/such/file", "cpu", tokenizer_path=str(tmp_path))
    try:
        import clip as _openai_clip  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="--clip builtin:PATH"):
            load_clip_model(None, "cpu")

    # the img2img entry point, end to end on the host: the over-long prompt stops it before the GPU is asked for
    from PIL import Image
    png = tmp_path / "init.png"
    Image.fromarray((np.random.default_rng(0).random((256, 256, 3)) * 255).astype(np.uint8)).save(png)
    img2img = _script("img2img")
    built = []
    import sta.pipeline
    monkeypatch.setattr(sta.pipeline, "build_sd_v1", lambda *a, **k: built.append(1))
    args = ["--init-img", str(png), "--synthetic", "--opt_epochs", "3", "--clip", "builtin:synthetic"]
    with pytest.raises(SystemExit, match="too long"):
        img2img.main(args + ["--prompt", " ".join(["word"] * 80)])
    with pytest.raises(SystemExit, match="no such weights file"):
        img2img.main(args[:-1] + ["builtin:/no/such/file", "--prompt", "a cat"])
    assert not built
