"""CLIP ViT-B/32 for the fidelity loss, and the loss's image front end.

The reference's loss model is the OpenAI `clip` package's ViT-B/32 (plms.py:21-61). This module is that model without the
package: `ClipViTB32` has the package's parameter names (the published weights load by name, `strict=True`) and its
arithmetic (pre-LN residual blocks, QuickGELU, LayerNorm eps 1e-5 evaluated in fp32, class-token / end-of-text pooling,
projection matrices applied on the right). The image is NOT normalised by mean / std: the reference's loss feeds raw [0, 1]
pixels (plms.py:28-44) and so does this one.

The front end: `clip_views(img, boxes, dtype)` gives the patch rows [n_views, 49, 3072] of the 224^2 views of `img`
(global view: x7 nearest upsample + average pool; crop views: bilinear resize of a box). On the GPU that is
sta_clip_views / sta_clip_views_bwd (csrc/sta_clip.hip) behind an autograd Function; on the CPU `views_reference`, the
same two rules in plain torch. `ClipViTB32.encode_patches` takes those rows: the patch embedding is one GEMM.

Attention of both towers is batched matmul + fp32 softmax: 50 / 77 tokens, no fused kernel behind it.
"""
import collections
import math
import os
import sys
import zlib

import torch
import torch.nn.functional as F
from torch import nn

from . import lib

VIEW = 224
SOT, EOT, CONTEXT = 49406, 49407, 77
_DT = {torch.bfloat16: lib.STA_BF16, torch.float16: lib.STA_F16}


# ---------------------------------------------------------------------------------------------------- the model
class _LayerNorm(nn.LayerNorm):
    """fp32 statistics whatever the tower's type (OpenAI CLIP model.py `LayerNorm`)."""

    def forward(self, x):
        if x.dtype == torch.float32 or x.dtype == torch.float64:
            return super().forward(x)
        return F.layer_norm(x.float(), self.normalized_shape, self.weight.float(), self.bias.float(), self.eps).to(x.dtype)


class _QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class _Attention(nn.Module):
    """nn.MultiheadAttention's parameters (in_proj_weight [3D, D], in_proj_bias, out_proj) with the product written out:
    softmax(q k^T / sqrt(d) + mask) v, the softmax in fp32."""

    def __init__(self, width, heads):
        super().__init__()
        assert width % heads == 0
        self.heads = heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * width))
        self.out_proj = nn.Linear(width, width)

    def forward(self, x, mask=None):
        B, L, D = x.shape
        h = self.heads
        q, k, v = F.linear(x, self.in_proj_weight, self.in_proj_bias).view(B, L, 3, h, D // h).permute(2, 0, 3, 1, 4)
        s = torch.matmul(q * (D // h) ** -0.5, k.transpose(-1, -2))
        acc = torch.float32 if s.dtype in (torch.float16, torch.bfloat16) else s.dtype
        s = s.to(acc)
        if mask is not None:
            s = s + mask.to(acc)
        o = torch.matmul(torch.softmax(s, dim=-1).to(v.dtype), v)
        return self.out_proj(o.transpose(1, 2).reshape(B, L, D))


class _Block(nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        self.attn = _Attention(width, heads)
        self.ln_1 = _LayerNorm(width)
        self.mlp = nn.Sequential(collections.OrderedDict([("c_fc", nn.Linear(width, 4 * width)), ("gelu", _QuickGELU()),
                                                          ("c_proj", nn.Linear(4 * width, width))]))
        self.ln_2 = _LayerNorm(width)

    def forward(self, x, mask=None):
        x = x + self.attn(self.ln_1(x), mask)
        return x + self.mlp(self.ln_2(x))


class _Transformer(nn.Module):
    def __init__(self, width, layers, heads):
        super().__init__()
        self.resblocks = nn.ModuleList([_Block(width, heads) for _ in range(layers)])

    def forward(self, x, mask=None):
        for blk in self.resblocks:
            x = blk(x, mask)
        return x


class _Visual(nn.Module):
    def __init__(self, resolution, patch, width, layers, heads, embed_dim):
        super().__init__()
        assert resolution % patch == 0
        self.resolution, self.patch, self.width = resolution, patch, width
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch, stride=patch, bias=False)
        self.class_embedding = nn.Parameter(torch.empty(width))
        self.positional_embedding = nn.Parameter(torch.empty((resolution // patch) ** 2 + 1, width))
        self.ln_pre = _LayerNorm(width)
        self.transformer = _Transformer(width, layers, heads)
        self.ln_post = _LayerNorm(width)
        self.proj = nn.Parameter(torch.empty(width, embed_dim))

    def forward_patches(self, rows):
        """rows [B, (R/P)^2, 3 P P], columns in (c, dy, dx) order = conv1.weight.view(width, -1)'s."""
        x = F.linear(rows, self.conv1.weight.view(self.width, -1))
        cls = self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1)
        x = torch.cat([cls, x], dim=1) + self.positional_embedding.to(x.dtype)
        x = self.transformer(self.ln_pre(x))
        return self.ln_post(x[:, 0, :]) @ self.proj


def patchify(img, patch):
    """[n, 3, R, R] -> [n, (R/P)^2, 3 P P], one row per patch, columns (c, dy, dx)."""
    n, c, R, _ = img.shape
    g = R // patch
    return img.reshape(n, c, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n, g * g, c * patch * patch)


def unpatchify(rows, patch, channels=3):
    n, gg, _ = rows.shape
    g = int(round(math.sqrt(gg)))
    return rows.reshape(n, g, g, channels, patch, patch).permute(0, 3, 1, 4, 2, 5).reshape(n, channels, g * patch, g * patch)


class ClipViTB32(nn.Module):
    """OpenAI CLIP with a ViT image tower; the defaults are ViT-B/32. `encode_image(img [B, 3, R, R])`,
    `encode_text(tokens [B, 77])` as `DCLIPLoss` calls them; `encode_patches(rows)` for the batched loss."""

    def __init__(self, embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32, vision_heads=12,
                 context_length=CONTEXT, vocab_size=49408, transformer_width=512, transformer_heads=8, transformer_layers=12):
        super().__init__()
        self.context_length = context_length
        self.visual = _Visual(image_resolution, vision_patch_size, vision_width, vision_layers, vision_heads, embed_dim)
        self.transformer = _Transformer(transformer_width, transformer_layers, transformer_heads)
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = _LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.tokenize = None
        with torch.no_grad():                       # OpenAI CLIP's initialisation; real use loads weights over it
            nn.init.normal_(self.token_embedding.weight, std=0.02)
            nn.init.normal_(self.positional_embedding, std=0.01)
            nn.init.normal_(self.text_projection, std=transformer_width ** -0.5)
            nn.init.normal_(self.visual.class_embedding, std=vision_width ** -0.5)
            nn.init.normal_(self.visual.positional_embedding, std=vision_width ** -0.5)
            nn.init.normal_(self.visual.proj, std=vision_width ** -0.5)
            for tower in (self.visual.transformer, self.transformer):
                for blk in tower.resblocks:
                    nn.init.normal_(blk.attn.in_proj_weight, std=blk.attn.in_proj_weight.shape[1] ** -0.5)
                    nn.init.zeros_(blk.attn.in_proj_bias)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_patches(self, rows):
        return self.visual.forward_patches(rows.to(self.dtype))

    def encode_image(self, image):
        v = self.visual
        if image.shape[-1] != v.resolution or image.shape[-2] != v.resolution:
            raise ValueError("encode_image takes %dx%d images, got %s" % (v.resolution, v.resolution, tuple(image.shape)))
        return self.encode_patches(patchify(image.to(self.dtype), v.patch))

    def encode_text(self, tokens):
        x = self.token_embedding(tokens) + self.positional_embedding.to(self.dtype)
        L = x.shape[1]
        mask = torch.full((L, L), float("-inf"), device=x.device).triu_(1)
        x = self.ln_final(self.transformer(x, mask))
        return x[torch.arange(x.shape[0], device=x.device), tokens.argmax(dim=-1)] @ self.text_projection


# ---------------------------------------------------------------------------------------------------- weights
_SCRIPT_EXTRAS = ("input_resolution", "context_length", "vocab_size")


def from_hf_state_dict(sd):
    """A Hugging Face `CLIPModel` state_dict under the OpenAI names: q / k / v concatenated into in_proj_*, the two projection
    Linears transposed, `pre_layrnorm` -> `ln_pre`, ... Buffers (position_ids) are dropped."""
    out = {}

    def tower(src, dst):
        layers = sorted({int(k[len(src):].split(".")[0]) for k in sd if k.startswith(src)})
        for i in layers:
            s, d = "%s%d." % (src, i), "%s%d." % (dst, i)
            for leaf in ("weight", "bias"):
                out[d + "attn.in_proj_" + leaf] = torch.cat([sd[s + "self_attn.%s_proj.%s" % (n, leaf)] for n in "qkv"], dim=0)
                out[d + "attn.out_proj." + leaf] = sd[s + "self_attn.out_proj." + leaf]
                out[d + "ln_1." + leaf] = sd[s + "layer_norm1." + leaf]
                out[d + "ln_2." + leaf] = sd[s + "layer_norm2." + leaf]
                out[d + "mlp.c_fc." + leaf] = sd[s + "mlp.fc1." + leaf]
                out[d + "mlp.c_proj." + leaf] = sd[s + "mlp.fc2." + leaf]

    tower("vision_model.encoder.layers.", "visual.transformer.resblocks.")
    tower("text_model.encoder.layers.", "transformer.resblocks.")
    direct = {"vision_model.embeddings.class_embedding": "visual.class_embedding",
              "vision_model.embeddings.patch_embedding.weight": "visual.conv1.weight",
              "vision_model.embeddings.position_embedding.weight": "visual.positional_embedding",
              "text_model.embeddings.token_embedding.weight": "token_embedding.weight",
              "text_model.embeddings.position_embedding.weight": "positional_embedding",
              "logit_scale": "logit_scale"}
    for a, b in (("vision_model.pre_layrnorm.", "visual.ln_pre."), ("vision_model.post_layernorm.", "visual.ln_post."),
                 ("text_model.final_layer_norm.", "ln_final.")):
        for leaf in ("weight", "bias"):
            direct[a + leaf] = b + leaf
    for a, b in direct.items():
        if a in sd:
            out[b] = sd[a]
    if "visual_projection.weight" in sd:
        out["visual.proj"] = sd["visual_projection.weight"].t().contiguous()
    if "text_projection.weight" in sd:
        out["text_projection"] = sd["text_projection.weight"].t().contiguous()
    return out


def check_state_dict(model, sd):
    """Raise with the first offending names unless `sd` has exactly the model's tensors."""
    want = model.state_dict()
    missing = [k for k in want if k not in sd]
    extra = [k for k in sd if k not in want]
    shape = ["%s %s (want %s)" % (k, tuple(sd[k].shape), tuple(want[k].shape)) for k in want
             if k in sd and tuple(sd[k].shape) != tuple(want[k].shape)]
    if missing or extra or shape:
        part = lambda name, xs: "%d %s%s" % (len(xs), name, (": " + ", ".join(xs[:4]) + (" ..." if len(xs) > 4 else "")) if xs else "")
        raise ValueError("not a CLIP ViT-B/32 state_dict: %s; %s; %s" % (part("missing", missing), part("unexpected", extra),
                                                                          part("mis-shaped", shape)))


def read_state_dict(path):
    """OpenAI names from any of: a plain state_dict file, the official TorchScript archive, a Hugging Face CLIPModel state_dict."""
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()          # the archive `clip.load` downloads
    except RuntimeError:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    if not isinstance(sd, dict) or not all(torch.is_tensor(v) for v in sd.values()):
        raise ValueError("%s does not hold a state_dict" % path)
    sd = {k: v for k, v in sd.items() if k not in _SCRIPT_EXTRAS}
    if any(k.startswith(("text_model.", "vision_model.")) for k in sd):
        sd = from_hf_state_dict(sd)
    return sd


def _frozen(model, device, dtype):
    model = model.to(device=device, dtype=dtype).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def load(path, device="cuda", dtype=torch.float16):
    """ClipViTB32 with the weights of `path` (see read_state_dict), frozen, on `device` in `dtype`."""
    if not os.path.isfile(path):
        raise FileNotFoundError("CLIP weights %s not found" % path)
    sd = read_state_dict(path)
    model = ClipViTB32()
    check_state_dict(model, sd)
    model.load_state_dict(sd, strict=True)
    return _frozen(model, device, dtype)


def synthetic(device="cuda", seed=0, dtype=torch.float16, **arch):
    """ViT-B/32 shape (or `arch`) with seeded_fill_ weights and the hashing tokeniser: for timing and tests. Like
    sta.synth.SyntheticCLIP it says nothing about image quality."""
    from .synth import _tensor_for
    model = ClipViTB32(**arch)
    with torch.no_grad():                                   # synth.seeded_fill_'s values; the scalar logit_scale keeps ln(1 / 0.07)
        for name, t in sorted(model.state_dict().items()):
            if t.dim():
                t.copy_(torch.from_numpy(_tensor_for(name, t.shape, seed)))
    model.tokenize = hash_tokenize
    return _frozen(model, device, dtype)


# ---------------------------------------------------------------------------------------------------- tokens
def _pack(ids, text):
    if len(ids) > CONTEXT - 2:
        raise RuntimeError("Input %s is too long for context length %d" % (text, CONTEXT))      # clip.tokenize's refusal
    row = torch.zeros(CONTEXT, dtype=torch.long)
    row[:len(ids) + 2] = torch.tensor([SOT] + list(ids) + [EOT], dtype=torch.long)
    return row


class ClipTokenize:
    """`clip.tokenize` over a Hugging Face CLIPTokenizer (same BPE vocabulary): list[str] | str -> [n, 77] int64, 49406 first,
    49407 behind the last token, zeros after it; more than 75 tokens are refused."""

    def __init__(self, tok):
        self.tok = tok

    def __call__(self, texts):
        texts = [texts] if isinstance(texts, str) else list(texts)
        return torch.stack([_pack(self.tok(t, add_special_tokens=False)["input_ids"], t) for t in texts])


def tokenizer(path):
    from transformers import CLIPTokenizer
    return ClipTokenize(CLIPTokenizer.from_pretrained(path, local_files_only=True))


def hash_tokenize(texts):
    """Stand-in for runs without a vocabulary file (synthetic weights only): one id per whitespace-separated word, from its CRC."""
    texts = [texts] if isinstance(texts, str) else list(texts)
    return torch.stack([_pack([1 + zlib.crc32(w.encode("utf-8")) % (SOT - 1) for w in t.lower().split()], t) for t in texts])


def loss_strings(prompt, object_names):
    """Every string the loss tokenises for one prompt (plms.py:252, :266-273)."""
    return [prompt] + ["A photo of " + n.lower().replace("the ", "") for n in object_names]


def builtin(spec, device, dtype=torch.float16, tokenizer_path=None):
    """`--clip builtin:<weights | synthetic>` -> (model, tokenize)."""
    if spec == "synthetic":
        model = synthetic(device, dtype=dtype)
        if tokenizer_path is None:
            print("--clip builtin:synthetic without --clip_tokenizer: using the hashing stand-in tokeniser", file=sys.stderr)
            return model, hash_tokenize
        return model, tokenizer(tokenizer_path)
    if tokenizer_path is None:
        raise RuntimeError("--clip builtin:%s needs --clip_tokenizer (directory with the CLIP vocabulary files)" % spec)
    if not os.path.isfile(spec):
        raise FileNotFoundError("CLIP weights %s not found" % spec)
    tok = tokenizer(tokenizer_path)
    return load(spec, device, dtype), tok


# ---------------------------------------------------------------------------------------------------- the views
def check_view_shapes(H, W, boxes=None, B=None):
    """The shape rules of sta_clip_views (include/sta_unet.h), for callers to test before sampling."""
    if H != W or H % 32 or not 256 <= H <= 1024:
        raise ValueError("the CLIP loss front end takes square images with a side that is a multiple of 32 in [256, 1024], got %dx%d" % (H, W))
    if boxes is None:
        return
    if len(boxes) * 49 * 3072 >= 2 ** 31:
        raise ValueError("%d views: the patch rows pass 2^31 elements" % len(boxes))
    prev = 0
    for v, (i, y1, y2, x1, x2) in enumerate(boxes):
        if i < 0 or (B is not None and i >= B):
            raise ValueError("view %d names image %d of %s" % (v, i, B))
        if y1 < 0 or y2 > H or x1 < 0 or x2 > W or y2 - y1 < 2 or x2 - x1 < 2:
            raise ValueError("view %d: box [%d:%d, %d:%d] must be at least 2x2 and inside the %dx%d image" % (v, y1, y2, x1, x2, H, W))
        if i < prev:
            raise ValueError("view %d: boxes must be grouped by image, in image order" % v)
        prev = i


def view_images(img, boxes):
    """The two view rules in plain torch -> [n_views, 3, 224, 224] (differentiable; the global view materialises the 7H x 7W
    upsampled image like DCLIPLoss.forward_2)."""
    B, _, H, W = img.shape
    boxes = [tuple(int(q) for q in bx) for bx in boxes]
    check_view_shapes(H, W, boxes, B)
    p = 7 * H // VIEW
    out = []
    for i, y1, y2, x1, x2 in boxes:
        x = img[i:i + 1]
        if (y1, y2, x1, x2) == (0, H, 0, W):
            out.append(F.avg_pool2d(F.interpolate(x, scale_factor=7, mode="nearest"), p))
        else:
            out.append(F.interpolate(x[:, :, y1:y2, x1:x2], size=(VIEW, VIEW), mode="bilinear", align_corners=False))
    return torch.cat(out)


def views_reference(img, boxes, dtype=None):
    """sta_clip_views in plain torch: [B, 3, H, W] -> patch rows [n_views, 49, 3072] (in img's dtype unless `dtype`)."""
    rows = patchify(view_images(img, boxes), 32)
    return rows if dtype is None else rows.to(dtype)


class _ViewsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, boxes_dev, boxes_host, dtype):
        B, _, H, W = img.shape
        n = boxes_host.shape[0]
        x = img.detach().to(torch.float32).contiguous()
        out = torch.empty((n, 49, 3072), dtype=dtype, device=img.device)
        lib.check(lib.load().sta_clip_views(x.data_ptr(), boxes_dev.data_ptr(), boxes_host.data_ptr(), out.data_ptr(), B, H, W, n,
                                            _DT[dtype], torch.cuda.current_stream(img.device).cuda_stream), "sta_clip_views")
        ctx.boxes, ctx.shape, ctx.dt, ctx.in_dtype = (boxes_dev, boxes_host), (B, H, W), dtype, img.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        B, H, W = ctx.shape
        boxes_dev, boxes_host = ctx.boxes
        d = dout.to(ctx.dt).contiguous()
        dimg = torch.empty((B, 3, H, W), dtype=torch.float32, device=dout.device)
        lib.check(lib.load().sta_clip_views_bwd(d.data_ptr(), boxes_dev.data_ptr(), boxes_host.data_ptr(), dimg.data_ptr(), B, H, W,
                                                boxes_host.shape[0], _DT[ctx.dt], torch.cuda.current_stream(dout.device).cuda_stream),
                  "sta_clip_views_bwd")
        return dimg.to(ctx.in_dtype), None, None, None


def clip_views(img, boxes, dtype=torch.float16):
    """Patch rows [n_views, 49, 3072] of the views `boxes` ([(image, y1, y2, x1, x2)], grouped by image) of img [B, 3, H, W].
    GPU: the HIP kernel pair (16-bit `dtype` only; a missing library is an error); CPU: views_reference."""
    B, C, H, W = img.shape
    boxes = [tuple(int(q) for q in bx) for bx in boxes]
    if C != 3:
        raise ValueError("clip_views takes RGB images, got %d channels" % C)
    check_view_shapes(H, W, boxes, B)
    if not img.is_cuda:
        return views_reference(img, boxes, dtype)
    if dtype not in _DT:
        raise TypeError("sta_clip_views writes fp16 or bf16 rows, not %s" % dtype)
    host = torch.tensor(boxes, dtype=torch.int32).reshape(-1, 5)
    return _ViewsFn.apply(img, host.to(img.device), host, dtype)
