"""Per-object attention heat maps during sampling: where an object's tokens attend, and how much of that lies in its disc.

The blocks blend each object's local prompt into its disc with weights that are optimised per step (attention.py:278-294); whether
that worked is visible in the cross-attention itself, without any other model: the softmax mass the pixels put on the object's
name tokens — inside the global prompt (context 1) and inside its own local prompt (context 2 + i).

  token_maps            sta_xattn_token_maps (csrc/sta_xattn.hip): R weighted key sums per pixel, head mean, one launch
  token_maps_backward   sta_xattn_token_maps_bwd (csrc/sta_xattn_maps_bwd.hip): the gradient of the maps w.r.t. q, one launch
  token_maps_tracked    the differentiable readout (TokenMapsFn: forward = the launch above, backward = that one) — what
                        sta.attnloss builds the attention-layout loss on
  token_maps_reference  the same formula in plain torch on unpacked keys — the oracle of the GPU tests and what host-logic tests
                        on a CPU run (the product path has no CPU fall-back: a CPU tensor with a real packed image raises)
  token_weights         which keys a readout weighs: the positions of an object's name tokens in a tokenised prompt
  AttnCapture           context manager that makes the transformer blocks of one resolution record into one buffer over a trajectory

A "readout" r is a context c_r and a weight row w[r][:M] over its keys; the map is
    out[i][r][p] = mean_h sum_m w[i][r][m] softmax_m(scale q_h[p] . K_{i, c_r, h}[m])
with q row 0 for context 0 and q row 1 for the others, exactly as the forward attends them. The disc mask plays no part.
"""
import collections
import ctypes
import re

import torch

from . import lib as _lib
from . import ops as _ops


def _expand_w(w, n_img, R, M, device, dtype=torch.float32):
    w = torch.as_tensor(w).to(dtype)
    if w.dim() == 2:
        w = w.unsqueeze(0).expand(n_img, -1, -1)
    if tuple(w.shape) != (n_img, R, M):
        raise ValueError("w must be [R=%d, M=%d] or [n_img=%d, R, M], got %s" % (R, M, n_img, tuple(w.shape)))
    return w.to(device).contiguous()


def _check_sel(sel_ctx, n_ctx):
    sel = [int(c) for c in sel_ctx]
    if not 1 <= len(sel) <= _lib.MAX_READOUTS:
        raise ValueError("need 1..%d readouts, got %d" % (_lib.MAX_READOUTS, len(sel)))
    if any(c < 0 or c >= n_ctx for c in sel):
        raise ValueError("sel_ctx %s names a context outside 0..%d" % (sel, n_ctx - 1))
    return sel


def token_maps_reference(q, k, sel_ctx, w, heads, scale):
    """q [2 I, N, C], k [I (K + 2), M, C] unpacked keys (image-major), w [R, M] or [I, R, M] -> [I, R, N].
    Plain torch in float32 (float64 inputs stay float64): softmax per head, head mean, weighted key sum."""
    if q.dim() != 3 or q.shape[0] % 2 or k.dim() != 3 or k.shape[0] % (q.shape[0] // 2):
        raise ValueError("q must be [2 I, N, C] and k [I (K + 2), M, C], got %s and %s" % (tuple(q.shape), tuple(k.shape)))
    I, N, C = q.shape[0] // 2, q.shape[1], q.shape[2]
    n_ctx, M = k.shape[0] // I, k.shape[1]
    sel = _check_sel(sel_ctx, n_ctx)
    dt = torch.promote_types(q.dtype, torch.float32)
    w = _expand_w(w, I, len(sel), M, q.device, dt)
    d = C // heads
    out = torch.empty((I, len(sel), N), dtype=dt, device=q.device)
    for i in range(I):
        probs = {}
        for r, c in enumerate(sel):
            if c not in probs:
                qh = q[2 * i + (0 if c == 0 else 1)].to(dt).reshape(N, heads, d).permute(1, 0, 2)
                kh = k[i * n_ctx + c].to(dt).reshape(M, heads, d).permute(1, 0, 2)
                probs[c] = (torch.einsum("hid,hjd->hij", qh, kh) * scale).softmax(dim=-1).mean(dim=0)      # [N, M]
            out[i, r] = probs[c] @ w[i, r]
    return out


def token_maps(q, packed, sel_ctx, w, scale, out=None, accumulate=False):
    """q [2 I, N, C] (per image: uncond row, cond row), packed: sta.ops.pack_kv image of the I (K + 2) contexts, sel_ctx: R context
    indices (host), w [R, M] or [I, R, M] fp32 -> out [I, R, N] fp32 (`out` given: written in place; accumulate: added to it)."""
    I = packed.n_img
    if q.dim() != 3 or q.shape[0] != 2 * I:
        raise ValueError("q must be [2 * n_img, N, C] with n_img=%d, got %s" % (I, tuple(q.shape)))
    N, C = q.shape[1], q.shape[2]
    if C != packed.C:
        raise ValueError("q has C=%d but K/V were packed with C=%d" % (C, packed.C))
    sel = _check_sel(sel_ctx, packed.n_ctx)
    R, M = len(sel), packed.M
    w = _expand_w(w, I, R, M, q.device)
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the buffer to add to (out=)")
        out = torch.empty((I, R, N), dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != (I, R, N) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != q.device:
        raise ValueError("out must be a contiguous float32 [%d, %d, %d] on %s" % (I, R, N, q.device))
    if not q.is_cuda:
        # host-logic tests: the stand-in of tests/cpu_backend.py keeps the unpacked keys; a real image has no CPU reader
        if not hasattr(packed, "k"):
            raise RuntimeError("token_maps needs CUDA/HIP tensors (there is no CPU path)")
        fresh = token_maps_reference(q, packed.k, sel, w, packed.heads, scale).to(torch.float32)
        if accumulate:
            out.add_(fresh)
        else:
            out.copy_(fresh)
        return out
    if q.dtype != packed.dtype:
        raise TypeError("q is %s but K/V were packed as %s" % (q.dtype, packed.dtype))
    q = q.contiguous()
    sel_arr = (ctypes.c_int32 * R)(*sel)
    _lib.check(_lib.load().sta_xattn_token_maps(q.data_ptr(), packed.buf.data_ptr(), ctypes.cast(sel_arr, ctypes.c_void_p), w.data_ptr(),
                                                out.data_ptr(), I, N, C, packed.heads, M, packed.n_ctx - 2, R, float(scale),
                                                1 if accumulate else 0, _ops._dtype_code(q), _ops._stream(q)), "sta_xattn_token_maps")
    return out


def token_maps_backward(q, packed, sel_ctx, w, dmaps, scale, out=None):
    """dq [2 I, N, C] (q's dtype) of token_maps(accumulate=False) for the upstream dmaps [I, R, N] fp32; arguments as token_maps.
    `out` given: overwritten completely (a q row no readout names comes back zero). Only q has a gradient: the keys, the key
    weights and the text embeddings are constants of the optimisation."""
    I = packed.n_img
    if q.dim() != 3 or q.shape[0] != 2 * I:
        raise ValueError("q must be [2 * n_img, N, C] with n_img=%d, got %s" % (I, tuple(q.shape)))
    N, C = q.shape[1], q.shape[2]
    if C != packed.C:
        raise ValueError("q has C=%d but K/V were packed with C=%d" % (C, packed.C))
    sel = _check_sel(sel_ctx, packed.n_ctx)
    R, M = len(sel), packed.M
    if not q.is_cuda:
        raise RuntimeError("token_maps_backward needs CUDA/HIP tensors (there is no CPU path)")
    if q.dtype != packed.dtype:
        raise TypeError("q is %s but K/V were packed as %s" % (q.dtype, packed.dtype))
    w = _expand_w(w, I, R, M, q.device)
    if tuple(dmaps.shape) != (I, R, N) or dmaps.device != q.device:
        raise ValueError("dmaps must be [%d, %d, %d] on %s, got %s" % (I, R, N, q.device, tuple(dmaps.shape)))
    dmaps = dmaps.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty((2 * I, N, C), dtype=q.dtype, device=q.device)
    elif tuple(out.shape) != (2 * I, N, C) or out.dtype != q.dtype or not out.is_contiguous() or out.device != q.device:
        raise ValueError("out must be a contiguous %s [%d, %d, %d] on %s" % (q.dtype, 2 * I, N, C, q.device))
    q = q.contiguous()
    sel_arr = (ctypes.c_int32 * R)(*sel)
    _lib.check(_lib.load().sta_xattn_token_maps_bwd(q.data_ptr(), packed.buf.data_ptr(), ctypes.cast(sel_arr, ctypes.c_void_p), w.data_ptr(),
                                                    dmaps.data_ptr(), out.data_ptr(), I, N, C, packed.heads, M, packed.n_ctx - 2, R,
                                                    float(scale), _ops._dtype_code(q), _ops._stream(q)), "sta_xattn_token_maps_bwd")
    return out


class TokenMapsFn(torch.autograd.Function):
    """maps = token_maps(q, ...) (accumulate = 0) under autograd; backward = sta_xattn_token_maps_bwd. Only q gets a gradient."""

    @staticmethod
    def forward(ctx, q, packed, sel_ctx, w, scale):
        ctx.packed, ctx.sel, ctx.scale = packed, list(sel_ctx), float(scale)
        ctx.save_for_backward(q, w)
        return token_maps(q, packed, sel_ctx, w, scale)

    @staticmethod
    def backward(ctx, dmaps):
        q, w = ctx.saved_tensors
        return token_maps_backward(q, ctx.packed, ctx.sel, w, dmaps, ctx.scale), None, None, None, None


def token_maps_tracked(q, packed, sel_ctx, w, scale):
    """token_maps as a differentiable function of q -> [I, R, N] fp32. GPU: TokenMapsFn (both directions are HIP launches). CPU
    tensors with the host-logic stand-in (packed.k: tests/cpu_backend.py) run token_maps_reference under autograd; a CPU tensor with
    a real packed image raises, as token_maps does."""
    if q.is_cuda:
        I = packed.n_img
        sel = _check_sel(sel_ctx, packed.n_ctx)
        return TokenMapsFn.apply(q, packed, sel, _expand_w(w, I, len(sel), packed.M, q.device), scale)
    if not hasattr(packed, "k"):
        raise RuntimeError("token_maps needs CUDA/HIP tensors (there is no CPU path)")
    return token_maps_reference(q, packed.k, sel_ctx, w, packed.heads, scale).to(torch.float32)


# ---------------------------------------------------------------------------------------------------
# which keys a readout weighs
# ---------------------------------------------------------------------------------------------------
def _words(text):
    return re.findall(r"[a-z0-9]+", text.lower())


def content_tokenizer(hf_tokenizer):
    """str -> token ids WITHOUT the begin / end tokens, from a Hugging Face CLIPTokenizer (FrozenCLIPEmbedder.tokenizer)."""
    return lambda text: list(hf_tokenizer(text, add_special_tokens=False)["input_ids"])


def _positions(tokenize, text, name, M):
    """Key positions of the first occurrence of `name` in `text`; key 0 is the begin token, so content token j sits at key j + 1.
    Keys from M - 1 on are not the prompt's any more (truncation; the last key is the end token). [] if not found."""
    seq, sub = (_words(text), _words(name)) if tokenize is None else (list(tokenize(text)), list(tokenize(name)))
    if not sub:
        return []
    for a in range(len(seq) - len(sub) + 1):
        if seq[a:a + len(sub)] == sub:
            return [a + 1 + j for j in range(len(sub)) if a + 1 + j < M - 1]
    return []


def token_weights(tokenize, prompt, names, local_prompts, M=77):
    """(sel_ctx [R], w [R, M] fp32, found [R] bool) for R = 2 K readouts: row i weighs the positions of object i's name tokens
    inside the tokenised prompt (first matching subsequence, 1 / len each) and reads the global context 1; row K + i does the same
    inside local prompt i and reads context 2 + i. A name that is not found gives a zero row and found = False; nothing raises.
    tokenize: str -> content token ids (no begin / end token; see content_tokenizer), or None — without a tokenizer (synthetic text
    embeddings) positions are the whitespace word index + 1, a STAND-IN that matches no real vocabulary's sub-word split."""
    K = len(names)
    if len(local_prompts) != K:
        raise ValueError("need one local prompt per object, got %d for %d" % (len(local_prompts), K))
    sel = [1] * K + [2 + i for i in range(K)]
    w = torch.zeros((2 * K, M), dtype=torch.float32)
    found = torch.zeros(2 * K, dtype=torch.bool)
    for r, (text, name) in enumerate([(prompt, n) for n in names] + list(zip(local_prompts, names))):
        pos = _positions(tokenize, text, name, M)
        if pos:
            w[r, pos] = 1.0 / len(pos)
            found[r] = True
    return sel, w, found


# ---------------------------------------------------------------------------------------------------
# capture over a trajectory
# ---------------------------------------------------------------------------------------------------
AttnResult = collections.namedtuple("AttnResult", "maps per_call in_disc_mass block_calls calls sel_ctx found")


class AttnCapture:
    """with AttnCapture(unet, resolution=16) as cap: every BasicTransformerBlock whose N == resolution^2 adds its token maps to ONE
    buffer [I, R, N] per UNet call it runs under torch.no_grad() (blocks of other resolutions and calls under autograd record
    nothing). A capturing block needs q in HBM: where it would run to_q inside the attention kernel (levels 0 and 1) it takes the
    to_q GEMM + sta_xattn_fwd path while it captures, as its keep_maps hook does; at the default 16 x 16 (C = 1280) q exists anyway
    and the sampled image does not change. per_call: one buffer per UNet call (a new call starts when a block records a second time).

    Readouts come from set_readouts(sel_ctx, w, objects), or — samplers call begin(centres, texts, names) — from token_weights over
    the prompts with local prompts "a photo of <name>" (sta.pipeline.conditionings) and `tokenize` (None: the whitespace stand-in).
    result() -> AttnResult: maps [I, R, res, res] (mean over block-calls), per_call [calls, I, R, res, res] or None, in_disc_mass
    [I, R] = share of a map's sum inside the disc of the readout's object (sta.ops.disc_masks; nan for a readout without object)."""

    def __init__(self, unet, resolution=16, per_call=False, tokenize=None, M=77):
        self.unet, self.resolution, self.per_call, self.tokenize, self.M = unet, int(resolution), bool(per_call), tokenize, int(M)
        self.recording = False
        self._explicit = None
        self._reset()

    def _reset(self):
        self.sel_ctx = self.w = self.objects = self.found = self.centres = None
        self._bufs, self._seen, self.block_calls, self.calls, self._w_dev = [], set(), 0, 0, None

    # -- configuration ------------------------------------------------------------------------------
    def set_readouts(self, sel_ctx, w, objects=None, found=None):
        """Explicit readouts for the following trajectories. objects[r]: the object whose disc in_disc_mass measures readout r against
        (-1: none); default: r % K for the 2 K rows of token_weights, else the object of a local context."""
        self._explicit = (list(sel_ctx), torch.as_tensor(w, dtype=torch.float32), objects, found)

    def begin(self, centres, texts=None, names=None):
        """Start a new accumulation. centres: per image the K (x, y) disc centres; texts / names per image when the readouts are to be
        derived from the prompts."""
        self._reset()
        self.centres = [[(float(c[0]), float(c[1])) for c in cs] for cs in centres]
        K = len(self.centres[0]) if self.centres else 0
        if self._explicit is not None:
            self.sel_ctx, self.w, objects, found = self._explicit
        else:
            if texts is None or names is None:
                raise ValueError("no readouts: call set_readouts(...) or give begin() the prompts and object names")
            if K == 0:
                return self          # prompts without objects have no name tokens to read: this trajectory records nothing
            rows = [token_weights(self.tokenize, t, nm, ["a photo of " + n for n in nm], self.M) for t, nm in zip(texts, names)]
            self.sel_ctx, self.w, found, objects = rows[0][0], torch.stack([r[1] for r in rows]), torch.stack([r[2] for r in rows]), None
        R = len(self.sel_ctx)
        if objects is None:
            objects = [r % K for r in range(R)] if K and R == 2 * K else [c - 2 if c >= 2 else -1 for c in self.sel_ctx]
        if len(objects) != R or any(o >= K for o in objects):
            raise ValueError("objects %s do not fit %d readouts of %d objects" % (objects, R, K))
        self.objects, self.found = list(objects), found
        return self

    def __enter__(self):
        if self.centres is None:
            raise RuntimeError("AttnCapture has no readouts yet: call begin(...) before entering it")
        from ldm.modules.attention import BasicTransformerBlock
        self._blocks = [m for m in self.unet.modules() if isinstance(m, BasicTransformerBlock)]
        for blk in self._blocks:
            blk._attn_capture = self
        self.recording = True
        return self

    def __exit__(self, *exc):
        self.recording = False
        for blk in self._blocks:
            blk._attn_capture = None
        return False

    # -- what the blocks call -----------------------------------------------------------------------
    def wants(self, n):
        return self.recording and self.sel_ctx is not None and n == self.resolution * self.resolution and not torch.is_grad_enabled()

    def record(self, block, q, cache):
        I, N = q.shape[0] // 2, q.shape[1]
        new_call = id(block) in self._seen or not self._bufs
        if new_call:
            self._seen.clear()
            self.calls += 1
            if self.per_call or not self._bufs:
                self._bufs.append(torch.zeros((I, len(self.sel_ctx), N), dtype=torch.float32, device=q.device))
        self._seen.add(id(block))
        if self._w_dev is None or self._w_dev.device != q.device:          # one host -> device copy per trajectory, not per block call
            self._w_dev = _expand_w(self.w, I, len(self.sel_ctx), cache.packed.M, q.device)
        with torch.no_grad():
            token_maps(q.detach(), cache.packed, self.sel_ctx, self._w_dev, block.attn2.scale, out=self._bufs[-1], accumulate=True)
        self.block_calls += 1

    # -- result -------------------------------------------------------------------------------------
    def result(self):
        if not self._bufs:
            return None
        res = self.resolution
        stack = torch.stack(self._bufs)                                   # [calls or 1, I, R, N]
        I, R = stack.shape[1], stack.shape[2]
        maps = (stack.sum(0) / self.block_calls).reshape(I, R, res, res)
        per_call = None
        if self.per_call:
            per_call = (stack / (self.block_calls / len(self._bufs))).reshape(len(self._bufs), I, R, res, res)
        mass = torch.full((I, R), float("nan"))
        flat = maps.reshape(I, R, -1).float().cpu()
        for i in range(I):
            disc = _ops.disc_masks(self.centres[i], res).float() if self.centres and self.centres[i] else None
            for r, o in enumerate(self.objects):
                if o >= 0 and disc is not None:
                    total = float(flat[i, r].sum())
                    mass[i, r] = float((flat[i, r] * disc[o]).sum()) / total if total > 0 else 0.0
        return AttnResult(maps, per_call, mass, self.block_calls, self.calls, list(self.sel_ctx), self.found)


def overlay(image_hwc_u8, heat, centre, radius=0.2, alpha=0.6):
    """uint8 [H, W, 3] image with the heat map [res, res] (scaled to its own maximum, nearest-upsampled, red channel ramp) laid over
    it and the outline of the disc of `centre` (x, y in 0..1; attention.py:251-262: dx^2 + dy^2 < 0.04) in white. numpy only."""
    import numpy as np
    img = np.asarray(image_hwc_u8).astype(np.float32)
    H, W = img.shape[:2]
    heat = np.asarray(heat, dtype=np.float32)
    heat = heat / heat.max() if heat.max() > 0 else heat
    ys = np.minimum((np.arange(H) * heat.shape[0]) // H, heat.shape[0] - 1)
    xs = np.minimum((np.arange(W) * heat.shape[1]) // W, heat.shape[1] - 1)
    up = heat[ys][:, xs][..., None]
    colour = np.stack([np.full_like(up[..., 0], 255.0), 255.0 * (1 - up[..., 0]), 255.0 * (1 - up[..., 0])], axis=-1)
    out = img * (1 - alpha * up) + colour * (alpha * up)
    dist = np.sqrt((np.arange(W)[None, :] / W - centre[0]) ** 2 + (np.arange(H)[:, None] / H - centre[1]) ** 2)
    out[np.abs(dist - radius) < 1.5 / max(H, W)] = 255.0
    return np.clip(out, 0, 255).astype(np.uint8)


def save_result(outdir, prompt_idx, names, centres, attn, image=None, index=0):
    """<outdir>/attn/<prompt index>.npz (maps [R, res, res], per_call if kept, names, centres, sel_ctx, found, in_disc_mass of image
    `index` of an AttnResult) and, with `image` ([3, H, W] in [0, 1]), one PNG per readout with an object: the heat map over the image
    with the disc outline. Returns the lines that report the in-disc mass per object."""
    import os
    import numpy as np
    folder = os.path.join(outdir, "attn")
    os.makedirs(folder, exist_ok=True)
    maps = attn.maps[index].float().cpu().numpy()
    mass = attn.in_disc_mass[index].numpy()
    found = attn.found if attn.found is not None else torch.ones(maps.shape[0], dtype=torch.bool)
    found = (found[index] if found.dim() == 2 else found).numpy()
    extra = {} if attn.per_call is None else {"per_call": attn.per_call[:, index].float().cpu().numpy()}
    np.savez(os.path.join(folder, "%d.npz" % prompt_idx), maps=maps, names=np.asarray(list(names)), centres=np.asarray(centres, dtype=np.float32),
             sel_ctx=np.asarray(attn.sel_ctx), found=found, in_disc_mass=mass, block_calls=attn.block_calls, **extra)
    K, lines = len(names), []
    img8 = None if image is None else (255.0 * image.detach().float().clamp(0, 1).cpu().numpy().transpose(1, 2, 0)).astype(np.uint8)
    for r, c in enumerate(attn.sel_ctx):
        o = r % K if K and maps.shape[0] == 2 * K else (c - 2 if c >= 2 else -1)
        if o < 0:
            continue
        where = "global prompt" if c == 1 else "local prompt %d" % (c - 2)
        lines.append("prompt %d  %-20s in %-15s in-disc mass %.3f%s" % (prompt_idx, names[o], where, mass[r], "" if found[r] else "  (name not found: zero map)"))
        if img8 is not None:
            from PIL import Image
            Image.fromarray(overlay(img8, maps[r], centres[o])).save(os.path.join(folder, "%d_%s_ctx%d.png" % (prompt_idx, re.sub(r"\W+", "_", names[o]), c)))
    return lines
