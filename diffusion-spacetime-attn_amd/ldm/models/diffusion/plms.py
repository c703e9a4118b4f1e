"""PLMS sampler with per-object, per-timestep blend-weight optimisation.

Counterpart of the reference's ldm/models/diffusion/plms.py (PLMSSampler.sample :114-180,
plms_sampling :182-293, p_sample_plms :296-358, DCLIPLoss :21-61). Same `sample(...)` keyword
surface and the same numerics:
  * timesteps flip(1, 21, ..., 981) for S = 50; `index = S-1-i`; CFG batch [uncond, cond];
  * first step evaluates the UNet twice with the SAME weights column (pseudo improved Euler);
    Adams-Bashforth orders 2-4 afterwards; DDIM update with eta = 0;
  * weights W[K, S] start at 5/K, Adam(lr 5e-3), `opt_epochs` (default 3) full trajectories each
    followed by one optimiser step on the fidelity loss of the decoded image; the image of the last
    epoch is written to result_outputs/final{E-1}_s{seed}_index_{prompt_idx}.png.
Generalised where the reference hard-wires a constant: the width of W follows S (reference: 50),
the crop size follows the decoded image (reference: 512), the first timestep is announced to the
blocks instead of being compared with 981.

MI355X-specific: with `opt_epochs=0` (fixed weights; BASELINE config 2) the whole CFG UNet call is
captured once into a hipGraph and replayed for the 51 calls of a trajectory (sta.graphs).
"""
import collections
import contextlib
import math
import os

import numpy as np

import torch

from ldm.modules.diffusionmodules.util import make_ddim_sampling_parameters, make_ddim_timesteps
from sta import fused as _fused
from sta import prompt_state as _ps

mode = _ps.MODE


class DCLIPLoss(torch.nn.Module):
    """1 - cos(CLIP(image), CLIP(text)) with the reference's two image front-ends:
    `forward_2` (global): x7 nearest upsample then 16x16 average pool -> 224^2 for a 512^2 image (:36-44);
    `forward_3` (local crop): bilinear resize to 224^2 (:28-35, torchvision `Resize((224, 224))`).
    The CLIP model is third-party (OpenAI CLIP ViT-B/32, unpinned in the reference) and must be supplied: any
    object with `encode_image(img[1,3,224,224])` and `encode_text(tokens)`. `tokenize` is the reference's
    `clip.tokenize` (:31,:38): a callable list[str] -> token tensor; None hands the raw string to `encode_text`
    (stand-in models). See `load_clip_model` for how the entry points obtain both."""

    def __init__(self, clip_model=None, tokenize=None):
        super().__init__()
        if clip_model is None:
            raise RuntimeError("DCLIPLoss needs a CLIP model (encode_image/encode_text); none is bundled. "
                               "Pass loss_model=... to PLMSSampler, or opt_epochs=0 for fixed weights.")
        self.model = clip_model
        self.tokenize = tokenize if tokenize is not None else getattr(clip_model, "tokenize", None)
        self.upsample = torch.nn.Upsample(scale_factor=7)
        self.avg_pool = torch.nn.AvgPool2d(kernel_size=16)

    def _text(self, text, device):
        if self.tokenize is None:
            return text
        return self.tokenize([text]).to(device)                      # :31, :38

    def _loss(self, image224, text):
        fi, ft = self.model.encode_image(image224), self.model.encode_text(self._text(text, image224.device))
        return 1 - torch.nn.functional.cosine_similarity(fi, ft)

    def forward_2(self, image, text):
        return self._loss(self.avg_pool(self.upsample(image.unsqueeze(0))), text)

    def forward_3(self, image, text):
        # torchvision 0.12.0 (the reference's pin, environment_replicate.yml:10) resizes TENSORS with plain bilinear
        # interpolation, align_corners=False, no antialiasing
        img = torch.nn.functional.interpolate(image.unsqueeze(0), size=(224, 224), mode="bilinear", align_corners=False)
        return self._loss(img, text)

    # ------------------------------------------------------------------ the whole step's views as one batch (sta.clip)
    TEXT_CACHE = 4096

    def batch_ready(self, images):
        """The sampler takes `forward_batch` only for the built-in ViT-B/32 with the image on the GPU (the HIP view kernels);
        every other loss model keeps the view-by-view calls."""
        from sta.clip import ClipViTB32
        return isinstance(self.model, ClipViTB32) and images.is_cuda

    def text_feature(self, text, device):
        """encode_text of one string, computed once (text features are constant over a prompt's epochs); the last TEXT_CACHE
        strings are kept."""
        cache = self.__dict__.setdefault("_text_cache", collections.OrderedDict())
        key = (text, str(device))
        if key in cache:
            cache.move_to_end(key)
            return cache[key]
        with torch.no_grad():
            ft = self.model.encode_text(self._text(text, device))[0].detach()
        cache[key] = ft
        while len(cache) > self.TEXT_CACHE:
            cache.popitem(last=False)
        return ft

    def forward_batch(self, images, texts, boxes, names, local_weight=5.0):
        """sum_i (1 - cos(global_i, text_i)) + local_weight sum_k (1 - cos(crop_ik, "A photo of " + name_ik)) over images
        [b, 3, H, W]: the sum of PLMSSampler._fidelity_loss over the batch (same crop rule and name normalisation), with the
        b (1 + K) views built by one sta_clip_views launch (CPU tensors: sta.clip.views_reference) and run through the image
        tower as one batch. Global view: AvgPool(7 H / 224) of the x7 upsample, forward_2's 16 at 512^2."""
        from sta import clip as _clip
        b, _, hgt, wid = images.shape
        assert len(texts) == len(boxes) == len(names) == b
        view_boxes, strings, weights = [], [], []
        for i in range(b):
            view_boxes.append((i, 0, hgt, 0, wid))
            strings.append(texts[i])
            weights.append(1.0)
            for centre, name in zip(boxes[i], names[i]):
                view_boxes.append((i,) + tuple(object_crop_box(centre, hgt, wid)))
                strings.append("A photo of " + name.lower().replace("the ", ""))                    # :266-267
                weights.append(float(local_weight))
        tower = self.model.dtype
        rows = _clip.clip_views(images.float(), view_boxes, tower if images.is_cuda else torch.float32)
        fi = self.model.encode_patches(rows).float()
        ft = torch.stack([self.text_feature(s, images.device) for s in strings]).float()
        w = torch.tensor(weights, dtype=torch.float32, device=images.device)
        return (w * (1 - torch.nn.functional.cosine_similarity(fi, ft))).sum()


def load_clip_model(spec=None, device="cuda", dtype=torch.float16, tokenizer_path=None):
    """(model, tokenize) for the fidelity loss.
      spec None           the reference's own call: `clip.load("ViT-B/32")` + `clip.tokenize` (plms.py:24,31) — needs the
                          OpenAI `clip` package and its weights on disk;
      "module:callable"   import `module`, call `callable(device)` -> model or (model, tokenize);
      path to a .pt file  `clip.load(path)`;
      "builtin:<weights>" this project's own ViT-B/32 (sta.clip) with a state_dict file, the official TorchScript archive or a
                          Hugging Face CLIPModel state_dict; "builtin:synthetic" = seeded weights. No `clip` package involved;
                          the tokeniser comes from `tokenizer_path` (the CLIPTokenizer directory of --clip_tokenizer).
    Raises with the reason when nothing can be loaded — callers do this BEFORE sampling (a trajectory is 51 UNet
    calls; the reference would fail at import time, plms.py:11)."""
    import importlib
    if spec and spec.startswith("builtin:"):
        from sta import clip as _clip
        return _clip.builtin(spec[len("builtin:"):], device, dtype, tokenizer_path)
    if spec and ":" in spec and not os.path.exists(spec):
        mod, fn = spec.split(":", 1)
        got = getattr(importlib.import_module(mod), fn)(device)
        return got if isinstance(got, tuple) else (got, getattr(got, "tokenize", None))
    try:
        clip = importlib.import_module("clip")
    except ImportError as e:
        raise RuntimeError("the fidelity loss needs a CLIP model: the OpenAI `clip` package is not installed; pass "
                           "--clip builtin:PATH (this project's ViT-B/32 with CLIP weights from PATH, plus --clip_tokenizer), "
                           "--clip module:callable (returns an object with encode_image/encode_text, optionally a "
                           "tokenizer), or --opt_epochs 0 for fixed blend weights") from e
    model, _ = clip.load(spec or "ViT-B/32", device=device)
    return model, clip.tokenize


def object_crop_box(centre, height, width, half=0.2):
    """Pixel box [y1:y2, x1:x2] of the square centre +- 0.2 clipped to the image (reference :256-270)."""
    cx, cy = centre
    x1, x2 = max(cx - half, 0), min(cx + half, 1)
    y1, y2 = max(cy - half, 0), min(cy + half, 1)
    return int(height * y1), int(height * y2), int(width * x1), int(width * x2)


class _CallRecompute(torch.autograd.Function):
    """Activation recomputation at UNet-CALL granularity (second half): the forward of a tracked epoch
    runs the whole CFG UNet call WITHOUT autograd — through the inference kernels and the captured hipGraph, exactly like a
    fixed-weight trajectory — and keeps only the call's inputs (the 16 KB latent per image and the weights column). Backward
    re-runs that one call eagerly with autograd and differentiates it w.r.t. (x, coef). The reference checkpoints every block
    instead (util.py:105-145) because 51 calls of saved activations do not fit its GPU; here one call's activations
    (~1.6 GiB per prompt at 512^2) exist only while that call is differentiated, so 32 prompts per step fit in 288 GB and the
    launch-bound eager autograd is amortised over all of them. The gradient is the recomputed call's (16-bit roundings of the
    two forward chains differ in the last bit; tests/test_modules_gpu.py holds dW to the float64 chain).
    `inject` (an _AttnInject, only passed while an attention-layout loss is attached): that loss is a sum of per-call terms E_k,
    each a function of its own call's activations alone, so the recomputed call needs nothing from the forward — the eager re-run
    records E_k and it is differentiated together with the call's output, seeded with d(scaled loss) / dE_k."""

    @staticmethod
    def forward(ctx, fast_fn, slow_fn, t, x, coef, inject=None):
        ctx.slow_fn, ctx.t, ctx.inject = slow_fn, t, inject
        ctx.save_for_backward(x, coef)
        with torch.no_grad():
            return fast_fn(x, t, coef).clone()          # the graph's output buffer is reused by the next replay

    @staticmethod
    def backward(ctx, grad_out):
        x, coef = ctx.saved_tensors
        need_x, need_c = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        x_ = x.detach().requires_grad_(need_x)          # the first call of a trajectory starts from x_T: no dx chain through conv_in
        c_ = coef.detach().requires_grad_(need_c)
        gx = gc = None
        with torch.enable_grad():
            out = ctx.slow_fn(x_, ctx.t, c_)
            term = None if ctx.inject is None else ctx.inject.term()        # E_k of this re-run (None: nothing attached / recorded)
            wrt = [t for t, need in ((x_, need_x), (c_, need_c)) if need]
            if wrt:
                if term is None:
                    grads = list(torch.autograd.grad(out, wrt, grad_out.to(out.dtype), allow_unused=True))
                else:
                    grads = list(torch.autograd.grad([out, term], wrt, [grad_out.to(out.dtype), ctx.inject.seed(term)], allow_unused=True))
                gx = grads.pop(0) if need_x else None
                gc = grads.pop(0) if need_c else None
        ctx.slow_fn = ctx.inject = None
        return (None, None, None, gx, gc) + ((None,) if len(ctx.needs_input_grad) > 5 else ())


class _AttnInject:
    """What a recomputed call needs to differentiate its own term of the attention-layout loss: the collector and the factor
    d(scaled loss) / dE_k = attn_loss_weight * loss scale / n_calls (the scale is known only right before backward)."""

    def __init__(self, loss, weight, n_calls):
        self.loss, self.weight, self.n_calls, self.scale = loss, float(weight), int(n_calls), 1.0

    def term(self):
        return self.loss.take_call()

    def seed(self, term):
        return torch.full_like(term, self.weight * self.scale / self.n_calls)


class PLMSSampler(object):
    def __init__(self, model, schedule="linear", loss_model=None, opt_epochs=3, lr=0.005, weight_init=5.0,
                 local_loss_weight=5.0, use_graph=True, save_images=True, outdir="result_outputs/", loss_scale=None, keep_calls=None,
                 batched_loss=True, attn_capture=None, attn_loss=None, attn_loss_weight=1.0, latent_guidance=None, canvas_guidance=None, **kwargs):
        """`canvas_guidance`: a sta.guidance.CanvasGuidance, the latent guidance of CANVAS trajectories (sample_canvas, inpaint_canvas,
        DDIMSampler.decode_canvas): the first `steps` UNet calls of a canvas are each preceded by its updates on the canvas state (eager
        evaluations of the 2 P T window rows; the ordinary calls run as before); `last_guidance` as below. `sample` / `sample_batch` never
        look at it, and a canvas never looks at `latent_guidance` (which stays refused there). None: nothing changes.
        `latent_guidance`: a sta.guidance.AttnGuidance. In every trajectory that runs WITHOUT autograd (the fixed-weight one, the kept
        last epoch) its first `steps` UNet calls are each preceded by its latent updates (eager evaluations; the ordinary calls run as
        before, graph replay included); what they saw is left in `last_guidance`. Tracked epochs are never guided. None: nothing changes.
        `attn_loss`: a sta.attnloss.AttnLayoutLoss. Tracked epochs then minimise [the fidelity loss if `loss_model` is given] +
        attn_loss_weight x the attention-layout loss, recorded inside the tracked UNet calls; with `loss_model=None` they decode
        nothing. The last epoch is untouched (never tracked: the loss records nothing there). None: nothing changes.
        `attn_capture`: a sta.attnmaps.AttnCapture. The trajectory whose image is kept (the last epoch's, never tracked) then runs
        eagerly — no hipGraph replay — with the capture attached, and its AttnResult is left in `last_attn`; earlier (tracked) epochs
        record nothing. None: nothing changes.
        `loss_scale`: the fidelity loss is multiplied by it before backward and W.grad divided by it before the Adam step.
        None = 1 for bf16 / fp32 models; for an fp16 model the power of two that brings the scaled loss to [2^15, 2^16)
        (2^12 for the synthetic CLIP stand-in's loss of ~11; the same gradients whatever the loss model's own scale is:
        tests/test_modules_gpu.py::test_fp16_small_gradients_survive_with_loss_scaling drives a loss 2^-16 of that one), and
        a tracked epoch whose W.grad comes back non-finite is re-run at 2^-8 of the scale. The backward of a tracked epoch runs through 2 x 51 UNet calls
        and the VAE decoder in the model's 16-bit type: with a CLIP loss the per-pixel gradients are ~1e-6 and smaller, i.e.
        fp16-subnormal or zero, and W.grad would lose precision or flush to 0 silently (bf16 has fp32's exponent range and needs
        nothing). A power of two scales exactly, so the unscaled W.grad equals the unscaled computation wherever that one is
        representable (the reference relies on CUDA autocast with fp32 parameters and no scaler, scripts/txt2img-gpt.py:301)."""
        super().__init__()
        self.loss_scale = loss_scale
        self.batched_loss = batched_loss  # False: view-by-view loss calls even where the loss model offers forward_batch (tests, tools)
        self.keep_calls = keep_calls      # per-call recomputation: how many trailing calls keep their activations (None = sized to HBM)
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.clip_loss_model = loss_model
        self.opt_epochs, self.lr, self.weight_init, self.local_loss_weight = opt_epochs, lr, weight_init, local_loss_weight
        self.use_graph, self.save_images, self.outdir = use_graph, save_images, outdir
        self.last_result = None
        self.attn_capture, self.last_attn = attn_capture, None
        self.attn_loss, self.attn_loss_weight = attn_loss, float(attn_loss_weight)
        self._attn_inject = None          # _AttnInject while a tracked epoch with an attention loss runs
        self.latent_guidance, self.last_guidance = latent_guidance, None
        self.canvas_guidance = canvas_guidance
        self._graphs = None
        self._call_key = None             # (latent shape, object count) of the trajectory being sampled: keys the measured activation size

    def register_buffer(self, name, attr):
        if isinstance(attr, np.ndarray):
            attr = torch.from_numpy(attr)
        if torch.is_tensor(attr):
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, verbose=True):
        if ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize, num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        acp = self.model.alphas_cumprod
        assert acp.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        acp32 = acp.detach().to(torch.float32).cpu().numpy()          # float32 copy, as the reference registers it
        sig, a, a_prev = make_ddim_sampling_parameters(acp32, self.ddim_timesteps, eta=ddim_eta, verbose=verbose)
        # host-side float tables: indexing them never touches the device (no sync inside the step loop)
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = sig, a, a_prev
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1.0 - a)

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0.0, mask=None, x0=None, temperature=1.0, noise_dropout=0.0, score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, text_index=None, curr_text="", bboxs_curr=None, seed=None,
               prompt_idx=None, object_names=None, local_conditionings=None, **kwargs):
        """Same keywords as the reference (:114-143) plus `local_conditionings`: the K embeddings of
        "a photo of <object>" handed over in memory (the reference passes them through files)."""
        if mask is not None or x0 is not None or quantize_x0 or score_corrector is not None or noise_dropout:
            raise NotImplementedError("inpainting / quantisation / score correction are not on this path")
        if conditioning is not None and conditioning.shape[0] != batch_size:
            print("Warning: Got %d conditionings but batch-size is %d" % (conditioning.shape[0], batch_size))
        if batch_size != 1:
            raise ValueError("the spatial-temporal blocks work on one image per CFG batch (n_samples must be 1)")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print("Data shape for PLMS sampling is %s" % (size,))
        self.plms_sampling(conditioning, size, x_T=x_T, temperature=temperature,
                           unconditional_guidance_scale=unconditional_guidance_scale,
                           unconditional_conditioning=unconditional_conditioning, text_index=text_index,
                           curr_text=curr_text, bboxs_curr=bboxs_curr, seed=seed, prompt_idx=prompt_idx,
                           object_names=object_names, local_conditionings=local_conditionings)
        return None

    def sample_batch(self, S, shape, conditionings, unconditional_conditionings, bboxs, object_names, local_conditionings,
                     curr_texts=None, x_T=None, unconditional_guidance_scale=7.5, eta=0.0, seed=1, prompt_indices=None,
                     verbose=False):
        """MI355X extension: I independent prompts (same number of objects) through ONE CFG batch of 2I
        per UNet call — the reference loops over prompts with n_samples = 1 (scripts/txt2img-gpt.py:305).
        Arguments are per-image lists; every image keeps its own x_T, weights W[i] and Adam state, so the
        result of image i equals `sample(...)` on prompt i alone."""
        I = len(conditionings)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        cond = torch.cat(list(conditionings))
        uncond = torch.cat(list(unconditional_conditionings)) if isinstance(unconditional_conditionings, (list, tuple)) \
            else unconditional_conditionings.expand(I, -1, -1)
        self.plms_sampling(cond, (I, C, H, W), x_T=x_T, unconditional_guidance_scale=unconditional_guidance_scale,
                           unconditional_conditioning=uncond, text_index=0,
                           curr_text=list(curr_texts) if curr_texts is not None else [""] * I, bboxs_curr=list(bboxs), seed=seed,
                           prompt_idx=list(prompt_indices) if prompt_indices is not None else list(range(I)),
                           object_names=list(object_names), local_conditionings=list(local_conditionings), batched=True)
        return None

    _canvas = None               # the sta.canvas.Grid while sample_canvas / inpaint_canvas runs (set like _start / _inpaint, cleared in `finally`)
    canvas_fused_step = True     # step-kernel samplers on a canvas: one sta_sampler_step_windows launch per call (False: fuse + step + split)
    _disc_scale = 1.0            # the discs' radius in units of 0.2 window sides while a canvas trajectory runs (set and cleared with _canvas)
    canvas_wrap_margin = 8       # wrapped canvases: latent cells of circular padding per side around the ONE decode (0: none; <= the axis)

    def sample_canvas(self, S, canvas, window, stride=None, conditionings=None, unconditional_conditionings=None, bboxs=None,
                      object_names=None, local_conditionings=None, x_T=None, unconditional_guidance_scale=7.5, eta=0.0, seed=1,
                      prompt_indices=None, curr_texts=None, mask=None, x0=None, channels=4, verbose=False, wrap="", disc_scale=1.0):
        """P wide or tall canvases (same number of objects), each sampled as T overlapping square windows (sta.canvas): every UNet call
        sees the 2 P T window rows as one CFG batch — an ordinary batch of P T images for the blocks, graph replay included —, the T
        predictions are averaged where windows overlap and the sampler step runs on the canvas.
        canvas = (Hc, Wc), window = s, stride (default s / 2): latent pixels, the grid rules of sta.canvas.window_grid. The other
        arguments are per-canvas lists as in `sample_batch`; `bboxs` are normalised to the canvas (every window's blocks get them
        re-expressed in its own coordinates: a disc has radius 0.2 disc_scale s latent pixels in every window; disc_scale = 1.0, the
        default, is 0.2 s everywhere, and a refine of an upscaled picture passes the upscale factor so that an object keeps its share of
        the canvas; on a wrapped axis of length L a disc_scale with L - s < 0.4 disc_scale s is refused); the prompt, the unconditional context,
        the local contexts and the blend weights W[p] belong to the canvas and are repeated per window. x_T: [P, channels, Hc, Wc].
        `last_result`: x0 [P, channels, Hc, Wc], image [P, 3, 8 Hc, 8 Wc] from ONE decode of the whole canvas, W [P, K, S].
        wrap = "x" | "y" | "xy": the canvas closes on itself along those axes (360 degree panorama: "x"; tileable image: "xy"): the
        windows run over the seam (sta.canvas.window_grid's ring rules) and the decode sees `canvas_wrap_margin` latent cells of the
        other side on each wrapped border (`_decode_canvas`).
        Fixed weights only. ValueError before any UNet call for opt_epochs > 1 (the loss front end takes square images:
        sta.clip.check_view_shapes), an attached attn_capture, attn_loss or latent_guidance (layout guidance on a canvas is the sampler's
        `canvas_guidance`, a sta.guidance.CanvasGuidance), mask= / x0= (inpainting) and a non-zero
        `_start` (img2img decodes): none of them is defined on a canvas by this method (inpainting: `inpaint_canvas` of the step-kernel
        samplers)."""
        if mask is not None or x0 is not None:
            raise ValueError("sample_canvas: mask= / x0= (inpainting) is not defined on a canvas (see inpaint_canvas)")
        return self._sample_canvas("sample_canvas", S, canvas, window, stride, conditionings, unconditional_conditionings, bboxs, object_names,
                                   local_conditionings, x_T, unconditional_guidance_scale, eta, seed, prompt_indices, curr_texts, channels,
                                   verbose, wrap=wrap, disc_scale=disc_scale)

    def inpaint_canvas(self, S, canvas, window, stride=None, *, mask=None, x0=None, image=None, mask_px=None, **kwargs):
        """Inpainting / outpainting on a canvas: the step-kernel samplers only (SolverSamplerBase.inpaint_canvas), as `sample(mask=)`."""
        raise NotImplementedError("inpainting / quantisation / score correction are not on this path (masked PLMS is not supported: "
                                  "inpaint_canvas runs on DDIMSampler and DPMSolverSampler)")

    def _sample_canvas(self, what, S, canvas, window, stride, conditionings, unconditional_conditionings, bboxs, object_names,
                       local_conditionings, x_T, unconditional_guidance_scale, eta, seed, prompt_indices, curr_texts, channels, verbose,
                       prepare=None, wrap="", decode_from=None, disc_scale=1.0):
        """The body of sample_canvas, inpaint_canvas and DDIMSampler.decode_canvas: every refusal, then the epoch loop on the canvas with
        `_canvas` set. prepare(P, channels, grid): the caller's own checks and state once the canvas is known (inpaint_canvas: the inpaint
        state). decode_from: None, or the call decode_canvas starts at — its explicit permission for a non-zero `_start`, which it sets
        itself once every refusal has passed (S is then the schedule's own length, and the schedule is not made again)."""
        from sta import canvas as _cv
        if self.opt_epochs > 1:
            raise ValueError("%s samples with fixed blend weights: opt_epochs = %d tracks epochs, and the loss front end "
                             "takes square images (use opt_epochs 0)" % (what, self.opt_epochs))
        for name in ("attn_capture", "attn_loss", "latent_guidance"):
            if getattr(self, name) is not None:
                raise ValueError("%s: an attached %s reads one square image's attention maps; detach it for canvases" % (what, name))
        if getattr(self, "_start", 0):      # set from outside: decode_canvas passes decode_from and leaves `_start` at 0 until here
            raise ValueError("%s: a trajectory that starts at call %d (img2img) is not defined on a canvas" % (what, self._start))
        Hc, Wc = canvas
        grid = _cv.window_grid(Hc, Wc, window, window // 2 if stride is None else stride, wrap)
        disc_scale = _cv.check_disc_scale(grid, disc_scale)
        margin = int(self.canvas_wrap_margin)
        for axis, L in (("x", grid.Wc), ("y", grid.Hc)):
            if axis in grid.wrap and not 0 <= margin <= L:
                raise ValueError("%s: canvas_wrap_margin = %d latent cells does not fit the wrapped %s axis of %d (need 0 .. %d)"
                                 % (what, margin, axis, L, L))
        P = len(conditionings)
        if not (len(bboxs) == len(object_names) == len(local_conditionings) == P):
            raise ValueError("%s takes per-canvas lists of equal length (%d conditionings, %d bboxs, %d object_names, %d "
                             "local_conditionings)" % (what, P, len(bboxs), len(object_names), len(local_conditionings)))
        if x_T is not None and tuple(x_T.shape) != (P, channels, grid.Hc, grid.Wc):
            raise ValueError("x_T %s must be [%d, %d, %d, %d]" % (tuple(x_T.shape), P, channels, grid.Hc, grid.Wc))
        cond = torch.cat(list(conditionings))
        uncond = torch.cat(list(unconditional_conditionings)) if isinstance(unconditional_conditionings, (list, tuple)) \
            else unconditional_conditionings.expand(P, -1, -1)
        if prepare is not None:
            prepare(P, channels, grid)
        self._canvas, self._disc_scale = grid, disc_scale
        try:
            if decode_from is None:
                self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
            else:
                self._start = int(decode_from)
            # the blocks see P T images: the canvas's local contexts once per window
            self.plms_sampling(cond, (P, channels, grid.Hc, grid.Wc), x_T=x_T, unconditional_guidance_scale=unconditional_guidance_scale,
                               unconditional_conditioning=uncond, text_index=0,
                               curr_text=list(curr_texts) if curr_texts is not None else [""] * P, bboxs_curr=list(bboxs), seed=seed,
                               prompt_idx=list(prompt_indices) if prompt_indices is not None else list(range(P)),
                               object_names=list(object_names),
                               local_conditionings=[loc for loc in local_conditionings for _ in range(grid.T)], batched=True)
        finally:
            self._canvas, self._disc_scale = None, 1.0
            if decode_from is not None:
                self._start = 0
        return None

    def _encode_canvas(self, image, grid, first_stage_model=None):
        """The one encode of a canvas picture: image [P, 3, 8 Hc, 8 Wc] in [-1, 1] -> h [P, 8, Hc, Wc], the encoder's conv_out result the
        fused entry launch reads (DDIMSampler.encode_step_canvas). On a wrapped canvas the encoder must see across the seam, as the
        decoder does (`_decode_canvas`): the image is padded circularly by 8 `canvas_wrap_margin` pixels on both sides of every wrapped
        axis, encoded once and cropped by the margin in latent cells (a view: the launch takes its contiguous NHWC copy). (That bounds the
        convolutional seam only: the VAE's mid-block attention is global.)"""
        vae = self.model.first_stage_model if first_stage_model is None else first_stage_model
        m = int(self.canvas_wrap_margin)
        if tuple(image.shape[-2:]) != (8 * grid.Hc, 8 * grid.Wc):
            raise ValueError("image %s is not the canvas's %d x %d pixels" % (tuple(image.shape), 8 * grid.Hc, 8 * grid.Wc))
        if not grid.wrap or m == 0:
            return vae.encode_moments_input(image)
        mx, my = m if "x" in grid.wrap else 0, m if "y" in grid.wrap else 0
        h = vae.encode_moments_input(torch.nn.functional.pad(image, (8 * mx, 8 * mx, 8 * my, 8 * my), mode="circular"))
        return h[..., my:h.shape[-2] - my, mx:h.shape[-1] - mx]

    def _decode_canvas(self, img):
        """The one decode of the final latent. On a wrapped canvas the decoder must see across the seam: the latent is padded circularly
        by `canvas_wrap_margin` cells on both sides of every wrapped axis, decoded once and cropped by 8 margin pixels per side. (That
        bounds the convolutional seam only: the VAE's mid-block attention is global.)"""
        grid, m = self._canvas, int(self.canvas_wrap_margin)
        if grid is None or not grid.wrap or m == 0:
            return self.model.decode_first_stage(img)
        mx, my = m if "x" in grid.wrap else 0, m if "y" in grid.wrap else 0
        out = self.model.decode_first_stage(torch.nn.functional.pad(img, (mx, mx, my, my), mode="circular"))
        return out[..., 8 * my:out.shape[-2] - 8 * my, 8 * mx:out.shape[-1] - 8 * mx].contiguous()

    def _window_unet(self, cond, uncond, scale, bboxs_curr, text_index, graph, img):
        """The canvas trajectory's UNet call -> (grid, unet(xin, t, coef)): xin the [2 P T] window input pairs, t [P] and coef [P, K] of
        the canvases (repeated per window here), the result the UNet's raw [2 P T] output. It is the ordinary eps function of a batch
        of P T images — repeated contexts, every window's own centres —, so graph replay and the fused kernels run as they are."""
        from sta import canvas as _cv
        grid = self._canvas
        P, T = img.shape[0], grid.T
        rep = lambda v: v.repeat_interleave(T, dim=0)
        boxes = [wc for bx in bboxs_curr for wc in _cv.window_centres(bx, grid)]
        inner = self._make_eps_fn(rep(cond), rep(uncond.expand(P, -1, -1)), scale, boxes, text_index, graph, img.new_empty((P * T, 0)),
                                  raw=True)
        def unet(xin, t, coef):
            return inner(xin, rep(t), rep(coef))
        unet.eager_call = lambda xin, t, coef: inner.eager_call(xin, rep(t), rep(coef))      # sta.guidance.CanvasGuidance: never the graph
        return grid, unet

    def _canvas_eps_fn(self, cond, uncond, scale, bboxs_curr, text_index, graph, img):
        """eps(x, t, coef) of a canvas state x [P, C, Hc, Wc] with classifier-free guidance: split into windows, one UNet call, overlap
        mean (sta.canvas) — what _plms_update and _x_prev need to run on canvas tensors unchanged."""
        from sta import canvas as _cv
        grid, unet = self._window_unet(cond, uncond, scale, bboxs_curr, text_index, graph, img)
        wdtype = next(self.model.model.parameters()).dtype
        P = img.shape[0]

        def eps(x, t, coef):
            # the UNet answers in its input's type: `sample` hands it the float32 state, so the guidance arithmetic below runs in x's type
            out = _cv.window_fuse(unet(_cv.window_split(x, grid, wdtype), t, coef), grid).to(x.dtype)
            out = out.reshape(P, 2, *out.shape[1:])
            e_u, e_c = out[:, 0], out[:, 1]
            return e_u + scale * (e_c - e_u)
        eps.eager_call = unet.eager_call
        return eps

    # --------------------------------------------------------------------------------------------------
    def plms_sampling(self, cond, shape, x_T=None, temperature=1.0, unconditional_guidance_scale=1.0,
                      unconditional_conditioning=None, text_index=None, curr_text="", bboxs_curr=None, seed=None,
                      prompt_idx=None, object_names=None, local_conditionings=None, batched=False, **ignored):
        assert seed is not None
        bboxs_curr = [] if bboxs_curr is None else bboxs_curr
        object_names = [] if object_names is None else object_names
        device = self.model.device
        b = shape[0]
        if not batched:          # the reference's single-image call: wrap into one-element batches
            assert len(bboxs_curr) == len(object_names)
            boxes, names, texts, pidx = [bboxs_curr], [object_names], [curr_text], [prompt_idx]
            local = None if local_conditionings is None else [local_conditionings]
        else:
            boxes, names, texts, pidx, local = bboxs_curr, object_names, curr_text, prompt_idx, local_conditionings
            assert len(boxes) == len(names) == b and all(len(bx) == len(nm) for bx, nm in zip(boxes, names))
        K = len(boxes[0])
        assert all(len(bx) == K for bx in boxes), "images of a batch must have the same number of objects"
        time_range = self._time_range()          # the model times of the trajectory's UNet calls, one column of W each
        S = len(time_range)
        img_input = (torch.randn(shape, device=device) if x_T is None else x_T.to(device)).clone()

        # tell the 16 blocks a new prompt (batch) starts (replaces the `time == 981` test + cwd files)
        _ps.begin_prompt(local if (batched or local is None) else local[0], first_timestep=int(time_range[self._first_call()]),
                         disc_radius=0.2 * self._disc_scale)      # 1.0 outside a canvas trajectory: `sample` and `sample_batch` never scale
        block_boxes = boxes if batched else boxes[0]

        W = torch.full((b, K, S), self.weight_init / K if K else 0.0, device=device, dtype=torch.float32)   # :204-209
        W.requires_grad_(self.opt_epochs > 0 and K > 0)
        optimizer = torch.optim.Adam([W], lr=self.lr) if W.requires_grad else None
        if W.requires_grad and self.opt_epochs > 1 and self.clip_loss_model is None and self.attn_loss is None:      # before the first trajectory, not after it
            raise RuntimeError("opt_epochs > 0 needs a loss_model (see DCLIPLoss / load_clip_model) or an attn_loss (sta.attnloss); "
                               "use opt_epochs=0 for fixed weights")

        epochs = max(self.opt_epochs, 1)
        result = {}
        for epoch in range(epochs):
            last = epoch == epochs - 1
            # Only the image of the last epoch is kept and the weights are discarded afterwards, so the
            # backward + Adam step of the last epoch cannot change any output (reference :275-288).
            track = W.requires_grad and not last
            scale_backoff = 1.0
            by_call = track and getattr(self.model, "sta_call_recompute", False)
            cap = self.attn_capture if last else None
            if cap is not None:
                cap.begin(boxes, texts=texts, names=names)
            lg = self.latent_guidance if not track else None
            if lg is not None:
                lg.begin(boxes, texts=texts, names=names)
            elif self._canvas is not None and self.canvas_guidance is not None:      # a canvas (never tracked; latent_guidance is refused there)
                lg = self.canvas_guidance.begin(boxes, texts=texts, names=names, grid=self._canvas)
            al = self.attn_loss if track else None
            decode = not track or self.clip_loss_model is not None or al is None      # tracked with the attention loss alone: no decode
            while True:
                if al is not None:
                    al.begin(boxes, texts=texts, names=names, n_calls=self._n_calls(S))
                    self._attn_inject = _AttnInject(al, self.attn_loss_weight, self._n_calls(S))
                # tracked epochs: eager autograd through the 51 calls, or (sta.pipeline.set_recompute mode "call") the
                # fixed-weight forward per call + one re-run of the call under autograd in backward, with the glue passes of
                # the trunk as autograd Functions over the HIP kernels (sta.fused.tracked)
                with torch.set_grad_enabled(track), _fused.tracked(by_call), (cap if cap is not None else contextlib.nullcontext()), \
                        (self._attn_epoch(al) if al is not None else contextlib.nullcontext()):
                    img = self._trajectory(img_input.clone(), cond, unconditional_conditioning, unconditional_guidance_scale,
                                           time_range, W if batched else W[0], block_boxes, text_index,
                                           graph=self.use_graph and (not track or by_call) and cap is None, call_recompute=by_call)
                    x_img = None
                    if not decode:
                        pass
                    elif self.model.first_stage_model is not None and self._paste() is not None:
                        # inpainting with a pixel-space pair: the result (and what the loss sees) is the original outside the mask
                        from sta import solver as _solver
                        x_img = _solver.image_composite(self._decode_canvas(img), *self._paste())
                    elif self.model.first_stage_model is not None:
                        x_img = torch.clamp((self._decode_canvas(img) + 1.0) / 2.0, min=0.0, max=1.0)   # :249-250
                    if track:
                        lm = self.clip_loss_model
                        if not decode:
                            loss = None
                        elif self.batched_loss and getattr(lm, "batch_ready", None) is not None and lm.batch_ready(x_img):
                            loss = lm.forward_batch(x_img, texts, boxes, names, self.local_loss_weight)
                        else:
                            loss = sum(self._fidelity_loss(x_img[i].float(), texts[i], boxes[i], names[i]) for i in range(b))
                        optimizer.zero_grad()
                        if al is None:
                            scale = self._loss_scale(float(loss.detach())) * scale_backoff
                            (loss * scale if scale != 1.0 else loss).backward()
                        else:
                            loss, scale = self._backward_with_attn_loss(loss, al, img, by_call, scale_backoff)
                        # checked whatever the scale (a backoff can land on exactly 1.0): Adam must never see a non-finite gradient
                        if not bool(torch.isfinite(W.grad).all()):
                            if scale_backoff > 2.0 ** -24:
                                scale_backoff /= 256.0         # an fp16 overflow somewhere in the backward: same epoch again, smaller scale
                                continue
                            raise FloatingPointError("the gradient of the blend weights is not finite even with the loss scale backed "
                                                     "off to %g: refusing to step the optimizer on it" % scale)
                        if scale != 1.0:
                            W.grad.div_(scale)
                        optimizer.step()
                        # (with an attention loss: the whole value, every call's term, whichever way it was differentiated)
                        result.setdefault("losses", []).append(float(loss.detach()))
                break
            if last:
                result.update(x0=img.detach(), image=None if x_img is None else x_img.detach(),
                              W=(W if batched else W[0]).detach().clone())
                if cap is not None:
                    self.last_attn = cap.result()
                if lg is not None:
                    self.last_guidance = lg.result()
                if self.save_images and x_img is not None:
                    for i in range(b):
                        self._save(x_img[i], epochs - 1, seed, pidx[i], index=i)
        self.last_result = result
        return None

    @contextlib.contextmanager
    def _attn_epoch(self, al):
        """The collector attached to the blocks for one tracked trajectory and its backward; detached whatever happens."""
        try:
            with al:
                yield al
        finally:
            self._attn_inject = None

    def _backward_with_attn_loss(self, image_loss, al, img, by_call, scale_backoff):
        """Backward of a tracked epoch with an attention-layout loss attached -> (the whole loss value, the loss scale used).
        The calls recorded under plain autograd (every call in modes none / res / all, the kept trailing calls in mode call) are
        ordinary autograd values; the recomputed calls of mode `call` differentiate their own term inside _CallRecompute.backward,
        seeded with the same weight and loss scale. Without an image loss nothing hangs off the final state, so the backward is
        rooted there with a zero gradient: it then still reaches every recompute node."""
        recorded = al.graph_value()
        if recorded is None and not by_call:
            raise RuntimeError("the attention loss recorded nothing: no transformer block works at %d x %d in this UNet"
                               % (al.resolution, al.resolution))
        parts = [p for p in (image_loss, None if recorded is None else self.attn_loss_weight * recorded) if p is not None]
        known = sum(parts) if parts else None
        scale = self._loss_scale(float(known.detach()) if known is not None else 0.0) * scale_backoff
        self._attn_inject.scale = scale
        roots, seeds = [], []
        if known is not None:
            roots.append(known * scale if scale != 1.0 else known)
            seeds.append(None)
        if by_call and image_loss is None and img.requires_grad:
            roots.append(img)
            seeds.append(torch.zeros_like(img))
        torch.autograd.backward(roots, seeds)
        total = self.attn_loss_weight * al.value().to(img.device)
        return (total if image_loss is None else image_loss.detach() + total), scale

    def _n_calls(self, S):
        """UNet calls of a trajectory over S timesteps: the first PLMS step evaluates the UNet twice."""
        return S + 1

    def _loss_scale(self, loss_value):
        if self.loss_scale is not None:
            return float(self.loss_scale)
        if next(self.model.model.parameters()).dtype != torch.float16 or not (0.0 < abs(loss_value) < float("inf")):
            return 1.0
        return float(2.0 ** min(max(math.floor(math.log2(65536.0 / abs(loss_value))), 0), 60))

    def _fidelity_loss(self, image, curr_text, bboxs_curr, object_names):
        if self.clip_loss_model is None:
            raise RuntimeError("opt_epochs > 0 needs a loss_model (see DCLIPLoss); use opt_epochs=0 for fixed weights")
        lm = self.clip_loss_model
        loss = lm.forward_2(image, curr_text)                                                       # :252
        hgt, wid = image.shape[-2], image.shape[-1]
        for centre, name in zip(bboxs_curr, object_names):
            y1, y2, x1, x2 = object_crop_box(centre, hgt, wid)
            obj = name.lower().replace("the ", "")                                                  # :266-267
            loss = loss + self.local_loss_weight * lm.forward_3(image[:, y1:y2, x1:x2], "A photo of " + obj)   # :268-273
        return loss.sum()

    def _paste(self):
        """(orig [b, 3, H, W] in [0, 1], keep_px [b, 1, H, W]) of an inpainting call with a pixel-space pair, else None."""
        return None

    def _to_u8(self, image, index=0):
        return (255.0 * image.detach().float().cpu().numpy().transpose(1, 2, 0)).astype(np.uint8)

    def _save(self, image, epoch, seed, prompt_idx, index=0):
        from PIL import Image
        arr = self._to_u8(image, index)
        os.makedirs(self.outdir, exist_ok=True)
        Image.fromarray(arr).save(os.path.join(self.outdir, "final%d_s%d_index_%d.png" % (epoch, seed, prompt_idx)))

    # --------------------------------------------------------------------------------------------------
    def _time_range(self):
        return np.flip(self.ddim_timesteps)

    def _first_call(self):
        return 0

    def _trajectory(self, img, cond, uncond, scale, time_range, W, bboxs_curr, text_index, graph=False, call_recompute=False):
        """W: [K, S] for one image or [I, K, S] for a batch; column i of every image is used at step i."""
        S, b, device = len(time_range), img.shape[0], img.device
        self._call_key = (tuple(img.shape[1:]), int(W.shape[-2]))     # what one call's saved activations depend on, per image
        keep = self._calls_to_keep(S + 1, b) if call_recompute and torch.is_grad_enabled() else 0
        if call_recompute and torch.is_grad_enabled():
            self.last_kept_calls = keep
        if self._canvas is not None:
            eps_fn = self._canvas_eps_fn(cond, uncond, scale, bboxs_curr, text_index, graph, img)
        else:
            eps_fn = self._make_eps_fn(cond, uncond, scale, bboxs_curr, text_index, graph, img, call_recompute, keep_last=keep, n_calls=S + 1)
        guide = self._guide(eps_fn) if self._canvas is None else self._canvas_guide(eps_fn)
        old_eps = []
        for i, step in enumerate(time_range):
            index = S - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            ts_next = torch.full((b,), int(time_range[min(i + 1, S - 1)]), device=device, dtype=torch.long)
            if guide is not None and i < guide.steps:          # before the step's first evaluation; old_eps stays as it is
                img, _ = guide.update(img, None, ts, W[..., i], i, float(self.ddim_alphas[index]))
            img, _, e_t = self._plms_update(eps_fn, img, ts, ts_next, index, old_eps, W[..., i])
            old_eps.append(e_t)
            if len(old_eps) >= 4:
                old_eps.pop(0)
        return img

    def _calls_to_keep(self, n_calls, batch):
        """Per-call recomputation re-runs every call's forward in backward; the LAST calls of a trajectory are differentiated
        first and freed first, so as many of them as HBM holds simply keep their activations (no re-run). The size of one call's
        saved activations is measured on the first kept call (none is assumed before that: the first tracked epoch of a
        sampler keeps one call); four calls' worth + 24 GiB stay free for the calls that are recomputed and the VAE backward."""
        if not torch.cuda.is_available() or self.keep_calls == 0:
            return 0
        if self.keep_calls is not None:
            return min(int(self.keep_calls), n_calls)
        per_image = getattr(self, "_call_bytes_per_image", None)
        if per_image is None or getattr(self, "_call_bytes_key", None) != self._call_key:
            return 1                          # nothing measured for this (latent shape, object count) yet: keep one call and measure it
        est = per_image * batch
        free, _ = torch.cuda.mem_get_info()
        free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
        return int(max(0, min(n_calls, (free - 4 * est - (24 << 30)) // max(est, 1))))

    def _make_eps_fn(self, cond, uncond, scale, bboxs_curr, text_index, graph, img, call_recompute=False, keep_last=0, n_calls=0,
                     raw=False):
        """eps(x, t, coef) with classifier-free guidance. The UNet batch is [uncond_0, cond_0, uncond_1, cond_1, ...]:
        for one image this is the reference's `cat([uc, c])` (:304-308); for a batch the pairs stay adjacent,
        which is the layout the fused kernel indexes (image-major, row 0 = uncond, row 1 = cond).
        raw=True (the step-kernel samplers, SolverSamplerBase): returns the UNet's [2b] output itself, and x may already be
        that batch's input pair [2b] (sta_sampler_step writes it in the UNet's dtype)."""
        if uncond is None or scale == 1.0:
            raise ValueError("the spatial-temporal path needs classifier-free guidance (scale != 1, uc given): "
                             "the blend subtracts the unconditional row (attention.py:290)")
        wdtype = next(self.model.model.parameters()).dtype
        b = img.shape[0]
        pair = lambda u, c: torch.stack([u, c], dim=1).reshape(2 * b, *u.shape[1:])
        c_in = pair(uncond.expand(b, -1, -1), cond).to(wdtype)      # built once per trajectory (the reference: per call)
        apply_fn = self.model.apply_model_extra
        if graph and img.is_cuda:
            from sta.graphs import GraphedEps
            if self._graphs is None:
                self._graphs = GraphedEps(self.model)
            apply_fn = self._graphs.bind(c_in, bboxs_curr, text_index)

        def unet(fn, x, t, coef):
            return fn(x if x.shape[0] == 2 * b else pair(x, x), text_index, pair(t, t), c_in, coef=coef, bboxs_curr=bboxs_curr)

        calls = [0]

        def eps(x, t, coef):
            k = calls[0]
            calls[0] += 1
            if self._attn_inject is not None and torch.is_grad_enabled():
                self._attn_inject.loss.next_call()          # a new UNet call starts: close the one the attention loss was recording
            if call_recompute and torch.is_grad_enabled() and k >= n_calls - keep_last:
                # one of the last calls: plain autograd, its activations stay until backward reaches it (_calls_to_keep)
                before = torch.cuda.memory_allocated() if x.is_cuda else 0
                out = unet(self.model.apply_model_extra, x, t, coef)
                if x.is_cuda and k == n_calls - 1:
                    self._call_bytes_per_image = max(torch.cuda.memory_allocated() - before, 1) // b
                    self._call_bytes_key = self._call_key
            elif call_recompute and torch.is_grad_enabled():
                out = _CallRecompute.apply(lambda x_, t_, c_: unet(apply_fn, x_, t_, c_),
                                           lambda x_, t_, c_: unet(self.model.apply_model_extra, x_, t_, c_), t, x, coef,
                                           *(() if self._attn_inject is None else (self._attn_inject,)))
            else:
                out = unet(apply_fn, x, t, coef)
            if raw:
                return out
            out = out.reshape(b, 2, *out.shape[1:])
            e_u, e_c = out[:, 0], out[:, 1]
            return e_u + scale * (e_c - e_u)
        eps.eager_call = lambda x_, t_, c_: unet(self.model.apply_model_extra, x_, t_, c_)      # sta.guidance: never the graph
        return eps

    def _guide(self, eps_fn):
        """The latent guidance of this trajectory, bound to its eager UNet call, or None: trajectories under autograd (tracked epochs)
        are never guided, nor are prompts without objects."""
        lg = self.latent_guidance
        if lg is None or torch.is_grad_enabled() or not lg.ready:
            return None
        return lg.bind(eps_fn.eager_call)

    def _canvas_guide(self, unet):
        """`_guide` for a canvas trajectory: its CanvasGuidance bound to the eager call on the window rows (`unet.eager_call`, read only
        when there is something to guide), or None."""
        cg = self.canvas_guidance
        if cg is None or torch.is_grad_enabled() or not cg.ready:
            return None
        return cg.bind(unet.eager_call)

    def _x_prev(self, x, e_t, index):
        """DDIM step with sigma = 0 (:321-338); the tables live on the host as Python floats."""
        f32 = np.float32                     # the reference evaluates these scalars in float32 on the device
        a_t, a_prev = f32(self.ddim_alphas[index]), f32(self.ddim_alphas_prev[index])
        s1m = f32(self.ddim_sqrt_one_minus_alphas[index])
        pred_x0 = (x - float(s1m) * e_t) / float(np.sqrt(a_t))
        return float(np.sqrt(a_prev)) * pred_x0 + float(np.sqrt(f32(1.0) - a_prev)) * e_t, pred_x0

    def _plms_update(self, eps_fn, x, t, t_next, index, old_eps, coef):
        e_t = eps_fn(x, t, coef)
        n = len(old_eps)
        if n == 0:      # pseudo improved Euler: second evaluation at t_next with the same coef (:341-345)
            x_mid, _ = self._x_prev(x, e_t, index)
            e_prime = (e_t + eps_fn(x_mid, t_next, coef)) / 2
        elif n == 1:    # Adams-Bashforth 2 (:348)
            e_prime = (3 * e_t - old_eps[-1]) / 2
        elif n == 2:    # Adams-Bashforth 3 (:351)
            e_prime = (23 * e_t - 16 * old_eps[-1] + 5 * old_eps[-2]) / 12
        else:           # Adams-Bashforth 4 (:354)
            e_prime = (55 * e_t - 59 * old_eps[-1] + 37 * old_eps[-2] - 9 * old_eps[-3]) / 24
        x_prev, pred_x0 = self._x_prev(x, e_prime, index)
        return x_prev, pred_x0, e_t

    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1.0, unconditional_conditioning=None, old_eps=None, t_next=None,
                      text_index=None, coef=None, bboxs_curr=None):
        """Reference-compatible single step (:296-358) for callers that drive the loop themselves."""
        if use_original_steps or quantize_denoised or score_corrector is not None or noise_dropout:
            raise NotImplementedError("option not on the spatial-temporal path")
        eps_fn = self._make_eps_fn(c, unconditional_conditioning, unconditional_guidance_scale,
                                   [] if bboxs_curr is None else bboxs_curr, text_index, False, x)
        return self._plms_update(eps_fn, x, t, t_next, index, [] if old_eps is None else old_eps, coef)


class SolverSamplerBase(PLMSSampler):
    """The epoch loop, weights and keyword surface of PLMSSampler around a trajectory of exactly S UNet calls whose per-call
    arithmetic is one sta_sampler_step launch (sta.solver): DPMSolverSampler (dpm_solver/sampler.py) and DDIMSampler (ddim.py).
    Call i uses column i of W[K, S]. With fixed weights on the GPU the kernel also writes the next call's 16-bit input pair, so
    nothing but the (graph-replayed) UNet call and that one launch runs per step; tracked epochs differentiate through
    sta.solver.SolverStepFn (backward = sta_sampler_step_bwd), per-call recomputation included.
    Inpainting (`mask=` / `x0=`): sta_latent_blend re-noises the kept region before the first call, and the step of calls
    start .. S - 2 is sta_sampler_step_masked, which blends for the NEXT call in the same launch (tracked: SolverStepMaskedFn); the
    last call takes the plain step. Draw order: blend draw of call i, eta draw of call i, blend draw of call i + 1, ...
    On a canvas (`inpaint_canvas`) the same with sta_window_blend and sta_sampler_step_windows_masked on canvas-shaped tensors.
    A trajectory may start at call `_start` > 0 (DDIMSampler.decode: img2img): calls _start .. S - 1 run, with columns _start .. S - 1,
    and `_xin0` (if set) is the first call's 16-bit input pair, written by the fused encode step."""
    t_dtype = torch.float32
    tables = None
    _start = 0
    _xin0 = None
    _inpaint = None          # dict(x0, keep, image, keep_px) while a masked call runs (set like _start / _xin0, cleared in `finally`)
    mask_noise = None        # the blend noise n_i: None (torch.randn on the device), a list indexed by call, or callable (i, shape, device)

    def __init__(self, model, schedule="linear", mask_noise=None, **kwargs):
        super().__init__(model, schedule=schedule, **kwargs)
        self.mask_noise = mask_noise

    def _first_call(self):
        return self._start

    def _n_calls(self, S):
        return S - self._start

    # ------------------------------------------------------------------------------------------------ inpainting
    def _set_inpaint(self, mask, x0, image=None, mask_px=None, batch=None):
        """Checks and keeps the inpaint state of one call. mask: keep [b, 1, h, w] in [0, 1], 1 = keep the original (the reference's
        convention, ddim.py:147); x0 [b, 4, h, w]: the clean latent; image / mask_px: the original [b, 3, H, W] in [0, 1] and its keep
        mask [b, 1, H, W] for the pixel-space paste. Per-image lists are concatenated."""
        cat = lambda v: torch.cat([t for t in v]) if isinstance(v, (list, tuple)) else v
        mask, x0, image, mask_px = cat(mask), cat(x0), cat(image), cat(mask_px)
        if mask is None and x0 is None and image is None and mask_px is None:
            return False
        if mask is None or x0 is None:
            raise ValueError("inpainting needs both mask= and x0= (reference ddim.py:145: assert x0 is not None)")
        if (image is None) != (mask_px is None):
            raise ValueError("the pixel-space paste needs both image= and mask_px=")
        dev = self.model.device
        mask, x0 = mask.detach().to(dev, torch.float32), x0.detach().to(dev, torch.float32)
        if mask.dim() != 4 or mask.shape[1] != 1 or x0.dim() != 4 or mask.shape[0] != x0.shape[0] or mask.shape[-2:] != x0.shape[-2:]:
            raise ValueError("mask %s must be [b, 1, h, w] for x0 %s" % (tuple(mask.shape), tuple(x0.shape)))
        if batch is not None and x0.shape[0] != batch:
            raise ValueError("x0 holds %d latents for a batch of %d" % (x0.shape[0], batch))
        if float(mask.min()) < 0.0 or float(mask.max()) > 1.0:
            raise ValueError("mask values must lie in [0, 1]")
        if image is not None:
            image, mask_px = image.detach().to(dev, torch.float32), mask_px.detach().to(dev, torch.float32)
            if image.dim() != 4 or image.shape[0] != x0.shape[0] or tuple(mask_px.shape) != (image.shape[0], 1) + tuple(image.shape[-2:]):
                raise ValueError("image %s / mask_px %s must be [b, 3, H, W] / [b, 1, H, W]" % (tuple(image.shape), tuple(mask_px.shape)))
        self._inpaint = dict(x0=x0, keep=mask, image=image, keep_px=mask_px)
        return True

    def _paste(self):
        inp = self._inpaint
        return None if inp is None or inp["image"] is None else (inp["image"], inp["keep_px"])

    def _to_u8(self, image, index=0):
        """The saved pixels: where keep_px == 1 exactly the original's 8-bit values (a 16-bit composite does not round-trip them)."""
        arr = super()._to_u8(image, index)
        if self._paste() is not None:
            orig, keep_px = self._paste()
            kept = (keep_px[index, 0] == 1.0).cpu().numpy()
            o8 = np.rint(255.0 * orig[index].float().cpu().numpy().transpose(1, 2, 0)).astype(np.uint8)
            arr[kept] = o8[kept]
        return arr

    def _blend_coefs(self, i):
        """(q_a, q_b) of q_sample at call i: the state the call's UNet input carries is q_a x0 + q_b n."""
        raise NotImplementedError

    def _mask_noise(self, j, x):
        if self.mask_noise is None:
            return torch.randn(x.shape, device=x.device)
        if callable(self.mask_noise):
            return self.mask_noise(j, tuple(x.shape), x.device)
        return self.mask_noise[j].to(x.device)

    def _blend(self, i, x):
        from sta import solver
        inp = self._inpaint
        q_a, q_b = self._blend_coefs(i)
        return solver.Blend(inp["x0"], inp["keep"], self._mask_noise(i - self._start, x), q_a, q_b)

    def sample(self, S, batch_size, shape, conditioning=None, mask=None, x0=None, image=None, mask_px=None, **kwargs):
        """PLMSSampler.sample's keywords; with mask= / x0= the kept region (mask == 1) is re-noised from x0 before every UNet call
        (reference ddim.py:144-147), with image= / mask_px= the original is pasted over the decoded image (sta_image_composite)."""
        try:
            self._set_inpaint(mask, x0, image, mask_px, batch=batch_size)
            return super().sample(S, batch_size, shape, conditioning=conditioning, **kwargs)
        finally:
            self._inpaint = None

    def sample_batch(self, S, shape, conditionings, *args, mask=None, x0=None, image=None, mask_px=None, **kwargs):
        """PLMSSampler.sample_batch with per-image masks and latents (lists of [1, ...] tensors, or stacked)."""
        try:
            self._set_inpaint(mask, x0, image, mask_px, batch=len(conditionings))
            return super().sample_batch(S, shape, conditionings, *args, **kwargs)
        finally:
            self._inpaint = None

    def inpaint_canvas(self, S, canvas, window, stride=None, *, mask=None, x0=None, image=None, mask_px=None, conditionings=None,
                       unconditional_conditionings=None, bboxs=None, object_names=None, local_conditionings=None, x_T=None,
                       unconditional_guidance_scale=7.5, eta=0.0, seed=1, prompt_indices=None, curr_texts=None, channels=4, verbose=False,
                       wrap="", disc_scale=1.0):
        """`sample_canvas` with the kept region (mask == 1) of every canvas re-noised from x0 before every UNet call: outpainting (x0 holds
        an existing picture's latent on its footprint, mask is 1 there) and the repaint of a region of a canvas sampled earlier.
        mask [P, 1, Hc, Wc] in [0, 1], 1 = keep; x0 [P, channels, Hc, Wc]; image [P, 3, 8 Hc, 8 Wc] in [0, 1] / mask_px [P, 1, 8 Hc, 8 Wc]:
        the original and its keep mask for the pixel-space paste over the ONE decode of the whole canvas (sta_image_composite); the other
        keywords are sample_canvas's (disc_scale= and wrap= included: the launches take the grid's wrap mask, and the pixel-space paste on the cropped decode). On the GPU
        one sta_window_blend launch runs before call 0, one sta_sampler_step_windows_masked launch after calls 0 .. S - 2 and the plain
        sta_sampler_step_windows after the last call. The blend draws are canvas-shaped, in the order of `sample(mask=)`: blend draw of call i, eta draw of call i, blend draw of call i + 1, ...
        ValueError before any UNet call: what sample_canvas refuses, a missing mask or x0, shapes that are not the canvas's, mask values
        outside [0, 1], image without mask_px or the reverse."""
        if mask is None or x0 is None:
            raise ValueError("inpaint_canvas needs both mask= and x0=")
        if (image is None) != (mask_px is None):
            raise ValueError("inpaint_canvas: the pixel-space paste needs both image= and mask_px=")

        def prepare(P, channels, grid):
            self._set_inpaint(mask, x0, image, mask_px, batch=P)
            inp = self._inpaint
            want = dict(x0=(P, channels, grid.Hc, grid.Wc), keep=(P, 1, grid.Hc, grid.Wc), image=(P, 3, 8 * grid.Hc, 8 * grid.Wc),
                        keep_px=(P, 1, 8 * grid.Hc, 8 * grid.Wc))
            for name, shape in want.items():
                if inp[name] is not None and tuple(inp[name].shape) != shape:
                    raise ValueError("inpaint_canvas: %s %s must be [%d, %d, %d, %d] on this canvas"
                                     % (dict(keep="mask", keep_px="mask_px").get(name, name), tuple(inp[name].shape), *shape))
        try:
            return self._sample_canvas("inpaint_canvas", S, canvas, window, stride, conditionings, unconditional_conditionings, bboxs,
                                       object_names, local_conditionings, x_T, unconditional_guidance_scale, eta, seed, prompt_indices,
                                       curr_texts, channels, verbose, prepare=prepare, wrap=wrap, disc_scale=disc_scale)
        finally:
            self._inpaint = None

    def _time_range(self):
        return self.tables["t_in"]

    def _coef(self, i, scale):
        raise NotImplementedError

    def _noise(self, i, x):
        return None

    def _trajectory(self, img, cond, uncond, scale, time_range, W, bboxs_curr, text_index, graph=False, call_recompute=False):
        from sta import solver
        if self._canvas is not None:
            return self._canvas_trajectory(img, cond, uncond, scale, time_range, W, bboxs_curr, text_index, graph)
        S, b, device = len(time_range), img.shape[0], img.device
        self._call_key = (tuple(img.shape[1:]), int(W.shape[-2]))
        grad = torch.is_grad_enabled()
        start = self._start
        keep = self._calls_to_keep(S - start, b) if call_recompute and grad else 0
        if call_recompute and grad:
            self.last_kept_calls = keep
        eps_fn = self._make_eps_fn(cond, uncond, scale, bboxs_curr, text_index, graph, img, call_recompute, keep_last=keep,
                                   n_calls=S - start, raw=True)
        wdtype = next(self.model.model.parameters()).dtype
        fast = img.is_cuda and not grad
        masked = self._inpaint is not None
        x, m_prev = img, None
        xin = None
        if masked:           # the blend of the first call (also when decoding from an encoded latent, as the reference does)
            x, xin = solver.latent_blend(x, self._blend(start, x), dtype=wdtype, want_xin=fast)
        elif fast:
            xin = self._xin0 if self._xin0 is not None else solver._pair(img).to(wdtype)
        guide = self._guide(eps_fn)
        for i in range(start, S):
            t_val = float(time_range[i]) if self.t_dtype.is_floating_point else int(time_range[i])
            t = torch.full((b,), t_val, device=device, dtype=self.t_dtype)
            if guide is not None and i - start < guide.steps:
                # after the blend of a masked trajectory (the kept region is not guided); alpha_cumprod of the call's time is alpha_t^2 in
                # both tables; m_prev stays as it is
                x, xin = guide.update(x, xin, t, W[..., i], i - start, float(self.tables["alpha_t"][i]) ** 2,
                                      self._inpaint["keep"] if masked else None)
            out = eps_fn(x if xin is None else xin, t, W[..., i])
            c = self._coef(i, scale)
            noise = self._noise(i - start, x) if c.c_n else None           # the eta draw of call i, then the blend draw of call i + 1
            if masked and i + 1 < S:
                x, m_prev, xin = solver.solver_step_masked(out, x, m_prev, noise, c, self._blend(i + 1, x), dtype=wdtype, want_xin=fast)
            else:            # no blend after the last step (the reference has none either)
                x, m_prev, xin = solver.solver_step(out, x, m_prev, noise, c, dtype=wdtype, want_xin=fast and i + 1 < S)
        return x

    def _canvas_trajectory(self, img, cond, uncond, scale, time_range, W, bboxs_curr, text_index, graph):
        """The calls `_start` .. S - 1 of a canvas (fixed weights, no autograd; sample_canvas / inpaint_canvas: from call 0; DDIMSampler.
        decode_canvas: img2img, from call S - t_start with weight column i, eta draw i - _start and blend draw i - _start, the draw order
        of `_trajectory`; m_prev starts as None). The first call's window inputs are `_xin0` (the fused encode step's) or come from
        window_split; after every UNet call ONE sta_sampler_step_windows launch reads the windows' output, forms the overlap means,
        steps the canvas state and writes the next call's window inputs: x and m_prev stay canvas-shaped, and nothing but the
        (graph-replayed) UNet call and that launch runs per step. `canvas_fused_step = False` takes window_fuse + solver_step +
        window_split instead (three launches; the means are then rounded to the UNet's type before the step).
        Inpainting (inpaint_canvas: `_inpaint` set): sta_window_blend re-noises the kept region and writes the first window inputs, and
        the launch after calls 0 .. S - 2 is sta_sampler_step_windows_masked, which blends for the NEXT call; the last call takes the
        plain step. Unfused: latent_blend + window_split, then window_fuse + solver_step_masked + window_split.
        `canvas_guidance`: the first `steps` calls (counted from `_start`) are each preceded by its updates of x and xin, one
        sta_latent_guide_windows launch per update (sta.guidance.CanvasGuidance)."""
        from sta import canvas as _cv
        from sta import solver
        grid, unet = self._window_unet(cond, uncond, scale, bboxs_curr, text_index, graph, img)
        wdtype = next(self.model.model.parameters()).dtype
        S, P, device = len(time_range), img.shape[0], img.device
        fused, masked = self.canvas_fused_step, self._inpaint is not None
        start = self._start        # > 0: DDIMSampler.decode_canvas (img2img): calls start .. S - 1 with weight column i, draws i - start
        x, m_prev = img, None
        if masked and fused:       # the blend of the first call replaces a given `_xin0`, as in `_trajectory`
            x, xin = _cv.window_blend(x, self._blend(start, x), grid, dtype=wdtype, want_xin=True)
        elif masked:
            x, _ = solver.latent_blend(x, self._blend(start, x), dtype=wdtype)
            xin = _cv.window_split(x, grid, wdtype)
        else:
            xin = self._xin0 if self._xin0 is not None else _cv.window_split(x, grid, wdtype)
        guide = self._canvas_guide(unet)
        for i in range(start, S):
            t_val = float(time_range[i]) if self.t_dtype.is_floating_point else int(time_range[i])
            t = torch.full((P,), t_val, device=device, dtype=self.t_dtype)
            if guide is not None and i - start < guide.steps:
                # after the blend of a masked trajectory (the kept region is not guided), counted from `_start`; m_prev stays as it is
                x, xin = guide.update(x, xin, t, W[..., i], i - start, float(self.tables["alpha_t"][i]) ** 2,
                                      self._inpaint["keep"] if masked else None)
            out = unet(xin, t, W[..., i])
            c = self._coef(i, scale)
            noise = self._noise(i - start, x) if c.c_n else None   # the eta draw of call i, then the blend draw of call i + 1
            bl = self._blend(i + 1, x) if masked and i + 1 < S else None       # no blend after the last step
            if fused and bl is not None:
                x, m_prev, xin = _cv.sampler_step_windows_masked(out, x, m_prev, noise, c, bl, grid, dtype=wdtype, want_xin=True)
            elif fused:
                x, m_prev, xin = _cv.sampler_step_windows(out, x, m_prev, noise, c, grid, dtype=wdtype, want_xin=i + 1 < S)
            else:
                mean = _cv.window_fuse(out, grid)
                if bl is not None:
                    x, m_prev, _ = solver.solver_step_masked(mean, x, m_prev, noise, c, bl, dtype=wdtype)
                else:
                    x, m_prev, _ = solver.solver_step(mean, x, m_prev, noise, c, dtype=wdtype)
                xin = _cv.window_split(x, grid, wdtype) if i + 1 < S else None
        return x
