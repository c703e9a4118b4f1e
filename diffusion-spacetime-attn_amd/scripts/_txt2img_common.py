"""Shared body of scripts/txt2img-{gpt,mscoco,vsr}.py — the reference's three entry points differ only
in the dataset they read (scripts/txt2img-gpt.py vs -mscoco.py vs -vsr.py: lines 255-261).

Kept from the reference CLI (txt2img-gpt.py:105-247): --plms / --dpm_solver / neither (DDIM; sampler_choice) --ddim_steps --H --W --C --f --n_samples --scale
--ddim_eta --fixed_code --config --ckpt --precision --outdir --seed --process_id (+ the flags it parses and
ignores, accepted for compatibility). Added: --layout (JSON replacing the layout-predictor call),
--dataset (path override), --opt_epochs (0 = fixed weights), --limit/--start, --dtype, --synthetic,
--clip (the fidelity-loss model; checked BEFORE sampling), --clip_tokenizer (vocabulary of the text encoder),
--attn_guidance ETA / --attn_guidance_steps / --attn_guidance_iters (attention-guided latent updates, sta.guidance; shared with
img2img.py and inpaint.py through add_guidance_arguments / check_guidance_option / make_guidance / report_guidance),
--canvas HxW / --canvas_stride PX (a wide or tall canvas sampled as overlapping --H x --W windows, sta.canvas; the layout's centres are
then normalised to the canvas; fixed blend weights only; --canvas_guidance ETA: attention guidance on the canvas, sta.guidance.
CanvasGuidance), --canvas_wrap x|y|xy (the canvas closes on itself along those axes: a 360 degree
panorama or a tileable image), --hires HxW / --hires_strength F / --hires_stride PX (the hi-res fix: every first pass — a --H x --W image
or a --canvas, any of the three samplers — is followed by a second, DDIM pass on the same model that upscales the first pass's latent on
the GPU to H x W pixels (DDIMSampler.hires_canvas: one sta_latent_upscale_step_windows launch), noises it to t_start = int(F x
--ddim_steps) and refines it as overlapping --H x --W windows under the same layout, the discs scaled with the picture; fixed blend
weights in the second pass; both passes' images are saved, the second pass's in the subdirectory hires/ of the first pass's).
With torch.distributed.run the prompts are sharded round-robin over the ranks (one GPU each).
"""
import argparse
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import torch  # noqa: E402


def build_parser(default_dataset):
    p = argparse.ArgumentParser()
    p.add_argument("--prompt", type=str, nargs="?", default="a painting of a virus monster playing guitar",
                   help="parsed and ignored, as in the reference (prompts come from the dataset)")
    p.add_argument("--outdir", type=str, nargs="?", default="outputs/notuse")
    p.add_argument("--skip_grid", action="store_true")
    p.add_argument("--skip_save", action="store_true")
    p.add_argument("--ddim_steps", type=int, default=50)
    p.add_argument("--plms", action="store_true")
    p.add_argument("--dpm_solver", action="store_true")
    p.add_argument("--laion400m", action="store_true")
    p.add_argument("--fixed_code", action="store_true")
    p.add_argument("--ddim_eta", type=float, default=0.0)
    p.add_argument("--n_iter", type=int, default=2)
    p.add_argument("--H", type=int, default=512)
    p.add_argument("--W", type=int, default=512)
    p.add_argument("--C", type=int, default=4)
    p.add_argument("--f", type=int, default=8)
    p.add_argument("--n_samples", type=int, default=1)
    p.add_argument("--n_rows", type=int, default=0)
    p.add_argument("--scale", type=float, default=7.5)
    p.add_argument("--from-file", type=str)
    p.add_argument("--config", type=str, default="configs/stable-diffusion/v1-inference.yaml")
    p.add_argument("--ckpt", type=str, default="models/ldm/stable-diffusion-v1/model.ckpt")
    p.add_argument("--seed", type=int, default=42, help="parsed and ignored: the reference uses seed = 1 for every prompt")
    p.add_argument("--process_id", type=int, default=0)
    p.add_argument("--precision", type=str, choices=["full", "autocast"], default="autocast")
    # additions
    p.add_argument("--dataset", type=str, default=default_dataset)
    p.add_argument("--layout", type=str, default=None, help="JSON {prompt | index: {object: [x, y]}}")
    p.add_argument("--opt_epochs", type=int, default=3, help="weight-optimisation epochs (reference: 3; 0 = fixed weights)")
    p.add_argument("--start", type=int, default=0)
    p.add_argument("--limit", type=int, default=500)
    p.add_argument("--dtype", type=str, choices=["bf16", "fp16"], default="fp16",
                   help="fp16 = the reference's autocast type and the one within 1e-3 on the attention maps (DESIGN.md section 2)")
    p.add_argument("--clip", type=str, default=None,
                   help="fidelity-loss model for --opt_epochs > 0: 'module:callable' (called with the device, returns a model with "
                        "encode_image/encode_text or (model, tokenize)), a CLIP .pt path, 'synthetic' (frozen stand-in, for "
                        "timing the gradient path), or 'builtin:PATH' = this project's own CLIP ViT-B/32 (sta.clip) with the weights of "
                        "PATH (a state_dict file, the official TorchScript archive or a Hugging Face CLIPModel state_dict; needs "
                        "--clip_tokenizer; 'builtin:synthetic' = seeded weights). Default: clip.load('ViT-B/32') as the reference "
                        "(plms.py:24)")
    p.add_argument("--fp8", action="store_true",
                   help="store the Linear weights of the transformer blocks as OCP e4m3 with per-channel scales (BASELINE configs[4]): half "
                        "the weight memory; their GEMMs become hipBLASLt's row-scaled e4m3 GEMMs behind a per-row activation quantiser, "
                        "which measures SLOWER than 16 bit here (a memory option, not a rate option: DESIGN.md section 5); fixed blend "
                        "weights only (--opt_epochs 0)")
    p.add_argument("--mxfp8", action="store_true",
                   help="store the same Linear weights as OCP MXFP8 (e4m3 elements, one e8m0 scale per 32 inputs) and run their GEMMs on "
                        "this project's block-scaled fp8 MFMA kernel (csrc/sta_mxfp8.hip; sta.mxfp8); exclusive with --fp8; fixed blend "
                        "weights only (--opt_epochs 0)")
    p.add_argument("--clip_tokenizer", type=str, default=None, help="directory with the CLIP tokenizer files (with --ckpt)")
    p.add_argument("--synthetic", action="store_true", help="synthetic weights/text embeddings when no checkpoint is available")
    p.add_argument("--batch_prompts", type=int, default=1,
                   help="sample up to this many prompts with the same object count together (one CFG batch of 2I per UNet call)")
    p.add_argument("--attn_maps", action="store_true",
                   help="capture per-object cross-attention heat maps over the kept trajectory (sta.attnmaps; that trajectory runs without "
                        "graph replay): <outdir>/attn/<prompt index>.npz, one PNG overlay per object, and the in-disc mass per object")
    p.add_argument("--attn_res", type=int, choices=[8, 16, 32, 64], default=16,
                   help="side of the transformer level whose blocks are captured (16 = the C = 1280 level of a 512 x 512 image)")
    p.add_argument("--attn_loss", type=_positive_float, default=None, metavar="LAMBDA",
                   help="add LAMBDA x the attention-layout loss (sta.attnloss: (1 - in-disc share of each object's token maps)^2, recorded "
                        "at --attn_res inside the tracked UNet calls) to the loss of --opt_epochs > 1; without --clip it is the only loss "
                        "and the tracked epochs neither need CLIP weights nor decode")
    p.add_argument("--canvas", type=str, default=None, metavar="HxW",
                   help="sample a canvas of H x W pixels as overlapping --H x --W windows (which must be square) in one CFG batch per UNet "
                        "call, averaged where they overlap (sta.canvas); a multiple of 8 x --f and at least the window; the centres of "
                        "--layout are then normalised to the canvas; fixed blend weights only (--opt_epochs 0 or 1), no --attn_maps / "
                        "--attn_loss / --attn_guidance (layout guidance on a canvas: --canvas_guidance)")
    p.add_argument("--canvas_stride", type=int, default=None, metavar="PX",
                   help="distance between neighbouring windows of --canvas in pixels: a multiple of 8 x --f, at most the window "
                        "(default: half the window)")
    p.add_argument("--canvas_wrap", type=str, default=None, choices=("x", "y", "xy"),
                   help="the --canvas closes on itself along these axes (x: a 360 degree panorama whose right edge continues into the left "
                        "one; xy: a tileable image): the windows run over the seam. A wrapped axis must be a multiple of the stride and at "
                        "least 1.5 windows long")
    p.add_argument("--hires", type=str, default=None, metavar="HxW",
                   help="the hi-res fix: after the first pass (--H x --W, or --canvas) upscale its latent on the GPU to H x W pixels "
                        "(multiples of 64, at least the first pass's size, the same ratio on both axes) and refine it with DDIM "
                        "(--ddim_steps, --ddim_eta) as overlapping --H x --W windows under the same layout, every disc scaled by the "
                        "upscale factor; needs --hires_strength; --canvas_wrap and --canvas_guidance carry over to the second pass; the "
                        "second pass runs with fixed blend weights (handing it weights optimised in the first pass is out of scope); no "
                        "--attn_maps / --attn_loss; the second pass's images go to the subdirectory hires/ of the first pass's")
    p.add_argument("--hires_strength", type=float, default=None, metavar="F",
                   help="in (0, 1], required with --hires (no default): the second pass runs the last int(F x --ddim_steps) DDIM calls")
    p.add_argument("--hires_stride", type=int, default=None, metavar="PX",
                   help="distance between neighbouring windows of the second pass in pixels (default: half the window)")
    add_guidance_arguments(p)
    return p


def add_guidance_arguments(p, attn_res=False):
    """The flags of attention-guided sampling; attn_res=True adds --attn_res for a parser that does not have it yet."""
    p.add_argument("--attn_guidance", type=_positive_float, default=None, metavar="ETA",
                   help="step the latent down the gradient of the attention-layout energy (sta.guidance) before each of the first "
                        "--attn_guidance_steps UNet calls of the kept trajectory: x <- x - ETA (1 - alphas_cumprod_t) g / rms(g), read at "
                        "--attn_res on the encoder side of the UNet; needs no epochs and no CLIP; prompts without objects are not guided")
    p.add_argument("--canvas_guidance", type=_positive_float, default=None, metavar="ETA",
                   help="--attn_guidance on a --canvas (sta.guidance.CanvasGuidance): the energy is read per window, its gradient goes back "
                        "to the canvas latent through the windows' split (one sta_latent_guide_windows launch per update) and the part of "
                        "the canvas that receives gradient moves by ETA (1 - alphas_cumprod_t) in rms; reuses --attn_guidance_steps / "
                        "--attn_guidance_iters / --attn_res (a level of the WINDOW); needs --canvas")
    p.add_argument("--attn_guidance_steps", type=_non_negative_int, default=10, metavar="N", help="guided UNet calls per trajectory")
    p.add_argument("--attn_guidance_iters", type=_positive_int, default=1, metavar="N", help="updates before each guided call")
    if attn_res:
        p.add_argument("--attn_res", type=int, choices=[8, 16, 32, 64], default=16,
                       help="side of the transformer level whose blocks feed the guidance (16 = the C = 1280 level of a 512 x 512 image)")


def _positive_int(text):
    value = int(text)
    if value < 1:
        raise argparse.ArgumentTypeError("must be >= 1, got %s" % text)
    return value


def _non_negative_int(text):
    value = int(text)
    if value < 0:
        raise argparse.ArgumentTypeError("must be >= 0, got %s" % text)
    return value


def _positive_float(text):
    value = float(text)
    if not value > 0:
        raise argparse.ArgumentTypeError("must be > 0, got %s" % text)
    return value


def attn_levels(opt):
    """Sides of the UNet's four transformer levels for the latent of --H / --W."""
    return [opt.H // opt.f // s for s in (1, 2, 4, 8)]


def check_attn_option(opt):
    """--attn_maps / --attn_loss: refusals that need no GPU."""
    if opt.attn_loss is not None and opt.opt_epochs <= 1:
        raise SystemExit("--attn_loss needs --opt_epochs > 1: with %d no epoch is tracked and nothing would be optimised" % opt.opt_epochs)
    if opt.opt_epochs > 1 and opt.clip is None and opt.attn_loss is None and importlib.util.find_spec("clip") is None:
        raise SystemExit("--opt_epochs %d needs a loss: --clip (the fidelity loss needs a CLIP model; the OpenAI `clip` package of the "
                         "default is not installed) and / or --attn_loss LAMBDA (the attention-layout loss, which needs no other model), "
                         "or --opt_epochs 0 for fixed blend weights" % opt.opt_epochs)
    if not opt.attn_maps and opt.attn_loss is None and opt.attn_guidance is None:
        return
    if opt.H != opt.W or opt.H % (8 * opt.f):
        raise SystemExit("--attn_maps / --attn_loss / --attn_guidance need a square image whose latent side is a multiple of 8 (got %d x %d, --f %d)" % (opt.H, opt.W, opt.f))
    if opt.attn_res not in attn_levels(opt):
        raise SystemExit("--attn_res %d: no transformer level of a %d x %d image has that side (levels: %s)"
                         % (opt.attn_res, opt.H, opt.W, ", ".join(str(v) for v in attn_levels(opt))))


def check_guidance_option(opt, side=None):
    """--attn_guidance of the entry points that read their image size from a file (img2img.py, inpaint.py): the same refusals as
    check_attn_option, against the square image of `side` pixels once it is known."""
    if opt.attn_guidance is None or side is None:
        return
    levels = [side // opt.f // s for s in (1, 2, 4, 8)]
    if side % (8 * opt.f):
        raise SystemExit("--attn_guidance needs a square image whose latent side is a multiple of 8 (got %d, --f %d)" % (side, opt.f))
    if opt.attn_res not in levels:
        raise SystemExit("--attn_res %d: no transformer level of a %d x %d image has that side (levels: %s)"
                         % (opt.attn_res, side, side, ", ".join(str(v) for v in levels)))


def make_guidance(opt, model):
    """The sta.guidance.AttnGuidance of --attn_guidance, or None."""
    if opt.attn_guidance is None:
        return None
    from sta import attnmaps, guidance
    tok = getattr(model.cond_stage_model, "tokenizer", None)
    return guidance.AttnGuidance(model.model.diffusion_model, resolution=opt.attn_res, scale=opt.attn_guidance, steps=opt.attn_guidance_steps,
                                 iters=opt.attn_guidance_iters, tokenize=None if tok is None else attnmaps.content_tokenizer(tok))


def make_canvas_guidance(opt, model):
    """The sta.guidance.CanvasGuidance of --canvas_guidance, or None."""
    if getattr(opt, "canvas_guidance", None) is None:
        return None
    from sta import attnmaps, guidance
    tok = getattr(model.cond_stage_model, "tokenizer", None)
    return guidance.CanvasGuidance(model.model.diffusion_model, resolution=opt.attn_res, scale=opt.canvas_guidance,
                                   steps=opt.attn_guidance_steps, iters=opt.attn_guidance_iters,
                                   tokenize=None if tok is None else attnmaps.content_tokenizer(tok))


def report_guidance(sampler, indices, tag=""):
    """After sampling: per prompt the energy before the first and before the last update (with one update per call the last figure is
    the energy the last guided call started from), and the skipped updates."""
    res = getattr(sampler, "last_guidance", None)
    if getattr(sampler, "latent_guidance", None) is None and getattr(sampler, "canvas_guidance", None) is None:
        return
    if res is None:
        print("%sprompts %s: no objects (or no guided call), not guided" % (tag, list(indices)))
        return
    for j, i in enumerate(indices):
        print("%sprompt %d: attention-layout energy %.4f before the first update, %.4f before the last of %d (%d skipped in the batch)"
              % (tag, i, res["energy"][0, j].item(), res["energy"][-1, j].item(), len(res["calls"]), res["skipped"]))


def canvas_grid(opt):
    """The sta.canvas.Grid of --canvas / --canvas_stride in latent pixels, or None without --canvas; every refusal that needs no GPU."""
    wrap = getattr(opt, "canvas_wrap", None) or ""
    if opt.canvas is None:
        if opt.canvas_stride is not None:
            raise SystemExit("--canvas_stride %d needs --canvas HxW" % opt.canvas_stride)
        if wrap:
            raise SystemExit("--canvas_wrap %s needs --canvas HxW" % wrap)
        if getattr(opt, "canvas_guidance", None) is not None and getattr(opt, "hires", None) is None:      # --hires: its second pass is a canvas
            raise SystemExit("--canvas_guidance %s needs --canvas HxW (a square image is guided with --attn_guidance)" % opt.canvas_guidance)
        return None
    parts = opt.canvas.lower().split("x")
    if len(parts) != 2 or not all(v.isdigit() for v in parts):
        raise SystemExit("--canvas %s: expected HxW in pixels, e.g. 512x2048" % opt.canvas)
    Hpx, Wpx = int(parts[0]), int(parts[1])
    unit = 8 * opt.f
    if opt.H != opt.W:
        raise SystemExit("--canvas is sampled as square windows: --H %d and --W %d differ" % (opt.H, opt.W))
    stride = opt.H // 2 if opt.canvas_stride is None else opt.canvas_stride
    for name, v in (("--canvas height", Hpx), ("--canvas width", Wpx), ("--H / --W", opt.H), ("--canvas_stride", stride)):
        if v <= 0 or v % unit:
            raise SystemExit("%s %d is not a positive multiple of %d pixels (8 x --f %d)" % (name, v, unit, opt.f))
    if opt.opt_epochs > 1:
        raise SystemExit("--canvas samples with fixed blend weights: --opt_epochs %d tracks epochs, and the loss front end takes square "
                         "images (use --opt_epochs 0)" % opt.opt_epochs)
    for flag, on in (("--attn_maps", opt.attn_maps), ("--attn_loss", opt.attn_loss is not None), ("--attn_guidance", opt.attn_guidance is not None)):
        if on:
            raise SystemExit("%s reads one square image's attention maps and is not defined on a --canvas" % flag)
    if getattr(opt, "canvas_guidance", None) is not None:
        levels = [opt.H // opt.f // d for d in (1, 2, 4, 8)]
        if opt.attn_res not in levels:
            raise SystemExit("--attn_res %d: no transformer level of a %d x %d window has that side (levels: %s)"
                             % (opt.attn_res, opt.H, opt.H, ", ".join(str(v) for v in levels)))
    from sta import canvas
    try:
        return canvas.window_grid(Hpx // opt.f, Wpx // opt.f, opt.H // opt.f, stride // opt.f, wrap)
    except ValueError as e:
        raise SystemExit("--canvas %s (latent pixels): %s" % (opt.canvas, e))


def hires_plan(opt):
    """--hires / --hires_strength / --hires_stride -> (the second pass's sta.canvas.Grid in latent pixels, t_start, disc_scale), or None
    without --hires; every refusal that needs no GPU."""
    if opt.hires is None:
        for flag, v in (("--hires_strength", opt.hires_strength), ("--hires_stride", opt.hires_stride)):
            if v is not None:
                raise SystemExit("%s %s needs --hires HxW" % (flag, v))
        return None
    parts = opt.hires.lower().split("x")
    if len(parts) != 2 or not all(v.isdigit() for v in parts):
        raise SystemExit("--hires %s: expected HxW in pixels, e.g. 1024x1024" % opt.hires)
    Hpx, Wpx = int(parts[0]), int(parts[1])
    unit = max(64, 8 * opt.f)
    if opt.H != opt.W:
        raise SystemExit("--hires refines square windows: --H %d and --W %d differ" % (opt.H, opt.W))
    stride = opt.H // 2 if opt.hires_stride is None else opt.hires_stride
    for name, v, u in (("--hires height", Hpx, unit), ("--hires width", Wpx, unit), ("--H / --W", opt.H, 8 * opt.f),
                       ("--hires_stride", stride, 8 * opt.f)):
        if v <= 0 or v % u:
            raise SystemExit("%s %d is not a positive multiple of %d pixels" % (name, v, u))
    first = canvas_grid(opt)
    H1, W1 = (opt.H, opt.W) if first is None else (first.Hc * opt.f, first.Wc * opt.f)
    if Hpx < H1 or Wpx < W1:
        raise SystemExit("--hires %s is smaller than the first pass's %d x %d pixels (upscale only)" % (opt.hires, H1, W1))
    if Hpx * W1 != Wpx * H1:
        raise SystemExit("--hires %s is not a uniform upscale of the first pass's %d x %d pixels (a non-uniform ratio would turn the "
                         "layout's discs into ellipses)" % (opt.hires, H1, W1))
    if opt.hires_strength is None:
        raise SystemExit("--hires needs --hires_strength F in (0, 1] (there is no default)")
    if not 0.0 < opt.hires_strength <= 1.0:
        raise SystemExit("--hires_strength %s must be in (0, 1]" % opt.hires_strength)
    t_start = int(opt.hires_strength * opt.ddim_steps)
    if not 1 <= t_start <= opt.ddim_steps:
        raise SystemExit("t_start = int(hires_strength * ddim_steps) = %d must be in 1 .. %d" % (t_start, opt.ddim_steps))
    for flag, on in (("--attn_maps", opt.attn_maps), ("--attn_loss", opt.attn_loss is not None)):
        if on:
            raise SystemExit("%s reads one square image's attention maps and is not defined on the canvas of --hires" % flag)
    if getattr(opt, "canvas_guidance", None) is not None:
        levels = [opt.H // opt.f // d for d in (1, 2, 4, 8)]
        if opt.attn_res not in levels:
            raise SystemExit("--attn_res %d: no transformer level of a %d x %d window has that side (levels: %s)"
                             % (opt.attn_res, opt.H, opt.H, ", ".join(str(v) for v in levels)))
    from sta import canvas
    disc_scale = Hpx / H1
    try:
        grid = canvas.window_grid(Hpx // opt.f, Wpx // opt.f, opt.H // opt.f, stride // opt.f, getattr(opt, "canvas_wrap", None) or "")
        canvas.check_disc_scale(grid, disc_scale)
    except ValueError as e:
        raise SystemExit("--hires %s (latent pixels): %s" % (opt.hires, e))
    return grid, t_start, disc_scale


def builtin_clip(opt):
    """What follows `builtin:` in --clip when the fidelity loss will be evaluated (opt_epochs > 1), else None."""
    if opt.opt_epochs > 1 and opt.clip and opt.clip.startswith("builtin:"):
        return opt.clip[len("builtin:"):]
    return None


def check_clip_option(opt, side=None):
    """--clip builtin:...: refusals that need no GPU, no model and no tokenizer. `side` = (H, W) of the decoded image if known."""
    spec = builtin_clip(opt)
    if spec is None:
        return
    if spec != "synthetic" and not os.path.isfile(spec):
        raise SystemExit("--clip builtin:%s: no such weights file" % spec)
    if spec != "synthetic" and not opt.clip_tokenizer:
        raise SystemExit("--clip builtin:%s needs --clip_tokenizer (the directory with the CLIP vocabulary files)" % spec)
    if opt.clip_tokenizer and not os.path.isdir(opt.clip_tokenizer):
        raise SystemExit("--clip_tokenizer %s: no such directory" % opt.clip_tokenizer)
    if side is not None:
        from sta.clip import check_view_shapes
        try:
            check_view_shapes(*side)
        except ValueError as e:
            raise SystemExit("--clip %s: %s" % (opt.clip, e))


def loss_tokenizer(opt):
    """The tokeniser of the built-in loss model, made before any model is: the CLIPTokenizer of --clip_tokenizer, or the hashing
    stand-in for builtin:synthetic without one."""
    from sta import clip
    if opt.clip_tokenizer:
        return clip.tokenizer(opt.clip_tokenizer)
    return clip.hash_tokenize


def check_loss_texts(tokenize, items):
    """Every string the loss will tokenise — each prompt and each "A photo of <object>" — through `tokenize` now: clip.tokenize
    refuses more than 75 tokens, and it would do so after the first 51-call trajectory. items: (prompt, object names)."""
    from sta.clip import loss_strings
    for prompt, names in items:
        for text in loss_strings(prompt, names):
            try:
                tokenize([text])
            except RuntimeError as e:
                raise SystemExit("the fidelity loss cannot tokenise a text of this run: %s" % e)


def check_options(opt):
    """Refusals that need no GPU (raised before anything is built)."""
    if opt.mxfp8 and opt.fp8:
        raise SystemExit("--mxfp8 and --fp8 are exclusive")
    if opt.mxfp8 and opt.opt_epochs > 0:
        raise SystemExit("--mxfp8 is an inference option: use --opt_epochs 0")
    canvas_grid(opt)
    hires_plan(opt)
    check_clip_option(opt, (opt.H, opt.W))
    check_attn_option(opt)


def sampler_choice(opt):
    """(sampler class name, eta) as the reference picks them (txt2img-gpt.py:268-273): --dpm_solver -> DPM-Solver++ (order 2,
    multistep; --ddim_eta ignored), else --plms -> PLMS, else DDIM with --ddim_eta."""
    if opt.dpm_solver:
        return "DPMSolverSampler", 0.0
    if opt.plms:
        return "PLMSSampler", opt.ddim_eta
    return "DDIMSampler", opt.ddim_eta


def sampler_class(name):
    if name == "DPMSolverSampler":
        from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
        return DPMSolverSampler
    if name == "DDIMSampler":
        from ldm.models.diffusion.ddim import DDIMSampler
        return DDIMSampler
    from ldm.models.diffusion.plms import PLMSSampler
    return PLMSSampler


def run(kind, default_dataset):
    opt = build_parser(default_dataset).parse_args()
    check_options(opt)
    sampler_name, eta = sampler_choice(opt)
    if opt.n_samples != 1:
        raise SystemExit("--n_samples must be 1 (the blocks reshape to the CFG batch of 2, attention.py:282)")
    from sta import datasets, parallel
    from sta.pipeline import build_sd_v1, conditionings, use_shipped_miopen_db

    rank, world, local = parallel.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("a GPU is required (the fused cross-attention has no CPU path)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dtype = torch.bfloat16 if opt.dtype == "bf16" else torch.float16
    use_shipped_miopen_db(local)      # per-rank copy of the shipped MIOpen find-db; a different MIOpen build ignores it

    prompts = datasets.load_prompts(opt.dataset, kind, opt.limit)
    layouts = datasets.load_layouts(opt.layout) if opt.layout else None
    ckpt = opt.ckpt if (os.path.exists(opt.ckpt) and not opt.synthetic) else None
    if ckpt is None and not opt.synthetic:
        raise SystemExit("checkpoint %s not found (pass --synthetic to run with synthetic weights)" % opt.ckpt)
    loss_tokenize = None
    if builtin_clip(opt) is not None:
        loss_tokenize = loss_tokenizer(opt)
        check_loss_texts(loss_tokenize, [(p, list((datasets.layout_for(layouts, p, i) or {}).keys())) for i, p in enumerate(prompts)])
    loss_model = None
    if opt.opt_epochs > 1 and (opt.clip is not None or opt.attn_loss is None):
        # the sampler evaluates the loss only when an epoch is tracked (opt_epochs > 1); fail here, not after the first 51-call trajectory
        # (--attn_loss without --clip: the attention-layout loss alone, no CLIP model is looked for)
        from ldm.models.diffusion.plms import DCLIPLoss, load_clip_model
        if opt.clip == "synthetic":
            from sta.synth import SyntheticCLIP
            loss_model = DCLIPLoss(SyntheticCLIP().to(dev))
        else:
            try:
                clip_model, tokenize = load_clip_model(opt.clip, dev, dtype=dtype, tokenizer_path=opt.clip_tokenizer)
                loss_model = DCLIPLoss(clip_model, loss_tokenize or tokenize)
            except Exception as e:
                raise SystemExit("--opt_epochs %d: %s" % (opt.opt_epochs, e))
    model = build_sd_v1(dev, dtype, ckpt=ckpt if rank == 0 else None, init_weights=(rank == 0), use_checkpoint=opt.opt_epochs > 1,
                        clip_tokenizer=opt.clip_tokenizer, real_text_encoder=ckpt is not None)
    if opt.opt_epochs > 1 and torch.device(dev).type == "cuda" and opt.H * opt.W <= 512 * 512:
        from sta.pipeline import set_recompute
        set_recompute(model, "auto", max(opt.batch_prompts, 1))      # sized to 288 GB of HBM at 512x512; larger images keep the reference's policy
    parallel.broadcast_module_(model)                                   # one RCCL broadcast of the frozen weights
    if opt.fp8:
        if opt.opt_epochs > 0:
            raise SystemExit("--fp8 is an inference option: use --opt_epochs 0")
        from sta import fp8
        n, before, after = fp8.convert_transformer_linears_(model.model.diffusion_model)
        print("[rank %d] %d Linear layers -> e4m3: %.2f GB -> %.2f GB" % (rank, n, before / 1e9, after / 1e9))
    if opt.mxfp8:
        from sta import mxfp8
        n, before, after = mxfp8.convert_transformer_linears_mx_(model.model.diffusion_model)
        print("[rank %d] %d Linear layers -> MXFP8: %.2f GB -> %.2f GB" % (rank, n, before / 1e9, after / 1e9))
    capture = attn_loss = None
    if opt.attn_maps or opt.attn_loss is not None:
        from sta import attnmaps
        # name tokens are located with the text encoder's own tokenizer; the synthetic embedder has none (whitespace stand-in)
        tok = getattr(model.cond_stage_model, "tokenizer", None)
        tokenize = None if tok is None else attnmaps.content_tokenizer(tok)
    if opt.attn_maps:
        capture = attnmaps.AttnCapture(model.model.diffusion_model, resolution=opt.attn_res, tokenize=tokenize)
    if opt.attn_loss is not None:
        from sta import attnloss
        attn_loss = attnloss.AttnLayoutLoss(model.model.diffusion_model, resolution=opt.attn_res, tokenize=tokenize)
    sampler = sampler_class(sampler_name)(model, opt_epochs=opt.opt_epochs, loss_model=loss_model, attn_capture=capture,
                                          attn_loss=attn_loss, attn_loss_weight=opt.attn_loss if attn_loss is not None else 1.0,
                                          latent_guidance=make_guidance(opt, model), canvas_guidance=make_canvas_guidance(opt, model))
    os.makedirs(opt.outdir, exist_ok=True)
    hires = hires_plan(opt)
    if hires is not None:       # the second pass: DDIM on the same model, fixed weights, its own output directory
        hires_sampler = sampler_class("DDIMSampler")(model, opt_epochs=0, outdir=os.path.join(sampler.outdir, "hires"),
                                                     canvas_guidance=make_canvas_guidance(opt, model))
        hires_sampler.make_schedule(opt.ddim_steps, ddim_eta=opt.ddim_eta, verbose=False)

    seed = 1                                                            # txt2img-gpt.py:304
    shape = [opt.C, opt.H // opt.f, opt.W // opt.f]
    todo = list(enumerate(prompts))[opt.start: opt.start + 500]
    mine = [todo[j] for j in parallel.shard_indices(len(todo), rank, world)]

    def report_attn(group):
        """--attn_maps: files and the in-disc mass of every object of the prompts just sampled (prompts without objects have no readouts)."""
        if capture is None or sampler.last_attn is None:
            return
        image = sampler.last_result.get("image")
        for j, (i, _, l) in enumerate(group):
            for line in attnmaps.save_result(opt.outdir, i, list(l.keys()), [l[n] for n in l], sampler.last_attn,
                                             None if image is None else image[j], index=j):
                print("[rank %d] %s" % (rank, line))

    def refine(group):
        """--hires: the second pass on the latents the first pass just left in sampler.last_result["x0"] (one per prompt of `group`)."""
        if hires is None:
            return
        g2, t_start, disc_scale = hires
        conds = [conditionings(model, p, list(l.keys()), dtype) for _, p, l in group]
        print("[rank %d] hi-res fix for prompts %s: %s pixels, %d windows each, the last %d of %d DDIM calls, discs x %g"
              % (rank, [i for i, _, _ in group], opt.hires, g2.T, t_start, opt.ddim_steps, disc_scale))
        hires_sampler.hires_canvas(sampler.last_result["x0"], (g2.Hc, g2.Wc), g2.s, g2.stride, t_start=t_start, disc_scale=disc_scale,
                                   wrap=g2.wrap, seed=seed, conditionings=[c[1] for c in conds],
                                   unconditional_conditionings=[c[0] for c in conds], bboxs=[[l[n] for n in l] for _, _, l in group],
                                   object_names=[list(l.keys()) for _, _, l in group], local_conditionings=[c[2] for c in conds],
                                   unconditional_guidance_scale=opt.scale, prompt_indices=[i for i, _, _ in group],
                                   curr_texts=[p for _, p, _ in group])
        report_guidance(hires_sampler, [i for i, _, _ in group], "[rank %d] hires: " % rank)

    def run_one(prompt_idx, prompt, layout):
        torch.manual_seed(seed)                                         # seed_everything(seed), :306
        print("[rank %d] Start inference for %dth prompt: %s" % (rank, prompt_idx, prompt))
        names = list(layout.keys())
        uc, c, local_c = conditionings(model, prompt, names, dtype)
        x_T = torch.randn([opt.n_samples, *shape], device=dev) if opt.fixed_code else None
        sampler.sample(S=opt.ddim_steps, conditioning=c, batch_size=opt.n_samples, shape=shape, verbose=False,
                       unconditional_guidance_scale=opt.scale, unconditional_conditioning=uc, eta=eta, x_T=x_T,
                       text_index=0, curr_text=prompt, bboxs_curr=[layout[n] for n in names], seed=seed,
                       prompt_idx=prompt_idx, object_names=names, local_conditionings=local_c)
        report_attn([(prompt_idx, prompt, layout)])
        report_guidance(sampler, [prompt_idx], "[rank %d] " % rank)
        refine([(prompt_idx, prompt, layout)])

    def run_group(group):
        """Prompts with the same number of objects share one CFG batch; every image keeps the reference's
        per-prompt start: seed_everything(1) then randn, i.e. the same x_T for each."""
        torch.manual_seed(seed)
        x1 = torch.randn([1, *shape], device=dev)
        conds = [conditionings(model, p, list(l.keys()), dtype) for _, p, l in group]
        print("[rank %d] Start inference for prompts %s" % (rank, [i for i, _, _ in group]))
        sampler.sample_batch(S=opt.ddim_steps, shape=shape, conditionings=[c[1] for c in conds],
                             unconditional_conditionings=[c[0] for c in conds],
                             bboxs=[[l[n] for n in l] for _, _, l in group], object_names=[list(l.keys()) for _, _, l in group],
                             local_conditionings=[c[2] for c in conds], curr_texts=[p for _, p, _ in group],
                             x_T=x1.expand(len(group), -1, -1, -1), unconditional_guidance_scale=opt.scale, eta=eta,
                             seed=seed, prompt_indices=[i for i, _, _ in group])
        report_attn(group)
        report_guidance(sampler, [i for i, _, _ in group], "[rank %d] " % rank)
        refine(group)

    grid = canvas_grid(opt)

    def run_canvases(group):
        """--canvas: the prompts of `group` (same object count) as P canvases in one CFG batch of 2 P T window rows per UNet call; every
        canvas keeps the per-prompt start (seed_everything(1) then randn)."""
        torch.manual_seed(seed)
        x1 = torch.randn([1, opt.C, grid.Hc, grid.Wc], device=dev)
        conds = [conditionings(model, p, list(l.keys()), dtype) for _, p, l in group]
        print("[rank %d] Start inference for prompts %s on a %s canvas (%d windows each)" % (rank, [i for i, _, _ in group], opt.canvas, grid.T))
        sampler.sample_canvas(S=opt.ddim_steps, canvas=(grid.Hc, grid.Wc), window=grid.s, stride=grid.stride,
                              conditionings=[c[1] for c in conds], unconditional_conditionings=[c[0] for c in conds],
                              bboxs=[[l[n] for n in l] for _, _, l in group], object_names=[list(l.keys()) for _, _, l in group],
                              local_conditionings=[c[2] for c in conds], curr_texts=[p for _, p, _ in group],
                              x_T=x1.expand(len(group), -1, -1, -1).contiguous(), unconditional_guidance_scale=opt.scale, eta=eta, seed=seed,
                              prompt_indices=[i for i, _, _ in group], channels=opt.C, wrap=grid.wrap)
        report_guidance(sampler, [i for i, _, _ in group], "[rank %d] " % rank)
        refine(group)

    items = [(i, p, datasets.layout_for(layouts, p, i) or {}) for i, p in mine]
    if grid is not None:
        run_one = lambda i, p, l: run_canvases([(i, p, l)])
        run_group = run_canvases
    if opt.batch_prompts <= 1:
        for i, p, l in items:
            run_one(i, p, l)
    else:
        by_k = {}
        for it in items:
            by_k.setdefault(len(it[2]), []).append(it)
        for k in sorted(by_k):
            g = by_k[k]
            for a in range(0, len(g), opt.batch_prompts):
                run_group(g[a:a + opt.batch_prompts])
    parallel.barrier()
