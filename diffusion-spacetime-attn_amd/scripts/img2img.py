"""Layout-guided image-to-image (SDEdit) on the spatial-temporal UNet (reference: scripts/img2img.py).

Kept from the reference CLI: --prompt --from-file --init-img --outdir --skip_grid --skip_save --ddim_steps --plms --fixed_code
--ddim_eta --n_iter --C --f --n_samples --n_rows --scale --strength --config --ckpt --seed --precision (parsed; --config,
--precision, --skip_grid, --fixed_code, --n_iter, --n_rows have no effect here). Added, as in txt2img: --layout (JSON keyed by prompt
or prompt index; prompts without an entry run with K = 0, plain SD img2img on the same UNet) --opt_epochs --dtype --synthetic --clip
--clip_tokenizer --batch_prompts (prompts with the same object count and image size decode in one CFG batch).

--init-img is one image file, which every prompt starts from (encoded once), or a directory where prompt i starts from <dir>/<i>.png
(or .jpg); the images of one CFG batch are encoded in one encoder call. Images load as the reference's load_img: sides rounded down
to a multiple of 32, LANCZOS, scaled to [-1, 1]. Output files are named as txt2img names them (final{E-1}_s{seed}_index_{i}.png).

--canvas HxW / --canvas_stride PX / --canvas_wrap x|y|xy / --window PX (default 512): img2img on a wide, tall or wrap-around canvas decoded
as overlapping --window x --window windows (sta.canvas; the flags mean what they mean in the txt2img scripts, with --window as their --H =
--W). The init image may then be of any size: it is resized to the canvas with LANCZOS at load time (printed), so a 512^2 picture with
--canvas 1024x1024 --strength 0.4 is a tiled upscale-and-refine pass. The whole canvas is encoded once (on a wrapped canvas with circular
padding, so the encoder sees across the seam), one sta_vae_encode_step_windows launch writes the canvas state and the first call's window
inputs, and DDIMSampler.decode_canvas runs the last t_enc calls. The layout's centres are normalised to the canvas; prompts with the same
object count run as P canvases of one batch (--batch_prompts); the draws below are canvas-shaped. --canvas_guidance ETA guides the decode
from its first call (sta.guidance.CanvasGuidance; needs --canvas). --disc_scale F (default 1.0; needs --canvas): the layout's discs have radius 0.2 F
window sides in every window; an upscale-and-refine pass gives the upscale factor (2.0 for 512^2 -> 1024x1024) so that every object keeps
its share of the picture. Refused with --canvas before a model is
built: --opt_epochs > 1, --attn_guidance, a --window that is no multiple of 8 x --f, and every refusal of the txt2img scripts' canvas
grid. Not claimed: image quality or seam visibility with real weights; the VAE's mid-block attention is global over the canvas, O((Hc
Wc)^2) memory in its chunked form, for the encoder as for the one decode; without --disc_scale a disc keeps its radius of 0.2 window sides, so
objects shrink relative to an upscaled canvas.

Refused before anything is built: --plms (the reference raises NotImplementedError too), --dpm_solver, t_enc = int(strength S) outside
1 .. S - 1 (at t_enc = S the reference indexes past its tables), --n_samples != 1, a non-square image or a side that is not a multiple
of 64 (the blocks need square latents and the UNet downsamples three times), mixed image sizes.

Seed / draw order (the result of a prompt depends only on the prompt and its image, not on batching or on the prompts before it):
  1. for every image, right before its posterior draw: torch.manual_seed(--seed), then n_post = torch.randn([1, 4, h, w]) on the CPU
     default generator (DiagonalGaussianDistribution.sample, distributions.py:35-37), one image per draw;
  2. for every prompt, right before its stochastic_encode draw: torch.manual_seed(--seed), then n_enc = torch.randn([1, 4, h, w]) on the
     device (torch.randn_like on the latent, ddim.py:216-217);
  3. DDIM noise at eta > 0: torch.randn on the device after each UNet call, in the sampler's order (the batch's draws are shared).
Exact parity of draws with the reference CLI is not possible: its model construction consumes the generator after seed_everything.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _txt2img_common  # noqa: E402,F401  (sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build_parser(canvas=False):
    """canvas=True: img2img.py's own parser, with --canvas / --canvas_stride / --canvas_wrap / --window. inpaint.py and outpaint.py build
    on this parser and take it without them (outpaint.py defines its own --canvas flags, inpaint.py has no canvas form)."""
    p = argparse.ArgumentParser()
    p.add_argument("--prompt", type=str, nargs="?", default="a painting of a virus monster playing guitar")
    p.add_argument("--init-img", type=str, nargs="?", help="path to the input image, or a directory with <prompt index>.png|jpg")
    p.add_argument("--outdir", type=str, nargs="?", default="outputs/img2img-samples")
    p.add_argument("--skip_grid", action="store_true")
    p.add_argument("--skip_save", action="store_true")
    p.add_argument("--ddim_steps", type=int, default=50)
    p.add_argument("--plms", action="store_true")
    p.add_argument("--dpm_solver", action="store_true")
    p.add_argument("--fixed_code", action="store_true")
    p.add_argument("--ddim_eta", type=float, default=0.0)
    p.add_argument("--n_iter", type=int, default=1)
    p.add_argument("--C", type=int, default=4)
    p.add_argument("--f", type=int, default=8)
    p.add_argument("--n_samples", type=int, default=1)
    p.add_argument("--n_rows", type=int, default=0)
    p.add_argument("--scale", type=float, default=5.0)
    p.add_argument("--strength", type=float, default=0.75)
    p.add_argument("--from-file", type=str)
    p.add_argument("--config", type=str, default="configs/stable-diffusion/v1-inference.yaml")
    p.add_argument("--ckpt", type=str, default="models/ldm/stable-diffusion-v1/model.ckpt")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--precision", type=str, choices=["full", "autocast"], default="autocast")
    p.add_argument("--layout", type=str, default=None, help="JSON {prompt | index: {object: [x, y]}}")
    p.add_argument("--opt_epochs", type=int, default=3, help="weight-optimisation epochs (reference: 3; 0 = fixed weights)")
    p.add_argument("--dtype", type=str, choices=["bf16", "fp16"], default="fp16")
    p.add_argument("--clip", type=str, default=None, help="fidelity-loss model for --opt_epochs > 1 (see txt2img)")
    p.add_argument("--clip_tokenizer", type=str, default=None)
    p.add_argument("--synthetic", action="store_true", help="synthetic weights/text embeddings when no checkpoint is available")
    p.add_argument("--batch_prompts", type=int, default=1)
    if canvas:
        add_canvas_arguments(p)
    _txt2img_common.add_guidance_arguments(p, attn_res=True)
    return p


def add_canvas_arguments(p):
    p.add_argument("--canvas", type=str, default=None, metavar="HxW",
                   help="img2img on a canvas of H x W pixels, decoded as overlapping --window x --window windows in one CFG batch per UNet "
                        "call (sta.canvas); the init image, of any size, is resized to the canvas (LANCZOS): a smaller picture is upscaled "
                        "and refined window by window; fixed blend weights only (--opt_epochs 0 or 1), no --attn_guidance (on a canvas: "
                        "--canvas_guidance)")
    p.add_argument("--canvas_stride", type=int, default=None, metavar="PX",
                   help="distance between neighbouring windows of --canvas in pixels (default: half the window)")
    p.add_argument("--canvas_wrap", type=str, default=None, choices=("x", "y", "xy"),
                   help="the --canvas closes on itself along these axes (x: a 360 degree panorama)")
    p.add_argument("--window", type=int, default=512, metavar="PX", help="side of the square windows of --canvas in pixels")
    p.add_argument("--disc_scale", type=float, default=1.0, metavar="F",
                   help="the layout's discs have radius 0.2 F window sides on the --canvas (default 1.0); the upscale factor keeps every "
                        "object's share of an upscaled picture")


def canvas_grid(opt):
    """The sta.canvas.Grid of --canvas / --canvas_stride / --canvas_wrap / --window (the rules of the txt2img scripts,
    _txt2img_common.canvas_grid, with --window as their --H = --W), or None without --canvas; every refusal that needs no GPU."""
    view = argparse.Namespace(canvas=opt.canvas, canvas_stride=opt.canvas_stride, canvas_wrap=opt.canvas_wrap, H=opt.window, W=opt.window,
                              f=opt.f, opt_epochs=opt.opt_epochs, attn_maps=False, attn_loss=None, attn_guidance=opt.attn_guidance,
                              canvas_guidance=opt.canvas_guidance, attn_res=opt.attn_res)
    try:
        grid = _txt2img_common.canvas_grid(view)
    except SystemExit as e:
        raise SystemExit(str(e).replace("--H / --W", "--window").replace("--H x --W", "--window x --window"))
    if grid is None and opt.disc_scale != 1.0:
        raise SystemExit("--disc_scale %s needs --canvas HxW" % opt.disc_scale)
    if grid is not None:
        from sta import canvas
        try:
            canvas.check_disc_scale(grid, opt.disc_scale)
        except ValueError as e:
            raise SystemExit("--disc_scale %s: %s" % (opt.disc_scale, e))
    return grid


def check_options(opt):
    """Refusals that need nothing loaded. Returns t_enc."""
    if opt.plms:
        raise SystemExit("--plms: PLMS img2img is not supported (the reference raises NotImplementedError too)")
    if opt.dpm_solver:
        raise SystemExit("--dpm_solver: img2img runs the DDIM decode only")
    if opt.n_samples != 1:
        raise SystemExit("--n_samples must be 1 (the blocks reshape to the CFG batch of 2, attention.py:282)")
    if not 0.0 <= opt.strength <= 1.0:
        raise SystemExit("--strength must be in [0, 1]")
    t_enc = int(opt.strength * opt.ddim_steps)
    if not 1 <= t_enc <= opt.ddim_steps - 1:
        raise SystemExit("t_enc = int(strength * ddim_steps) = %d must be in 1 .. %d" % (t_enc, opt.ddim_steps - 1))
    if not opt.init_img:
        raise SystemExit("--init-img is required")
    _txt2img_common.check_clip_option(opt)
    return t_enc


def read_prompts(opt):
    if opt.from_file:
        with open(opt.from_file, "r") as f:
            return f.read().splitlines()
    if opt.prompt is None:
        raise SystemExit("--prompt or --from-file is required")
    return [opt.prompt]


def load_img(path, size=None):
    """The reference's load_img (img2img.py:47-57): [1, 3, h, w] in [-1, 1], sides rounded down to a multiple of 32, LANCZOS.
    size = (h, w): --canvas, the picture is resized to the canvas instead (any size in, LANCZOS; the resize is printed)."""
    from PIL import Image
    image = Image.open(path).convert("RGB")
    w, h = image.size
    if size is None:
        w, h = map(lambda x: x - x % 32, (w, h))
    else:
        print("%s: %d x %d resized to the %d x %d canvas (LANCZOS)" % (path, w, h, size[1], size[0]))
        h, w = size
    image = image.resize((w, h), resample=Image.LANCZOS)
    image = np.array(image).astype(np.float32) / 255.0
    image = torch.from_numpy(image[None].transpose(0, 3, 1, 2))
    return 2.0 * image - 1.0


def image_paths(init_img, n_prompts):
    """One path per prompt: the same file for every prompt, or <dir>/<i>.png|jpg."""
    if os.path.isdir(init_img):
        paths = []
        for i in range(n_prompts):
            for ext in (".png", ".jpg", ".jpeg"):
                cand = os.path.join(init_img, "%d%s" % (i, ext))
                if os.path.exists(cand):
                    paths.append(cand)
                    break
            else:
                raise SystemExit("--init-img %s: no %d.png or %d.jpg for prompt %d" % (init_img, i, i, i))
        return paths
    if not os.path.isfile(init_img):
        raise SystemExit("--init-img %s: no such file or directory" % init_img)
    return [init_img] * n_prompts


def check_images(images):
    """images: {path: [1, 3, h, w]}. Square, sides a multiple of 64, one size for all."""
    sizes = set()
    for path, im in images.items():
        h, w = im.shape[-2:]
        if h != w:
            raise SystemExit("%s: %d x %d is not square (the spatial-temporal blocks need square latents)" % (path, w, h))
        if h % 64:
            raise SystemExit("%s: side %d is not a multiple of 64 (the UNet downsamples the latent three times)" % (path, h))
        sizes.add(h)
    if len(sizes) > 1:
        raise SystemExit("--init-img: mixed image sizes %s" % sorted(sizes))
    return sizes.pop()


def posterior_noise(seed, shape):
    """Draw 1 of the seed / draw order: seeded right before each image's posterior draw, CPU default generator."""
    torch.manual_seed(seed)
    return torch.randn(shape)


def encode_noise(seed, shape, device):
    """Draw 2: seeded right before each prompt's stochastic_encode draw, on the device."""
    torch.manual_seed(seed)
    return torch.randn(shape, device=device)


def main(argv=None):
    opt = build_parser(canvas=True).parse_args(argv)
    t_enc = check_options(opt)
    grid = canvas_grid(opt)
    prompts = read_prompts(opt)
    paths = image_paths(opt.init_img, len(prompts))
    if grid is None:
        images = {p: load_img(p) for p in dict.fromkeys(paths)}
        size = check_images(images)
        _txt2img_common.check_clip_option(opt, (size, size))
        _txt2img_common.check_guidance_option(opt, size)
    else:           # any picture, resized to the canvas: --opt_epochs > 1 and --attn_guidance are refused above, nothing else reads the size
        images = {p: load_img(p, (grid.Hc * opt.f, grid.Wc * opt.f)) for p in dict.fromkeys(paths)}
    from sta import datasets
    layouts = datasets.load_layouts(opt.layout) if opt.layout else None
    loss_tokenize = None
    if _txt2img_common.builtin_clip(opt) is not None:
        loss_tokenize = _txt2img_common.loss_tokenizer(opt)
        _txt2img_common.check_loss_texts(loss_tokenize, [(p, list((datasets.layout_for(layouts, p, i) or {}).keys()))
                                                         for i, p in enumerate(prompts)])
    if not torch.cuda.is_available():
        raise SystemExit("a GPU is required (the fused cross-attention has no CPU path)")
    from ldm.models.diffusion.ddim import DDIMSampler
    from sta.pipeline import build_sd_v1, conditionings, use_shipped_miopen_db

    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if opt.dtype == "bf16" else torch.float16
    use_shipped_miopen_db(0)
    ckpt = opt.ckpt if (os.path.exists(opt.ckpt) and not opt.synthetic) else None
    if ckpt is None and not opt.synthetic:
        raise SystemExit("checkpoint %s not found (pass --synthetic to run with synthetic weights)" % opt.ckpt)
    loss_model = None
    if opt.opt_epochs > 1:
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
    model = build_sd_v1(dev, dtype, ckpt=ckpt, use_checkpoint=opt.opt_epochs > 1, clip_tokenizer=opt.clip_tokenizer,
                        real_text_encoder=ckpt is not None, with_encoder=True)
    vae = model.first_stage_model
    vae.encoder.to(memory_format=torch.channels_last)            # NHWC encoder: its convolutions on the HIP kernels
    sampler = DDIMSampler(model, opt_epochs=opt.opt_epochs, loss_model=loss_model, outdir=opt.outdir, save_images=not opt.skip_save,
                          latent_guidance=_txt2img_common.make_guidance(opt, model),
                          canvas_guidance=_txt2img_common.make_canvas_guidance(opt, model))
    sampler.make_schedule(opt.ddim_steps, ddim_eta=opt.ddim_eta, verbose=False)
    os.makedirs(opt.outdir, exist_ok=True)
    shape = (1, opt.C, size // opt.f, size // opt.f) if grid is None else (1, opt.C, grid.Hc, grid.Wc)
    print("target t_enc is %d steps" % t_enc)

    # posterior moments input h per distinct image, the images of one batch through one encoder call
    h_cache = {}

    def encode(batch_paths):
        todo = [p for p in dict.fromkeys(batch_paths) if p not in h_cache]
        if todo:
            with torch.no_grad():
                batch = torch.cat([images[p] for p in todo]).to(dev)
                # a canvas: one encode of the whole picture, which on a wrapped canvas sees across the seam (circular padding)
                h = vae.encode_moments_input(batch) if grid is None else sampler._encode_canvas(batch, grid, vae)
            for p, hp in zip(todo, h.split(1)):
                h_cache[p] = hp
        return torch.cat([h_cache[p] for p in batch_paths])

    post_noise = {p: posterior_noise(opt.seed, shape) for p in images}          # draw 1, one per image

    def run(group):
        """group: [(index, prompt, layout, path)] with the same object count."""
        h = encode([g[3] for g in group])
        n_post = torch.cat([post_noise[g[3]] for g in group])
        n_enc = torch.cat([encode_noise(opt.seed, shape, dev) for _ in group])  # draw 2, one per prompt
        with torch.no_grad():
            if grid is None:
                x, _, xin = sampler.encode_step(h, vae, t_enc, n_post, n_enc)
            else:       # the canvas state and the first call's window inputs in one launch
                x, _, xin = sampler.encode_step_canvas(h, vae, t_enc, n_post, n_enc, grid)
        conds = [conditionings(model, p, list(l.keys()), dtype) for _, p, l, _ in group]
        print("Start img2img for prompts %s" % [i for i, _, _, _ in group] + ("" if grid is None else " on a %s canvas (%d windows each)"
                                                                              % (opt.canvas, grid.T)))
        if grid is not None:        # the prompts of the group as P canvases of one CFG batch of 2 P T window rows per UNet call
            sampler.decode_canvas(x, (grid.Hc, grid.Wc), grid.s, grid.stride, t_start=t_enc, conditionings=[c[1] for c in conds],
                                  unconditional_conditionings=[c[0] for c in conds], bboxs=[[l[n] for n in l] for _, _, l, _ in group],
                                  object_names=[list(l.keys()) for _, _, l, _ in group], local_conditionings=[c[2] for c in conds],
                                  unconditional_guidance_scale=opt.scale, seed=opt.seed, prompt_indices=[i for i, _, _, _ in group],
                                  curr_texts=[p for _, p, _, _ in group], xin=xin, wrap=grid.wrap, disc_scale=opt.disc_scale)
        elif len(group) == 1:
            (i, p, l, _), (uc, c, local) = group[0], conds[0]
            names = list(l.keys())
            sampler.decode(x, c, t_enc, unconditional_guidance_scale=opt.scale, unconditional_conditioning=uc, text_index=0, curr_text=p,
                           bboxs_curr=[l[n] for n in names], seed=opt.seed, prompt_idx=i, object_names=names, local_conditionings=local,
                           xin=xin)
        else:
            sampler.decode_batch(x, [c[1] for c in conds], [c[0] for c in conds], [[l[n] for n in l] for _, _, l, _ in group],
                                 [list(l.keys()) for _, _, l, _ in group], [c[2] for c in conds], t_enc,
                                 curr_texts=[p for _, p, _, _ in group], unconditional_guidance_scale=opt.scale, seed=opt.seed,
                                 prompt_indices=[i for i, _, _, _ in group], xin=xin)
        _txt2img_common.report_guidance(sampler, [i for i, _, _, _ in group])

    items = [(i, p, datasets.layout_for(layouts, p, i) or {}, paths[i]) for i, p in enumerate(prompts)]
    by_k = {}
    for it in items:
        by_k.setdefault(len(it[2]), []).append(it)
    step = max(opt.batch_prompts, 1)
    for k in sorted(by_k):
        g = by_k[k]
        for a in range(0, len(g), step):
            run(g[a:a + step])
    print("Your samples are ready and waiting for you here: %s" % opt.outdir)


if __name__ == "__main__":
    main()
