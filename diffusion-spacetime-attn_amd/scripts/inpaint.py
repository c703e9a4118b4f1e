"""Layout-guided inpainting on the spatial-temporal UNet: repaint a region of an existing image with layout guidance and leave the rest
as it is (the mask arithmetic of the reference's ddim.py:144-147, which there only ran on the plain apply_model route).

The flags of scripts/img2img.py (same parser, same seed discipline, same refusals), plus exactly one of
  --mask FILE|DIR          white = repaint (the CompVis inpaint.py convention), one file for every prompt or <dir>/<i>.png|jpg per prompt;
                           loaded at the image's size, binarised at 0.5. A latent cell is repainted if any of its 8 x 8 pixels is
                           (max-pool); the sampler's mask is keep = 1 - repaint.
  --mask_from_layout R     repaint the union of the discs of radius R around the prompt's object centres: the blocks' own disc
                           definition (attention.py:251-262, sta.ops.disc_masks) at latent resolution.
--strength in (0, 1]: at 1 the repainted region starts from noise (sample / sample_batch; --dpm_solver is allowed); below 1 it starts
from the image's latent noised to t_enc = int(strength ddim_steps) (encode_step(want_z0=True), then decode / decode_batch; DDIM only).
The output is the composite: the original outside the pixel mask (its 8-bit values exactly), the decoded image inside it. The fidelity
loss of --opt_epochs sees the composite.

Refused before anything is built: what img2img refuses (--plms, --n_samples != 1, non-square / not-multiple-of-64 / mixed images),
--dpm_solver below strength 1, strength outside (0, 1], t_enc outside 1 .. S - 1 below strength 1, none or both of --mask and
--mask_from_layout, a mask of another size than its image, a prompt without layout objects under --mask_from_layout, a mask that
repaints nothing.

Seed / draw order (the result of a prompt depends only on the prompt, its image and its mask, not on batching or on the prompts before):
  1. for every image, right before its posterior draw: torch.manual_seed(--seed), n_post = torch.randn([1, 4, h, w]), CPU generator;
  2. for every prompt, right before its draw: torch.manual_seed(--seed), then torch.randn([1, 4, h, w]) on the device: the
     stochastic_encode noise below strength 1, the start latent x_T at strength 1;
  3. then, on the device, in the sampler's order: the blend draw of call i, the eta draw of call i (eta > 0), the blend draw of call
     i + 1, ... (the batch's draws are shared).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _txt2img_common  # noqa: E402,F401  (sys.path)
import img2img as _i2i  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build_parser():
    p = _i2i.build_parser()
    p.set_defaults(outdir="outputs/inpaint-samples")
    p.add_argument("--mask", type=str, default=None, help="mask image (white = repaint), or a directory with <prompt index>.png|jpg")
    p.add_argument("--mask_from_layout", type=float, default=None, metavar="R",
                   help="repaint the discs of radius R around the layout's object centres")
    return p


def check_options(opt):
    """Refusals that need nothing loaded. Returns t_enc (ddim_steps at strength 1: the whole trajectory, from noise)."""
    if opt.plms:
        raise SystemExit("--plms: masked PLMS is not supported (its step is not on the sampler-step kernel)")
    if opt.n_samples != 1:
        raise SystemExit("--n_samples must be 1 (the blocks reshape to the CFG batch of 2, attention.py:282)")
    if not 0.0 < opt.strength <= 1.0:
        raise SystemExit("--strength must be in (0, 1]")
    if opt.canvas_guidance is not None:
        raise SystemExit("--canvas_guidance %s needs --canvas HxW: inpaint.py repaints square images (--attn_guidance), a canvas is "
                         "outpaint.py's" % opt.canvas_guidance)
    if (opt.mask is None) == (opt.mask_from_layout is None):
        raise SystemExit("exactly one of --mask and --mask_from_layout must be given")
    if opt.mask_from_layout is not None and not opt.mask_from_layout > 0.0:
        raise SystemExit("--mask_from_layout: the radius must be positive")
    if opt.mask_from_layout is not None and not opt.layout:
        raise SystemExit("--mask_from_layout needs --layout")
    if opt.strength == 1.0:
        t_enc = opt.ddim_steps
    else:
        if opt.dpm_solver:
            raise SystemExit("--dpm_solver: below --strength 1 inpainting runs the DDIM decode only")
        t_enc = int(opt.strength * opt.ddim_steps)
        if not 1 <= t_enc <= opt.ddim_steps - 1:
            raise SystemExit("t_enc = int(strength * ddim_steps) = %d must be in 1 .. %d" % (t_enc, opt.ddim_steps - 1))
    if not opt.init_img:
        raise SystemExit("--init-img is required")
    _txt2img_common.check_clip_option(opt)
    return t_enc


def load_mask(path, size):
    """[1, 1, size, size] float32 REPAINT mask of a mask image: 1 where the image is white (>= 0.5 of full scale), 0 where it is black."""
    from PIL import Image
    m = Image.open(path).convert("L")
    if m.size != (size, size):
        raise SystemExit("--mask %s: %d x %d, the image is %d x %d" % (path, m.size[0], m.size[1], size, size))
    g = torch.from_numpy(np.array(m).astype(np.float32) / 255.0)
    return (g >= 0.5).to(torch.float32)[None, None]


def latent_repaint(repaint_px, f=8):
    """A latent cell is repainted if any of its f x f pixels is."""
    return torch.nn.functional.max_pool2d(repaint_px, f)


def layout_repaint(centres, lat, radius):
    """[1, 1, lat, lat] float32: the union of the blocks' discs (sta.ops.disc_masks) of `radius` around the centres, latent resolution."""
    from sta import ops
    if not len(centres):
        return torch.zeros(1, 1, lat, lat)
    m = ops.disc_masks([tuple(c) for c in centres], lat, radius_sq=radius * radius)
    return m.reshape(len(centres), lat, lat).amax(0).to(torch.float32)[None, None]


def masks_for(opt, index, layout, mask_path, size, f=8):
    """(keep [1, 1, lat, lat], keep_px [1, 1, size, size]) of one prompt: 1 = keep the original (the sampler's convention)."""
    lat = size // f
    if opt.mask is not None:
        repaint_px = load_mask(mask_path, size)
        repaint = latent_repaint(repaint_px, f)
    else:
        if not layout:
            raise SystemExit("--mask_from_layout: prompt %d has no layout objects" % index)
        repaint = layout_repaint(list(layout.values()), lat, opt.mask_from_layout)
        repaint_px = repaint.repeat_interleave(f, dim=-2).repeat_interleave(f, dim=-1)
    if float(repaint.max()) == 0.0:
        raise SystemExit("prompt %d: the mask repaints nothing" % index)
    return 1.0 - repaint, 1.0 - repaint_px


def main(argv=None):
    opt = build_parser().parse_args(argv)
    t_enc = check_options(opt)
    prompts = _i2i.read_prompts(opt)
    paths = _i2i.image_paths(opt.init_img, len(prompts))
    images = {p: _i2i.load_img(p) for p in dict.fromkeys(paths)}
    size = _i2i.check_images(images)
    _txt2img_common.check_clip_option(opt, (size, size))
    _txt2img_common.check_guidance_option(opt, size)
    from sta import datasets
    layouts = datasets.load_layouts(opt.layout) if opt.layout else None
    items = [(i, p, datasets.layout_for(layouts, p, i) or {}, paths[i]) for i, p in enumerate(prompts)]
    mask_paths = [None] * len(prompts)
    if opt.mask is not None:
        try:
            mask_paths = _i2i.image_paths(opt.mask, len(prompts))
        except SystemExit as e:
            raise SystemExit(str(e).replace("--init-img", "--mask"))
    masks = {i: masks_for(opt, i, l, mask_paths[i], size, opt.f) for i, _, l, _ in items}
    loss_tokenize = None
    if _txt2img_common.builtin_clip(opt) is not None:
        loss_tokenize = _txt2img_common.loss_tokenizer(opt)
        _txt2img_common.check_loss_texts(loss_tokenize, [(p, list(l.keys())) for _, p, l, _ in items])
    if not torch.cuda.is_available():
        raise SystemExit("a GPU is required (the fused cross-attention has no CPU path)")
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
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
    cls = DPMSolverSampler if opt.dpm_solver else DDIMSampler
    sampler = cls(model, opt_epochs=opt.opt_epochs, loss_model=loss_model, outdir=opt.outdir, save_images=not opt.skip_save,
                  latent_guidance=_txt2img_common.make_guidance(opt, model))
    sampler.make_schedule(opt.ddim_steps, ddim_eta=opt.ddim_eta, verbose=False)
    encoder = sampler                                            # the fused encode step lives on the DDIM sampler (its tables)
    if opt.dpm_solver:
        encoder = DDIMSampler(model, opt_epochs=0, save_images=False)
        encoder.make_schedule(opt.ddim_steps, ddim_eta=0.0, verbose=False)
    os.makedirs(opt.outdir, exist_ok=True)
    lat = size // opt.f
    shape = (1, opt.C, lat, lat)
    from_noise = t_enc == opt.ddim_steps
    print("inpainting from noise" if from_noise else "target t_enc is %d steps" % t_enc)

    h_cache = {}

    def encode(batch_paths):
        todo = [p for p in dict.fromkeys(batch_paths) if p not in h_cache]
        if todo:
            with torch.no_grad():
                h = vae.encode_moments_input(torch.cat([images[p] for p in todo]).to(dev))
            for p, hp in zip(todo, h.split(1)):
                h_cache[p] = hp
        return torch.cat([h_cache[p] for p in batch_paths])

    post_noise = {p: _i2i.posterior_noise(opt.seed, shape) for p in images}          # draw 1, one per image

    def run(group):
        """group: [(index, prompt, layout, path)] with the same object count."""
        h = encode([g[3] for g in group])
        n_post = torch.cat([post_noise[g[3]] for g in group])
        n_enc = torch.cat([_i2i.encode_noise(opt.seed, shape, dev) for _ in group])  # draw 2, one per prompt
        with torch.no_grad():
            # the clean latent z0 (and, below strength 1, the latent noised to t_enc); at strength 1 the start latent is the draw itself
            x, z0, _ = encoder.encode_step(h, vae, 0 if from_noise else t_enc, n_post, n_enc, want_z0=True)
        keep = torch.cat([masks[g[0]][0] for g in group]).to(dev)
        keep_px = torch.cat([masks[g[0]][1] for g in group]).to(dev)
        orig = torch.cat([(images[g[3]] + 1.0) / 2.0 for g in group]).to(dev)
        inp = dict(mask=keep, x0=z0, image=orig, mask_px=keep_px)
        conds = [conditionings(model, p, list(l.keys()), dtype) for _, p, l, _ in group]
        print("Start inpainting for prompts %s" % [i for i, _, _, _ in group])
        if len(group) == 1:
            (i, p, l, _), (uc, c, local) = group[0], conds[0]
            names = list(l.keys())
            kw = dict(unconditional_guidance_scale=opt.scale, unconditional_conditioning=uc, text_index=0, curr_text=p,
                      bboxs_curr=[l[n] for n in names], seed=opt.seed, prompt_idx=i, object_names=names, local_conditionings=local, **inp)
            if from_noise:
                sampler.sample(S=opt.ddim_steps, batch_size=1, shape=list(shape[1:]), conditioning=c, verbose=False, eta=opt.ddim_eta,
                               x_T=n_enc, **kw)
            else:
                sampler.decode(x, c, t_enc, **kw)
        else:
            args = ([c[1] for c in conds], [c[0] for c in conds], [[l[n] for n in l] for _, _, l, _ in group],
                    [list(l.keys()) for _, _, l, _ in group], [c[2] for c in conds])
            kw = dict(curr_texts=[p for _, p, _, _ in group], unconditional_guidance_scale=opt.scale, seed=opt.seed,
                      prompt_indices=[i for i, _, _, _ in group], **inp)
            if from_noise:
                sampler.sample_batch(opt.ddim_steps, list(shape[1:]), *args, x_T=n_enc, eta=opt.ddim_eta, **kw)
            else:
                sampler.decode_batch(x, *args, t_enc, **kw)
        _txt2img_common.report_guidance(sampler, [i for i, _, _, _ in group])

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
