"""Layout-guided outpainting on the spatial-temporal UNet: extend an existing square picture to a wide or tall canvas, with objects
placed by layout in the new area, and leave the picture as it is (the canvas of sta.canvas sampled as overlapping windows, with the mask
arithmetic of the reference's ddim.py:144-147 on the canvas: SolverSamplerBase.inpaint_canvas).

The flags of scripts/img2img.py (same parser, same seed discipline), plus
  --canvas HxW             the canvas in pixels, sampled as overlapping --H x --W windows (square; default 512), as in the txt2img scripts;
  --canvas_stride PX       distance between neighbouring windows (default: half a window);
  --place X,Y              where the picture's top-left corner lies on the canvas, in pixels (default 0,0);
  --canvas_wrap x|y|xy     the canvas closes on itself along these axes (sta.canvas: a 360 degree panorama, a tileable image); a side
                           of the picture on a wrapped border is then no border (--seam erodes it), and the picture may not cross the seam;
  --seam PX                the picture's footprint is eroded by this many pixels on every side that does not lie on the canvas border:
                           the strip is repainted, so the new area grows out of the picture instead of meeting it at a hard edge
                           (default 0).
--init-img is the square picture (one file for every prompt, or <dir>/<i>.png|jpg). It is encoded by the encoder path of inpaint.py
(encode_step(..., want_z0=True)); its latent is written into a zero canvas x0 at (Y / f, X / f); keep = 1 on the eroded footprint (latent
cells) and keep_px the same in pixels. The centres of --layout are normalised to the canvas. DDIM by default, DPM-Solver++ with
--dpm_solver. The output is the composite canvas image: the picture's 8-bit values exactly where keep_px == 1, one decode of the whole
canvas elsewhere. Fixed blend weights (--opt_epochs 0 or 1; the default here is 0).
  --canvas_guidance ETA    attention guidance on the canvas (sta.guidance.CanvasGuidance; --attn_guidance_steps / --attn_guidance_iters /
                           --attn_res as in the txt2img scripts): the objects of the new area are steered into their discs, the kept
                           picture is not guided.

Refused before a model is built: --plms, --strength != 1 (the new area starts from noise), --opt_epochs > 1, --attn_maps / --attn_loss /
--attn_guidance, --n_samples != 1, --place or --seam that is not a multiple of --f, a footprint outside the canvas, a seam that leaves
nothing kept, a footprint that leaves nothing to paint, and every canvas refusal of _txt2img_common.canvas_grid.

Seed / draw order (the result of a prompt depends only on the prompt, its picture and the canvas, not on batching):
  1. for every picture, right before its posterior draw: torch.manual_seed(--seed), n_post = torch.randn([1, 4, h, w]), CPU generator;
  2. for every prompt, right before its draw: torch.manual_seed(--seed), then torch.randn([1, 4, Hc, Wc]) on the device: the start
     latent x_T of the canvas;
  3. then, on the device, in the sampler's order: the blend draw of call i, the eta draw of call i (eta > 0), the blend draw of call
     i + 1, ... (canvas-shaped; the batch's draws are shared).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _txt2img_common  # noqa: E402,F401  (sys.path)
import img2img as _i2i  # noqa: E402

import torch  # noqa: E402


def build_parser():
    p = _i2i.build_parser()
    p.set_defaults(outdir="outputs/outpaint-samples", strength=1.0, opt_epochs=0)
    p.add_argument("--H", type=int, default=512, help="window height in pixels")
    p.add_argument("--W", type=int, default=512, help="window width in pixels")
    p.add_argument("--canvas", type=str, default=None, metavar="HxW", help="the canvas in pixels, sampled as overlapping --H x --W windows")
    p.add_argument("--canvas_stride", type=int, default=None, metavar="PX", help="distance between neighbouring windows (default: half a window)")
    p.add_argument("--canvas_wrap", type=str, default=None, choices=("x", "y", "xy"),
                   help="the canvas closes on itself along these axes (x: 360 degree panorama, xy: tileable image)")
    p.add_argument("--place", type=str, default="0,0", metavar="X,Y", help="top-left corner of --init-img on the canvas, pixels")
    p.add_argument("--seam", type=int, default=0, metavar="PX",
                   help="erode the picture's footprint by PX on every side that does not lie on the canvas border (that strip is repainted)")
    p.add_argument("--attn_maps", action="store_true", help="not defined on a canvas (refused)")
    p.add_argument("--attn_loss", type=float, default=None, help="not defined on a canvas (refused)")
    return p


def check_options(opt):
    """Refusals that need nothing loaded. Returns (the sta.canvas.Grid, (X, Y) of --place)."""
    if opt.plms:
        raise SystemExit("--plms: masked PLMS is not supported (its step is not on the sampler-step kernel)")
    if opt.n_samples != 1:
        raise SystemExit("--n_samples must be 1 (the blocks reshape to the CFG batch of 2, attention.py:282)")
    if opt.strength != 1.0:
        raise SystemExit("--strength %s: outpainting starts the new area from noise (--strength 1 only; img2img on a canvas is not defined)"
                         % opt.strength)
    grid = _txt2img_common.canvas_grid(opt)          # --opt_epochs > 1, --attn_maps / --attn_loss / --attn_guidance, every grid rule
    if grid is None:
        raise SystemExit("--canvas HxW is required")
    parts = opt.place.split(",")
    if len(parts) != 2 or not all(v.strip().isdigit() for v in parts):
        raise SystemExit("--place %s: expected X,Y in pixels, e.g. 512,0" % opt.place)
    place = (int(parts[0]), int(parts[1]))
    for name, v in (("--place X", place[0]), ("--place Y", place[1]), ("--seam", opt.seam)):
        if v < 0 or v % opt.f:
            raise SystemExit("%s %d is not a non-negative multiple of --f %d (the mask lives on latent cells)" % (name, v, opt.f))
    if not opt.init_img:
        raise SystemExit("--init-img is required")
    return grid, place


def keep_masks(size, place, seam, grid, f=8):
    """(keep [1, 1, Hc, Wc], keep_px [1, 1, f Hc, f Wc], (y0, x0) the picture's latent offset): 1 on the footprint of a size x size
    picture at pixel (X, Y) = place, eroded by `seam` pixels on every side that does not lie on the canvas border. The borders of a
    wrapped axis (grid.wrap) are no borders: the canvas goes on behind them, so the seam is eroded there too. A footprint that would
    itself cross the seam is refused like one outside the canvas."""
    X, Y = place
    Hpx, Wpx = grid.Hc * f, grid.Wc * f
    if X + size > Wpx or Y + size > Hpx:
        raise SystemExit("--place %d,%d: the %d x %d picture does not lie inside the %d x %d canvas" % (X, Y, size, size, Hpx, Wpx))
    wx, wy = "x" in grid.wrap, "y" in grid.wrap
    top, bottom = Y + (seam if Y > 0 or wy else 0), Y + size - (seam if Y + size < Hpx or wy else 0)
    left, right = X + (seam if X > 0 or wx else 0), X + size - (seam if X + size < Wpx or wx else 0)
    if top >= bottom or left >= right:
        raise SystemExit("--seam %d leaves nothing of the %d x %d picture kept" % (seam, size, size))
    keep_px = torch.zeros(1, 1, Hpx, Wpx)
    keep_px[:, :, top:bottom, left:right] = 1.0
    keep = torch.zeros(1, 1, grid.Hc, grid.Wc)
    keep[:, :, top // f:bottom // f, left // f:right // f] = 1.0
    if float(keep.min()) == 1.0:
        raise SystemExit("the picture covers the whole %d x %d canvas: nothing to paint" % (Hpx, Wpx))
    return keep, keep_px, (Y // f, X // f)


def main(argv=None):
    opt = build_parser().parse_args(argv)
    grid, place = check_options(opt)
    prompts = _i2i.read_prompts(opt)
    paths = _i2i.image_paths(opt.init_img, len(prompts))
    images = {p: _i2i.load_img(p) for p in dict.fromkeys(paths)}
    size = _i2i.check_images(images)
    keep1, keep_px1, (y0, x0) = keep_masks(size, place, opt.seam, grid, opt.f)
    from sta import datasets
    layouts = datasets.load_layouts(opt.layout) if opt.layout else None
    items = [(i, p, datasets.layout_for(layouts, p, i) or {}, paths[i]) for i, p in enumerate(prompts)]
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
    model = build_sd_v1(dev, dtype, ckpt=ckpt, use_checkpoint=False, clip_tokenizer=opt.clip_tokenizer, real_text_encoder=ckpt is not None,
                        with_encoder=True)
    vae = model.first_stage_model
    vae.encoder.to(memory_format=torch.channels_last)            # NHWC encoder: its convolutions on the HIP kernels
    cls = DPMSolverSampler if opt.dpm_solver else DDIMSampler
    sampler = cls(model, opt_epochs=opt.opt_epochs, loss_model=None, outdir=opt.outdir, save_images=not opt.skip_save,
                  canvas_guidance=_txt2img_common.make_canvas_guidance(opt, model))
    encoder = sampler                                            # the fused encode step lives on the DDIM sampler (its tables)
    if opt.dpm_solver:
        encoder = DDIMSampler(model, opt_epochs=0, save_images=False)
    encoder.make_schedule(opt.ddim_steps, ddim_eta=0.0 if opt.dpm_solver else opt.ddim_eta, verbose=False)
    os.makedirs(opt.outdir, exist_ok=True)
    lat = size // opt.f
    shape = (1, opt.C, lat, lat)
    canvas_shape = (1, opt.C, grid.Hc, grid.Wc)
    print("outpainting a %d x %d picture at %s to a %s canvas (%d windows)" % (size, size, opt.place, opt.canvas, grid.T))

    h_cache = {}

    def encode(batch_paths):
        todo = [p for p in dict.fromkeys(batch_paths) if p not in h_cache]
        if todo:
            with torch.no_grad():
                h = vae.encode_moments_input(torch.cat([images[p] for p in todo]).to(dev))
            for p, hp in zip(todo, h.split(1)):
                h_cache[p] = hp
        return torch.cat([h_cache[p] for p in batch_paths])

    post_noise = {p: _i2i.posterior_noise(opt.seed, shape) for p in images}          # draw 1, one per picture

    def run(group):
        """group: [(index, prompt, layout, path)] with the same object count, as P canvases of one CFG batch."""
        P = len(group)
        h = encode([g[3] for g in group])
        n_post = torch.cat([post_noise[g[3]] for g in group])
        with torch.no_grad():
            # only the clean latent z0 is used: the canvas starts from noise, so the noised latent of index 0 is dropped
            _, z0, _ = encoder.encode_step(h, vae, 0, n_post, torch.zeros((P,) + shape[1:], device=dev), want_z0=True)
        x_T = torch.cat([_i2i.encode_noise(opt.seed, canvas_shape, dev) for _ in group])            # draw 2, one per prompt
        x0c = torch.zeros((P,) + canvas_shape[1:], device=dev)
        x0c[:, :, y0:y0 + lat, x0:x0 + lat] = z0
        orig = torch.zeros(P, 3, grid.Hc * opt.f, grid.Wc * opt.f)
        for k, g in enumerate(group):
            orig[k, :, place[1]:place[1] + size, place[0]:place[0] + size] = (images[g[3]][0] + 1.0) / 2.0
        conds = [conditionings(model, p, list(l.keys()), dtype) for _, p, l, _ in group]
        print("Start outpainting for prompts %s" % [i for i, _, _, _ in group])
        sampler.inpaint_canvas(S=opt.ddim_steps, canvas=(grid.Hc, grid.Wc), window=grid.s, stride=grid.stride,
                               mask=keep1.expand(P, -1, -1, -1).to(dev), x0=x0c, image=orig.to(dev),
                               mask_px=keep_px1.expand(P, -1, -1, -1).to(dev), conditionings=[c[1] for c in conds],
                               unconditional_conditionings=[c[0] for c in conds], bboxs=[[l[n] for n in l] for _, _, l, _ in group],
                               object_names=[list(l.keys()) for _, _, l, _ in group], local_conditionings=[c[2] for c in conds],
                               curr_texts=[p for _, p, _, _ in group], x_T=x_T, unconditional_guidance_scale=opt.scale, eta=opt.ddim_eta,
                               seed=opt.seed, prompt_indices=[i for i, _, _, _ in group], channels=opt.C, wrap=grid.wrap)
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
