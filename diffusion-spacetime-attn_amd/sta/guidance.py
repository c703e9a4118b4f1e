"""Attention-guided latent updates during sampling: training-free layout control with the attention-layout energy.

sta.attnloss turns "does object i appear inside disc i" into an energy E of the cross-attention token maps and uses it as a training
signal for the blend weights W over tracked epochs. Cross-attention layout guidance uses the same energy differently: before the
first few UNet calls of ONE trajectory the LATENT steps down the energy's gradient,

    x <- x - s g / rms(g),   s = scale (1 - alpha_cumprod_t),   g = dE / dx,

no epochs, no CLIP, no VAE backward. The heavy pieces exist: the differentiable readout (attnmaps.TokenMapsFn, sta_xattn_token_maps_bwd)
and the input gradients of the trunk (sta.fused.tracked, the attention backwards). Here:

  guide_reference   the update formula in torch (the CPU path and the test oracle)
  latent_guide      CUDA: sta_latent_guide (csrc/sta_guide.hip), CPU: guide_reference
  AttnGuidance      owns an AttnLayoutLoss, evaluates E and dE / d(input pair) with one eager UNet call and applies the update
  CanvasGuidance    the same on a canvas sampled as overlapping windows (sta.canvas): one energy per window image, the gradient w.r.t.
                    the window pairs, the update on the canvas state through sta.canvas.latent_guide_windows

The UNet's input is the 16-bit CFG pair (x, x) per image, so autograd returns the gradient as a pair; dE / dx is the sum of its two
rows, which the kernel forms in fp32 (a 16-bit sum on the host would round once more and cost a launch).

What is NOT claimed: anything about image quality. The update is pinned numerically (tests/test_guidance_*.py); whether guided images
follow their layouts better needs real weights.
"""
import math

import torch

from . import attnloss as _al
from . import fused as _fused
from . import lib

_DT = {torch.bfloat16: lib.STA_BF16, torch.float16: lib.STA_F16}


def _pair(x):
    b = x.shape[0]
    return torch.stack([x, x], dim=1).reshape(2 * b, *x.shape[1:])


def _bcast(v, x):
    return v.reshape(-1, *([1] * (x.dim() - 1)))


def guide_reference(g_pair, x, step, keep=None, normalize=True, inv_scale=1.0):
    """The update in torch, arithmetic in x's dtype (float64 x: the oracle) -> (x_out, rms [b]).
    g_pair [2b, ...]: gradient w.r.t. the CFG input pair; x [b, ...]; step [b] (or a number); keep [b, 1, h, w] or None.
    d = (g[2i] + g[2i+1]) (1 - keep), rms_i = sqrt(mean d^2), s_i = step_i / rms_i (normalize) or step_i inv_scale,
    x_out = x - s_i d where rms_i is finite and > 0, else x itself."""
    b = x.shape[0]
    g = g_pair.detach().reshape(b, 2, *x.shape[1:]).to(x.dtype)
    d = g[:, 0] + g[:, 1]
    if keep is not None:
        d = d * (1.0 - keep.to(x.device, x.dtype))
    rms = d.reshape(b, -1).square().mean(1).sqrt()
    live = torch.isfinite(rms) & (rms > 0)
    step = torch.as_tensor(step, dtype=x.dtype, device=x.device).reshape(-1).expand(b)
    s = torch.where(live, step / rms if normalize else step * inv_scale, torch.zeros_like(rms))
    return torch.where(_bcast(live, x), x - _bcast(s, x) * d, x), rms


def latent_guide(g_pair, x, step, keep=None, normalize=True, inv_scale=1.0, dtype=None, want_xin=False, want_stats=True):
    """One update -> (x_out, xin or None, rms [b] or None). CUDA: sta_latent_guide (g_pair must be the UNet's 16-bit gradient; xin in
    the same type); CPU: guide_reference (xin: the pair of x_out in `dtype`)."""
    if x.dtype != torch.float32:
        raise TypeError("sampler state x must be float32, got %s" % x.dtype)
    b, n = x.shape[0], x[0].numel()
    if g_pair.shape[0] != 2 * b or g_pair[0].numel() != n:
        raise ValueError("g %s must be the gradient of the CFG pair batch of x %s" % (tuple(g_pair.shape), tuple(x.shape)))
    if keep is not None and tuple(keep.shape) != (b, 1) + tuple(x.shape[-2:]):
        raise ValueError("keep %s must be [b, 1, h, w] of the state %s" % (tuple(keep.shape), tuple(x.shape)))
    if not x.is_cuda:
        x_out, rms = guide_reference(g_pair, x, step, keep, normalize, inv_scale)
        return x_out, (_pair(x_out).to(dtype or g_pair.dtype) if want_xin else None), (rms if want_stats else None)
    if g_pair.dtype not in _DT:
        raise TypeError("sta_latent_guide takes the gradient in the UNet's 16-bit type, got %s" % g_pair.dtype)
    g = g_pair.detach().contiguous()
    xc = x.detach().contiguous()
    kp = None if keep is None else keep.detach().to(x.device, torch.float32).contiguous()
    st = torch.as_tensor(step, dtype=torch.float32, device=x.device).reshape(-1).expand(b).contiguous()
    hw = x.shape[-2] * x.shape[-1] if x.dim() >= 3 else n
    x_out = torch.empty_like(xc)
    xin = torch.empty_like(g) if want_xin else None
    stats = torch.empty(b, dtype=torch.float32, device=x.device) if want_stats else None
    ptr = lambda t: 0 if t is None else t.data_ptr()
    lib.check(lib.load().sta_latent_guide(g.data_ptr(), xc.data_ptr(), ptr(kp), st.data_ptr(), x_out.data_ptr(), ptr(xin), ptr(stats), b, n, hw,
                                          int(bool(normalize)), float(inv_scale), _DT[g.dtype], torch.cuda.current_stream(x.device).cuda_stream),
              "sta_latent_guide")
    return x_out, xin, stats


def loss_scale_for(dtype, value):
    """The project's loss-scale rule (PLMSSampler._loss_scale): 1 unless the backward runs in fp16; there the power of two that brings
    the scaled loss to [2^15, 2^16)."""
    if dtype != torch.float16 or not (0.0 < abs(value) < float("inf")):
        return 1.0
    return float(2.0 ** min(max(math.floor(math.log2(65536.0 / abs(value))), 0), 60))


class AttnGuidance:
    """Latent guidance of one sampler (`latent_guidance=` of PLMSSampler / DDIMSampler / DPMSolverSampler).

    The first `steps` UNet calls of a trajectory that runs without autograd are each preceded by `iters` updates. One update: the
    input pair becomes a leaf, ONE eager UNet call runs under autograd with the AttnLayoutLoss attached and the tracked glue ops
    (sta.fused.tracked), E [I] is taken, grad(sum E x loss scale, pair) goes through latent_guide with step_i = scale (1 - acp_t);
    images whose E <= threshold get step 0. fp16: the loss scale is the project's rule; with normalize=True it cancels in the
    kernel, otherwise inv_scale undoes it. An image whose gradient is not finite (or exactly 0) is skipped and counted.

    blocks="down": only the recording blocks of the encoder side (UNetModel.input_blocks) feed the energy and the evaluation's
    forward stops right behind the q of the last of them — no mid block, no decoder. blocks="all": every block at the resolution,
    the whole forward. The refusals are AttnLayoutLoss's (it owns one and uses its begin / readouts / discs / take_call).

    result(): dict(calls=[(call, iteration)], energy [n, I] (E BEFORE each update), rms [n, I] (of the unscaled gradient),
    skipped=int). With iters >= 2 the energy of iteration j + 1 is the energy after update j."""

    def __init__(self, unet, resolution=16, scale=0.1, steps=10, iters=1, threshold=0.0, normalize=True, blocks="down", tokenize=None):
        if blocks not in ("down", "all"):
            raise ValueError("blocks must be 'down' or 'all', got %r" % (blocks,))
        if steps < 0 or iters < 1 or not scale >= 0:
            raise ValueError("need steps >= 0, iters >= 1 and scale >= 0 (got %s, %s, %s)" % (steps, iters, scale))
        self.unet, self.resolution, self.scale, self.steps, self.iters = unet, int(resolution), float(scale), int(steps), int(iters)
        self.threshold, self.normalize, self.blocks = float(threshold), bool(normalize), blocks
        self._encoder = self._encoder_blocks(unet)           # [(block, downsampling factor of its level)]
        enc = {id(b) for b, _ in self._encoder}
        self.loss = _al.AttnLayoutLoss(unet, resolution=resolution, tokenize=tokenize,
                                       block_filter=(lambda blk: id(blk) in enc) if blocks == "down" else None)
        self.ready = False
        self._call = None
        self._rec = []

    @staticmethod
    def _encoder_blocks(unet):
        from ldm.modules.attention import BasicTransformerBlock
        from ldm.modules.diffusionmodules.openaimodel import Downsample
        out, ds = [], 1
        for stage in unet.input_blocks:
            out += [(m, ds) for m in stage.modules() if isinstance(m, BasicTransformerBlock)]
            if any(isinstance(m, Downsample) for m in stage):
                ds *= 2
        return out

    @property
    def enabled(self):
        return self.steps > 0 and self.scale > 0

    # -- what the sampler calls ---------------------------------------------------------------------
    def begin(self, centres, texts=None, names=None):
        """A new trajectory: the readouts and discs of its prompts. Prompts without objects are not guided (`ready` stays False)."""
        self._rec, self._call, self.ready = [], None, False
        if not self.enabled:
            return self
        self.loss.begin(centres, texts=texts, names=names, n_calls=1)
        self.ready = self.loss.sel_ctx is not None
        return self

    def bind(self, call):
        """call(pair, t, coef): one eager CFG UNet call of the trajectory being sampled."""
        self._call = call
        return self

    def _last_block(self, side):
        if side % self.resolution:
            raise RuntimeError("a %d x %d latent has no level of side %d" % (side, side, self.resolution))
        hit = [b for b, ds in self._encoder if ds == side // self.resolution]
        if not hit:
            raise RuntimeError("no encoder-side transformer block works at %d x %d in this UNet (latent side %d)"
                               % (self.resolution, self.resolution, side))
        return hit[-1]

    def update(self, x, xin, t, coef, call_index, alpha_cumprod_t, keep=None):
        """`iters` updates before UNet call `call_index` at time t -> (x, xin). x [I, C, h, w] fp32; xin: its 16-bit pair or None (then
        the pair is formed here in the UNet's dtype and None is returned); keep [I, 1, h, w] or None."""
        if self._call is None:
            raise RuntimeError("AttnGuidance.update needs bind(call) first (the sampler does that per trajectory)")
        loss = self.loss
        wdtype = next(self.unet.parameters()).dtype
        step_size = self.scale * (1.0 - float(alpha_cumprod_t))
        for it in range(self.iters):
            pair = (xin if xin is not None else _pair(x).to(wdtype)).detach().requires_grad_(True)
            loss.stop_after = self._last_block(x.shape[-1]) if self.blocks == "down" else None
            try:
                with torch.enable_grad(), _fused.tracked(True), loss:
                    try:
                        self._call(pair, t, coef)
                    except _al._EarlyExit:
                        pass
                    energy = loss.take_call()                              # [I], an autograd value of this call alone
                    if energy is None:
                        raise RuntimeError("the guidance recorded nothing: no %stransformer block works at %d x %d in this UNet"
                                           % ("encoder-side " if self.blocks == "down" else "", self.resolution, self.resolution))
                    total = energy.sum()
                    ls = loss_scale_for(wdtype, float(total.detach())) if wdtype == torch.float16 else 1.0
                    (g,) = torch.autograd.grad(total * ls if ls != 1.0 else total, pair)
            finally:
                loss.stop_after = None
            e = energy.detach().float()
            step = torch.where(e > self.threshold, torch.full_like(e, step_size), torch.zeros_like(e))
            x, new_xin, rms = latent_guide(g, x, step, keep=keep, normalize=self.normalize, inv_scale=1.0 / ls, dtype=wdtype,
                                           want_xin=xin is not None)
            xin = new_xin if xin is not None else None
            self._rec.append((int(call_index), it, e, rms / ls))
        return x, xin

    def result(self):
        """What the trajectory's updates saw (see the class docstring), or None if nothing was guided."""
        if not self._rec:
            return None
        energy = torch.stack([r[2] for r in self._rec]).cpu()
        rms = torch.stack([r[3] for r in self._rec]).cpu()
        skipped = int((~(torch.isfinite(rms) & (rms > 0))).sum())
        return dict(calls=[(r[0], r[1]) for r in self._rec], energy=energy, rms=rms, skipped=skipped)


class CanvasGuidance(AttnGuidance):
    """Latent guidance of a canvas trajectory (`canvas_guidance=` of the samplers: sample_canvas, inpaint_canvas, decode_canvas; never
    used by sample / sample_batch). Same constructor as AttnGuidance; `resolution` must be a level of the WINDOW.

    The evaluation is the canvas trajectory's own UNet call run eagerly: the 2 P T window rows, every window with its own centres. The
    loss is begun on the per-window centres (sta.canvas.window_centres, batch order p T + w) with disc_required=True: a window in which
    no disc has a set pixel at the recording resolution has no valid readout, gives exactly 0 and no gradient — it is NON-CONTRIBUTING.
        E[p] = sum_w E[p, w] / max(1, number of contributing windows of p);   differentiated: sum_p sum_w E[p, w] x the fp16 loss scale
    The gradient w.r.t. the window pairs goes through sta.canvas.latent_guide_windows (the split's adjoint: a sum over the covering
    windows) with step_p = scale (1 - acp_t), 0 where E[p] <= threshold, and count_p = the canvas elements covered by a contributing
    window, so that the part of the canvas that receives gradient moves by step_p in rms.

    result(): dict(calls=[(call, iteration)], energy [n, P], window_energy [n, P, T], rms [n, P], skipped=int)."""

    grid = contributing = None

    def begin(self, centres, texts=None, names=None, grid=None):
        """A new canvas trajectory: centres normalised to the canvas, per canvas; texts / names per canvas (repeated per window here)."""
        from . import canvas as _cv
        self._rec, self._call, self.ready, self.grid, self.contributing, self._counts = [], None, False, grid, None, {}
        if not self.enabled:
            return self
        if grid is None:
            raise ValueError("CanvasGuidance.begin needs grid= (the sta.canvas.Grid of the trajectory)")
        if grid.s % self.resolution:
            raise ValueError("a %d x %d window has no level of side %d" % (grid.s, grid.s, self.resolution))
        P = len(centres)
        rep = lambda v: None if v is None else [v[p] for p in range(P) for _ in range(grid.T)]
        self.loss.begin([wc for bx in centres for wc in _cv.window_centres(bx, grid)], texts=rep(texts), names=rep(names), n_calls=1,
                        disc_required=True)
        self.ready = self.loss.sel_ctx is not None
        if self.ready:
            self.contributing = self.loss._valid.any(1).reshape(P, grid.T).cpu()
        return self

    def _count(self, C, device):
        from . import canvas as _cv
        if (C, device) not in self._counts:
            self._counts[(C, device)] = _cv.guide_count(self.grid, self.contributing, C).to(device)
        return self._counts[(C, device)]

    def update(self, x, xin, t, coef, call_index, alpha_cumprod_t, keep=None):
        """`iters` updates before UNet call `call_index` -> (x, xin). x [P, C, Hc, Wc] fp32; xin: the 16-bit window input pairs
        [2 P T, C, s, s] or None (then they are split here in the UNet's dtype and None is returned); t [P] / coef [P, K] belong to the
        canvases (the bound call repeats them per window); keep [P, 1, Hc, Wc] or None."""
        from . import canvas as _cv
        if self._call is None:
            raise RuntimeError("CanvasGuidance.update needs bind(call) first (the sampler does that per trajectory)")
        loss, grid = self.loss, self.grid
        P, T = x.shape[0], grid.T
        wdtype = next(self.unet.parameters()).dtype
        step_size = self.scale * (1.0 - float(alpha_cumprod_t))
        n_contrib = self.contributing.sum(1).clamp(min=1).to(x.device, torch.float32)
        count = self._count(x.shape[1], x.device)
        for it in range(self.iters):
            pair = (xin if xin is not None else _cv.window_split(x, grid, wdtype)).detach().requires_grad_(True)
            loss.stop_after = self._last_block(grid.s) if self.blocks == "down" else None
            try:
                with torch.enable_grad(), _fused.tracked(True), loss:
                    try:
                        self._call(pair, t, coef)
                    except _al._EarlyExit:
                        pass
                    energy = loss.take_call()                              # [P T], one energy per window image
                    if energy is None:
                        raise RuntimeError("the guidance recorded nothing: no %stransformer block works at %d x %d in this UNet"
                                           % ("encoder-side " if self.blocks == "down" else "", self.resolution, self.resolution))
                    total = energy.sum()
                    ls = loss_scale_for(wdtype, float(total.detach())) if wdtype == torch.float16 else 1.0
                    (g,) = torch.autograd.grad(total * ls if ls != 1.0 else total, pair)
            finally:
                loss.stop_after = None
            ew = energy.detach().float().reshape(P, T)
            e = ew.sum(1) / n_contrib
            step = torch.where(e > self.threshold, torch.full_like(e, step_size), torch.zeros_like(e))
            x, new_xin, rms = _cv.latent_guide_windows(g, x, step, count, grid, keep=keep, normalize=self.normalize, inv_scale=1.0 / ls,
                                                       dtype=wdtype, want_xin=xin is not None)
            xin = new_xin if xin is not None else None
            self._rec.append((int(call_index), it, e, rms / ls, ew))
        return x, xin

    def result(self):
        out = super().result()
        if out is not None:
            out["window_energy"] = torch.stack([r[4] for r in self._rec]).cpu()
        return out
