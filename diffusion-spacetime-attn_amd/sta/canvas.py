"""Wide and tall canvases sampled as overlapping square windows (MultiDiffusion), host side of csrc/sta_window.hip.

The canvas latent is [P, C, Hc, Wc]. Every UNet call sees T = ny nx square windows of side s of each canvas as T images of one CFG
batch; the T predictions are averaged where windows overlap and the sampler step runs on the canvas.

Grid: offsets along an axis of length L are 0, stride, 2 stride, ... while o + s <= L, plus L - s if that is not already the last one
(the last window is clamped to the edge). s, stride, Hc and Wc are multiples of 8 (every window's 2x / 4x / 8x coarser levels lie on the
canvas's coarse grid, and a lane's 8-element vector never straddles a window edge), s <= Hc, s <= Wc, 8 <= stride <= s (no gaps), at
most MAX_WINDOW_OFFSETS offsets per axis. Window w = j nx + i has its corner at (oy[j], ox[i]). The UNet batch is canvas-major, then
window, then (uncond, cond): row 2 (p T + w) + r, the pair layout of PLMSSampler._make_eps_fn and the fused kernels.

Layout: centres are normalised to the canvas (x in [0, 1] of the width, y of the height); window (j, i) gets
((x Wc - ox[i]) / s, (y Hc - oy[j]) / s), in Python floats, and its blocks rasterise that with the unchanged disc rule (sta.ops.disc_masks):
the disc has radius 0.2 disc_scale s latent pixels in every window (`disc_scale`, a keyword of the samplers' canvas methods, default 1.0:
0.2 s everywhere; an upscaled refine passes the upscale factor, so an object keeps its share of the canvas), and an object outside a
window sets no mask bit there. `check_disc_scale` holds the one extra rule of a wrapped axis.

Fuse: per canvas element the covering windows are summed in ascending w in fp32, starting from the first one's value, and divided by their
count with an IEEE fp32 division; a 16-bit result is rounded to nearest even once. One writer per element: bit-reproducible.

`window_split`, `window_fuse` and `sampler_step_windows` run the HIP kernels for CUDA tensors (there is no other GPU path) and the torch
restatements `window_split_reference`, `window_fuse_reference`, `step_windows_reference` for CPU tensors (explicit loops over the windows
in ascending order): the restatements are what the kernels are tested against and what the CPU suite's sampler tests run on.

Inpainting and outpainting (a solver.Blend with canvas-shaped x0 / noise and keep [P, 1, Hc, Wc]): `window_blend` is the first call's
blend and the split in one launch (sta_window_blend), `sampler_step_windows_masked` the step of call i with the blend of call i + 1 on
x_next (sta_sampler_step_windows_masked); restatements `window_blend_reference` and `step_windows_masked_reference`.

Wrap-around canvases (`window_grid(..., wrap="x" | "y" | "xy")`: a 360 degree panorama closes along x, a tileable image along both axes):
the offsets of a wrapped axis of length L are 0, stride, ..., L - stride (L % stride == 0, L >= 1.5 s), and the window at offset o covers
the canvas positions (o + d) mod L, d = 0 .. s - 1: the last windows run over the seam, so the first and the last column share a UNet
window. Every window sees a centre at the representative nearest to it (`window_centres`), the restatements index modulo L, and the CUDA
dispatchers hand the C entry points the grid's wrap mask; a grid without wrap (mask 0) is the clamped grid above.

img2img on a canvas (`encode_step_windows`, restatement `encode_step_windows_reference`): from the VAE encoder's output on the whole canvas
to the canvas state noised to the decode's start and the first call's window input pairs, one sta_vae_encode_step_windows launch
(sta_vae_encode_step and sta_window_split in one); DDIMSampler.encode_step_canvas / decode_canvas are its users.

The hi-res fix on a canvas (`upscale_step_windows`, restatement `upscale_step_windows_reference`): from a smaller latent, the x0 of a
finished trajectory, to the bilinearly upscaled canvas state noised to the decode's start and the first call's window input pairs, one
sta_latent_upscale_step_windows launch; DDIMSampler.upscale_step_canvas / hires_canvas are its users.

Attention guidance on a canvas (`latent_guide_windows`, restatement `guide_windows_reference`, `guide_count`): the gradient of the
attention-layout energy w.r.t. the window input pairs goes back to the canvas state through the split's adjoint (a sum over the covering
windows), the state steps as in sta.guidance and the next window inputs are written, one sta_latent_guide_windows launch;
sta.guidance.CanvasGuidance is its user.
"""
import ctypes
from collections import namedtuple

import torch

from sta import lib, solver

MAX_WINDOW_OFFSETS = lib.MAX_WINDOW_OFFSETS
Grid = namedtuple("Grid", "Hc Wc s stride oy ox ny nx T wrap", defaults=("",))
WRAPS = {"": 0, "x": 1, "y": 2, "xy": 3}         # Grid.wrap -> the C-ABI's wrap mask (bit 0 = x, bit 1 = y)
_DT = solver._DT


# ---------------------------------------------------------------------------------------------------- grid and layout
def _offsets(L, s, stride):
    o = list(range(0, L - s + 1, stride))
    if o[-1] != L - s:
        o.append(L - s)
    return tuple(o)


def _ring_offsets(L, s, stride, axis):
    """The offsets 0, stride, ..., L - stride of a wrapped axis of length L (the windows behind L - s run over the seam)."""
    if L % stride:
        raise ValueError("wrapped %s axis: length %d is not a multiple of the stride %d (the ring of windows would not close evenly)"
                         % (axis, L, stride))
    if 2 * L < 3 * s:
        raise ValueError("wrapped %s axis: length %d is shorter than 1.5 windows of %d (a disc of diameter 0.4 s could enter one window "
                         "from both sides)" % (axis, L, s))
    return tuple(range(0, L, stride))


def window_grid(Hc, Wc, s, stride, wrap=""):
    """The window grid of an Hc x Wc canvas latent (sides in latent pixels) -> Grid(Hc, Wc, s, stride, oy, ox, ny, nx, T, wrap).
    wrap: "" (the clamped grid), "x", "y" or "xy": the axes that close on themselves."""
    Hc, Wc, s, stride = int(Hc), int(Wc), int(s), int(stride)
    if wrap not in WRAPS:
        raise ValueError("wrap = %r is none of '', 'x', 'y', 'xy' (canvas %d x %d, window %d, stride %d)" % (wrap, Hc, Wc, s, stride))
    for name, v in (("window side s", s), ("stride", stride), ("canvas height Hc", Hc), ("canvas width Wc", Wc)):
        if v <= 0 or v % 8:
            raise ValueError("%s = %d is not a positive multiple of 8 (canvas %d x %d, window %d, stride %d)" % (name, v, Hc, Wc, s, stride))
    if s > Hc or s > Wc:
        raise ValueError("the canvas %d x %d is smaller than the window %d" % (Hc, Wc, s))
    if stride > s:
        raise ValueError("stride %d > window %d would leave gaps between windows" % (stride, s))
    oy = _ring_offsets(Hc, s, stride, "y") if "y" in wrap else _offsets(Hc, s, stride)
    ox = _ring_offsets(Wc, s, stride, "x") if "x" in wrap else _offsets(Wc, s, stride)
    if len(oy) > MAX_WINDOW_OFFSETS or len(ox) > MAX_WINDOW_OFFSETS:
        raise ValueError("canvas %d x %d with window %d and stride %d needs %d x %d window offsets; at most %d per axis"
                         % (Hc, Wc, s, stride, len(oy), len(ox), MAX_WINDOW_OFFSETS))
    return Grid(Hc, Wc, s, stride, oy, ox, len(oy), len(ox), len(oy) * len(ox), wrap)


def windows(grid):
    """[(oy[j], ox[i])] in window order w = j nx + i."""
    return [(y0, x0) for y0 in grid.oy for x0 in grid.ox]


def _centre(u, L, o, s, wrapped):
    """Canvas-normalised coordinate u on an axis of length L -> the window's own coordinate (offset o, side s). Wrapped axis: of the
    images u L + k L the one nearest the window's middle, so an object near the seam is seen by the windows on both sides of it."""
    c = float(u) * L - o
    if wrapped:
        c = ((c - s / 2 + L / 2) % L) + s / 2 - L / 2
    return c / s


def window_centres(centres, grid):
    """Canvas-normalised centres [(x, y)] -> per window (in window order) the list of that window's centres."""
    wx, wy = "x" in grid.wrap, "y" in grid.wrap
    return [[[_centre(x, grid.Wc, x0, grid.s, wx), _centre(y, grid.Hc, y0, grid.s, wy)] for x, y in centres] for y0, x0 in windows(grid)]


def _region(grid, y0, x0, device=None):
    """The index of window (y0, x0) into the last two axes of a canvas tensor: slices on the clamped grid, index tensors modulo the
    axis length on a wrapped one (s <= L: no position twice)."""
    if not grid.wrap:
        return slice(y0, y0 + grid.s), slice(x0, x0 + grid.s)
    ys = (y0 + torch.arange(grid.s, device=device)) % grid.Hc
    xs = (x0 + torch.arange(grid.s, device=device)) % grid.Wc
    return ys[:, None], xs[None, :]


def cover_count(grid):
    """[Hc, Wc] int32: how many windows cover each canvas element (>= 1 everywhere)."""
    n = torch.zeros((grid.Hc, grid.Wc), dtype=torch.int32)
    for y0, x0 in windows(grid):
        n[_region(grid, y0, x0)] += 1
    return n


# ---------------------------------------------------------------------------------------------------- torch restatements
def _canvases(n_rows, rows, what):
    if n_rows % rows:
        raise ValueError("%s holds %d images, not a multiple of %d" % (what, n_rows, rows))
    return n_rows // rows


def window_split_reference(src, grid, dtype=None, rows=1):
    """src [P rows, C, Hc, Wc] -> [2 P T, C, s, s] in `dtype` (default: src's). rows = 1: canvas states, to both rows of each window's
    pair; rows = 2: input pairs, row r to row r."""
    if rows not in (1, 2) or tuple(src.shape[-2:]) != (grid.Hc, grid.Wc):
        raise ValueError("window_split: src %s, rows %s for a %d x %d canvas" % (tuple(src.shape), rows, grid.Hc, grid.Wc))
    P, C, s = _canvases(src.shape[0], rows, "src"), src.shape[1], grid.s
    v = src.to(dtype or src.dtype).reshape(P, rows, C, grid.Hc, grid.Wc)
    out = torch.empty((P, grid.T, 2, C, s, s), dtype=v.dtype, device=src.device)
    for w, (y0, x0) in enumerate(windows(grid)):
        for r in range(2):
            out[:, w, r] = v[:, r if rows == 2 else 0][(Ellipsis,) + _region(grid, y0, x0, src.device)]
    return out.reshape(2 * P * grid.T, C, s, s)


def _fuse32(eps, grid):
    """eps [2 P T, C, s, s] -> the overlap mean [2 P, C, Hc, Wc] in fp32, not rounded."""
    s = grid.s
    if tuple(eps.shape[-2:]) != (s, s):
        raise ValueError("window_fuse: eps %s for windows of side %d" % (tuple(eps.shape), s))
    P, C = _canvases(eps.shape[0], 2 * grid.T, "eps"), eps.shape[1]
    e = eps.reshape(P, grid.T, 2, C, s, s)
    acc = torch.zeros((P, 2, C, grid.Hc, grid.Wc), dtype=torch.float32, device=eps.device)
    seen = torch.zeros((grid.Hc, grid.Wc), dtype=torch.bool, device=eps.device)
    for w, (y0, x0) in enumerate(windows(grid)):
        v = e[:, w].to(torch.float32)
        at = _region(grid, y0, x0, eps.device)
        region = acc[(Ellipsis,) + at]
        acc[(Ellipsis,) + at] = torch.where(seen[at], region + v, v)      # the first covering window's value starts the sum
        seen[at] = True
    return (acc / cover_count(grid).to(eps.device, torch.float32)).reshape(2 * P, C, grid.Hc, grid.Wc)


def window_fuse_reference(eps, grid, dtype=None):
    """eps [2 P T, C, s, s] -> [2 P, C, Hc, Wc] in `dtype` (default: eps's): fp32 sum in ascending w / count, rounded once."""
    return _fuse32(eps, grid).to(dtype or eps.dtype)


def step_windows_reference(eps, x, m_prev, noise, c, grid, dtype=None, want_xin=False):
    """solver.step_reference on the fp32 overlap means of the windows' UNet output -> (x_next, m, xin): x, m_prev, noise, x_next, m are
    canvas tensors [P, C, Hc, Wc]; xin (want_xin) = window_split_reference(x_next) in `dtype` (default: eps's)."""
    x_next, m = solver.step_reference(_fuse32(eps, grid), x, m_prev, noise, c)
    return x_next, m, (window_split_reference(x_next, grid, dtype or eps.dtype) if want_xin else None)


def step_windows_masked_reference(eps, x, m_prev, noise, c, bl, grid, dtype=None, want_xin=False):
    """step_windows_reference for call i, then solver.blend_reference with the blend `bl` of call i + 1 on x_next -> (blended x_next, the
    unblended m, xin): bl a solver.Blend with canvas-shaped x0 / noise and keep [P, 1, Hc, Wc]; xin (want_xin) = the split of the
    BLENDED state."""
    x_next, m, _ = step_windows_reference(eps, x, m_prev, noise, c, grid)
    x_next = solver.blend_reference(x_next, bl)
    return x_next, m, (window_split_reference(x_next, grid, dtype or eps.dtype) if want_xin else None)


def window_blend_reference(x, bl, grid, dtype=None, want_xin=False):
    """The blend of the first call on a canvas state x [P, C, Hc, Wc] -> (x', xin): solver.blend_reference, xin (want_xin) = the split
    of x' in `dtype` (default: x's)."""
    xb = solver.blend_reference(x, bl)
    return xb, (window_split_reference(xb, grid, dtype or x.dtype) if want_xin else None)


def _check_encode(h, n_post, n_enc, grid):
    if h.dim() != 4 or h.shape[1] != 8 or tuple(h.shape[-2:]) != (grid.Hc, grid.Wc):
        raise ValueError("encode_step_windows: h %s must be [P, 8, %d, %d], the encoder's output on the whole canvas" % (tuple(h.shape), grid.Hc, grid.Wc))
    want = (h.shape[0], 4, grid.Hc, grid.Wc)
    if tuple(n_post.shape) != want or tuple(n_enc.shape) != want:
        raise ValueError("encode_step_windows: noises %s / %s must be [P, 4, Hc, Wc] = %s" % (tuple(n_post.shape), tuple(n_enc.shape), want))


def encode_step_windows_reference(h, qw, qb, n_post, n_enc, sf, sa, s1m, grid, dtype=None, want_z0=False, want_xin=True):
    """img2img's entry into a canvas trajectory, restated: the encoder's conv_out result h [P, 8, Hc, Wc] on the whole canvas -> (x, z0,
    xin). float32 arithmetic in the kernel's order per latent pixel (sta_vae_encode_step's): moments = qb + sum_i qw[:, i] h[i] with i
    ascending, logvar clamped to [-30, 20], z0 = sf (mean + exp(logvar / 2) n_post), x = sa z0 + s1m n_enc; x, z0 [P, 4, Hc, Wc] float32
    (z0 None unless want_z0); xin (want_xin) = window_split_reference(x) in `dtype` (default: h's). qw [8, 8] (or the 1x1 conv's
    [8, 8, 1, 1]), qb [8]; sf, sa, s1m Python floats, rounded to float32 as the C-ABI takes them."""
    _check_encode(h, n_post, n_enc, grid)
    f32 = torch.float32
    hf = h.detach().to(f32)
    qw, qb = qw.detach().reshape(8, 8).to(hf.device, f32), qb.detach().reshape(8).to(hf.device, f32)
    n_post, n_enc = n_post.detach().to(hf.device, f32), n_enc.detach().to(hf.device, f32)
    sf, sa, s1m = (torch.tensor(float(v), dtype=f32, device=hf.device) for v in (sf, sa, s1m))
    mo = qb.reshape(1, 8, 1, 1).expand(hf.shape[0], 8, grid.Hc, grid.Wc).clone()
    for i in range(8):
        mo = mo + qw[:, i].reshape(1, 8, 1, 1) * hf[:, i:i + 1]
    z0 = sf * (mo[:, :4] + torch.exp(0.5 * mo[:, 4:].clamp(-30.0, 20.0)) * n_post)
    x = sa * z0 + s1m * n_enc
    return x, (z0 if want_z0 else None), (window_split_reference(x, grid, dtype or h.dtype) if want_xin else None)


def check_disc_scale(grid, disc_scale):
    """disc_scale (discs of radius 0.2 disc_scale window sides) on this grid -> float(disc_scale). ValueError unless it is positive and
    finite, and on a wrapped axis of length L unless L - s >= 0.4 disc_scale s: a disc must not enter one window from both sides (at
    disc_scale 1 the 1.5-window rule of the ring offsets already says so)."""
    d = float(disc_scale)
    if not 0.0 < d < float("inf"):
        raise ValueError("disc_scale = %r must be positive and finite" % (disc_scale,))
    for axis, L in (("x", grid.Wc), ("y", grid.Hc)):
        if axis in grid.wrap and L - grid.s < 0.4 * d * grid.s:
            raise ValueError("wrapped %s axis: length %d leaves %d beside a window of %d, less than a disc's diameter 0.4 x %g x %d (a disc "
                             "could enter one window from both sides)" % (axis, L, L - grid.s, grid.s, d, grid.s))
    return d


def _upscale_taps(L_out, L_in, wrapped, device):
    """The taps and weights of one axis of the bilinear upscale -> (i0, i1 long [L_out], l0, l1 float32 [L_out]); every operation is one
    float32 torch operation, in the kernel's order."""
    f32 = torch.float32
    scale = torch.tensor(float(L_in), dtype=f32, device=device) / torch.tensor(float(L_out), dtype=f32, device=device)
    src = (torch.arange(L_out, dtype=f32, device=device) + 0.5) * scale - 0.5
    if not wrapped:
        src = src.clamp_min(0.0)
    fl = src.floor()
    l1 = src - fl
    l0 = 1.0 - l1
    i0 = fl.to(torch.long)
    if wrapped:
        i0 = i0 % L_in
        i1 = (i0 + 1) % L_in
    else:
        i0 = i0.clamp_max(L_in - 1)
        i1 = (i0 + 1).clamp_max(L_in - 1)
    return i0, i1, l0, l1


def _check_upscale(z, noise, grid):
    if z.dim() != 4 or z.dtype != torch.float32:
        raise ValueError("upscale_step_windows: z must be a float32 latent [P, C, h, w], got %s %s" % (z.dtype, tuple(z.shape)))
    P, C, h, w = z.shape
    if h <= 0 or w <= 0 or h % 8 or w % 8:
        raise ValueError("upscale_step_windows: the source %d x %d is not made of positive multiples of 8" % (h, w))
    if grid.Hc < h or grid.Wc < w:
        raise ValueError("upscale_step_windows: the canvas %d x %d is smaller than the source %d x %d (upscale only)" % (grid.Hc, grid.Wc, h, w))
    if tuple(noise.shape) != (P, C, grid.Hc, grid.Wc):
        raise ValueError("upscale_step_windows: noise %s must be [P, C, Hc, Wc] = %s" % (tuple(noise.shape), (P, C, grid.Hc, grid.Wc)))


def upscale_step_windows_reference(z, noise, sa, s1m, grid, dtype=None, want_z_up=False, want_xin=True):
    """The hi-res fix's entry into a canvas trajectory, restated: z [P, C, h, w] float32 (the x0 of a finished trajectory) -> (x, z_up,
    xin). Per canvas element and axis (output length L_out, source length L_in), float32, one torch operation per rounding, in the
    kernel's order: scale = float32(L_in) / float32(L_out); src = (d + 0.5) scale - 0.5; a clamped axis takes max(src, 0), i0 =
    floor(src), i1 = min(i0 + 1, L_in - 1) — torch.nn.functional.interpolate(mode="bilinear", align_corners=False); a wrapped axis of
    the grid does not clamp and takes both taps modulo L_in (index tensors: the source is itself closed on that axis and the filter
    crosses the seam); l1 = src - i0, l0 = 1 - l1; z_up = l0y (l0x z00 + l1x z01) + l1y (l0x z10 + l1x z11); x = sa z_up + s1m noise.
    x, z_up [P, C, Hc, Wc] float32 (z_up None unless want_z_up); xin (want_xin) = window_split_reference(x) in `dtype` (default: x's).
    sa, s1m Python floats, rounded to float32 as the C-ABI takes them."""
    _check_upscale(z, noise, grid)
    f32 = torch.float32
    z = z.detach()
    noise = noise.detach().to(z.device, f32)
    h, w = z.shape[-2:]
    y0, y1, l0y, l1y = _upscale_taps(grid.Hc, h, "y" in grid.wrap, z.device)
    x0, x1, l0x, l1x = _upscale_taps(grid.Wc, w, "x" in grid.wrap, z.device)
    l0y, l1y = l0y[:, None], l1y[:, None]
    r0, r1 = z[:, :, y0], z[:, :, y1]
    z_up = l0y * (l0x * r0[..., x0] + l1x * r0[..., x1]) + l1y * (l0x * r1[..., x0] + l1x * r1[..., x1])
    sa, s1m = (torch.tensor(float(v), dtype=f32, device=z.device) for v in (sa, s1m))
    x = sa * z_up + s1m * noise
    return x, (z_up if want_z_up else None), (window_split_reference(x, grid, dtype or x.dtype) if want_xin else None)


def guide_count(grid, contributing, C):
    """The `count` of latent_guide_windows: per canvas the number of canvas elements (the C channels included) covered by at least one
    CONTRIBUTING window. contributing [P, T] bool (window order) -> [P] float32. All windows contributing: C Hc Wc; none: 0."""
    contributing = torch.as_tensor(contributing, dtype=torch.bool).reshape(-1, grid.T)
    out = torch.zeros(contributing.shape[0], dtype=torch.float32)
    for p in range(contributing.shape[0]):
        hit = torch.zeros((grid.Hc, grid.Wc), dtype=torch.bool)
        for w, (y0, x0) in enumerate(windows(grid)):
            if contributing[p, w]:
                hit[_region(grid, y0, x0)] = True
        out[p] = float(C * int(hit.sum()))
    return out


def guide_windows_reference(g, x, step, count, grid, keep=None, normalize=True, inv_scale=1.0):
    """The attention-guidance update on a canvas, restated in torch, arithmetic in x's dtype (float64 x: the oracle) -> (x_out, rms [P]).
    g [2 P T, C, s, s]: the gradient w.r.t. the window input pairs; x [P, C, Hc, Wc]; step, count [P] (or numbers); keep [P, 1, Hc, Wc]
    or None. The windows are window_split(x), so the gradient w.r.t. x is the split's adjoint: per canvas element the covering windows'
    (g_u + g_c) summed in ascending w, starting from the first one's value (a sum, not the overlap mean), times (1 - keep);
    rms_p = sqrt(sum d^2 / count[p]), s_p = step_p / rms_p (normalize) or step_p inv_scale, x_out = x - s_p d where rms_p is finite and
    > 0, else x itself. With one window this is sta.guidance.guide_reference."""
    s = grid.s
    if x.dim() != 4 or tuple(x.shape[-2:]) != (grid.Hc, grid.Wc):
        raise ValueError("guide_windows: the state %s is not a [P, C, %d, %d] canvas" % (tuple(x.shape), grid.Hc, grid.Wc))
    P, C = x.shape[0], x.shape[1]
    if tuple(g.shape) != (2 * P * grid.T, C, s, s):
        raise ValueError("g %s must be the gradient of the window pair batch [%d, %d, %d, %d] of x %s" % (tuple(g.shape), 2 * P * grid.T, C, s, s, tuple(x.shape)))
    gw = g.detach().reshape(P, grid.T, 2, C, s, s).to(x.dtype)
    d = torch.zeros_like(x)
    seen = torch.zeros((grid.Hc, grid.Wc), dtype=torch.bool, device=x.device)
    for w, (y0, x0) in enumerate(windows(grid)):
        v = gw[:, w, 0] + gw[:, w, 1]
        at = _region(grid, y0, x0, x.device)
        region = d[(Ellipsis,) + at]
        d[(Ellipsis,) + at] = torch.where(seen[at], region + v, v)          # the first covering window's value starts the sum
        seen[at] = True
    if keep is not None:
        d = d * (1.0 - keep.to(x.device, x.dtype))
    as_p = lambda v: torch.as_tensor(v, dtype=x.dtype, device=x.device).reshape(-1).expand(P)
    rms = (d.reshape(P, -1).square().sum(1) / as_p(count)).sqrt()
    live = torch.isfinite(rms) & (rms > 0)
    step = as_p(step)
    sc = torch.where(live, step / rms if normalize else step * inv_scale, torch.zeros_like(rms))
    b = lambda v: v.reshape(-1, 1, 1, 1)
    return torch.where(b(live), x - b(sc) * d, x), rms


# ---------------------------------------------------------------------------------------------------- HIP entry points
_TABLES = {}


def _grid_args(grid):
    """(ny, nx, oy, ox, s, wrap) as the C-ABI takes them; the host offset arrays are kept per grid."""
    key = (grid.oy, grid.ox)
    if key not in _TABLES:
        _TABLES[key] = ((ctypes.c_int * grid.ny)(*grid.oy), (ctypes.c_int * grid.nx)(*grid.ox))
    oy, ox = _TABLES[key]
    return grid.ny, grid.nx, ctypes.addressof(oy), ctypes.addressof(ox), grid.s, WRAPS[grid.wrap]


def _launch(name, *args):
    lib.check(getattr(lib.load(), name)(*args), name)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _check_state(what, x, grid):
    if x.dtype != torch.float32 or x.dim() != 4 or tuple(x.shape[-2:]) != (grid.Hc, grid.Wc):
        raise ValueError("%s: the state must be a float32 [P, C, %d, %d] canvas, got %s %s" % (what, grid.Hc, grid.Wc, x.dtype, tuple(x.shape)))


def _pairs(P, C, grid, dtype, device):
    """The window pair batch [2 P T, C, s, s] of P canvases, not initialised."""
    return torch.empty((2 * P * grid.T, C, grid.s, grid.s), dtype=dtype, device=device)


def window_split(src, grid, dtype=None, rows=1):
    """window_split_reference on the GPU (sta_window_split): src float32 or already `dtype`, the UNet's 16-bit type."""
    if not src.is_cuda:
        return window_split_reference(src, grid, dtype, rows)
    dtype = dtype or src.dtype
    if dtype not in _DT or src.dtype not in (torch.float32, dtype):
        raise TypeError("sta_window_split writes 16-bit window inputs from float32 or the same 16-bit type (src %s, dtype %s)" % (src.dtype, dtype))
    if rows not in (1, 2) or src.dim() != 4 or tuple(src.shape[-2:]) != (grid.Hc, grid.Wc):
        raise ValueError("window_split: src %s, rows %s for a %d x %d canvas" % (tuple(src.shape), rows, grid.Hc, grid.Wc))
    P, C = _canvases(src.shape[0], rows, "src"), src.shape[1]
    src = src.detach().contiguous()
    xin = _pairs(P, C, grid, dtype, src.device)
    _launch("sta_window_split", src.data_ptr(), xin.data_ptr(), P, rows, C, grid.Hc, grid.Wc, *_grid_args(grid),
            lib.STA_SRC_F32 if src.dtype == torch.float32 else _DT[dtype], _DT[dtype], _stream(src))
    return xin


def window_fuse(eps, grid):
    """window_fuse_reference on the GPU (sta_window_fuse): eps 16-bit, the result in the same type."""
    if not eps.is_cuda:
        return window_fuse_reference(eps, grid)
    if eps.dtype not in _DT:
        raise TypeError("sta_window_fuse takes the UNet's 16-bit output, got %s" % eps.dtype)
    if eps.dim() != 4 or tuple(eps.shape[-2:]) != (grid.s, grid.s):
        raise ValueError("window_fuse: eps %s for windows of side %d" % (tuple(eps.shape), grid.s))
    P, C = _canvases(eps.shape[0], 2 * grid.T, "eps"), eps.shape[1]
    eps = eps.detach().contiguous()
    out = torch.empty((2 * P, C, grid.Hc, grid.Wc), dtype=eps.dtype, device=eps.device)
    _launch("sta_window_fuse", eps.data_ptr(), out.data_ptr(), P, C, grid.Hc, grid.Wc, *_grid_args(grid), _DT[eps.dtype], _stream(eps))
    return out


def sampler_step_windows(eps, x, m_prev, noise, c, grid, dtype=None, want_xin=False):
    """One sampler step on a canvas after a CFG UNet call on its windows -> (x_next, m, xin): eps [2 P T, C, s, s] 16-bit, x / m_prev /
    noise [P, C, Hc, Wc] float32 (m_prev / noise may be None), c a solver.StepCoef; xin (want_xin): the next call's window input pairs.
    CUDA: one sta_sampler_step_windows launch (no autograd: canvases are sampled with fixed weights); CPU: step_windows_reference."""
    if not x.is_cuda:
        return step_windows_reference(eps, x, m_prev, noise, c, grid, dtype, want_xin)
    return _step_windows(eps, x, m_prev, noise, c, None, grid, want_xin)


def _prep_step(what, eps, x, m_prev, noise, c, grid):
    """The shape and dtype checks of a step on a canvas -> (eps, x, m_prev, noise) as the kernel takes them (m_prev / noise None where
    their coefficient is 0)."""
    _check_state(what, x, grid)
    if eps.dtype not in _DT:
        raise TypeError("sta_%s takes the UNet's 16-bit output, got %s" % (what, eps.dtype))
    P, C = x.shape[0], x.shape[1]
    if tuple(eps.shape) != (2 * P * grid.T, C, grid.s, grid.s):
        raise ValueError("eps %s must be the window pair batch [%d, %d, %d, %d] of x %s" % (tuple(eps.shape), 2 * P * grid.T, C, grid.s, grid.s, tuple(x.shape)))
    if c.c_p and m_prev is None or c.c_n and noise is None:
        raise ValueError("c_p / c_n != 0 need m_prev / noise")
    f = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    return eps.detach().contiguous(), x.detach().contiguous(), f(m_prev if c.c_p else None), f(noise if c.c_n else None)


def _step_windows(eps, x, m_prev, noise, c, bl, grid, want_xin):
    """The CUDA side of sampler_step_windows (bl None) and sampler_step_windows_masked (bl a solver.Blend): one launch."""
    what = "sampler_step_windows" if bl is None else "sampler_step_windows_masked"
    eps, x, m_prev, noise = _prep_step(what, eps, x, m_prev, noise, c, grid)
    x_next, m = torch.empty_like(x), torch.empty_like(x)
    xin = torch.empty_like(eps) if want_xin else None
    blend, q = (), ()
    if bl is not None:
        x0, keep, qn, _ = solver._prep_blend(x, bl)
        blend, q = (x0.data_ptr(), keep.data_ptr(), qn.data_ptr()), (bl.q_a, bl.q_b)
    args = (eps.data_ptr(), x.data_ptr(), _ptr(m_prev), _ptr(noise)) + blend + (x_next.data_ptr(), m.data_ptr(), _ptr(xin))
    args += (x.shape[0], x.shape[1], grid.Hc, grid.Wc) + _grid_args(grid) + tuple(c) + q + (_DT[eps.dtype], _stream(x))
    _launch("sta_" + what, *args)
    return x_next, m, xin


def sampler_step_windows_masked(eps, x, m_prev, noise, c, bl, grid, dtype=None, want_xin=False):
    """sampler_step_windows for call i with the inpainting blend `bl` of call i + 1 applied to x_next -> (blended x_next, the unblended m,
    xin of the blended state): bl a solver.Blend with canvas-shaped x0 / noise [P, C, Hc, Wc] and keep [P, 1, Hc, Wc] (1 = keep the
    original). CUDA: one sta_sampler_step_windows_masked launch; CPU: step_windows_masked_reference."""
    if bl is None:
        raise ValueError("sampler_step_windows_masked needs a Blend")
    if not x.is_cuda:
        return step_windows_masked_reference(eps, x, m_prev, noise, c, bl, grid, dtype, want_xin)
    return _step_windows(eps, x, m_prev, noise, c, bl, grid, want_xin)


def window_blend(x, bl, grid, dtype=None, want_xin=False):
    """The inpainting blend of the first call on a canvas state x [P, C, Hc, Wc] float32 -> (x', xin): xin (want_xin) the window input
    pairs of x' in `dtype`, the UNet's 16-bit type. CUDA: one sta_window_blend launch (sta_latent_blend and sta_window_split in one);
    CPU: window_blend_reference."""
    if not x.is_cuda:
        return window_blend_reference(x, bl, grid, dtype, want_xin)
    _check_state("window_blend", x, grid)
    if dtype not in _DT:
        raise TypeError("sta_window_blend writes 16-bit window inputs (dtype %s)" % dtype)
    x0, keep, qn, _ = solver._prep_blend(x, bl)
    x = x.detach().contiguous()
    P, C = x.shape[0], x.shape[1]
    out = torch.empty_like(x)
    xin = _pairs(P, C, grid, dtype, x.device) if want_xin else None
    _launch("sta_window_blend", x.data_ptr(), x0.data_ptr(), keep.data_ptr(), qn.data_ptr(), out.data_ptr(), _ptr(xin), P, C, grid.Hc, grid.Wc,
            *_grid_args(grid), bl.q_a, bl.q_b, _DT[dtype], _stream(x))
    return out, xin


def latent_guide_windows(g, x, step, count, grid, keep=None, normalize=True, inv_scale=1.0, dtype=None, want_xin=False, want_stats=True):
    """One attention-guidance update of a canvas state -> (x_out, xin or None, rms [P] or None): g [2 P T, C, s, s] the gradient w.r.t.
    the window input pairs, x [P, C, Hc, Wc] float32, step / count [P] (or numbers), keep [P, 1, Hc, Wc] or None. CUDA: ONE
    sta_latent_guide_windows launch (g must be the UNet's 16-bit gradient, xin comes in the same type): the adjoint gather,
    sta_latent_guide and sta_window_split in one; CPU: guide_windows_reference and window_split_reference (xin in `dtype`, default g's)."""
    if x.dtype != torch.float32:
        raise TypeError("sampler state x must be float32, got %s" % x.dtype)
    if x.dim() != 4 or tuple(x.shape[-2:]) != (grid.Hc, grid.Wc):
        raise ValueError("latent_guide_windows: the state must be a float32 [P, C, %d, %d] canvas, got %s" % (grid.Hc, grid.Wc, tuple(x.shape)))
    P, C = x.shape[0], x.shape[1]
    if tuple(g.shape) != (2 * P * grid.T, C, grid.s, grid.s):
        raise ValueError("g %s must be the gradient of the window pair batch [%d, %d, %d, %d] of x %s"
                         % (tuple(g.shape), 2 * P * grid.T, C, grid.s, grid.s, tuple(x.shape)))
    if keep is not None and tuple(keep.shape) != (P, 1, grid.Hc, grid.Wc):
        raise ValueError("keep %s must be [P, 1, Hc, Wc] of the state %s" % (tuple(keep.shape), tuple(x.shape)))
    if not x.is_cuda:
        x_out, rms = guide_windows_reference(g, x, step, count, grid, keep, normalize, inv_scale)
        return x_out, (window_split_reference(x_out, grid, dtype or g.dtype) if want_xin else None), (rms if want_stats else None)
    if g.dtype not in _DT:
        raise TypeError("sta_latent_guide_windows takes the gradient in the UNet's 16-bit type, got %s" % g.dtype)
    g, xc = g.detach().contiguous(), x.detach().contiguous()
    kp = None if keep is None else keep.detach().to(x.device, torch.float32).contiguous()
    per_canvas = lambda v: torch.as_tensor(v, dtype=torch.float32, device=x.device).reshape(-1).expand(P).contiguous()
    st, cnt = per_canvas(step), per_canvas(count)
    x_out = torch.empty_like(xc)
    xin = torch.empty_like(g) if want_xin else None
    stats = torch.empty(P, dtype=torch.float32, device=x.device) if want_stats else None
    _launch("sta_latent_guide_windows", g.data_ptr(), xc.data_ptr(), _ptr(kp), st.data_ptr(), cnt.data_ptr(), x_out.data_ptr(), _ptr(xin),
            _ptr(stats), P, C, grid.Hc, grid.Wc, *_grid_args(grid), int(bool(normalize)), float(inv_scale), _DT[g.dtype], _stream(x))
    return x_out, xin, stats


def encode_step_windows(h, qw, qb, n_post, n_enc, sf, sa, s1m, grid, dtype=None, want_z0=False, want_xin=True):
    """The encoder's conv_out result h [P, 8, Hc, Wc] on the whole canvas (16-bit CUDA; taken as NHWC) -> (x, z0, xin): the canvas state
    x [P, 4, Hc, Wc] float32 noised to the decode's start, the posterior's sample z0 (want_z0) and the first UNet call's window input
    pairs xin [2 P T, 4, s, s] (want_xin). CUDA: ONE sta_vae_encode_step_windows launch (sta_vae_encode_step and sta_window_split in
    one); CPU: encode_step_windows_reference."""
    if not h.is_cuda:
        return encode_step_windows_reference(h, qw, qb, n_post, n_enc, sf, sa, s1m, grid, dtype, want_z0, want_xin)
    _check_encode(h, n_post, n_enc, grid)
    if h.dtype not in _DT or (dtype or h.dtype) != h.dtype:
        raise TypeError("sta_vae_encode_step_windows reads 16-bit h and writes window inputs of the same type (h %s, dtype %s)" % (h.dtype, dtype))
    P = h.shape[0]
    h = h.detach().contiguous(memory_format=torch.channels_last)
    f = lambda t: t.detach().to(device=h.device, dtype=torch.float32).contiguous()
    qw, qb, n_post, n_enc = f(qw.reshape(8, 8)), f(qb), f(n_post), f(n_enc)
    x = torch.empty((P, 4, grid.Hc, grid.Wc), dtype=torch.float32, device=h.device)
    z0 = torch.empty_like(x) if want_z0 else None
    xin = _pairs(P, 4, grid, h.dtype, h.device) if want_xin else None
    _launch("sta_vae_encode_step_windows", h.data_ptr(), qw.data_ptr(), qb.data_ptr(), n_post.data_ptr(), n_enc.data_ptr(), x.data_ptr(), _ptr(z0),
            _ptr(xin), P, grid.Hc, grid.Wc, *_grid_args(grid), float(sf), float(sa), float(s1m), _DT[h.dtype], _stream(h))
    return x, z0, xin


def upscale_step_windows(z, noise, sa, s1m, grid, dtype=None, want_z_up=False, want_xin=True):
    """A smaller latent z [P, C, h, w] float32 (the x0 of a finished trajectory, a square image or a canvas) -> (x, z_up, xin): the canvas
    state x [P, C, Hc, Wc] float32, z upscaled bilinearly and noised to the decode's start (x = sa z_up + s1m noise), the upscaled latent
    z_up (want_z_up) and the first UNet call's window input pairs xin [2 P T, C, s, s] in `dtype`, the UNet's 16-bit type (want_xin).
    CUDA: ONE sta_latent_upscale_step_windows launch; CPU: upscale_step_windows_reference."""
    if not z.is_cuda:
        return upscale_step_windows_reference(z, noise, sa, s1m, grid, dtype, want_z_up, want_xin)
    _check_upscale(z, noise, grid)
    if want_xin and dtype not in _DT:
        raise TypeError("sta_latent_upscale_step_windows writes 16-bit window inputs (dtype %s)" % dtype)
    P, C, h, w = z.shape
    z = z.detach().contiguous()
    noise = noise.detach().to(device=z.device, dtype=torch.float32).contiguous()
    x = torch.empty((P, C, grid.Hc, grid.Wc), dtype=torch.float32, device=z.device)
    z_up = torch.empty_like(x) if want_z_up else None
    xin = _pairs(P, C, grid, dtype, z.device) if want_xin else None
    _launch("sta_latent_upscale_step_windows", z.data_ptr(), noise.data_ptr(), x.data_ptr(), _ptr(z_up), _ptr(xin), P, C, h, w, grid.Hc, grid.Wc,
            *_grid_args(grid), float(sa), float(s1m), _DT[dtype] if want_xin else lib.STA_F16, _stream(z))
    return x, z_up, xin
