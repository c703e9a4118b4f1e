// sta_window.hip — wide canvases sampled as overlapping square windows (gfx950). C-ABI in include/sta_unet.h (sta_window_split /
// sta_window_fuse / sta_sampler_step_windows / sta_sampler_step_windows_masked / sta_window_blend / sta_vae_encode_step_windows /
// sta_latent_guide_windows / sta_latent_upscale_step_windows; each takes `wrap`, the mask of the axes on which the canvas closes on
// itself, which the kernels take at compile time as WRAP: 0 = the clamped grid). #included at the end of sta_sampler.hip (its flags: no
// fast-math flag of any kind, the overlap mean relies on hipcc's correctly rounded fp32 division). The step on the overlap means is
// step1 of sta_step_dev.h, the definition the square kernels use, with that header's V8T / F4 / load8 / store8 / round8 / StepCoef.
// Conventions of sta_sampler.hip: 256-lane groups, grid-stride, a lane owns 8 consecutive elements of one CANVAS row, 16-byte loads and
// stores, fp32 arithmetic. Window sides, offsets and canvas sides are multiples of 8, so a lane's vector lies inside or outside a window
// as a whole. The offset tables travel by value in the kernel arguments: nothing device-side to fill, the launches are capturable.
// A canvas element is owned by exactly one lane, which visits the windows that cover it in ascending w = j nx + i: no atomics, no LDS,
// one writer per output element, the same bits from launch to launch.
// Inpainting on a canvas (sta_sampler_step_windows_masked / sta_window_blend): the blend is blend1 of sta_blend_dev.h, the definition
// sta_inpaint.hip uses for square images.
// img2img on a canvas (sta_vae_encode_step_windows): from the encoder's output on the whole canvas to the canvas
// state and the first call's window inputs in one launch; the per-pixel arithmetic is sta_encode_dev.h's, the definition
// sta_vae_encode_step (sta_encode.hip) uses for square images.
// Attention guidance on a canvas (sta_latent_guide_windows): the adjoint of the split applied to the window pairs'
// gradient, then sta_latent_guide's update (sta_guide.hip, included before this file: its guide_overlap and GUIDE_MAX_PARTS) and the split.
// The hi-res fix on a canvas (sta_latent_upscale_step_windows): a smaller latent upscaled bilinearly to the canvas
// (on a wrapped axis across the seam), noised with sta_encode_dev.h's noise1 and split, one launch.

#include "sta_blend_dev.h"
#include "sta_encode_dev.h"
#include "sta_step_dev.h"

namespace {

struct WinGrid {
  int ny, nx, s;
  int oy[STA_MAX_WINDOW_OFFSETS], ox[STA_MAX_WINDOW_OFFSETS];
};

// vector v of a [rows][C][Hc][Wc] tensor -> its row (image), channel and the position of its first element
struct CanvasPos {
  long row;
  int c, y, x;
};

__device__ __forceinline__ CanvasPos canvas_pos(long v, int C, int Hc, int wvec) {
  CanvasPos p;
  const long line = v / wvec;
  p.x = (int)(v - line * wvec) * 8;
  const long plane = line / Hc;
  p.y = (int)(line - plane * Hc);
  p.row = plane / C;
  p.c = (int)(plane - p.row * C);
  return p;
}

// first element of the lane's vector inside image `img` of a [.][C][s][s] window tensor; (dy, dx) = position inside the window
__device__ __forceinline__ long window_at(long img, int C, int c, int s, int dy, int dx) {
  return ((img * C + c) * s + dy) * (long)s + dx;
}

// position of canvas coordinate `at` inside the window at offset o of an axis of length L: on a cyclic axis (WRAPPED) the window covers
// (o + d) mod L for d = 0 .. s - 1, so a negative distance is taken once round the ring (d < 0 ? d + L : d, on the sign bits: no lane
// mask); the window covers `at` iff (unsigned)d < s
template <bool WRAPPED>
__device__ __forceinline__ int window_dist(int at, int o, int L) {
  int d = at - o;
  if constexpr (WRAPPED) d += (d >> 31) & L;
  return d;
}

// The windows that cover the lane's vector at q, visited in ascending w = j nx + i: body(j, i, dy, dx) with (dy, dx) the vector's position
// inside window (j, i). The one statement of the rule that the bit-for-bit determinism of every canvas launch rests on.
// WRAP: the cyclic axes, bit 0 = x (length Wc), bit 1 = y (length Hc); 0 = the clamped grid.
// The bodies are lambdas marked always_inline, so that walk and body are inlined in the same pass (profiles/window_one_entry.md).
template <int WRAP, typename F>
__device__ __forceinline__ void for_covering_windows(const WinGrid& g, int Hc, int Wc, const CanvasPos& q, F&& body) {
  for (int j = 0; j < g.ny; ++j) {
    const int dy = window_dist<(WRAP & 2) != 0>(q.y, g.oy[j], Hc);
    if ((unsigned)dy >= (unsigned)g.s) continue;
    for (int i = 0; i < g.nx; ++i) {
      const int dx = window_dist<(WRAP & 1) != 0>(q.x, g.ox[i], Wc);
      if ((unsigned)dx >= (unsigned)g.s) continue;
      body(j, i, dy, dx);
    }
  }
}

// sum over the covering windows of pair row r (fp32, starting from the first one's value) -> count
template <typename T, int WRAP>
__device__ __forceinline__ int gather_sum(const T* __restrict__ eps, const WinGrid& g, long p, int r, int C, int Hc, int Wc, const CanvasPos& q,
                                          float* acc) {
  using V8 = typename V8T<T>::type;
  const long T_ = (long)g.ny * g.nx;
  int n = 0;
  for_covering_windows<WRAP>(g, Hc, Wc, q, [&](int j, int i, int dy, int dx) __attribute__((always_inline)) {
    const V8 e = *(const V8*)(eps + window_at(2 * (p * T_ + j * g.nx + i) + r, C, q.c, g.s, dy, dx));
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = n ? acc[k] + (float)e[k] : (float)e[k];
    ++n;
  });
  return n;
}

// o -> rows r0 .. r1 of the pair of every covering window
template <typename T, int WRAP>
__device__ __forceinline__ void scatter(T* __restrict__ xin, const WinGrid& g, long p, int r0, int r1, int C, int Hc, int Wc, const CanvasPos& q,
                                        const typename V8T<T>::type o) {
  using V8 = typename V8T<T>::type;
  const long T_ = (long)g.ny * g.nx;
  for_covering_windows<WRAP>(g, Hc, Wc, q, [&](int j, int i, int dy, int dx) __attribute__((always_inline)) {
    for (int r = r0; r <= r1; ++r) *(V8*)(xin + window_at(2 * (p * T_ + j * g.nx + i) + r, C, q.c, g.s, dy, dx)) = o;
  });
}

// src [P rows][C][Hc][Wc] (S = float or T) -> xin [2 P T][C][s][s]; rows == 1: the canvas state goes to both rows of every pair
template <typename S, typename T, int WRAP>
__global__ __launch_bounds__(256) void window_split_kernel(const S* __restrict__ src, T* __restrict__ xin, long nvec, int rows, int C, int Hc,
                                                           int Wc, WinGrid g) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const CanvasPos q = canvas_pos(v, C, Hc, Wc / 8);
    V8 o;
    if constexpr (sizeof(S) == 4) {
      float f[8];
      load8((const float*)src + 8 * v, f);
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = (T)f[k];
    } else {
      o = ((const V8*)src)[v];
    }
    const int r = rows == 2 ? (int)(q.row & 1) : 0;
    scatter<T, WRAP>(xin, g, rows == 2 ? q.row >> 1 : q.row, r, rows == 2 ? r : 1, C, Hc, Wc, q, o);
  }
}

// eps [2 P T][C][s][s] -> out [2 P][C][Hc][Wc]: the mean over the covering windows, fp32 sum / count, rounded once
template <typename T, int WRAP>
__global__ __launch_bounds__(256) void window_fuse_kernel(const T* __restrict__ eps, T* __restrict__ out, long nvec, int C, int Hc, int Wc,
                                                          WinGrid g) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const CanvasPos q = canvas_pos(v, C, Hc, Wc / 8);
    float acc[8] = {};
    const float cnt = (float)gather_sum<T, WRAP>(eps, g, q.row >> 1, (int)(q.row & 1), C, Hc, Wc, q, acc);
    V8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (T)(acc[k] / cnt);
    ((V8*)out)[v] = o;
  }
}

// sampler_step_kernel on the overlap means of the windows' UNet output (fp32, not rounded): the same step1;
// xin (null = not written): the rounded x_next to both rows of every covering window, the next call's input
template <typename T, int WRAP>
__global__ __launch_bounds__(256) void sampler_step_windows_kernel(const T* __restrict__ eps, const float* __restrict__ x,
                                                                   const float* __restrict__ m_prev, const float* __restrict__ noise,
                                                                   float* __restrict__ x_next, float* __restrict__ m, T* __restrict__ xin,
                                                                   long nvec, int C, int Hc, int Wc, WinGrid g, StepCoef c) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const CanvasPos q = canvas_pos(v, C, Hc, Wc / 8);
    float eu[8] = {}, ec[8] = {};
    const float cnt = (float)gather_sum<T, WRAP>(eps, g, q.row, 0, C, Hc, Wc, q, eu);
    gather_sum<T, WRAP>(eps, g, q.row, 1, C, Hc, Wc, q, ec);
    float xv[8], mp[8], nz[8], xn[8], mv[8];
    load8(x + 8 * v, xv);
    if (m_prev) load8(m_prev + 8 * v, mp);
    if (noise) load8(noise + 8 * v, nz);
#pragma unroll
    for (int k = 0; k < 8; ++k) xn[k] = step1(eu[k] / cnt, ec[k] / cnt, xv[k], mp + k, nz + k, m_prev, noise, c, mv[k]);
    store8(x_next + 8 * v, xn);
    store8(m + 8 * v, mv);
    if (xin) scatter<T, WRAP>(xin, g, q.row, 0, 1, C, Hc, Wc, q, round8<T>(xn));
  }
}

// first element of the lane's vector in a [P][Hc][Wc] mask, broadcast over the channels
__device__ __forceinline__ long mask_at(const CanvasPos& q, int Hc, int Wc) { return (q.row * Hc + q.y) * (long)Wc + q.x; }

// sampler_step_windows_kernel for call i (the same step1), then the inpainting blend of call i + 1 on x_next
// (blend1 of sta_blend_dev.h, as sampler_step_masked_kernel): x0 / qnoise canvas-shaped, keep [P][Hc][Wc]; m is the unblended data
// prediction; xin (null = not written): the rounded BLENDED x_next to both rows of every covering window. MP / NZ: m_prev / noise are
// given — compile-time here, since the three extra streams leave no scalar registers for the run-time tests' masks
template <typename T, bool MP, bool NZ, int WRAP>
__global__ __launch_bounds__(256) void sampler_step_windows_masked_kernel(const T* __restrict__ eps, const float* __restrict__ x,
                                                                          const float* __restrict__ m_prev, const float* __restrict__ noise,
                                                                          const float* __restrict__ x0, const float* __restrict__ keep,
                                                                          const float* __restrict__ qnoise, float* __restrict__ x_next,
                                                                          float* __restrict__ m, T* __restrict__ xin, long nvec, int C, int Hc,
                                                                          int Wc, WinGrid g, StepCoef c, float q_a, float q_b) {
  using V8 = typename V8T<T>::type;
  if constexpr (WRAP != 0) {      // the ring arithmetic costs this kernel its last scalar registers: the ten coefficients move to vector ones
    c = coef_in_vgprs(c);
    q_a = in_vgpr(q_a), q_b = in_vgpr(q_b);
  }
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const CanvasPos q = canvas_pos(v, C, Hc, Wc / 8);
    float eu[8] = {}, ec[8] = {};
    const float cnt = (float)gather_sum<T, WRAP>(eps, g, q.row, 0, C, Hc, Wc, q, eu);
    gather_sum<T, WRAP>(eps, g, q.row, 1, C, Hc, Wc, q, ec);
    float xv[8], mp[8], nz[8], xn[8], mv[8], z0[8], kp[8], qn[8];
    load8(x + 8 * v, xv);
    if constexpr (MP) load8(m_prev + 8 * v, mp);
    if constexpr (NZ) load8(noise + 8 * v, nz);
    load8(x0 + 8 * v, z0);
    load8(qnoise + 8 * v, qn);
    load8(keep + mask_at(q, Hc, Wc), kp);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float t = step1(eu[k] / cnt, ec[k] / cnt, xv[k], mp + k, nz + k, MP, NZ, c, mv[k]);
      xn[k] = blend1(kp[k], z0[k], qn[k], t, q_a, q_b);
    }
    store8(x_next + 8 * v, xn);
    store8(m + 8 * v, mv);
    if (xin) scatter<T, WRAP>(xin, g, q.row, 0, 1, C, Hc, Wc, q, round8<T>(xn));
  }
}

// the blend of the first call on a canvas, then the split: latent_blend_kernel and window_split_kernel (rows = 1) in one pass
template <typename T, int WRAP>
__global__ __launch_bounds__(256) void window_blend_kernel(const float* __restrict__ x, const float* __restrict__ x0,
                                                           const float* __restrict__ keep, const float* __restrict__ noise,
                                                           float* __restrict__ x_out, T* __restrict__ xin, long nvec, int C, int Hc, int Wc,
                                                           WinGrid g, float q_a, float q_b) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const CanvasPos q = canvas_pos(v, C, Hc, Wc / 8);
    float xv[8], z0[8], kp[8], qn[8], xo[8];
    load8(x + 8 * v, xv);
    load8(x0 + 8 * v, z0);
    load8(noise + 8 * v, qn);
    load8(keep + mask_at(q, Hc, Wc), kp);
#pragma unroll
    for (int k = 0; k < 8; ++k) xo[k] = blend1(kp[k], z0[k], qn[k], xv[k], q_a, q_b);
    store8(x_out + 8 * v, xo);
    if (xin) scatter<T, WRAP>(xin, g, q.row, 0, 1, C, Hc, Wc, q, round8<T>(xo));
  }
}

// img2img on a canvas: vae_encode_step_kernel (sta_encode.hip) on the whole canvas's encoder output, then the split — the same
// quant_moments / encode1 of sta_encode_dev.h per latent pixel, and window_split_kernel's (rows = 1) scatter of the rounded x.
// h [P][Hc][Wc][8] T (NHWC); n_post, n_enc, x, z0 [P][4][Hc][Wc] fp32 (z0 null = not written); xin (null = not written) [2 P T][4][s][s].
// A lane owns 8 consecutive canvas pixels of one row (vector v of [P][Hc][Wc / 8]): their 8 x 8 channels are 128 contiguous bytes of h,
// eight 16-byte loads; per latent channel it then reads the two noises' and writes x's (z0's) 8-vector and hands the rounded one to scatter.
template <typename T, int WRAP>
__global__ __launch_bounds__(256) void vae_encode_step_windows_kernel(const T* __restrict__ h, const float* __restrict__ qw,
                                                                      const float* __restrict__ qb, const float* __restrict__ n_post,
                                                                      const float* __restrict__ n_enc, float* __restrict__ x,
                                                                      float* __restrict__ z0, T* __restrict__ xin, long nvec, int Hc, int Wc,
                                                                      WinGrid g, float scale_factor, float sqrt_a, float sqrt_1ma) {
  using V8 = typename V8T<T>::type;
  QuantConv qc;
  quant_conv_load(qc, qw, qb);
#pragma unroll
  for (int o = 0; o < 8; ++o) {   // the offset tables fill the scalar file: the 72 quant_conv constants live in vector registers
    qc.bias[o] = in_vgpr(qc.bias[o]);
#pragma unroll
    for (int i = 0; i < 8; ++i) qc.w[o][i] = in_vgpr(qc.w[o][i]);
  }
  const int wvec = Wc / 8;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long line = v / wvec;                            // p Hc + y
    CanvasPos q;
    q.x = (int)(v - line * wvec) * 8;
    q.row = line / Hc;
    q.y = (int)(line - q.row * Hc);
    const V8* hp = (const V8*)h + 8 * v;                   // pixel (p, y, x) of h is its vector line Wc + x = 8 v
    float mo[8][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) quant_moments<T>(qc, hp[k], mo[k]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      q.c = c;
      const long at = ((q.row * 4 + c) * Hc + q.y) * (long)Wc + q.x;
      float np[8], ne[8], xx[8], zz[8];
      load8(n_post + at, np);
      load8(n_enc + at, ne);
#pragma unroll
      for (int k = 0; k < 8; ++k) xx[k] = encode1(mo[k][c], mo[k][4 + c], np[k], ne[k], scale_factor, sqrt_a, sqrt_1ma, zz[k]);
      store8(x + at, xx);
      if (z0) store8(z0 + at, zz);
      if (xin) scatter<T, WRAP>(xin, g, q.row, 0, 1, 4, Hc, Wc, q, round8<T>(xx));
    }
  }
}

// The hi-res fix on a canvas (sta_latent_upscale_step_windows): a finished trajectory's latent, upscaled
// bilinearly to the canvas, noised to the decode's start and split, one launch.
// The two taps and weights of output position d on one axis (source length L_in, scale = (float)L_in / (float)L_out, the host's):
// src = (d + 0.5) scale - 0.5; a clamped axis takes max(src, 0), i0 = floor(src), i1 = min(i0 + 1, L_in - 1) — the rule of
// torch.nn.functional.interpolate(mode="bilinear", align_corners=False); a WRAPPED axis does not clamp and takes both taps modulo L_in
// (i0 lies in -1 .. L_in - 1: one conditional step each, no division), so the filter crosses the seam of a source that is itself a
// ring. l1 = src - i0 (before the wrap), l0 = 1 - l1. Every operation is rounded on its own: no contraction in these two functions.
struct Tap {
  int i0, i1;
  float l0, l1;
};

template <bool WRAPPED>
__device__ __forceinline__ Tap upscale_tap(int d, float scale, int L_in) {
#pragma clang fp contract(off)
  float src = ((float)d + 0.5f) * scale;
  src = src - 0.5f;
  if constexpr (!WRAPPED) src = fmaxf(src, 0.f);
  const float fl = floorf(src);
  Tap t;
  t.l1 = src - fl;
  t.l0 = 1.0f - t.l1;
  t.i0 = (int)fl;
  if constexpr (WRAPPED) {
    t.i0 += (t.i0 >> 31) & L_in;
    t.i1 = t.i0 + 1;
    t.i1 -= t.i1 >= L_in ? L_in : 0;
  } else {
    t.i0 = min(t.i0, L_in - 1);        // holds already for Hc >= h (src < L_in - 0.5); kept so that no tap can leave the source
    t.i1 = min(t.i0 + 1, L_in - 1);
  }
  return t;
}

__device__ __forceinline__ float bilinear1(float z00, float z01, float z10, float z11, const Tap& ty, const Tap& tx) {
#pragma clang fp contract(off)
  const float a0 = tx.l0 * z00, a1 = tx.l1 * z01, b0 = tx.l0 * z10, b1 = tx.l1 * z11;
  const float a = a0 + a1, b = b0 + b1;
  const float ya = ty.l0 * a, yb = ty.l1 * b;
  return ya + yb;
}

// z [P][C][h][w] fp32 -> x, z_up (null = not written) [P][C][Hc][Wc] fp32 and xin (null = not written) [2 P T][C][s][s]: z_up = the
// bilinear upscale, x = noise1(z_up, noise) of sta_encode_dev.h, xin = window_split_kernel's (rows = 1) scatter of the rounded x.
// A lane owns 8 consecutive canvas pixels of one row: the y taps and weights once per lane, the x taps per element; its 4 x 8 source
// values are dword loads from the two source rows (at most 10 distinct columns per row; the source of one image stays in L2).
template <typename T, int WRAP>
__global__ __launch_bounds__(256) void latent_upscale_step_windows_kernel(const float* __restrict__ z, const float* __restrict__ noise,
                                                                          float* __restrict__ x, float* __restrict__ z_up,
                                                                          T* __restrict__ xin, long nvec, int C, int h, int w, int Hc, int Wc,
                                                                          WinGrid g, float scale_y, float scale_x, float sqrt_a,
                                                                          float sqrt_1ma) {
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const CanvasPos q = canvas_pos(v, C, Hc, Wc / 8);
    const Tap ty = upscale_tap<(WRAP & 2) != 0>(q.y, scale_y, h);
    const float* plane = z + (q.row * C + q.c) * ((long)h * w);
    const float* r0 = plane + (long)ty.i0 * w;
    const float* r1 = plane + (long)ty.i1 * w;
    float nz[8], zu[8], xx[8];
    load8(noise + 8 * v, nz);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const Tap tx = upscale_tap<(WRAP & 1) != 0>(q.x + k, scale_x, w);
      zu[k] = bilinear1(r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1], ty, tx);
      xx[k] = noise1(zu[k], nz[k], sqrt_a, sqrt_1ma);
    }
    store8(x + 8 * v, xx);
    if (z_up) store8(z_up + 8 * v, zu);
    if (xin) scatter<T, WRAP>(xin, g, q.row, 0, 1, C, Hc, Wc, q, round8<T>(xx));
  }
}

// Attention guidance on a canvas (sta_latent_guide_windows): latent_guide_kernel of sta_guide.hip carried to a
// canvas. g [2 P T][C][s][s] is the gradient w.r.t. the window input pairs; the windows are window_split(x), so the gradient w.r.t. the
// canvas state is the split's adjoint, a SUM over the covering windows and both pair rows (not the overlap mean).
// d of one lane's 8 canvas elements: the covering windows' (g_u + g_c) in ascending w, fp32, starting from the first one's value, times
// (1 - keep); kp == nullptr: factor 1. With one window this is guide_d.
template <typename T, int WRAP>
__device__ __forceinline__ void guide_windows_d(const T* __restrict__ g, const WinGrid& gr, int C, int Hc, int Wc, const CanvasPos& q,
                                                const float* __restrict__ kp, float* d) {
  using V8 = typename V8T<T>::type;
  const long T_ = (long)gr.ny * gr.nx;
  int n = 0;
  for_covering_windows<WRAP>(gr, Hc, Wc, q, [&](int j, int i, int dy, int dx) __attribute__((always_inline)) {
    const long at = window_at(2 * (q.row * T_ + j * gr.nx + i), C, q.c, gr.s, dy, dx);
    const V8 gu = *(const V8*)(g + at), gc = *(const V8*)(g + at + (long)C * gr.s * gr.s);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float sum = (float)gu[k] + (float)gc[k];
      d[k] = n ? d[k] + sum : sum;
    }
    ++n;
  });
  if (kp) {
    float k8[8];
    load8(kp, k8);
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = d[k] * (1.0f - k8[k]);
  }
}

// One launch, no atomics, no hand-off between workgroups: a canvas is shared by `parts` workgroups and EVERY one of them reduces the whole
// canvas's sum of d^2 itself in the same fixed order (lane t takes canvas vectors t, t + 256, ..., the 8 squares of each in element order,
// then latent_guide_kernel's LDS tree), so all of them hold the same bits of rms_p; each then forms d again for its own slice (the
// gradient is served by L2 the second time), writes x_out and scatters the rounded vector to the covering windows' pairs. One writer per
// output element; a canvas's outputs depend on that canvas's inputs alone.
// canvec = C Hc Wc / 8 vectors per canvas; count [P]: the elements that receive gradient (the host's), rms_p = sqrt(sum d^2 / count[p]).
template <typename T, int WRAP>
__global__ __launch_bounds__(256) void latent_guide_windows_kernel(const T* __restrict__ g, const float* __restrict__ x,
                                                                   const float* __restrict__ keep, const float* __restrict__ step,
                                                                   const float* __restrict__ count, float* __restrict__ x_out,
                                                                   T* __restrict__ xin, float* __restrict__ stats, long canvec, int C, int Hc,
                                                                   int Wc, WinGrid gr, int parts, long chunk, int normalize, float inv_scale) {
  __shared__ float red[256];
  const long p = blockIdx.x / parts;
  const int part = (int)(blockIdx.x - p * parts);
  const int tid = threadIdx.x;
  const int wvec = Wc / 8;

  float acc = 0.f;
  for (long v = tid; v < canvec; v += 256) {
    const CanvasPos q = canvas_pos(p * canvec + v, C, Hc, wvec);
    float d[8] = {};
    guide_windows_d<T, WRAP>(g, gr, C, Hc, Wc, q, keep ? keep + mask_at(q, Hc, Wc) : nullptr, d);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += d[k] * d[k];
  }
  red[tid] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const float rms = sqrtf(red[0] / count[p]);
  const bool live = (__float_as_uint(rms) & 0x7f800000u) != 0x7f800000u && rms > 0.f;      // finite (neither Inf nor NaN) and positive
  const float s = !live ? 0.f : normalize ? step[p] / rms : step[p] * inv_scale;

  const long end = (part + 1) * chunk < canvec ? (part + 1) * chunk : canvec;
  for (long v = part * chunk + tid; v < end; v += 256) {
    const CanvasPos q = canvas_pos(p * canvec + v, C, Hc, wvec);
    float xv[8];
    load8(x + 8 * (p * canvec + v), xv);
    if (live) {
      float d[8] = {};
      guide_windows_d<T, WRAP>(g, gr, C, Hc, Wc, q, keep ? keep + mask_at(q, Hc, Wc) : nullptr, d);
#pragma unroll
      for (int k = 0; k < 8; ++k) xv[k] = xv[k] - s * d[k];
    }
    store8(x_out + 8 * (p * canvec + v), xv);
    if (xin) scatter<T, WRAP>(xin, gr, p, 0, 1, C, Hc, Wc, q, round8<T>(xv));
  }
  if (stats && part == 0 && tid == 0) stats[p] = rms;
}

// offsets along one axis of length L: 0 first, multiples of 8, ascending, no gap (step <= s), the last window ends at L. ring: the axis
// is CYCLIC (s <= L is the caller's rule: a window covers an element at most once): every offset on the axis instead (o < L; a window
// may run over the seam), and the ring closes (L - last <= s)
int window_axis_ok(const char* what, const char* axis, int n, const int* o, int s, int L, bool ring) {
  if (n < 1 || n > STA_MAX_WINDOW_OFFSETS) return sta_fail(STA_E_ARG, "%s: n%s=%d (need 1 .. %d offsets)", what, axis, n, STA_MAX_WINDOW_OFFSETS);
  for (int k = 0; k < n; ++k) {
    const int prev = k ? o[k - 1] : 0;
    if (o[k] % 8) return sta_fail(STA_E_ARG, "%s: o%s[%d]=%d is not a multiple of 8", what, axis, k, o[k]);
    if (ring && (o[k] < 0 || o[k] >= L)) return sta_fail(STA_E_ARG, "%s: o%s[%d]=%d is not on the wrapped axis (length %d)", what, axis, k, o[k], L);
    if (!ring && (o[k] < 0 || (long)o[k] + s > L)) return sta_fail(STA_E_ARG, "%s: o%s[%d]=%d out of range (s=%d, length %d)", what, axis, k, o[k], s, L);
    if (k ? o[k] <= prev : o[k] != 0) return sta_fail(STA_E_ARG, "%s: o%s[%d]=%d unsorted (after %d; the first offset is 0)", what, axis, k, o[k], prev);
    if (o[k] - prev > s) return sta_fail(STA_E_ARG, "%s: gap between o%s[%d]=%d and o%s[%d]=%d (s=%d)", what, axis, k - 1, prev, axis, k, o[k], s);
  }
  if (ring && L - o[n - 1] > s)
    return sta_fail(STA_E_ARG, "%s: the ring does not close behind o%s[%d]=%d (s=%d, wrapped length %d)", what, axis, n - 1, o[n - 1], s, L);
  if (!ring && o[n - 1] + s != L) return sta_fail(STA_E_ARG, "%s: gap behind o%s[%d]=%d (s=%d, length %d)", what, axis, n - 1, o[n - 1], s, L);
  return STA_OK;
}

// wrap: the cyclic axes (bit 0 = x, bit 1 = y), 0 = the clamped grid
int window_grid_ok(const char* what, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, WinGrid* g) {
  if (!oy || !ox) return sta_fail(STA_E_ARG, "null pointer");
  if (wrap < 0 || wrap > 3) return sta_fail(STA_E_ARG, "%s: wrap=%d (need 0 .. 3: bit 0 = x, bit 1 = y)", what, wrap);
  if (P <= 0 || C <= 0) return sta_fail(STA_E_ARG, "%s: P=%ld C=%d", what, P, C);
  if (s < 8 || Hc < s || Wc < s || s % 8 || Hc % 8 || Wc % 8)
    return sta_fail(STA_E_ARG, "%s: s=%d Hc=%d Wc=%d (need multiples of 8 and 8 <= s <= Hc, Wc)", what, s, Hc, Wc);
  if (const int rc = window_axis_ok(what, "y", ny, oy, s, Hc, wrap & 2)) return rc;
  if (const int rc = window_axis_ok(what, "x", nx, ox, s, Wc, wrap & 1)) return rc;
  *g = WinGrid{};
  g->ny = ny, g->nx = nx, g->s = s;
  for (int k = 0; k < ny; ++k) g->oy[k] = oy[k];
  for (int k = 0; k < nx; ++k) g->ox[k] = ox[k];
  return STA_OK;
}

// every listed pointer is null or 16-byte aligned
bool all_aligned16(std::initializer_list<const void*> tensors) {
  for (const void* p : tensors)
    if (!sta_aligned16(p)) return false;
  return true;
}

// The tail of every launcher: f(T{}, std::integral_constant<int, wrap>{}) with T = the element type of `dtype` (sta_by_dtype refuses any
// other) and a wrap window_grid_ok has accepted (0 .. 3) — the kernels take the cyclic axes at compile time — ...
template <typename F>
int by_dtype_and_wrap(int dtype, int wrap, F&& f) {
  return sta_by_dtype(dtype, [&](auto tag) {
    switch (wrap) {
      case 1: return f(tag, std::integral_constant<int, 1>{});
      case 2: return f(tag, std::integral_constant<int, 2>{});
      case 3: return f(tag, std::integral_constant<int, 3>{});
      default: return f(tag, std::integral_constant<int, 0>{});
    }
  });
}

// ... where f launches its kernel on `groups` 256-lane groups
template <auto Kernel, typename... A>
STA_INLINE int launch_groups(const char* what, unsigned groups, void* stream, A... a) {
  return sta_launch<Kernel>(what, dim3(groups), dim3(256), 0, (hipStream_t)stream, a...);
}

}  // namespace

// The launches (C-ABI); `what` names the entry point in the texts.
extern "C" {

int sta_window_split(const void* src, void* xin, long P, int rows, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s,
                     int wrap, int src_dtype, int dtype, void* stream) {
  const char* what = "window_split";
  g_sta_err[0] = 0;
  if (!src || !xin) return sta_fail(STA_E_ARG, "null pointer");
  WinGrid g;
  if (const int rc = window_grid_ok(what, P, C, Hc, Wc, ny, nx, oy, ox, s, wrap, &g)) return rc;
  if (rows != 1 && rows != 2) return sta_fail(STA_E_ARG, "%s: rows=%d (1: canvas states, 2: input pairs)", what, rows);
  if (!all_aligned16({src, xin})) return sta_fail(STA_E_ARG, "%s: every tensor must be 16-byte aligned", what);
  if (src_dtype != STA_SRC_F32 && src_dtype != dtype)
    return sta_fail(STA_E_UNSUP, "%s: src_dtype %d (float32 = %d, or the output's dtype %d)", what, src_dtype, STA_SRC_F32, dtype);
  const long nvec = P * rows * C * Hc * (Wc / 8);
  return by_dtype_and_wrap(dtype, wrap, [&](auto tag, auto w) {
    using T = decltype(tag);
    constexpr int W = decltype(w)::value;
    if (src_dtype == STA_SRC_F32)
      return launch_groups<window_split_kernel<float, T, W>>(what, sta_grid_for(nvec), stream, (const float*)src, (T*)xin, nvec, rows, C, Hc, Wc, g);
    return launch_groups<window_split_kernel<T, T, W>>(what, sta_grid_for(nvec), stream, (const T*)src, (T*)xin, nvec, rows, C, Hc, Wc, g);
  });
}

int sta_window_fuse(const void* eps, void* out, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap,
                    int dtype, void* stream) {
  const char* what = "window_fuse";
  g_sta_err[0] = 0;
  if (!eps || !out) return sta_fail(STA_E_ARG, "null pointer");
  WinGrid g;
  if (const int rc = window_grid_ok(what, P, C, Hc, Wc, ny, nx, oy, ox, s, wrap, &g)) return rc;
  if (!all_aligned16({eps, out})) return sta_fail(STA_E_ARG, "%s: every tensor must be 16-byte aligned", what);
  const long nvec = 2 * P * C * Hc * (Wc / 8);
  return by_dtype_and_wrap(dtype, wrap, [&](auto tag, auto w) {
    using T = decltype(tag);
    return launch_groups<window_fuse_kernel<T, decltype(w)::value>>(what, sta_grid_for(nvec), stream, (const T*)eps, (T*)out, nvec, C, Hc, Wc, g);
  });
}

int sta_sampler_step_windows(const void* eps, const float* x, const float* m_prev, const float* noise, float* x_next, float* m, void* xin, long P,
                             int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, float scale, float sigma_t,
                             float alpha_t, float c_x, float c_m, float c_p, float c_e, float c_n, int dtype, void* stream) {
  const char* what = "sampler_step_windows";
  const StepCoef c{scale, sigma_t, alpha_t, c_x, c_m, c_p, c_e, c_n};
  g_sta_err[0] = 0;
  WinGrid g;
  if (const int rc = sta_step_args_ok(what, eps, x, m_prev, noise, x_next, m, xin, false, nullptr, nullptr, nullptr, c.alpha_t,
                                      [&] { return window_grid_ok(what, P, C, Hc, Wc, ny, nx, oy, ox, s, wrap, &g); }))
    return rc;
  const long nvec = P * C * Hc * (Wc / 8);
  return by_dtype_and_wrap(dtype, wrap, [&](auto tag, auto w) {
    using T = decltype(tag);
    return launch_groups<sampler_step_windows_kernel<T, decltype(w)::value>>(what, sta_grid_for(nvec), stream, (const T*)eps, x, m_prev, noise,
                                                                             x_next, m, (T*)xin, nvec, C, Hc, Wc, g, c);
  });
}

int sta_sampler_step_windows_masked(const void* eps, const float* x, const float* m_prev, const float* noise, const float* x0,
                                    const float* keep, const float* qnoise, float* x_next, float* m, void* xin, long P, int C, int Hc, int Wc,
                                    int ny, int nx, const int* oy, const int* ox, int s, int wrap, float scale, float sigma_t, float alpha_t,
                                    float c_x, float c_m, float c_p, float c_e, float c_n, float q_a, float q_b, int dtype, void* stream) {
  const char* what = "sampler_step_windows_masked";
  const StepCoef c{scale, sigma_t, alpha_t, c_x, c_m, c_p, c_e, c_n};
  g_sta_err[0] = 0;
  WinGrid g;
  if (const int rc = sta_step_args_ok(what, eps, x, m_prev, noise, x_next, m, xin, true, x0, keep, qnoise, c.alpha_t,
                                      [&] { return window_grid_ok(what, P, C, Hc, Wc, ny, nx, oy, ox, s, wrap, &g); }))
    return rc;
  const long nvec = P * C * Hc * (Wc / 8);
  return by_dtype_and_wrap(dtype, wrap, [&](auto tag, auto w) {
    using T = decltype(tag);
    auto launch = [&](auto mp, auto nz) {
      return launch_groups<sampler_step_windows_masked_kernel<T, decltype(mp)::value, decltype(nz)::value, decltype(w)::value>>(
          what, sta_grid_for(nvec), stream, (const T*)eps, x, m_prev, noise, x0, keep, qnoise, x_next, m, (T*)xin, nvec, C, Hc, Wc, g, c, q_a, q_b);
    };
    using Yes = std::true_type;
    using No = std::false_type;
    return m_prev ? (noise ? launch(Yes{}, Yes{}) : launch(Yes{}, No{})) : (noise ? launch(No{}, Yes{}) : launch(No{}, No{}));
  });
}

int sta_window_blend(const float* x, const float* x0, const float* keep, const float* noise, float* x_out, void* xin, long P, int C, int Hc,
                     int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, float q_a, float q_b, int dtype, void* stream) {
  const char* what = "window_blend";
  g_sta_err[0] = 0;
  if (!x || !x0 || !keep || !noise || !x_out) return sta_fail(STA_E_ARG, "%s: null pointer", what);
  WinGrid g;
  if (const int rc = window_grid_ok(what, P, C, Hc, Wc, ny, nx, oy, ox, s, wrap, &g)) return rc;
  if (!all_aligned16({x, x0, keep, noise, x_out, xin})) return sta_fail(STA_E_ARG, "%s: every tensor must be 16-byte aligned", what);
  const long nvec = P * C * Hc * (Wc / 8);
  return by_dtype_and_wrap(dtype, wrap, [&](auto tag, auto w) {
    using T = decltype(tag);
    return launch_groups<window_blend_kernel<T, decltype(w)::value>>(what, sta_grid_for(nvec), stream, x, x0, keep, noise, x_out, (T*)xin, nvec, C,
                                                                     Hc, Wc, g, q_a, q_b);
  });
}

int sta_vae_encode_step_windows(const void* h, const float* quant_w, const float* quant_b, const float* n_post, const float* n_enc, float* x,
                                float* z0, void* xin, long P, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap,
                                float scale_factor, float sqrt_a, float sqrt_1ma, int dtype, void* stream) {
  const char* what = "vae_encode_step_windows";
  g_sta_err[0] = 0;
  if (!h || !quant_w || !quant_b || !n_post || !n_enc || !x) return sta_fail(STA_E_ARG, "%s: null pointer", what);
  WinGrid g;
  if (const int rc = window_grid_ok(what, P, 4, Hc, Wc, ny, nx, oy, ox, s, wrap, &g)) return rc;
  if (!all_aligned16({h, n_post, n_enc, x, z0, xin})) return sta_fail(STA_E_ARG, "%s: every tensor must be 16-byte aligned", what);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_ARG, "%s: dtype %d (STA_BF16 or STA_F16)", what, dtype);
  const long nvec = P * Hc * (Wc / 8);
  return by_dtype_and_wrap(dtype, wrap, [&](auto tag, auto w) {
    using T = decltype(tag);
    return launch_groups<vae_encode_step_windows_kernel<T, decltype(w)::value>>(what, sta_grid_for(nvec), stream, (const T*)h, quant_w, quant_b,
                                                                                n_post, n_enc, x, z0, (T*)xin, nvec, Hc, Wc, g, scale_factor,
                                                                                sqrt_a, sqrt_1ma);
  });
}

int sta_latent_upscale_step_windows(const float* z, const float* noise, float* x, float* z_up, void* xin, long P, int C, int h, int w, int Hc,
                                    int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap, float sqrt_a, float sqrt_1ma, int dtype,
                                    void* stream) {
  const char* what = "latent_upscale_step_windows";
  g_sta_err[0] = 0;
  if (!z || !noise || !x) return sta_fail(STA_E_ARG, "%s: null pointer", what);
  WinGrid g;
  if (const int rc = window_grid_ok(what, P, C, Hc, Wc, ny, nx, oy, ox, s, wrap, &g)) return rc;
  if (h < 8 || w < 8 || h % 8 || w % 8) return sta_fail(STA_E_ARG, "%s: source h=%d w=%d (need positive multiples of 8)", what, h, w);
  if (Hc < h || Wc < w) return sta_fail(STA_E_ARG, "%s: canvas %d x %d is smaller than the source %d x %d (upscale only)", what, Hc, Wc, h, w);
  if (!all_aligned16({z, noise, x, z_up, xin})) return sta_fail(STA_E_ARG, "%s: every tensor must be 16-byte aligned", what);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_ARG, "%s: dtype %d (STA_BF16 or STA_F16)", what, dtype);
  const long nvec = P * C * Hc * (Wc / 8);
  const float scale_y = (float)h / (float)Hc, scale_x = (float)w / (float)Wc;
  return by_dtype_and_wrap(dtype, wrap, [&](auto tag, auto wr) {
    using T = decltype(tag);
    return launch_groups<latent_upscale_step_windows_kernel<T, decltype(wr)::value>>(what, sta_grid_for(nvec), stream, z, noise, x, z_up, (T*)xin,
                                                                                     nvec, C, h, w, Hc, Wc, g, scale_y, scale_x, sqrt_a, sqrt_1ma);
  });
}

int sta_latent_guide_windows(const void* g, const float* x, const float* keep, const float* step, const float* count, float* x_out, void* xin,
                             float* stats, long P, int C, int Hc, int Wc, int ny, int nx, const int* oy, const int* ox, int s, int wrap,
                             int normalize, float inv_scale, int dtype, void* stream) {
  const char* what = "latent_guide_windows";
  g_sta_err[0] = 0;
  if (!g || !x || !step || !count || !x_out) return sta_fail(STA_E_ARG, "%s: null pointer", what);
  WinGrid gr;
  if (const int rc = window_grid_ok(what, P, C, Hc, Wc, ny, nx, oy, ox, s, wrap, &gr)) return rc;
  if (!all_aligned16({g, x, keep, x_out, xin}) || ((uintptr_t)step & 3) || ((uintptr_t)count & 3) || ((uintptr_t)stats & 3))
    return sta_fail(STA_E_ARG, "%s: every tensor must be 16-byte aligned (step, count and stats: 4-byte)", what);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_ARG, "%s: dtype %d (STA_BF16 or STA_F16)", what, dtype);
  const size_t plane = (size_t)Hc * Wc, f32 = (size_t)P * C * plane * 4, pairs = (size_t)2 * P * ny * nx * C * s * s * 2;
  const void* ins[] = {g, x, keep, step, count};
  const size_t in_bytes[] = {pairs, f32, (size_t)P * plane * 4, (size_t)P * 4, (size_t)P * 4};
  const void* outs[] = {x_out, xin, stats};
  const size_t out_bytes[] = {f32, pairs, (size_t)P * 4};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 5; ++i)
      if (guide_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return sta_fail(STA_E_ARG, "%s: an output aliases an input", what);
    for (int q = o + 1; q < 3; ++q)
      if (guide_overlap(outs[o], out_bytes[o], outs[q], out_bytes[q])) return sta_fail(STA_E_ARG, "%s: two outputs alias each other", what);
  }
  const long canvec = (long)C * Hc * (Wc / 8);
  long parts = (canvec + 255) / 256;                       // sta_latent_guide's rule
  if (parts > GUIDE_MAX_PARTS) parts = GUIDE_MAX_PARTS;
  const long chunk = (canvec + parts - 1) / parts;
  if (P * parts > 0x7fffffffL) return sta_fail(STA_E_UNSUP, "%s: P=%ld canvases need more than 2^31 - 1 workgroups", what, P);
  return by_dtype_and_wrap(dtype, wrap, [&](auto tag, auto w) {
    using T = decltype(tag);
    return launch_groups<latent_guide_windows_kernel<T, decltype(w)::value>>(what, (unsigned)(P * parts), stream, (const T*)g, x, keep, step, count,
                                                                             x_out, (T*)xin, stats, canvec, C, Hc, Wc, gr, (int)parts, chunk,
                                                                             normalize, inv_scale);
  });
}

}  // extern "C"
