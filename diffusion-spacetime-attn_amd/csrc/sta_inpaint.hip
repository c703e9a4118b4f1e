// sta_inpaint.hip — layout-guided inpainting: the sampler step with the next call's re-noising blend, its backward, the blend alone
// (first call) and the pixel-space paste of the original with its backward (gfx950). C-ABI in include/sta_unet.h.
// Conventions of sta_sampler.hip: every lane owns 8 consecutive elements of one image, 16-byte loads and stores, fp32 arithmetic,
// grid-stride loop under the same grid cap, coefficients computed on the host. The mask is [b][hw] fp32, broadcast over the channels:
// with hw % 8 == 0 a lane's 8 elements never straddle a channel, so its 8 mask values are two 16-byte loads at (8 col) % hw.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sta_xattn.h"
#include "sta_unet.h"
#include "sta_internal.h"
#include "sta_blend_dev.h"      // blend1: shared with the canvas kernels of sta_window.hip
#include "sta_step_dev.h"       // V8T / F4 / load8 / store8 / StepCoef, the step per element: shared with sta_sampler.hip

namespace {

// sta_sampler_step's step for call i (step1 of sta_step_dev.h), then the blend of call i + 1 on x_next.
template <typename T>
__global__ __launch_bounds__(256) void sampler_step_masked_kernel(const T* __restrict__ eps, const float* __restrict__ x,
                                                                  const float* __restrict__ m_prev, const float* __restrict__ noise,
                                                                  const float* __restrict__ x0, const float* __restrict__ keep,
                                                                  const float* __restrict__ qnoise, float* __restrict__ x_next,
                                                                  float* __restrict__ m, T* __restrict__ xin, long nvec, long rowvec,
                                                                  long hw, StepCoef c, float q_a, float q_b) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long img = v / rowvec, col = v - img * rowvec;
    const long iu = 2 * img * rowvec + col, ic = (2 * img + 1) * rowvec + col;      // rows 2 img, 2 img + 1 of eps and of xin
    const V8 eu = ((const V8*)eps)[iu], ec = ((const V8*)eps)[ic];
    float xv[8], mp[8], nz[8], xn[8], mv[8], z0[8], kp[8], qn[8];
    load8(x + 8 * v, xv);
    if (m_prev) load8(m_prev + 8 * v, mp);
    if (noise) load8(noise + 8 * v, nz);
    load8(x0 + 8 * v, z0);
    load8(qnoise + 8 * v, qn);
    load8(keep + img * hw + (8 * col) % hw, kp);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float t = step1((float)eu[k], (float)ec[k], xv[k], mp + k, nz + k, m_prev, noise, c, mv[k]);
      xn[k] = blend1(kp[k], z0[k], qn[k], t, q_a, q_b);
    }
    store8(x_next + 8 * v, xn);
    store8(m + 8 * v, mv);
    if (xin) {      // not store_pair: it would form the row indices of the eps loads again (profiles/step_one_definition.md)
      const V8 o = round8<T>(xn);
      ((V8*)xin)[iu] = o;
      ((V8*)xin)[ic] = o;
    }
  }
}

// sta_sampler_step_bwd with the incoming g_xn (the gradient of the BLENDED state) scaled by (1 - keep): x0, keep and the blend noise
// are constants of the graph.
template <typename T>
__global__ __launch_bounds__(256) void sampler_step_masked_bwd_kernel(const float* __restrict__ g_xn, const float* __restrict__ g_m,
                                                                      const float* __restrict__ keep, float* __restrict__ g_x,
                                                                      T* __restrict__ g_eps, float* __restrict__ g_mprev, long nvec,
                                                                      long rowvec, long hw, StepCoef c) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  const float inv_a = 1.0f / c.alpha_t;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long img = v / rowvec, col = v - img * rowvec;
    float gn[8], gm[8], gx[8], gp[8], kp[8];
    load8(g_xn + 8 * v, gn);
    if (g_m) load8(g_m + 8 * v, gm);
    load8(keep + img * hw + (8 * col) % hw, kp);
    V8 gu, gc;
#pragma unroll
    for (int k = 0; k < 8; ++k) step1_bwd<T>((1.0f - kp[k]) * gn[k], gm, g_m, inv_a, c, k, gx, gu, gc, gp);
    store8(g_x + 8 * v, gx);
    ((V8*)g_eps)[2 * img * rowvec + col] = gu;
    ((V8*)g_eps)[(2 * img + 1) * rowvec + col] = gc;
    if (g_mprev) store8(g_mprev + 8 * v, gp);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void latent_blend_kernel(const float* __restrict__ x, const float* __restrict__ x0,
                                                           const float* __restrict__ keep, const float* __restrict__ noise,
                                                           float* __restrict__ x_out, T* __restrict__ xin, long nvec, long rowvec, long hw,
                                                           float q_a, float q_b) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long img = v / rowvec, col = v - img * rowvec;
    float xv[8], z0[8], kp[8], qn[8], xo[8];
    load8(x + 8 * v, xv);
    load8(x0 + 8 * v, z0);
    load8(noise + 8 * v, qn);
    load8(keep + img * hw + (8 * col) % hw, kp);
#pragma unroll
    for (int k = 0; k < 8; ++k) xo[k] = blend1(kp[k], z0[k], qn[k], xv[k], q_a, q_b);
    store8(x_out + 8 * v, xo);
    if (xin) store_pair(xin, img, rowvec, col, xo);
  }
}

// out = keep_px orig + (1 - keep_px) clamp((dec + 1) / 2, 0, 1), rounded to T once. rowvec = 3 HW / 8 lanes per image.
template <typename T>
__global__ __launch_bounds__(256) void image_composite_kernel(const T* __restrict__ dec, const float* __restrict__ orig,
                                                              const float* __restrict__ keep_px, T* __restrict__ out, long nvec,
                                                              long rowvec, long hw) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long img = v / rowvec, col = v - img * rowvec;
    const V8 d = ((const V8*)dec)[v];
    float og[8], kp[8];
    load8(orig + 8 * v, og);
    load8(keep_px + img * hw + (8 * col) % hw, kp);
    V8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float g = fminf(fmaxf(((float)d[k] + 1.0f) * 0.5f, 0.0f), 1.0f);
      o[k] = (T)(kp[k] * og[k] + (1.0f - kp[k]) * g);
    }
    ((V8*)out)[v] = o;
  }
}

// g_dec = 0.5 (1 - keep_px) g where -1 <= dec <= 1 (inclusive, torch.clamp's gradient), 0 elsewhere.
template <typename T>
__global__ __launch_bounds__(256) void image_composite_bwd_kernel(const T* __restrict__ g, const T* __restrict__ dec,
                                                                  const float* __restrict__ keep_px, T* __restrict__ g_dec, long nvec,
                                                                  long rowvec, long hw) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long img = v / rowvec, col = v - img * rowvec;
    const V8 d = ((const V8*)dec)[v], gv = ((const V8*)g)[v];
    float kp[8];
    load8(keep_px + img * hw + (8 * col) % hw, kp);
    V8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float dv = (float)d[k];
      const bool inside = dv >= -1.0f && dv <= 1.0f;
      o[k] = (T)(inside ? 0.5f * (1.0f - kp[k]) * (float)gv[k] : 0.0f);
    }
    ((V8*)g_dec)[v] = o;
  }
}

// b images of n elements, masks of hw: n a whole number of hw-sized channels, hw % 8 == 0
int check_sizes(const char* what, long b, long n, long hw) {
  if (b <= 0 || n <= 0 || hw <= 0 || hw % 8 || n % hw)
    return sta_fail(STA_E_ARG, "%s: b=%ld n=%ld hw=%ld (need hw %% 8 == 0 and n a multiple of hw)", what, b, n, hw);
  return 0;
}

}  // namespace

extern "C" {

int sta_sampler_step_masked(const void* eps, const float* x, const float* m_prev, const float* noise, const float* x0, const float* keep,
                            const float* qnoise, float* x_next, float* m, void* xin, long b, long n, long hw, float scale, float sigma_t,
                            float alpha_t, float c_x, float c_m, float c_p, float c_e, float c_n, float q_a, float q_b, int dtype,
                            void* stream) {
  g_sta_err[0] = 0;
  if (const int rc = sta_step_args_ok("sampler_step_masked", eps, x, m_prev, noise, x_next, m, xin, true, x0, keep, qnoise, alpha_t,
                                      [&] { return check_sizes("sampler_step_masked", b, n, hw); }))
    return rc;
  const StepCoef c{scale, sigma_t, alpha_t, c_x, c_m, c_p, c_e, c_n};
  const long rowvec = n / 8, nvec = b * rowvec;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<sampler_step_masked_kernel<T>>("sampler_step_masked", dim3(sta_grid_for(nvec)), dim3(256), 0, (hipStream_t)stream, (const T*)eps, x, m_prev, noise,
                                                     x0, keep, qnoise, x_next, m, (T*)xin, nvec, rowvec, hw, c, q_a, q_b);
  });
}

int sta_sampler_step_masked_bwd(const float* g_xn, const float* g_m, const float* keep, float* g_x, void* g_eps, float* g_mprev, long b,
                                long n, long hw, float scale, float sigma_t, float alpha_t, float c_x, float c_m, float c_p, float c_e,
                                int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (const int rc = sta_step_bwd_args_ok("sampler_step_masked_bwd", g_xn, g_m, g_x, g_eps, g_mprev, true, keep, alpha_t,
                                          [&] { return check_sizes("sampler_step_masked_bwd", b, n, hw); }))
    return rc;
  const StepCoef c{scale, sigma_t, alpha_t, c_x, c_m, c_p, c_e, 0.f};
  const long rowvec = n / 8, nvec = b * rowvec;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<sampler_step_masked_bwd_kernel<T>>("sampler_step_masked_bwd", dim3(sta_grid_for(nvec)), dim3(256), 0, (hipStream_t)stream, g_xn,
                                                         g_m, keep, g_x, (T*)g_eps, g_mprev, nvec, rowvec, hw, c);
  });
}

int sta_latent_blend(const float* x, const float* x0, const float* keep, const float* noise, float* x_out, void* xin, long b, long n, long hw,
                     float q_a, float q_b, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !x0 || !keep || !noise || !x_out) return sta_fail(STA_E_ARG, "latent_blend: null pointer");
  if (check_sizes("latent_blend", b, n, hw)) return STA_E_ARG;
  if (!sta_aligned16(x) || !sta_aligned16(x0) || !sta_aligned16(keep) || !sta_aligned16(noise) || !sta_aligned16(x_out) || !sta_aligned16(xin))
    return sta_fail(STA_E_ARG, "latent_blend: every tensor must be 16-byte aligned");
  const long rowvec = n / 8, nvec = b * rowvec;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<latent_blend_kernel<T>>("latent_blend", dim3(sta_grid_for(nvec)), dim3(256), 0, (hipStream_t)stream, x, x0, keep, noise, x_out, (T*)xin, nvec,
                                              rowvec, hw, q_a, q_b);
  });
}

int sta_image_composite(const void* dec, const float* orig, const float* keep_px, void* out, long b, long hw, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!dec || !orig || !keep_px || !out) return sta_fail(STA_E_ARG, "image_composite: null pointer");
  if (check_sizes("image_composite", b, 3 * hw, hw)) return STA_E_ARG;
  if (!sta_aligned16(dec) || !sta_aligned16(orig) || !sta_aligned16(keep_px) || !sta_aligned16(out))
    return sta_fail(STA_E_ARG, "image_composite: every tensor must be 16-byte aligned");
  const long rowvec = 3 * hw / 8, nvec = b * rowvec;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<image_composite_kernel<T>>("image_composite", dim3(sta_grid_for(nvec)), dim3(256), 0, (hipStream_t)stream, (const T*)dec, orig, keep_px,
                                                 (T*)out, nvec, rowvec, hw);
  });
}

int sta_image_composite_bwd(const void* g, const void* dec, const float* keep_px, void* g_dec, long b, long hw, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!g || !dec || !keep_px || !g_dec) return sta_fail(STA_E_ARG, "image_composite_bwd: null pointer");
  if (check_sizes("image_composite_bwd", b, 3 * hw, hw)) return STA_E_ARG;
  if (!sta_aligned16(g) || !sta_aligned16(dec) || !sta_aligned16(keep_px) || !sta_aligned16(g_dec))
    return sta_fail(STA_E_ARG, "image_composite_bwd: every tensor must be 16-byte aligned");
  const long rowvec = 3 * hw / 8, nvec = b * rowvec;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<image_composite_bwd_kernel<T>>("image_composite_bwd", dim3(sta_grid_for(nvec)), dim3(256), 0, (hipStream_t)stream, (const T*)g,
                                                     (const T*)dec, keep_px, (T*)g_dec, nvec, rowvec, hw);
  });
}

}  // extern "C"
