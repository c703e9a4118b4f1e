// sta_sampler.hip — the per-call arithmetic of the DPM-Solver++(2M) and DDIM samplers in one pass (gfx950).
// C-ABI in include/sta_unet.h (sta_sampler_step / sta_sampler_step_bwd). Elementwise over the [b][n] latents: every lane owns
// 8 consecutive elements of one image, reads them with 16-byte loads (one for the 16-bit UNet rows, two per fp32 tensor) and
// writes them with 16-byte stores; fp32 arithmetic. The step coefficients are computed on the host (sta/solver.py) and arrive
// as kernel arguments, one launch per UNet call.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sta_xattn.h"
#include "sta_unet.h"
#include "sta_internal.h"

namespace {

template <typename T> struct V8T { typedef T type __attribute__((ext_vector_type(8))); };
typedef float F4 __attribute__((ext_vector_type(4)));

struct StepCoef {
  float scale;      // classifier-free guidance scale s
  float sigma_t;    // sigma and alpha of the time the UNet was called at
  float alpha_t;
  float c_x, c_m, c_p, c_e, c_n;
};

__device__ __forceinline__ void load8(const float* p, float* v) {
  const F4 a = *(const F4*)p, b = *(const F4*)(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = a[e];
    v[4 + e] = b[e];
  }
}

__device__ __forceinline__ void store8(float* p, const float* v) {
  F4 a, b;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = v[e];
    b[e] = v[4 + e];
  }
  *(F4*)p = a;
  *(F4*)(p + 4) = b;
}

// e = eps[2i] + s (eps[2i+1] - eps[2i]);  m = (x - sigma_t e) / alpha_t;  x_next = c_x x + c_m m + c_p m_prev + c_e e + c_n noise
// m_prev / noise may be null (their coefficient is then 0); xin (null = not written) = the next call's input pair (x_next, x_next).
template <typename T>
__global__ __launch_bounds__(256) void sampler_step_kernel(const T* __restrict__ eps, const float* __restrict__ x,
                                                           const float* __restrict__ m_prev, const float* __restrict__ noise,
                                                           float* __restrict__ x_next, float* __restrict__ m, T* __restrict__ xin,
                                                           long nvec, long rowvec, StepCoef c) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long img = v / rowvec, col = v - img * rowvec;
    const V8 eu = ((const V8*)eps)[2 * img * rowvec + col];
    const V8 ec = ((const V8*)eps)[(2 * img + 1) * rowvec + col];
    float xv[8], mp[8], nz[8], xn[8], mv[8];
    load8(x + 8 * v, xv);
    if (m_prev) load8(m_prev + 8 * v, mp);
    if (noise) load8(noise + 8 * v, nz);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float u = (float)eu[k];
      const float e = u + c.scale * ((float)ec[k] - u);
      mv[k] = (xv[k] - c.sigma_t * e) / c.alpha_t;
      float t = c.c_x * xv[k] + c.c_m * mv[k] + c.c_e * e;
      if (m_prev) t += c.c_p * mp[k];
      if (noise) t += c.c_n * nz[k];
      xn[k] = t;
    }
    store8(x_next + 8 * v, xn);
    store8(m + 8 * v, mv);
    if (xin) {
      V8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = (T)xn[k];
      ((V8*)xin)[2 * img * rowvec + col] = o;
      ((V8*)xin)[(2 * img + 1) * rowvec + col] = o;
    }
  }
}

// The step is linear in (eps, x, m_prev): with G_m = g_m + c_m g_xn (the use of m by the next step and by x_next),
//   g_x = c_x g_xn + G_m / alpha_t,  g_e = c_e g_xn - (sigma_t / alpha_t) G_m,  g_eps[2i] = (1 - s) g_e,  g_eps[2i+1] = s g_e,
//   g_m_prev = c_p g_xn.  The noise gets no gradient. g_m / g_m_prev may be null.
template <typename T>
__global__ __launch_bounds__(256) void sampler_step_bwd_kernel(const float* __restrict__ g_xn, const float* __restrict__ g_m,
                                                               float* __restrict__ g_x, T* __restrict__ g_eps,
                                                               float* __restrict__ g_mprev, long nvec, long rowvec, StepCoef c) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  const float inv_a = 1.0f / c.alpha_t;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long img = v / rowvec, col = v - img * rowvec;
    float gn[8], gm[8], gx[8], gp[8];
    load8(g_xn + 8 * v, gn);
    if (g_m) load8(g_m + 8 * v, gm);
    V8 gu, gc;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float Gm = (g_m ? gm[k] : 0.f) + c.c_m * gn[k];
      gx[k] = c.c_x * gn[k] + Gm * inv_a;
      const float ge = c.c_e * gn[k] - c.sigma_t * inv_a * Gm;
      gu[k] = (T)((1.0f - c.scale) * ge);
      gc[k] = (T)(c.scale * ge);
      gp[k] = c.c_p * gn[k];
    }
    store8(g_x + 8 * v, gx);
    ((V8*)g_eps)[2 * img * rowvec + col] = gu;
    ((V8*)g_eps)[(2 * img + 1) * rowvec + col] = gc;
    if (g_mprev) store8(g_mprev + 8 * v, gp);
  }
}

}  // namespace

extern "C" {

int sta_sampler_step(const void* eps, const float* x, const float* m_prev, const float* noise, float* x_next, float* m, void* xin,
                     long b, long n, float scale, float sigma_t, float alpha_t, float c_x, float c_m, float c_p, float c_e, float c_n,
                     int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!eps || !x || !x_next || !m) return sta_fail(STA_E_ARG, "null pointer");
  if (b <= 0 || n <= 0 || n % 8) return sta_fail(STA_E_ARG, "sampler_step: b=%ld n=%ld (need n %% 8 == 0)", b, n);
  if (!sta_aligned16(eps) || !sta_aligned16(x) || !sta_aligned16(m_prev) || !sta_aligned16(noise) || !sta_aligned16(x_next) || !sta_aligned16(m) || !sta_aligned16(xin))
    return sta_fail(STA_E_ARG, "sampler_step: every tensor must be 16-byte aligned");
  if (alpha_t == 0.f) return sta_fail(STA_E_ARG, "sampler_step: alpha_t == 0");
  const StepCoef c{scale, sigma_t, alpha_t, c_x, c_m, c_p, c_e, c_n};
  const long rowvec = n / 8, nvec = b * rowvec;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<sampler_step_kernel<T>>("sampler_step", dim3(sta_grid_for(nvec)), dim3(256), 0, (hipStream_t)stream, (const T*)eps, x,
                                              m_prev, noise, x_next, m, (T*)xin, nvec, rowvec, c);
  });
}

int sta_sampler_step_bwd(const float* g_xn, const float* g_m, float* g_x, void* g_eps, float* g_mprev, long b, long n, float scale,
                         float sigma_t, float alpha_t, float c_x, float c_m, float c_p, float c_e, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!g_xn || !g_x || !g_eps) return sta_fail(STA_E_ARG, "null pointer");
  if (b <= 0 || n <= 0 || n % 8) return sta_fail(STA_E_ARG, "sampler_step_bwd: b=%ld n=%ld (need n %% 8 == 0)", b, n);
  if (!sta_aligned16(g_xn) || !sta_aligned16(g_m) || !sta_aligned16(g_x) || !sta_aligned16(g_eps) || !sta_aligned16(g_mprev))
    return sta_fail(STA_E_ARG, "sampler_step_bwd: every tensor must be 16-byte aligned");
  if (alpha_t == 0.f) return sta_fail(STA_E_ARG, "sampler_step_bwd: alpha_t == 0");
  const StepCoef c{scale, sigma_t, alpha_t, c_x, c_m, c_p, c_e, 0.f};
  const long rowvec = n / 8, nvec = b * rowvec;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<sampler_step_bwd_kernel<T>>("sampler_step_bwd", dim3(sta_grid_for(nvec)), dim3(256), 0, (hipStream_t)stream, g_xn, g_m,
                                                  g_x, (T*)g_eps, g_mprev, nvec, rowvec, c);
  });
}

}  // extern "C"

// the latent update of attention-guided sampling (sta_latent_guide): same helpers, same flags, same pass through the hazard lint
#include "sta_guide.hip"

// wide canvases as overlapping windows (sta_window_split / sta_window_fuse / sta_sampler_step_windows): same helpers, same flags
#include "sta_window.hip"
