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
#include "sta_step_dev.h"      // V8T / F4 / load8 / store8 / StepCoef, the step per element: shared with sta_inpaint.hip

namespace {

// step1 of sta_step_dev.h on (eps[2i], eps[2i+1]) of every element. m_prev / noise may be null (their coefficient is then 0);
// xin (null = not written) = the next call's input pair (x_next, x_next).
template <typename T>
__global__ __launch_bounds__(256) void sampler_step_kernel(const T* __restrict__ eps, const float* __restrict__ x,
                                                           const float* __restrict__ m_prev, const float* __restrict__ noise,
                                                           float* __restrict__ x_next, float* __restrict__ m, T* __restrict__ xin,
                                                           long nvec, long rowvec, StepCoef c) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
    const long img = v / rowvec, col = v - img * rowvec;
    const long iu = 2 * img * rowvec + col, ic = (2 * img + 1) * rowvec + col;      // rows 2 img, 2 img + 1 of eps and of xin
    const V8 eu = ((const V8*)eps)[iu], ec = ((const V8*)eps)[ic];
    float xv[8], mp[8], nz[8], xn[8], mv[8];
    load8(x + 8 * v, xv);
    if (m_prev) load8(m_prev + 8 * v, mp);
    if (noise) load8(noise + 8 * v, nz);
#pragma unroll
    for (int k = 0; k < 8; ++k) xn[k] = step1((float)eu[k], (float)ec[k], xv[k], mp + k, nz + k, m_prev, noise, c, mv[k]);
    store8(x_next + 8 * v, xn);
    store8(m + 8 * v, mv);
    if (xin) {      // not store_pair: it would form the row indices of the eps loads again (profiles/step_one_definition.md)
      const V8 o = round8<T>(xn);
      ((V8*)xin)[iu] = o;
      ((V8*)xin)[ic] = o;
    }
  }
}

// step1_bwd of sta_step_dev.h on g_xn. g_m / g_m_prev may be null.
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
    for (int k = 0; k < 8; ++k) step1_bwd<T>(gn[k], gm, g_m, inv_a, c, k, gx, gu, gc, gp);
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
  if (const int rc = sta_step_args_ok("sampler_step", eps, x, m_prev, noise, x_next, m, xin, false, nullptr, nullptr, nullptr, alpha_t, [&] {
        return b <= 0 || n <= 0 || n % 8 ? sta_fail(STA_E_ARG, "sampler_step: b=%ld n=%ld (need n %% 8 == 0)", b, n) : STA_OK;
      }))
    return rc;
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
  if (const int rc = sta_step_bwd_args_ok("sampler_step_bwd", g_xn, g_m, g_x, g_eps, g_mprev, false, nullptr, alpha_t, [&] {
        return b <= 0 || n <= 0 || n % 8 ? sta_fail(STA_E_ARG, "sampler_step_bwd: b=%ld n=%ld (need n %% 8 == 0)", b, n) : STA_OK;
      }))
    return rc;
  const StepCoef c{scale, sigma_t, alpha_t, c_x, c_m, c_p, c_e, 0.f};
  const long rowvec = n / 8, nvec = b * rowvec;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<sampler_step_bwd_kernel<T>>("sampler_step_bwd", dim3(sta_grid_for(nvec)), dim3(256), 0, (hipStream_t)stream, g_xn, g_m,
                                                  g_x, (T*)g_eps, g_mprev, nvec, rowvec, c);
  });
}

}  // extern "C"

// the latent update of attention-guided sampling (sta_latent_guide): the helpers of sta_step_dev.h, same flags, same pass through the hazard lint
#include "sta_guide.hip"

// wide canvases as overlapping windows (sta_window_split / sta_window_fuse / sta_sampler_step_windows): the step of sta_step_dev.h, same flags
#include "sta_window.hip"
