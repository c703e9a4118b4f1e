// sta_step_dev.h — the sampler step per element, forward and backward, and the helpers of the elementwise kernels around it: ONE
// definition for the square kernels (sta_sampler.hip), their masked forms (sta_inpaint.hip) and the canvas kernels (sta_window.hip);
// sta_guide.hip uses the helpers. fp32, force-inlined, no fast-math flag in either unit: a kernel compiles to what it was with the
// expressions written out in it (profiles/step_one_definition.md). At the end, host side: the argument checks of the step's entry points.
#pragma once

#include <hip/hip_runtime.h>
#include "sta_internal.h"

namespace {      // internal to each unit, like the kernels that take a StepCoef

typedef float F4 __attribute__((ext_vector_type(4)));

struct StepCoef {
  float scale;      // classifier-free guidance scale s
  float sigma_t;    // sigma and alpha of the time the UNet was called at
  float alpha_t;
  float c_x, c_m, c_p, c_e, c_n;
};

// v held in a vector register from here on (an empty asm that only constrains where v lives), and a StepCoef held so: for a kernel
// whose grid tables and streams fill the scalar file to the last register (the wrapped masked step of sta_window.hip)
__device__ __forceinline__ float in_vgpr(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ StepCoef coef_in_vgprs(const StepCoef& c) {
  return StepCoef{in_vgpr(c.scale), in_vgpr(c.sigma_t), in_vgpr(c.alpha_t), in_vgpr(c.c_x), in_vgpr(c.c_m), in_vgpr(c.c_p), in_vgpr(c.c_e),
                  in_vgpr(c.c_n)};
}

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

// 8 floats rounded to T (to nearest even), once
template <typename T>
__device__ __forceinline__ typename V8T<T>::type round8(const float* v) {
  typename V8T<T>::type o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = (T)v[k];
  return o;
}

// v rounded to T -> vector col of rows 2 img and 2 img + 1 of the pair batch xin [2b][rowvec]: one image's (uncond, cond) input of the
// next UNet call. (The step kernels hold both row indices from their eps loads and store through those.)
template <typename T>
__device__ __forceinline__ void store_pair(T* xin, long img, long rowvec, long col, const float* v) {
  using V8 = typename V8T<T>::type;
  const V8 o = round8<T>(v);
  ((V8*)xin)[2 * img * rowvec + col] = o;
  ((V8*)xin)[(2 * img + 1) * rowvec + col] = o;
}

// The step on one element: u / cv = the uncond / cond UNet output (the 16-bit values, or the fp32 overlap means of a canvas),
//   e = u + s (cv - u);  m = (x - sigma_t e) / alpha_t;  x_next = c_x x + c_m m + c_e e + c_p m_prev + c_n noise  -> x_next
// *mp / *nz (m_prev / noise) are read only where has_mp / has_nz; their coefficient is 0 otherwise.
__device__ __forceinline__ float step1(float u, float cv, float x, const float* mp, const float* nz, bool has_mp, bool has_nz,
                                       const StepCoef& c, float& m) {
  const float e = u + c.scale * (cv - u);
  m = (x - c.sigma_t * e) / c.alpha_t;
  float t = c.c_x * x + c.c_m * m + c.c_e * e;
  if (has_mp) t += c.c_p * *mp;
  if (has_nz) t += c.c_n * *nz;
  return t;
}

// Its backward on element k of a lane's 8. The step is linear in (eps, x, m_prev): with g = the gradient of x_next and
// G_m = g_m + c_m g (the use of m by the next step and by x_next),
//   g_x = c_x g + G_m / alpha_t,  g_e = c_e g - (sigma_t / alpha_t) G_m,  g_eps[2i] = (1 - s) g_e,  g_eps[2i+1] = s g_e,  g_m_prev = c_p g.
// The noise gets no gradient. inv_a = 1 / alpha_t; gm[k] is read only where has_gm; g_u / g_c are rounded to T once.
template <typename T>
__device__ __forceinline__ void step1_bwd(float g, const float* gm, bool has_gm, float inv_a, const StepCoef& c, int k, float* g_x,
                                          typename V8T<T>::type& g_u, typename V8T<T>::type& g_c, float* g_mp) {
  const float Gm = (has_gm ? gm[k] : 0.f) + c.c_m * g;
  g_x[k] = c.c_x * g + Gm * inv_a;
  const float ge = c.c_e * g - c.sigma_t * inv_a * Gm;
  g_u[k] = (T)((1.0f - c.scale) * ge);
  g_c[k] = (T)(c.scale * ge);
  g_mp[k] = c.c_p * g;
}

// Host side. The argument checks the four forward entry points share (square, masked, windows, windows masked), reported in this
// order: the required pointers, the blend's (masked: x0 / keep / qnoise are arguments of `what`; null otherwise), the entry point's own
// sizes() (STA_OK or its sta_fail), alignment, alpha_t.
template <typename Sizes>
STA_INLINE int sta_step_args_ok(const char* what, const void* eps, const float* x, const float* m_prev, const float* noise, const float* x_next,
                                const float* m, const void* xin, bool masked, const float* x0, const float* keep, const float* qnoise,
                                float alpha_t, Sizes&& sizes) {
  if (!eps || !x || !x_next || !m) return sta_fail(STA_E_ARG, "null pointer");
  if (masked && (!x0 || !keep || !qnoise)) return sta_fail(STA_E_ARG, "%s: x0, keep and qnoise are required (null pointer)", what);
  if (const int rc = sizes()) return rc;
  if (!sta_aligned16(eps) || !sta_aligned16(x) || !sta_aligned16(m_prev) || !sta_aligned16(noise) || !sta_aligned16(x0) || !sta_aligned16(keep) ||
      !sta_aligned16(qnoise) || !sta_aligned16(x_next) || !sta_aligned16(m) || !sta_aligned16(xin))
    return sta_fail(STA_E_ARG, "%s: every tensor must be 16-byte aligned", what);
  if (alpha_t == 0.f) return sta_fail(STA_E_ARG, "%s: alpha_t == 0", what);
  return STA_OK;
}

// Likewise the two backward entry points (masked: keep is an argument of `what`).
template <typename Sizes>
STA_INLINE int sta_step_bwd_args_ok(const char* what, const float* g_xn, const float* g_m, const float* g_x, const void* g_eps, const float* g_mprev,
                                    bool masked, const float* keep, float alpha_t, Sizes&& sizes) {
  if (!g_xn || !g_x || !g_eps) return sta_fail(STA_E_ARG, "null pointer");
  if (masked && !keep) return sta_fail(STA_E_ARG, "%s: keep is required (null pointer)", what);
  if (const int rc = sizes()) return rc;
  if (!sta_aligned16(g_xn) || !sta_aligned16(g_m) || !sta_aligned16(keep) || !sta_aligned16(g_x) || !sta_aligned16(g_eps) || !sta_aligned16(g_mprev))
    return sta_fail(STA_E_ARG, "%s: every tensor must be 16-byte aligned", what);
  if (alpha_t == 0.f) return sta_fail(STA_E_ARG, "%s: alpha_t == 0", what);
  return STA_OK;
}

}  // namespace
