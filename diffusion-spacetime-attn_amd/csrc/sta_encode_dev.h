// sta_encode_dev.h — from the encoder's output to the noised latent, per latent pixel: ONE definition for the square kernel
// (vae_encode_step_kernel, sta_encode.hip) and the canvas kernel (vae_encode_step_windows_kernel, sta_window.hip). fp32, force-inlined,
// no fast-math flag in either unit. The fused multiply-adds are written out (the ones the compiler formed by contraction in the square
// kernel before this header existed): which products a compiler contracts depends on the code around them, and the canvas kernel,
// which it vectorises over a lane's 8 pixels, must round exactly as the square one does.
#pragma once

#include <hip/hip_runtime.h>
#include "sta_internal.h"

namespace {      // internal to each unit, like the kernels that take a QuantConv

// quant_conv (8x8 1x1 + bias) held in registers for a kernel's whole grid-stride loop
struct QuantConv {
  float w[8][8], bias[8];
};

__device__ __forceinline__ void quant_conv_load(QuantConv& q, const float* __restrict__ qw, const float* __restrict__ qb) {
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    q.bias[o] = qb[o];
#pragma unroll
    for (int i = 0; i < 8; ++i) q.w[o][i] = qw[8 * o + i];
  }
}

// the 8 channels of one NHWC pixel of h -> its 8 moments: mo[0:4] the posterior's mean, mo[4:8] its logvar (not yet clamped)
template <typename T>
__device__ __forceinline__ void quant_moments(const QuantConv& q, const typename V8T<T>::type hv, float* mo) {
  float hf[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) hf[i] = (float)hv[i];
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    float s = q.bias[o];
#pragma unroll
    for (int i = 0; i < 8; ++i) s = __builtin_fmaf(q.w[o][i], hf[i], s);
    mo[o] = s;
  }
}

// DDIM's stochastic_encode of one latent element: x = sqrt_a z0 + sqrt_1ma n_enc (the last step of encode1, and the noising of
// latent_upscale_step_windows_kernel, sta_window.hip)
__device__ __forceinline__ float noise1(float z0, float n_enc, float sqrt_a, float sqrt_1ma) {
  return __builtin_fmaf(sqrt_1ma, n_enc, sqrt_a * z0);
}

// one channel of one pixel: the posterior's sample z0 = scale_factor (mean + exp(clamp(logvar, -30, 20) / 2) n_post) -> zz, and
// noise1 of it -> the result
__device__ __forceinline__ float encode1(float mean, float logvar_raw, float n_post, float n_enc, float scale_factor, float sqrt_a,
                                         float sqrt_1ma, float& zz) {
  const float logvar = fminf(fmaxf(logvar_raw, -30.f), 20.f);
  zz = scale_factor * __builtin_fmaf(expf(0.5f * logvar), n_post, mean);
  return noise1(zz, n_enc, sqrt_a, sqrt_1ma);
}

}  // namespace
