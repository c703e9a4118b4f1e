// sta_blend_dev.h — the re-noising blend of inpainting, one definition for every kernel that applies it: the square-image kernels of
// sta_inpaint.hip and the canvas kernels of sta_window.hip (built with sta_sampler.hip). fp32, no fast-math flag in either unit.
#pragma once

#include <hip/hip_runtime.h>

// keep (q_a x0 + q_b n) + (1 - keep) x; keep == 0 hands x through untouched (bit-equal to the unmasked step, signed zeros included)
__device__ __forceinline__ float blend1(float kp, float x0, float n, float x, float q_a, float q_b) {
  const float q = q_a * x0 + q_b * n;
  return kp == 0.f ? x : kp * q + (1.0f - kp) * x;
}
