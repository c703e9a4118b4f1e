// sta_guide.hip — the latent update of attention-guided sampling (gfx950). C-ABI in include/sta_unet.h (sta_latent_guide).
// #included at the end of sta_sampler.hip (its flags: no -ffinite-math-only, a non-finite gradient must be seen); V8T / F4 / load8 /
// store8 / store_pair are those of sta_step_dev.h. Conventions of sta_sampler.hip / sta_inpaint.hip: a lane owns 8 consecutive elements
// of one image, 16-byte loads and stores, fp32 arithmetic, the mask [b][hw] read as 32 contiguous bytes at (8 col) % hw.
//
// The step needs the root mean square of an image's whole gradient before its first element can move. One launch, no atomics and no
// hand-off between workgroups: an image is shared by `parts` workgroups, and EVERY one of them reduces the whole image's gradient itself,
// in the same fixed order (lane t adds vectors t, t + 256, ... in turn, then a fixed LDS tree), so all of them hold the same bits of
// rms_i without talking to each other; each then updates its own slice of the image. The gradient of one image is 4 n bytes (64 KB at
// 512^2): the repeated reads and the second read of the slice are served by L2 / the Infinity Cache, HBM sees g once.
// The result depends on nothing but the image's own inputs: bit-reproducible from launch to launch, images independent of each other.

#include "sta_step_dev.h"

namespace {

constexpr int GUIDE_MAX_PARTS = 16;

// d = (g_u + g_c) (1 - keep) of one lane's 8 elements; kp == nullptr: factor 1
template <typename V8>
__device__ __forceinline__ void guide_d(const V8 gu, const V8 gc, const float* __restrict__ kp, float* d) {
  float k8[8];
  if (kp) load8(kp, k8);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float s = (float)gu[k] + (float)gc[k];
    d[k] = kp ? s * (1.0f - k8[k]) : s;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void latent_guide_kernel(const T* __restrict__ g, const float* __restrict__ x, const float* __restrict__ keep,
                                                           const float* __restrict__ step, float* __restrict__ x_out, T* __restrict__ xin,
                                                           float* __restrict__ stats, long rowvec, long hw, int parts, long chunk,
                                                           int normalize, float inv_scale) {
  using V8 = typename V8T<T>::type;
  __shared__ float red[256];
  const long img = blockIdx.x / parts;
  const int part = (int)(blockIdx.x - img * parts);
  const int tid = threadIdx.x;
  const V8* gu = (const V8*)g + 2 * img * rowvec;
  const V8* gc = gu + rowvec;
  const float* kp = keep ? keep + img * hw : nullptr;

  // the whole image's sum of squares, the same order in every workgroup of the image
  float acc = 0.f;
  for (long v = tid; v < rowvec; v += 256) {
    float d[8];
    guide_d<V8>(gu[v], gc[v], kp ? kp + (8 * v) % hw : nullptr, d);
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
  const float rms = sqrtf(red[0] / (float)(8 * rowvec));
  const bool live = (__float_as_uint(rms) & 0x7f800000u) != 0x7f800000u && rms > 0.f;      // finite (neither Inf nor NaN) and positive
  const float s = !live ? 0.f : normalize ? step[img] / rms : step[img] * inv_scale;

  // this workgroup's slice: x_out = x - s d (the slice's gradient read again), or x itself where the image is skipped
  const long end = (part + 1) * chunk < rowvec ? (part + 1) * chunk : rowvec;
  for (long v = part * chunk + tid; v < end; v += 256) {
    float xv[8], d[8];
    load8(x + 8 * (img * rowvec + v), xv);
    if (live) {
      guide_d<V8>(gu[v], gc[v], kp ? kp + (8 * v) % hw : nullptr, d);
#pragma unroll
      for (int k = 0; k < 8; ++k) xv[k] = xv[k] - s * d[k];
    }
    store8(x_out + 8 * (img * rowvec + v), xv);
    if (xin) store_pair(xin, img, rowvec, v, xv);
  }
  if (stats && part == 0 && tid == 0) stats[img] = rms;
}

inline bool guide_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int sta_latent_guide(const void* g, const float* x, const float* keep, const float* step, float* x_out, void* xin, float* stats,
                                long b, long n, long hw, int normalize, float inv_scale, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!g || !x || !step || !x_out) return sta_fail(STA_E_ARG, "latent_guide: null pointer");
  if (b <= 0 || n <= 0 || hw <= 0 || n % 8 || hw % 8 || n % hw)
    return sta_fail(STA_E_ARG, "latent_guide: b=%ld n=%ld hw=%ld (need n %% 8 == 0, hw %% 8 == 0 and n a multiple of hw)", b, n, hw);
  if (!sta_aligned16(g) || !sta_aligned16(x) || !sta_aligned16(keep) || !sta_aligned16(x_out) || !sta_aligned16(xin) ||
      ((uintptr_t)step & 3) || ((uintptr_t)stats & 3))
    return sta_fail(STA_E_ARG, "latent_guide: every tensor must be 16-byte aligned (step and stats: 4-byte)");
  const size_t f32 = (size_t)b * n * 4, pair16 = (size_t)b * n * 4;      // [b][n] fp32 and [2b][n] 16-bit are the same number of bytes
  const void* ins[] = {g, x, keep, step};
  const size_t in_bytes[] = {pair16, f32, (size_t)b * hw * 4, (size_t)b * 4};
  const void* outs[] = {x_out, xin, stats};
  const size_t out_bytes[] = {f32, pair16, (size_t)b * 4};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 4; ++i)
      if (guide_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return sta_fail(STA_E_ARG, "latent_guide: an output aliases an input");
    for (int p = o + 1; p < 3; ++p)
      if (guide_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) return sta_fail(STA_E_ARG, "latent_guide: two outputs alias each other");
  }
  const long rowvec = n / 8;
  long parts = (rowvec + 255) / 256;
  if (parts > GUIDE_MAX_PARTS) parts = GUIDE_MAX_PARTS;
  const long chunk = (rowvec + parts - 1) / parts;
  if (b * parts > 0x7fffffffL) return sta_fail(STA_E_UNSUP, "latent_guide: b=%ld images need more than 2^31 - 1 workgroups", b);
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<latent_guide_kernel<T>>("latent_guide", dim3((unsigned)(b * parts)), dim3(256), 0, (hipStream_t)stream, (const T*)g, x, keep,
                                              step, x_out, (T*)xin, stats, rowvec, hw, (int)parts, chunk, normalize, inv_scale);
  });
}
