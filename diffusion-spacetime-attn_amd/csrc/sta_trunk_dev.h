// sta_trunk_dev.h — the arithmetic the trunk glue kernels must agree on, ONE definition each: the residual add + LayerNorm of a row
// held by a wave (sta_unet.hip: add_layernorm_kernel and its query-fragment form, sta_lnqkv.hip: the front end of ln_qkv_kernel,
// sta_unet_bwd.hip: the statistics of layernorm_bwd_kernel), the query-fragment LDS tile, the geometry and workspace layout of the
// NHWC GroupNorm forward and backward, and the erf / sigmoid pieces of GEGLU and SiLU and of their backwards. The consumers compare
// these kernels with torch.equal (tests/test_fused_gpu.py, tests/test_ln_qkv_gpu.py): "bit-identical" holds because they call the same
// functions, not because copies were kept alike. fp32, force-inlined: a kernel compiles to what it was with the expressions written
// out in it (profiles/trunk_one_definition.md). V8T and the grid rule of the elementwise launches (sta_grid_for) are in sta_internal.h.
//
// The helpers are small on purpose: arithmetic on one 8-channel chunk, one value or one index, with no branch and no loop over chunks
// inside. The predicates (does the lane hold this chunk? is the operand there?) and the loops stay in the kernels. Helpers that held
// them compiled to other code than the kernels had (the compiler simplifies a helper on its own before it inlines it); that document
// lists the shapes tried, and the three places that stay written out for this reason (the bias add of ln_qkv_kernel, the in-place
// centring of layernorm_bwd_kernel, the fold of a column's 8 channel sums into its groups in the two GroupNorm statistics kernels).
//
// Not here, on purpose:
//   - the LayerNorm epilogue of sta_rowgemm.hip: it reduces over MFMA accumulator lanes with bfly_sum, another data layout;
//   - gn_silu_kernel (NCHW) of sta_unet.hip: a workgroup reduction over one contiguous slab, nothing shared with the NHWC split;
//   - anything of sta_ffgemm.hip. Its GELU folds 0.3275911 * 0.70710678 into one constant, which rounds differently from
//     gelu_gate_parts below: it is another function and stays its own;
//   - the per-channel-statistics branch (cs_a / cs_b) of gn_nhwc_apply_kernel: one user;
//   - the C-ABI: no symbol, argument list, check order, error text, launch count or grid depends on this header
//     (include/*.h, sta/lib.py's SYMBOLS and the Python callers are as they were); of the blocks, only that of the NHWC GroupNorm
//     forward (gn_nhwc_threads).
#pragma once

#include <hip/hip_runtime.h>
#include "sta_internal.h"
#include "sta_wring_dev.h"

namespace {      // internal to each unit, like the kernels

// --------------------------------------------------------------------------------------------------
// LayerNorm of a row held by a wave. Lane `lane` holds the row's 8-channel chunks lane, lane + 64, ... (NV of them, chunk j exists
// where lane + 64 j < nvec = C / 8) as float v[NV][8]. Sums run over chunk 0's eight values, then chunk 1's, ...: the order is part
// of the contract. A kernel calls, per chunk it holds: ln_add8 (f, bias), ln_round8 (where s is stored), ln_sum8; then ln_mean;
// per chunk ln_sq8; then ln_rstd; per value ln_affine.
// --------------------------------------------------------------------------------------------------
// v += b, one operand (f or bias) of the residual add. An absent operand is not added: the caller tests its pointer, it never passes a
// zero-filled chunk.
template <typename T>
__device__ __forceinline__ void ln_add8(float* v, const typename V8T<T>::type& b) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] += (float)b[e];
}

// Where s is stored the residual stream continues in the activation dtype, so what is stored is what is normalised:
// v rounded through T, -> the 8 values to store
template <typename T>
__device__ __forceinline__ typename V8T<T>::type ln_round8(float* v) {
  typename V8T<T>::type o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    o[e] = (T)v[e];
    v[e] = (float)o[e];
  }
  return o;
}

// sum + the eight values of one chunk, in order
__device__ __forceinline__ float ln_sum8(float sum, const float* v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) sum += v[e];
  return sum;
}

// q + the eight (v - mean)^2 of one chunk, in order
__device__ __forceinline__ float ln_sq8(float q, const float* v, float mean) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float dlt = v[e] - mean;
    q += dlt * dlt;
  }
  return q;
}

// The row's mean and rstd = 1 / sqrt(var + eps) from the lane's shares of the two sums: its existing chunks through ln_sum8 / ln_sq8
// in chunk order. (Apart from the sums, so that a wave that holds several rows can sum all of them before the first reduction.)
__device__ __forceinline__ float ln_mean(float lane_sum, int C) { return wave_sum(lane_sum) / (float)C; }
__device__ __forceinline__ float ln_rstd(float lane_sq, int C, float eps) { return rsqrtf(wave_sum(lane_sq) / (float)C + eps); }

// y = (v - mean) rstd gamma + beta of one value (the caller rounds it to T)
__device__ __forceinline__ float ln_affine(float v, float mean, float rstd, float gamma, float beta) { return (v - mean) * rstd * gamma + beta; }

// --------------------------------------------------------------------------------------------------
// The query-fragment LDS tile: the normalised chunks of 16 rows cross it on their way from [16 rows][C / 8 chunks] to
// [C / 8 chunks][16 rows] in 16-byte units. A chunk takes 16 rows x 16 B + 16 B of padding: conflict-free 16-byte writes and reads.
// --------------------------------------------------------------------------------------------------
constexpr int QFRAG_CHUNK = 272;

// byte offset in the tile of the 16 bytes of chunk `chunk` (8 channels) of row `row16` (0 .. 15) of the group. The normalising lane
// stores its chunk there; slot t of the group's output is (t >> 4, t & 15); ln_qkv_kernel reads MFMA operand (4 f + g, c) instead.
__device__ __forceinline__ int qfrag_tile_at(int chunk, int row16) { return chunk * QFRAG_CHUNK + row16 * 16; }

// --------------------------------------------------------------------------------------------------
// GroupNorm on NHWC activations, forward (sta_unet.hip) and backward (sta_unet_bwd.hip): a workgroup of GN_NT threads takes one of
// gn_nhwc_chunks(HW) chunks of pixels of one image and ALL channels; a thread keeps one 8-channel column of every R-th pixel.
// Workspace: part[b][chunk][group][2] partial sums, folded per group by every workgroup of the second kernel. The backward reads
// the forward's workspace, so both take the layout from here.
// --------------------------------------------------------------------------------------------------
constexpr int GN_NT = 512;          // threads per workgroup: C / 8 <= 512 columns
constexpr int GN_MAXG = 64;

inline int gn_nhwc_chunks(int HW) {
  int n = HW / 8;
  if (n > 32) n = 32;
  if (n < 1) n = 1;
  return n;
}

// Threads the forward kernels are launched with: the R = GN_NT / (C / 8) working rows of gn_split, rounded up to whole waves (C = 2560:
// 320 instead of 512, of which 192 would idle). gn_split itself does not depend on it, so the backward keeps GN_NT.
inline int gn_nhwc_threads(int C) {
  const int CV = C >> 3;
  return (GN_NT / CV * CV + 63) & ~63;
}

// The shapes the split serves; `what` starts the error text ("groupnorm nhwc", "groupnorm nhwc bwd").
STA_INLINE int gn_nhwc_shape_ok(const char* what, int B, int C, int HW, int G) {
  if (B <= 0 || C <= 0 || HW <= 0 || G <= 0 || G > GN_MAXG || C % G || C % 8 || (C / G < 8 && C / G != 4) || C / 8 > GN_NT)
    return sta_fail(STA_E_ARG, "%s: B=%d C=%d HW=%d G=%d (need C %% 8 == 0, C/G >= 8 or == 4, C <= %d, G <= %d)", what, B, C, HW, G,
                    8 * GN_NT, GN_MAXG);
  return STA_OK;
}

// A thread's place: column col (channels 8 col .. + 7) of the pixels row, row + R, ... of the chunk; threads with row >= R idle.
struct GnSplit {
  int CV, R, Cg, row, col;
};
__device__ __forceinline__ GnSplit gn_split(int C, int G) {
  GnSplit s;
  s.CV = C >> 3;
  s.R = GN_NT / s.CV;
  s.Cg = C / G;
  s.row = threadIdx.x / s.CV;
  s.col = threadIdx.x - s.row * s.CV;
  return s;
}

// the workspace: where the two partial sums of group g of chunk k of image b start
__device__ __forceinline__ size_t gn_part_at(int b, size_t nchunk, int k, int G, int g) { return ((size_t)b * nchunk + k) * 2 * G + 2 * g; }

// a group's mean and rstd from its sum s and sum of squares q; inv_n = 1 / (Cg HW)
__device__ __forceinline__ void gn_mean_rstd(float s, float q, float inv_n, float eps, float& mean, float& rstd) {
  const float m = s * inv_n;
  mean = m;
  rstd = rsqrtf(fmaxf(q * inv_n - m * m, 0.f) + eps);
}

// --------------------------------------------------------------------------------------------------
// GELU (exact erf form) and SiLU pieces, forward and backward
// --------------------------------------------------------------------------------------------------
// From the gate g: er = 1 - erf(|g| / sqrt 2) and ex = exp(-g^2 / 2). erf from Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7
// absolute: 2000x below one ulp of the 16-bit result around 1): a reciprocal, five fma and one exp2 instead of libm's branchy erff.
__device__ __forceinline__ void gelu_gate_parts(float g, float& er, float& ex) {
  const float x = fabsf(g) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, x, 1.0f));
  float p = __builtin_fmaf(1.061405429f, t, -1.453152027f);
  p = __builtin_fmaf(p, t, 1.421413741f);
  p = __builtin_fmaf(p, t, -0.284496736f);
  p = __builtin_fmaf(p, t, 0.254829592f);
  ex = __builtin_amdgcn_exp2f(-1.4426950408889634f * x * x);
  er = p * t * ex;
}

// Phi(g), the normal distribution function, from er
__device__ __forceinline__ float gelu_cdf(float g, float er) { return g >= 0.f ? 1.0f - 0.5f * er : 0.5f * er; }

__device__ __forceinline__ float sigmoid_f(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

}  // namespace
