// sta_unet.hip — HBM-bound glue kernels of the UNet trunk around the cross-attention path (gfx950).
// C-ABI in include/sta_unet.h. Every kernel is one pass over its activations with 16-byte accesses per lane,
// fp32 arithmetic, and no LDS beyond a few floats for workgroup reductions: the roofline that bounds them is
// HBM bandwidth (algorithmic bytes: read every input once, write every output once).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sta_xattn.h"
#include "sta_unet.h"
#include "sta_internal.h"
#include "sta_trunk_dev.h"

namespace {

// sum over the workgroup; `sh` holds NT/64 floats; every thread gets the result
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  if constexpr (NT == 64) return v;
  __syncthreads();                       // sh may still be read from a previous reduction
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) t += sh[w];
  return t;
}

__device__ __forceinline__ float silu_f(float v) { return v * sigmoid_f(v); }

// --------------------------------------------------------------------------------------------------
// GroupNorm (+ per-(b,c) pre-add) (+ SiLU), NCHW. One workgroup per (b, group) slab of Cg*HW contiguous
// elements. CACHED: the slab (<= NT*NV*8 elements) stays in registers between statistics and output.
// --------------------------------------------------------------------------------------------------
template <typename T, int NT, int NV, bool CACHED>
__global__ __launch_bounds__(NT) void gn_silu_kernel(const T* __restrict__ x, const float* __restrict__ add,
                                                    const T* __restrict__ gamma, const T* __restrict__ beta,
                                                    T* __restrict__ y, int C, int HW, int G, float eps, int silu) {
  using V8 = typename V8T<T>::type;
  __shared__ float sh[NT / 64];
  const int Cg = C / G;
  const int b = blockIdx.x / G, g = blockIdx.x % G;
  const size_t base = ((size_t)b * C + (size_t)g * Cg) * HW;
  const int n = Cg * HW, nvec = n >> 3;
  const int c0 = g * Cg;
  const V8* xv = (const V8*)(x + base);
  V8* yv = (V8*)(y + base);
  const float* addb = add ? add + (size_t)b * C + c0 : nullptr;
  const float inv_n = 1.0f / (float)n;

  if constexpr (CACHED) {
    float v[NV][8];
    int ch[NV];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = threadIdx.x + j * NT;
      ch[j] = 0;
      if (idx < nvec) {
        const V8 r = xv[idx];
        ch[j] = (idx << 3) / HW;
        const float a = addb ? addb[ch[j]] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[j][e] = (float)r[e] + a;
          s += v[j][e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
      }
    }
    const float mean = block_sum<NT>(s, sh) * inv_n;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
      if (threadIdx.x + j * NT < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float dlt = v[j][e] - mean;
          q += dlt * dlt;
        }
      }
    const float rstd = rsqrtf(block_sum<NT>(q, sh) * inv_n + eps);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = threadIdx.x + j * NT;
      if (idx < nvec) {
        const float gm = (float)gamma[c0 + ch[j]] * rstd;
        const float bt = (float)beta[c0 + ch[j]] - mean * gm;
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float t = v[j][e] * gm + bt;
          if (silu) t = silu_f(t);
          o[e] = (T)t;
        }
        yv[idx] = o;
      }
    }
  } else {
    float s = 0.f, q = 0.f;
    for (int idx = threadIdx.x; idx < nvec; idx += NT) {
      const V8 r = xv[idx];
      const float a = addb ? addb[(idx << 3) / HW] : 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t = (float)r[e] + a;
        s += t;
        q += t * t;
      }
    }
    const float mean = block_sum<NT>(s, sh) * inv_n;
    const float var = fmaxf(block_sum<NT>(q, sh) * inv_n - mean * mean, 0.f);
    const float rstd = rsqrtf(var + eps);
    for (int idx = threadIdx.x; idx < nvec; idx += NT) {
      const V8 r = xv[idx];                       // second read: L2 / Infinity Cache
      const int ch = (idx << 3) / HW;
      const float a = addb ? addb[ch] : 0.f;
      const float gm = (float)gamma[c0 + ch] * rstd;
      const float bt = (float)beta[c0 + ch] - mean * gm + a * gm;
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = (float)r[e] * gm + bt;
        if (silu) t = silu_f(t);
        o[e] = (T)t;
      }
      yv[idx] = o;
    }
  }
}

// --------------------------------------------------------------------------------------------------
// GroupNorm (+ pre-add) (+ SiLU) on NHWC ("channels_last") activations: x, y [B][HW][C].
// A (b, group) slab is strided here (Cg channels of every pixel), so the work is split the other way: a workgroup
// takes a chunk of pixels of one image and ALL channels — fully coalesced rows — and a thread keeps one fixed
// 8-channel column (16 bytes) of every R-th pixel. Kernel 1 writes per-chunk partial sums per group, kernel 2
// folds them (tiny) and normalises. x is read twice (the second time mostly from L2 / Infinity Cache). The split, the workspace
// layout and a group's mean / rstd come from sta_trunk_dev.h, as in the backward (sta_unet_bwd.hip).
//
// The streaming loop of both kernels takes U pixels per trip (statistics: GN_U; apply: 2 or 4, chosen by the launch): the U 16-byte
// loads are issued first, from a pixel index clamped to the image's last pixel (always a valid address, so nothing branches around a
// load), then the U transforms follow. The apply kernel's whole trips carry no predicate and one partial trip follows under p < p1;
// the statistics kernel predicates its sums. The apply kernel issues its first trip's loads and its gamma / beta /
// add vectors before the statistics fold and the barrier, so the fold runs under their latency. The fold gives 16 lanes to a
// group: lane l adds the group's channels (or chunks) l, l + 16, ... in this order, one DPP row reduction adds the 16 lanes — a
// fixed shape, no atomics. Both kernels are launched with gn_nhwc_threads(C) threads: the working rows, rounded up to whole waves.
// --------------------------------------------------------------------------------------------------
constexpr int GN_U = 2;             // pixels per trip of the statistics kernel
constexpr int GN_LONG_TRIPS = 10;   // pixels per thread from which the apply kernel runs 4 per trip with streaming loads

typedef __attribute__((ext_vector_type(4))) float gn_f4;
typedef __attribute__((ext_vector_type(2))) float gn_f2;

// the 8 pre-add values of image b's channels 8 col .. + 7 as two 16-byte loads (zeros without add)
__device__ __forceinline__ void gn_load_add8(const float* __restrict__ add, int b, int C, int col, float* a) {
  gn_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  if (add) {
    const gn_f4* ap = (const gn_f4*)(add + (size_t)b * C + col * 8);
    a0 = ap[0];
    a1 = ap[1];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = a0[e];
    a[4 + e] = a1[e];
  }
}

template <typename T>
__global__ __launch_bounds__(GN_NT) void gn_nhwc_stats_kernel(const T* __restrict__ x, const T* __restrict__ xb, int Ca, const float* __restrict__ add,
                                                             float* __restrict__ part, int C, int HW, int G, int chunk_px) {
  using V8 = typename V8T<T>::type;
  __shared__ float acc[2 * GN_MAXG];
  const GnSplit sp = gn_split(C, G);
  const int R = sp.R, Cg = sp.Cg, row = sp.row, col = sp.col;
  const int b = blockIdx.y, chunk = blockIdx.x;
  if (threadIdx.x < 2 * G) acc[threadIdx.x] = 0.f;
  __syncthreads();
  if (row < R) {
    float a[8], s[8], q[8];
    gn_load_add8(add, b, C, col, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[e] = 0.f;
      q[e] = 0.f;
    }
    const int p1 = min(HW, (chunk + 1) * chunk_px);
    // (xb: the input is the channel concatenation [x | xb] of two tensors with Ca and C - Ca channels, read in place)
    const bool second = xb && col * 8 >= Ca;
    const int ld = xb ? (second ? C - Ca : Ca) : C;
    const T* src = (second ? xb + (col * 8 - Ca) : x + col * 8) + (size_t)b * HW * ld;
    for (int p = chunk * chunk_px + row; p < p1; p += GN_U * R) {
      V8 v[GN_U];
#pragma unroll
      for (int j = 0; j < GN_U; ++j) v[j] = *(const V8*)(src + (size_t)min(p + j * R, HW - 1) * ld);
#pragma unroll
      for (int j = 0; j < GN_U; ++j)
        if (p + j * R < p1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float t = (float)v[j][e] + a[e];
            s[e] += t;
            q[e] += t * t;
          }
        }
    }
    // fold the 8 channels into their (at most two: Cg >= 8 or Cg == 4) groups, then one LDS atomic per group and moment
    // (gn_nhwc_bwd_kernel folds its two sums the same way)
    const int g0 = (col * 8) / Cg, g1 = (col * 8 + 7) / Cg;
    float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool first = (col * 8 + e) / Cg == g0;
      s0 += first ? s[e] : 0.f;
      q0 += first ? q[e] : 0.f;
      s1 += first ? 0.f : s[e];
      q1 += first ? 0.f : q[e];
    }
    atomicAdd(&acc[2 * g0], s0);
    atomicAdd(&acc[2 * g0 + 1], q0);
    if (g1 != g0) {
      atomicAdd(&acc[2 * g1], s1);
      atomicAdd(&acc[2 * g1 + 1], q1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * G) part[gn_part_at(b, gridDim.x, chunk, G, 0) + threadIdx.x] = acc[threadIdx.x];
}

// U: pixels per trip. STREAM: x is loaded non-temporally (it is read for the last time here — the statistics kernel, where there
// is one, has read it before). The launch picks <4, true> where a thread has at least GN_LONG_TRIPS pixels and <2, false> below:
// measured per shape in profiles/gn_stream.md (U = 4 holds 74 VGPRs, 6 waves per SIMD, and wins only with the streaming loads and
// enough trips to use them; U = 2 holds 62, 8 waves, and starts its few trips sooner).
template <typename T, int U, bool STREAM>
__global__ __launch_bounds__(GN_NT) void gn_nhwc_apply_kernel(const T* __restrict__ x, const T* __restrict__ xb, int Ca, const float* __restrict__ add,
                                                             const float* __restrict__ cs_a, const float* __restrict__ cs_b,
                                                             const T* __restrict__ gamma, const T* __restrict__ beta,
                                                             const float* __restrict__ part, T* __restrict__ y, int C, int HW,
                                                             int G, int chunk_px, float eps, int silu) {
  using V8 = typename V8T<T>::type;
  __shared__ float mean_s[GN_MAXG], rstd_s[GN_MAXG];
  const GnSplit sp = gn_split(C, G);
  const int R = sp.R, Cg = sp.Cg, row = sp.row, col = sp.col;
  const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  // A thread of a row past R (the last wave's spare lanes) keeps a valid column and an empty pixel range: it loads and stores nothing
  // of its own but takes part in the fold.
  const int p1 = min(HW, (chunk + 1) * chunk_px);
  const bool second = xb && col * 8 >= Ca;
  const int ld = xb ? (second ? C - Ca : Ca) : C;
  const T* src = (second ? xb + (col * 8 - Ca) : x + col * 8) + (size_t)b * HW * ld;
  T* dst = y + (size_t)b * HW * C + col * 8;
  int p = row < R ? chunk * chunk_px + row : p1;
  auto load = [&](int pix) {
    const V8* at = (const V8*)(src + (size_t)min(pix, HW - 1) * ld);
    if constexpr (STREAM) return __builtin_nontemporal_load(at);
    else return *at;
  };
  // in flight across the fold: the first trip's pixels and the column's parameters
  V8 v[U];
#pragma unroll
  for (int j = 0; j < U; ++j) v[j] = load(p + j * R);
  const V8 gv = *(const V8*)(gamma + col * 8), bv = *(const V8*)(beta + col * 8);
  float a[8];
  gn_load_add8(add, b, C, col, a);

  // The fold: lanes 16 g' .. 16 g' + 15 of the workgroup take group g' (+ blockDim / 16 per round), lane l its items l, l + 16, ...
  const int l16 = threadIdx.x & 15;
  for (int g = threadIdx.x >> 4; g < G; g += blockDim.x >> 4) {
    float s = 0.f, q = 0.f;
    if (cs_a) {
      // statistics accumulated per CHANNEL by the producing kernel (sum S_c, sum of squares Q_c of the stored values; csrc/sta_conv.hip,
      // sta_gemm.hip): with the per-(b, c) pre-add a, sum (x + a) = S + HW a and sum (x + a)^2 = Q + 2 a S + HW a^2
      const int Cb = C - Ca;
#pragma unroll 1
      for (int c = g * Cg + l16; c < (g + 1) * Cg; c += 16) {
        const gn_f2 st = *(const gn_f2*)((cs_b && c >= Ca) ? cs_b + ((size_t)b * Cb + (c - Ca)) * 2 : cs_a + ((size_t)b * (cs_b ? Ca : C) + c) * 2);
        const float ac = add ? add[(size_t)b * C + c] : 0.f;
        s += st[0] + (float)HW * ac;
        q += st[1] + 2.f * ac * st[0] + (float)HW * ac * ac;
      }
    } else {
#pragma unroll 2
      for (int k = l16; k < nchunk; k += 16) {
        const gn_f2 pr = *(const gn_f2*)(part + gn_part_at(b, nchunk, k, G, g));
        s += pr[0];
        q += pr[1];
      }
    }
    s = row16_sum(s);
    q = row16_sum(q);
    if (l16 == 0) gn_mean_rstd(s, q, 1.0f / ((float)Cg * (float)HW), eps, mean_s[g], rstd_s[g]);
  }
  __syncthreads();
  // a column lies in at most two groups (Cg >= 8 or Cg == 4): its first n0 channels in g0, the others in g0 + 1
  const int g0 = (col * 8) / Cg, g1 = min(g0 + 1, G - 1), n0 = (g0 + 1) * Cg - col * 8;
  const float mean0 = mean_s[g0], rstd0 = rstd_s[g0], mean1 = mean_s[g1], rstd1 = rstd_s[g1];
  float gm[8], bt[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    gm[e] = (float)gv[e] * (e < n0 ? rstd0 : rstd1);
    bt[e] = (float)bv[e] + (a[e] - (e < n0 ? mean0 : mean1)) * gm[e];
  }
  auto put = [&](int j) {
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = (float)v[j][e] * gm[e] + bt[e];
      if (silu) t = silu_f(t);
      o[e] = (T)t;
    }
    *(V8*)(dst + (size_t)(p + j * R) * C) = o;
  };
  // whole trips carry no predicate (every load is consumed before its registers are loaded again, so no wait drains the stores);
  // the last, partial trip follows once
  while (p + (U - 1) * R < p1) {
#pragma unroll
    for (int j = 0; j < U; ++j) put(j);
    p += U * R;
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = load(p + j * R);
  }
#pragma unroll
  for (int j = 0; j < U - 1; ++j)
    if (p + j * R < p1) put(j);
}

// partial[b][slot][c][2] (the epilogues of csrc/sta_conv.hip / sta_gemm.hip) -> stats[b][c][2]: fixed summation order, no atomics.
// A workgroup folds 64 consecutive floats of one image: 16 lanes x float4 across, 16 slot groups down (slots k = sg, sg + 16, ...),
// then a 16-way tree through LDS — 16-byte loads, at most slots / 16 of them in a thread's chain.
__global__ __launch_bounds__(256) void stats_finalize_kernel(const float* __restrict__ partial, float* __restrict__ stats, int slots, int C) {
  typedef __attribute__((ext_vector_type(4))) float f4;
  __shared__ f4 red[16][16];
  const int col = threadIdx.x & 15, sg = threadIdx.x >> 4, b = blockIdx.y;
  const int i = (blockIdx.x * 16 + col) * 4;                 // first of this lane's four floats inside the 2 C of an image
  f4 s = {0.f, 0.f, 0.f, 0.f};
  if (i < 2 * C) {
    const float* src = partial + (size_t)b * slots * 2 * C + i;
    for (int k = sg; k < slots; k += 16) s += *(const f4*)(src + (size_t)k * 2 * C);
  }
  red[sg][col] = s;
  __syncthreads();
  if (sg == 0 && i < 2 * C) {
#pragma unroll
    for (int k = 1; k < 16; ++k) s += red[k][col];
    *(f4*)(stats + (size_t)b * 2 * C + i) = s;
  }
}

// y = a + b + bias[c] over [rows][C] (NHWC activations or token tensors)
template <typename T>
__global__ __launch_bounds__(256) void add_bias_rows_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                          const T* __restrict__ bias, T* __restrict__ y, long nvec, int CV) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
    const V8 av = ((const V8*)a)[i];
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (float)av[e];
    if (b) {
      const V8 bv = ((const V8*)b)[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] += (float)bv[e];
    }
    if (bias) {
      const V8 cv = ((const V8*)bias)[(int)(i % CV)];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] += (float)cv[e];
    }
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (T)t[e];
    ((V8*)y)[i] = o;
  }
}

// --------------------------------------------------------------------------------------------------
// GEGLU: y[r][j] = x[r][j] * gelu(x[r][D + j])
// --------------------------------------------------------------------------------------------------
// exact-erf GELU with the polynomial erf of sta_trunk_dev.h instead of libm's branchy erff: 434 -> 410 us at [262144 x 2560] (4.9 TB/s
// of reads + writes), 216 -> 195 us at [65536 x 5120].
__device__ __forceinline__ float gelu_erf(float g) {
  float er, ex;
  gelu_gate_parts(g, er, ex);
  return g * gelu_cdf(g, er);
}

template <typename T>
__global__ __launch_bounds__(256) void geglu_kernel(const T* __restrict__ x, T* __restrict__ y, long nvec, int Dv) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;      // (4 vectors per thread and iteration measured no better: 418 vs 410 us)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
    const long r = i / Dv;
    const int j = (int)(i - r * Dv);
    const V8 a = ((const V8*)x)[r * 2 * Dv + j];
    const V8 gt = ((const V8*)x)[r * 2 * Dv + Dv + j];
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (T)((float)a[e] * gelu_erf((float)gt[e]));
    ((V8*)y)[i] = o;
  }
}

// --------------------------------------------------------------------------------------------------
// s = x + f + bias; y = LayerNorm(s) * gamma + beta. One wave per row, C <= 2048.
// --------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void add_layernorm_kernel(const T* __restrict__ x, const T* __restrict__ f,
                                                          const T* __restrict__ bias, const T* __restrict__ gamma,
                                                          const T* __restrict__ beta, T* s_out, T* __restrict__ y,
                                                          long R, int C, float eps) {
  using V8 = typename V8T<T>::type;
  constexpr int NV = 4;                                   // vectors per lane: C <= 64 * 4 * 8
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int lane = threadIdx.x & 63, nvec = C >> 3;
  const V8* xr = (const V8*)(x + row * C);
  const V8* fr = f ? (const V8*)(f + row * C) : nullptr;
  float v[NV][8];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = lane + 64 * j;
    if (idx < nvec) {
      const V8 a = xr[idx];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[j][e] = (float)a[e];
      if (fr) ln_add8<T>(v[j], fr[idx]);
      if (bias) ln_add8<T>(v[j], ((const V8*)bias)[idx]);
      if (s_out) ((V8*)(s_out + row * C))[idx] = ln_round8<T>(v[j]);
      sum = ln_sum8(sum, v[j]);
    }
  }
  const float mean = ln_mean(sum, C);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (lane + 64 * j < nvec) q = ln_sq8(q, v[j], mean);
  const float rstd = ln_rstd(q, C, eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = lane + 64 * j;
    if (idx < nvec) {
      const V8 gm = ((const V8*)gamma)[idx], bt = ((const V8*)beta)[idx];
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (T)ln_affine(v[j][e], mean, rstd, (float)gm[e], (float)bt[e]);
      ((V8*)(y + row * C))[idx] = o;
    }
  }
}

// --------------------------------------------------------------------------------------------------
// The same pass with y written in QUERY-FRAGMENT order — the layout sta_xattn_fwd_proj_qfrag consumes. y = norm2(x) at
// SD-v1 level 0 has exactly one consumer, the projection-fused cross-attention kernel, whose MFMA B operand wants lane
// (g, c) of a wave to hold 16 bytes of pixel c: read from row-major [R][C] that is 16 half-used 128-byte lines per load
// instruction (the shape profiles/r03_vmem_shapes.txt prices at 1.5x the adjacent-lane one). Here the 16 rows of a pixel
// group leave as C/32 fragments of 1 KiB: fragment s holds, at byte (16 g + c) * 16, channels 32 s + 8 g .. + 7 of row c —
// a transpose of [16 rows][C/8 chunks] to [C/8 chunks][16 rows] in 16-byte units, (R/16) * (C/32) KiB in all (the same
// bytes as row-major). One workgroup = one group of 16 rows, a wave takes 4 of them (the row helpers and lane assignment
// of add_layernorm_kernel: bit-identical values); the chunks cross the LDS tile of sta_trunk_dev.h so that the stores are
// 1-KiB contiguous per wave instruction. A lane holds NV chunks of each of its rows: NV = 1 for C <= 512 (SD-v1 level 0), NV = 2
// for 512 < C <= 1024 (level 1, C = 640: norm2's output feeding the locals-from-L2 projection-fused kernel of csrc/sta_xattn_proj.hip).
// --------------------------------------------------------------------------------------------------
template <typename T, int NV>
__global__ __launch_bounds__(256) void add_layernorm_qfrag_kernel(const T* __restrict__ x, const T* __restrict__ f,
                                                                const T* __restrict__ bias, const T* __restrict__ gamma,
                                                                const T* __restrict__ beta, T* s_out, T* __restrict__ y,
                                                                long R, int C, float eps) {
  using V8 = typename V8T<T>::type;
  __shared__ __attribute__((aligned(16))) char tile[64 * NV * QFRAG_CHUNK];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nvec = C >> 3;
  const long row0 = (long)blockIdx.x * 16 + 4 * wv;
  float v[4][NV][8];
  float sum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {                           // every load of the wave's four rows is issued before the first use
    const long row = row0 + r;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = lane + 64 * j;
      V8 a = {}, b = {};
      if (idx < nvec) {
        a = ((const V8*)(x + row * C))[idx];
        if (f) b = ((const V8*)(f + row * C))[idx];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[r][j][e] = (float)a[e];
      if (f) ln_add8<T>(v[r][j], b);
    }
  }
  V8 bs[NV] = {}, gm[NV] = {}, bt[NV] = {};
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = lane + 64 * j;
    if (idx < nvec) {
      if (bias) bs[j] = ((const V8*)bias)[idx];
      gm[j] = ((const V8*)gamma)[idx];
      bt[j] = ((const V8*)beta)[idx];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long row = row0 + r;
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = lane + 64 * j;
      if (bias) ln_add8<T>(v[r][j], bs[j]);
      if (s_out) {
        const V8 o = ln_round8<T>(v[r][j]);
        if (idx < nvec) ((V8*)(s_out + row * C))[idx] = o;
      }
      if (idx < nvec) t = ln_sum8(t, v[r][j]);
    }
    sum[r] = t;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float mean = ln_mean(sum[r], C);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
      if (lane + 64 * j < nvec) q = ln_sq8(q, v[r][j], mean);
    const float rstd = ln_rstd(q, C, eps);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int idx = lane + 64 * j;
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (T)ln_affine(v[r][j][e], mean, rstd, (float)gm[j][e], (float)bt[j][e]);
      if (idx < nvec) *(V8*)(tile + qfrag_tile_at(idx, 4 * wv + r)) = o;
    }
  }
  __syncthreads();
  V8* yo = (V8*)y + (size_t)blockIdx.x * nvec * 16;
  for (int t = threadIdx.x; t < nvec * 16; t += 256) yo[t] = *(const V8*)(tile + qfrag_tile_at(t >> 4, t & 15));
}

// --------------------------------------------------------------------------------------------------
// y = a + b + bias[c] over [B][C][HW]
// --------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void add_bias_nchw_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                          const T* __restrict__ bias, T* __restrict__ y, long nvec,
                                                          int C, int HWv) {
  using V8 = typename V8T<T>::type;
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
    const V8 av = ((const V8*)a)[i];
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (float)av[e];
    if (b) {
      const V8 bv = ((const V8*)b)[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] += (float)bv[e];
    }
    if (bias) {
      const float bc = (float)bias[(int)((i / HWv) % C)];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] += bc;
    }
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (T)t[e];
    ((V8*)y)[i] = o;
  }
}

template <typename T>
int gn_dispatch(const void* x, const float* add, const void* gamma, const void* beta, void* y, int B, int C, int HW,
                int G, float eps, int silu, hipStream_t st) {
  const long nvec = (long)(C / G) * HW / 8;
  const dim3 grid(B * G);
  const char* const what = "groupnorm_silu launch";
  const T *xt = (const T*)x, *g = (const T*)gamma, *b = (const T*)beta;
  T* yt = (T*)y;
  if (nvec <= 256 * 2) return sta_launch<gn_silu_kernel<T, 256, 2, true>>(what, grid, dim3(256), 0, st, xt, add, g, b, yt, C, HW, G, eps, silu);
  if (nvec <= 256 * 8) return sta_launch<gn_silu_kernel<T, 256, 8, true>>(what, grid, dim3(256), 0, st, xt, add, g, b, yt, C, HW, G, eps, silu);
  if (nvec <= 1024 * 4) return sta_launch<gn_silu_kernel<T, 1024, 4, true>>(what, grid, dim3(1024), 0, st, xt, add, g, b, yt, C, HW, G, eps, silu);
  if (nvec <= 1024 * 8) return sta_launch<gn_silu_kernel<T, 1024, 8, true>>(what, grid, dim3(1024), 0, st, xt, add, g, b, yt, C, HW, G, eps, silu);
  return sta_launch<gn_silu_kernel<T, 1024, 1, false>>(what, grid, dim3(1024), 0, st, xt, add, g, b, yt, C, HW, G, eps, silu);
}

}  // namespace

// the apply kernel's launch: pixels per trip and load policy by the pixels a thread has (chunk_px over the R rows of the split)
template <typename T>
static int gn_nhwc_apply_launch(const char* what, dim3 grid, hipStream_t st, const T* x, const T* xb, int Ca, const float* add, const float* cs_a,
                                const float* cs_b, const T* gamma, const T* beta, const float* part, T* y, int C, int HW, int G, int chunk_px, float eps,
                                int silu) {
  const dim3 block(gn_nhwc_threads(C));
  if (chunk_px / (GN_NT / (C >> 3)) >= GN_LONG_TRIPS)
    return sta_launch<gn_nhwc_apply_kernel<T, 4, true>>(what, grid, block, 0, st, x, xb, Ca, add, cs_a, cs_b, gamma, beta, part, y, C, HW, G, chunk_px, eps,
                                                        silu);
  return sta_launch<gn_nhwc_apply_kernel<T, 2, false>>(what, grid, block, 0, st, x, xb, Ca, add, cs_a, cs_b, gamma, beta, part, y, C, HW, G, chunk_px, eps,
                                                       silu);
}

extern "C" {

int sta_groupnorm_silu(const void* x, const float* add, const void* gamma, const void* beta, void* y, int B, int C,
                       int HW, int G, float eps, int silu, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !gamma || !beta || !y) return sta_fail(STA_E_ARG, "null pointer");
  if (B <= 0 || C <= 0 || HW <= 0 || G <= 0 || C % G || HW % 8)
    return sta_fail(STA_E_ARG, "groupnorm: B=%d C=%d HW=%d G=%d (need C %% G == 0, HW %% 8 == 0)", B, C, HW, G);
  return sta_by_dtype(dtype, [&](auto tag) {
    return gn_dispatch<decltype(tag)>(x, add, gamma, beta, y, B, C, HW, G, eps, silu, (hipStream_t)stream);
  });
}

int sta_geglu(const void* x, void* y, long R, int D, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !y) return sta_fail(STA_E_ARG, "null pointer");
  if (R <= 0 || D <= 0 || D % 8) return sta_fail(STA_E_ARG, "geglu: R=%ld D=%d (need D %% 8 == 0)", R, D);
  const long nvec = R * (D / 8);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<geglu_kernel<T>>("geglu launch", dim3(sta_grid_for(nvec)), dim3(256), 0, st, (const T*)x, (T*)y, nvec, D / 8);
  });
}

int sta_add_layernorm(const void* x, const void* f, const void* bias, const void* gamma, const void* beta, void* s,
                      void* y, long R, int C, float eps, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !gamma || !beta || !y) return sta_fail(STA_E_ARG, "null pointer");
  if (R <= 0 || C <= 0 || C % 8 || C > 2048) return sta_fail(STA_E_ARG, "add_layernorm: R=%ld C=%d (need C %% 8 == 0, C <= 2048)", R, C);
  const unsigned blocks = (unsigned)((R + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<add_layernorm_kernel<T>>("add_layernorm launch", dim3(blocks), dim3(256), 0, st, (const T*)x, (const T*)f, (const T*)bias,
                                               (const T*)gamma, (const T*)beta, (T*)s, (T*)y, R, C, eps);
  });
}

int sta_add_layernorm_qfrag(const void* x, const void* f, const void* bias, const void* gamma, const void* beta, void* s,
                            void* y, long R, int C, float eps, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !gamma || !beta || !y) return sta_fail(STA_E_ARG, "null pointer");
  if (R <= 0 || R % 16 || C <= 0 || C % 32 || C > 1024)
    return sta_fail(STA_E_ARG, "add_layernorm_qfrag: R=%ld C=%d (need R %% 16 == 0, C %% 32 == 0, C <= 1024)", R, C);
  const unsigned blocks = (unsigned)(R / 16);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const char* const what = "add_layernorm_qfrag launch";
    const T *xt = (const T*)x, *ft = (const T*)f, *bs = (const T*)bias, *g = (const T*)gamma, *b = (const T*)beta;
    if (C > 512)      // two chunks per lane
      return sta_launch<add_layernorm_qfrag_kernel<T, 2>>(what, dim3(blocks), dim3(256), 0, st, xt, ft, bs, g, b, (T*)s, (T*)y, R, C, eps);
    return sta_launch<add_layernorm_qfrag_kernel<T, 1>>(what, dim3(blocks), dim3(256), 0, st, xt, ft, bs, g, b, (T*)s, (T*)y, R, C, eps);
  });
}

int sta_add_bias_nchw(const void* a, const void* b, const void* bias, void* y, int B, int C, int HW, int dtype,
                      void* stream) {
  g_sta_err[0] = 0;
  if (!a || !y) return sta_fail(STA_E_ARG, "null pointer");
  if (B <= 0 || C <= 0 || HW <= 0 || HW % 8) return sta_fail(STA_E_ARG, "add_bias: B=%d C=%d HW=%d (need HW %% 8 == 0)", B, C, HW);
  const long nvec = (long)B * C * (HW / 8);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<add_bias_nchw_kernel<T>>("add_bias_nchw launch", dim3(sta_grid_for(nvec)), dim3(256), 0, st, (const T*)a, (const T*)b,
                                               (const T*)bias, (T*)y, nvec, C, HW / 8);
  });
}

size_t sta_groupnorm_nhwc_workspace_bytes(int B, int HW, int G) {
  if (B <= 0 || HW <= 0 || G <= 0) return 0;
  return (size_t)B * gn_nhwc_chunks(HW) * 2 * G * sizeof(float);
}

static int groupnorm_silu_nhwc_impl(const void* x, const void* xb, int Ca, const float* add, const void* gamma, const void* beta, void* y,
                                    void* workspace, int B, int C, int HW, int G, float eps, int silu, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !gamma || !beta || !y || !workspace) return sta_fail(STA_E_ARG, "null pointer");
  if (const int rc = gn_nhwc_shape_ok("groupnorm nhwc", B, C, HW, G)) return rc;
  if (xb && (Ca <= 0 || Ca >= C || Ca % 8)) return sta_fail(STA_E_ARG, "groupnorm nhwc cat: Ca=%d of C=%d (need 0 < Ca < C, Ca %% 8 == 0)", Ca, C);
  const int nchunk = gn_nhwc_chunks(HW), chunk_px = (HW + nchunk - 1) / nchunk;
  const dim3 grid(nchunk, B);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const char* const what = "groupnorm_silu_nhwc launch";
    if (const int rc = sta_launch<gn_nhwc_stats_kernel<T>>(what, grid, dim3(gn_nhwc_threads(C)), 0, st, (const T*)x, (const T*)xb, Ca, add, part, C, HW, G, chunk_px))
      return rc;
    return gn_nhwc_apply_launch<T>(what, grid, st, (const T*)x, (const T*)xb, Ca, add, nullptr, nullptr, (const T*)gamma, (const T*)beta, part, (T*)y, C,
                                   HW, G, chunk_px, eps, silu);
  });
}

int sta_groupnorm_silu_nhwc(const void* x, const float* add, const void* gamma, const void* beta, void* y,
                            void* workspace, int B, int C, int HW, int G, float eps, int silu, int dtype, void* stream) {
  return groupnorm_silu_nhwc_impl(x, nullptr, 0, add, gamma, beta, y, workspace, B, C, HW, G, eps, silu, dtype, stream);
}

int sta_groupnorm_silu_nhwc_cat(const void* xa, const void* xb, int Ca, const float* add, const void* gamma, const void* beta, void* y,
                                void* workspace, int B, int C, int HW, int G, float eps, int silu, int dtype, void* stream) {
  if (!xb) return sta_fail(STA_E_ARG, "null pointer");
  return groupnorm_silu_nhwc_impl(xa, xb, Ca, add, gamma, beta, y, workspace, B, C, HW, G, eps, silu, dtype, stream);
}

int sta_stats_finalize(const float* partial, float* stats, int B, int slots, int C, void* stream) {
  g_sta_err[0] = 0;
  if (!partial || !stats) return sta_fail(STA_E_ARG, "null pointer");
  if (B <= 0 || slots <= 0 || C <= 0 || C % 2) return sta_fail(STA_E_ARG, "stats_finalize: B=%d slots=%d C=%d (C even)", B, slots, C);
  return sta_launch<stats_finalize_kernel>("stats_finalize launch", dim3((2 * C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, partial, stats,
                                           slots, C);
}

int sta_groupnorm_silu_nhwc_cstats(const void* xa, const void* xb, int Ca, const float* stats_a, const float* stats_b, const float* add,
                                   const void* gamma, const void* beta, void* y, int B, int C, int HW, int G, float eps, int silu, int dtype,
                                   void* stream) {
  g_sta_err[0] = 0;
  if (!xa || !stats_a || !gamma || !beta || !y || (xb && !stats_b)) return sta_fail(STA_E_ARG, "null pointer");
  if (const int rc = gn_nhwc_shape_ok("groupnorm nhwc", B, C, HW, G)) return rc;
  if (xb && (Ca <= 0 || Ca >= C || Ca % 8)) return sta_fail(STA_E_ARG, "groupnorm nhwc cat: Ca=%d of C=%d (need 0 < Ca < C, Ca %% 8 == 0)", Ca, C);
  const int nchunk = gn_nhwc_chunks(HW), chunk_px = (HW + nchunk - 1) / nchunk;
  const dim3 grid(nchunk, B);
  hipStream_t st = (hipStream_t)stream;
  if (!xb) Ca = C;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return gn_nhwc_apply_launch<T>("groupnorm_silu_nhwc_cstats launch", grid, st, (const T*)xa, (const T*)xb, Ca, add, stats_a, stats_b, (const T*)gamma,
                                   (const T*)beta, nullptr, (T*)y, C, HW, G, chunk_px, eps, silu);
  });
}

int sta_add_bias_rows(const void* a, const void* b, const void* bias, void* y, long rows, int C, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!a || !y) return sta_fail(STA_E_ARG, "null pointer");
  if (rows <= 0 || C <= 0 || C % 8) return sta_fail(STA_E_ARG, "add_bias_rows: rows=%ld C=%d (need C %% 8 == 0)", rows, C);
  const long nvec = rows * (C / 8);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<add_bias_rows_kernel<T>>("add_bias_rows launch", dim3(sta_grid_for(nvec)), dim3(256), 0, st, (const T*)a, (const T*)b,
                                               (const T*)bias, (T*)y, nvec, C / 8);
  });
}

}  // extern "C"
