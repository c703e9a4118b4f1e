// sta_mxfp8.hip — OCP MX v1.0 fp8 (MXFP8: e4m3fn elements, one e8m0 scale per 32 consecutive K elements) for the transformer-block
// Linears of BASELINE configs[4] ("fp8 UNet weights on CDNA4 fp8 MFMA"), on gfx950's block-scaled MFMA
// v_mfma_scale_f32_32x32x64_f8f6f4, which runs e4m3 at twice the 16-bit rate (the non-block-scaled fp8 MFMA behind sta_fp8.hip's
// library GEMM runs at the 16-bit rate). C-ABI in include/sta_unet.h.
//
//   sta_mx8_quant_rows: x [rows][K] 16 bit -> xq [rows][K] e4m3fn bytes + xs [rows][K/32] e8m0 bytes (plain row-major: the ABI).
//   sta_mx8_gemm:       out[m][n] = sum_k P[m][k] 2^ps[m][k/32] * Q[n][k] 2^qs[n][k/32], fp32 accumulation, epilogue
//                       (col_scale[n], bias[n], or GEGLU), 16-bit output or, behind GEGLU, MXFP8 output.
//
// Scale rule (OCP MX v1.0, section 6.3): X = 2^(floor(log2 amax) - 8) (8 = e4m3's emax), exponent clamped to [-127, 127]; elements
// e4m3fn(x / X) rounded to nearest even and saturated to +-448. An all-zero block gets code-0 elements and scale byte 127 (X = 1).
// x / X is a power-of-two rescale, exact in fp32 (ldexp), so the conversion v_cvt_pk_fp8_f32 (round to nearest even) sees the exact
// quotient and the result is bit-exact with the plain-torch restatement sta.mxfp8.quant_rows_mx_reference. The quotient is clamped
// to +-448 in fp32 before the conversion (v_cvt_pk_fp8_f32 is not relied on for saturation; gfx950's v_cvt_scalef32_pk_fp8_f32 would
// fold the rescale into the conversion, but its saturation behaviour is not what the host rule states, so it is not used).
//
// Operand maps of v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 on both sides (cbsz = blgp = 0), established on MI355X with exact
// small-integer data, per-block power-of-two scales that differ and an asymmetric B (tests/test_mxfp8_gpu.py::test_gemm_layout_exact):
//   A (32 x 64): lane l (h = l >> 5) holds A[row l & 31][k] for k = 16 h + j in bytes j = 0..15 of its 8 VGPRs and
//                k = 32 + 16 h + j in bytes 16 + j: two 16-byte pieces, not one contiguous 32-byte run;
//   B (64 x 32): lane l holds B[k][col l & 31] for the same k;
//   scales:      byte 0 of lane l's scale VGPR (op_sel 0) scales 32-block h of the 64-deep step of row / col l & 31 — k 0..31
//                (bytes 0..15 of both lane halves) for lanes 0..31, k 32..63 (bytes 16..31 of both halves) for lanes 32..63;
//   C / D:       the shape's usual map, col = l & 31, row = 8 (r >> 2) + 4 (l >> 5) + (r & 3) for register r = 0..15.
// (A contiguous 32-byte run per lane computes the right products but scales k 16..47 of each step with the other block's scale:
// with P = identity that test failed on rows 16..47 and 80..111 of 128 exactly.) K % 64 == 32 is a half step whose second
// 16-byte piece is zero in every lane.
//
// GEMM structure: 256 threads, a 128 (m) x 128 (n) output tile, 4 waves of 64 x 64 (2 x 2 MFMA tiles). Q (the MFMA A operand: the
// output's column index n) and P (B operand: the output row m) are staged global -> LDS by 16-byte global_load_lds into two buffers of
// 128 rows x 128 K bytes each per operand (double buffering, one barrier per 128-deep stage). The LDS image is lane-linear per
// wave-instruction (rows of 128 B); the 16-byte chunk c of row r is stored at chunk c ^ ((r >> 1) & 7) (the swizzle is applied to the
// global SOURCE address), so the ds_read_b128 fragment reads of 16 consecutive rows hit 16 distinct 4-bank groups. Out-of-range rows
// are clamped to the last row and K bytes past the end to the row's start (no read leaves the operands; those lanes' fragments are
// zeroed or their outputs not stored). The scale bytes (8 per lane per stage) are plain loads issued beside the stage's LDS-DMA.
// Lanes carry the output row m and 16 output columns, 4 consecutive per register group, so the 16-bit store is 8 bytes per lane.
//
// GEGLU (reference attention.py:47-49, value first, gate second): Q is packed so that every 64-row group holds 32 value rows then the
// 32 gate rows of the same hidden columns (sta.mxfp8.pack_geglu_rows); a wave's two n tiles are then value and gate of the same 32
// columns and out[m][h] = value * gelu_erf(gate) is a register-wise product. With MXFP8 output the 16-bit-rounded values of one
// 32-column group (held by lanes l and l ^ 32) are quantised by the rule above: the scales equal those of sta_mx8_quant_rows of the
// 16-bit GEGLU output; the codes equal them bit for bit in bf16 and, measured in fp16, in all but a few elements (one e4m3 step).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sta_unet.h"
#include "sta_internal.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int E4M3_EMAX = 8;
constexpr float E4M3_MAX = 448.0f;
constexpr int TM = 128, TN = 128, BK = 128;          // output tile (P rows x Q rows), K bytes per stage
constexpr int OP_BYTES = TM * BK;                    // one operand's stage image: 16 KiB
constexpr int GL_ALL = STA_MX8_GEGLU | STA_MX8_MX_OUT;

template <typename T> struct Vec;
template <> struct Vec<_Float16> { typedef f16x8 v8; typedef f16x4 v4; };
template <> struct Vec<__bf16> { typedef bf16x8 v8; typedef bf16x4 v4; };

// e8m0 exponent of one 32-block from its amax (a finite fp32; 0 for an all-zero block). floor(log2 amax) is the exponent field of amax
// for a normal fp32; a subnormal one (bf16 subnormals) is below 2^-126 and clamps to -127 either way.
__device__ inline int mx_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  const int e = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 - E4M3_EMAX;
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

__device__ inline float mx_rescale(float v, int e) { return fminf(fmaxf(__builtin_ldexpf(v, -e), -E4M3_MAX), E4M3_MAX); }

__device__ inline unsigned pk4(float a, float b, float c, float d) {
  const unsigned w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
}

// ---- quantiser: one thread per 32-element block (64 B in, 32 B + 1 B out); HBM-bound, 3.03 bytes per element ----
template <typename T>
__global__ __launch_bounds__(256) void mx8_quant_kernel(const typename Vec<T>::v8* __restrict__ x, u32x4* __restrict__ xq,
                                                        uint8_t* __restrict__ xs, long nblk) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= nblk) return;
  float v[32];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const typename Vec<T>::v8 t = x[b * 4 + i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[8 * i + j] = (float)t[j];
      amax = fmaxf(amax, fabsf(v[8 * i + j]));
    }
  }
  const int e = mx_exp(amax);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float* s = v + 16 * i + 4 * w;
      o[w] = pk4(mx_rescale(s[0], e), mx_rescale(s[1], e), mx_rescale(s[2], e), mx_rescale(s[3], e));
    }
    xq[b * 2 + i] = o;
  }
  xs[b] = (uint8_t)(e + 127);
}

// first block of this launch's XCD share (blocks are dealt round-robin over the 8 XCDs): neighbouring tiles, which share a P tile,
// then run on one XCD and read it from the same L2
__device__ inline int xcd_remap(int bid, int nb) {
  const int q = nb / 8, r = nb % 8, xcd = bid % 8, idx = bid / 8;
  return xcd < r ? xcd * (q + 1) + idx : r * (q + 1) + (xcd - r) * q + idx;
}

__device__ inline float gelu_erf(float g) { return 0.5f * g * (1.0f + erff(g * 0.70710678118654752f)); }

template <typename T, int FL>
__global__ __launch_bounds__(256, 2) void mx8_gemm_kernel(const uint8_t* __restrict__ P, const uint8_t* __restrict__ Ps,
                                                          const uint8_t* __restrict__ Q, const uint8_t* __restrict__ Qs,
                                                          void* __restrict__ out, uint8_t* __restrict__ out_s,
                                                          const T* __restrict__ bias, const float* __restrict__ col_scale,
                                                          long M, int N, int K, long ldo, int ntiles) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * OP_BYTES];        // [buffer][P | Q][128 rows][128 B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const long m0 = (long)(bid / ntiles) * TM;
  const int n0 = (bid % ntiles) * TN;
  const int wm = wave >> 1, wn = wave & 1;                   // this wave's 64 x 64 quarter of the tile
  const int KB = K >> 5;                                     // scale bytes per row
  const int half = lane >> 5, l32 = lane & 31;

  // staging: thread tid, instruction i moves 16-B chunk q = 256 i + tid of the [128][128 B] image: row q >> 3, LDS chunk q & 7,
  // global chunk (q & 7) ^ ((row >> 1) & 7)
  const uint8_t* srcP[4];
  const uint8_t* srcQ[4];
  int gcb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = 256 * i + tid, row = q >> 3;
    gcb[i] = 16 * ((q & 7) ^ ((row >> 1) & 7));
    const long pr = m0 + row < M ? m0 + row : M - 1;
    const int qr = n0 + row < N ? n0 + row : N - 1;
    srcP[i] = P + pr * K;
    srcQ[i] = Q + (long)qr * K;
  }
  auto stage = [&](int st, int buf) __attribute__((always_inline)) {
    const int kb = st * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = kb + gcb[i] < K ? kb + gcb[i] : 0;       // past K: the row's first chunk (its lanes are zeroed later)
      uint8_t* dstP = lds + buf * 2 * OP_BYTES + (256 * i + 64 * wave) * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcP[i] + off),
                                       (__attribute__((address_space(3))) void*)dstP, 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcQ[i] + off),
                                       (__attribute__((address_space(3))) void*)(dstP + OP_BYTES), 16, 0, 0);
    }
  };
  // this lane's P rows (2 m tiles) and Q rows (2 n tiles), clamped
  const uint8_t* psrow[2];
  const uint8_t* qsrow[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const long pr = m0 + 64 * wm + 32 * t + l32;
    const int qr = n0 + 64 * wn + 32 * t + l32;
    psrow[t] = Ps + (pr < M ? pr : M - 1) * KB;
    qsrow[t] = Qs + (long)(qr < N ? qr : N - 1) * KB;
  }
  int scP[2][2], scQ[2][2];                                  // [k step][tile] scale bytes of the NEXT stage
  auto load_scales = [&](int st) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int kb = 4 * st + 2 * s + half;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        scP[s][t] = kb < KB ? (int)psrow[t][kb] : 127;
        scQ[s][t] = kb < KB ? (int)qsrow[t][kb] : 127;
      }
    }
  };

  f32x16 acc[2][2];                                          // [m tile][n tile]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int nst = (K + BK - 1) / BK;
  stage(0, 0);
  load_scales(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    int cP[2][2], cQ[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t) cP[s][t] = scP[s][t], cQ[s][t] = scQ[s][t];
    if (st + 1 < nst) {
      stage(st + 1, (st + 1) & 1);
      load_scales(st + 1);
    }
    const uint8_t* bP = lds + (st & 1) * 2 * OP_BYTES;
    const uint8_t* bQ = bP + OP_BYTES;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int k0 = st * BK + 64 * s;
      if (k0 >= K) break;                                    // wave-uniform: K % 128 == 64 or 96 has a missing last step
      const bool zero = k0 + 32 >= K;                        // K % 64 == 32: k 32..63 of the last step (every lane's second piece)
      i32x8 fp[2], fq[2];
      const int c0 = 4 * s + half;                           // 16-byte chunks c0 (k 16 h ..) and c0 + 2 (k 32 + 16 h ..) of the row
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int rp = 64 * wm + 32 * t + l32, rq = 64 * wn + 32 * t + l32;
        const int swp = (rp >> 1) & 7, swq = (rq >> 1) & 7;
        const i32x4 p0 = *(const i32x4*)(bP + rp * BK + 16 * (c0 ^ swp));
        i32x4 p1 = *(const i32x4*)(bP + rp * BK + 16 * ((c0 + 2) ^ swp));
        const i32x4 q0 = *(const i32x4*)(bQ + rq * BK + 16 * (c0 ^ swq));
        i32x4 q1 = *(const i32x4*)(bQ + rq * BK + 16 * ((c0 + 2) ^ swq));
        if (zero) p1 = i32x4{}, q1 = i32x4{};
        fp[t] = __builtin_shufflevector(p0, p1, 0, 1, 2, 3, 4, 5, 6, 7);
        fq[t] = __builtin_shufflevector(q0, q1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fq[b], fp[a], acc[a][b], 0, 0, 0, cQ[s][b], 0, cP[s][a]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // epilogue: register r of acc[a][b] is out[m][n], m = m0 + 64 wm + 32 a + l32, n = n0 + 64 wn + 32 b + 8 (r >> 2) + 4 half + (r & 3)
  if constexpr ((FL & STA_MX8_GEGLU) == 0) {
    T* o = (T*)out;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const long m = m0 + 64 * wm + 32 * a + l32;
      if (m >= M) continue;
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = n0 + 64 * wn + 32 * b + 8 * g + 4 * half;
          if (n >= N) continue;
          float y[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int nn = n + e < N ? n + e : N - 1;
            y[e] = acc[a][b][4 * g + e];
            if (col_scale) y[e] *= col_scale[nn];
            if (bias) y[e] += (float)bias[nn];
          }
          T* dst = o + m * ldo + n;
          if (n + 3 < N && (ldo & 3) == 0) {
            typename Vec<T>::v4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = (T)y[e];
            *(typename Vec<T>::v4*)dst = w;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (n + e < N) dst[e] = (T)y[e];
          }
        }
    }
  } else {
    // GEGLU: acc[a][0] = value, acc[a][1] = gate of hidden columns h = (n0 + 64 wn) / 2 + 8 (r >> 2) + 4 half + (r & 3); N % 64 == 0
    const int H = N >> 1;
    const int hb = (n0 + 64 * wn) >> 1;
    const int pb = n0 + 64 * wn;                             // packed bias index of the group's first value row
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const long m = m0 + 64 * wm + 32 * a + l32;
      float y[16];
      float amax = 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = 8 * g + 4 * half + e;
          float v = acc[a][0][4 * g + e], gt = acc[a][1][4 * g + e];
          if (bias && pb < N) v += (float)bias[pb + j], gt += (float)bias[pb + 32 + j];
          const float r16 = (float)(T)(v * gelu_erf(gt));  // the 16-bit output value
          y[4 * g + e] = r16;
          amax = fmaxf(amax, fabsf(r16));
        }
      if constexpr ((FL & STA_MX8_MX_OUT) != 0) {
        amax = fmaxf(amax, __shfl_xor(amax, 32));           // lanes l and l ^ 32 hold the two halves of the 32-column group
        const int ex = mx_exp(amax);
        if (m < M && hb < H) {
          uint8_t* oq = (uint8_t*)out + m * ldo + hb;
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *(unsigned*)(oq + 8 * g + 4 * half) = pk4(mx_rescale(y[4 * g], ex), mx_rescale(y[4 * g + 1], ex), mx_rescale(y[4 * g + 2], ex),
                                                       mx_rescale(y[4 * g + 3], ex));
          if (half == 0) out_s[m * (ldo >> 5) + (hb >> 5)] = (uint8_t)(ex + 127);
        }
      } else {
        if (m < M && hb < H) {
          T* o = (T*)out + m * ldo + hb;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            typename Vec<T>::v4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = (T)y[4 * g + e];
            *(typename Vec<T>::v4*)(o + 8 * g + 4 * half) = w;
          }
        }
      }
    }
  }
}

template <typename T, int FL>
int launch_gemm(const void* p, const void* ps, const void* q, const void* qs, void* out, void* out_s, const void* bias,
                 const float* col_scale, long M, int N, int K, long ldo, hipStream_t st) {
  const int ntiles = (N + TN - 1) / TN;
  const long nb = (M + TM - 1) / TM * ntiles;
  return sta_launch<mx8_gemm_kernel<T, FL>>("mx8_gemm launch", dim3((unsigned)nb), dim3(256), 0, st, (const uint8_t*)p, (const uint8_t*)ps,
                                            (const uint8_t*)q, (const uint8_t*)qs, out, (uint8_t*)out_s, (const T*)bias, col_scale, M, N, K, ldo,
                                            ntiles);
}

template <typename T>
int launch_gemm_flags(int flags, const void* p, const void* ps, const void* q, const void* qs, void* out, void* out_s, const void* bias,
                       const float* col_scale, long M, int N, int K, long ldo, hipStream_t st) {
  if (flags == 0) return launch_gemm<T, 0>(p, ps, q, qs, out, out_s, bias, col_scale, M, N, K, ldo, st);
  if (flags == STA_MX8_GEGLU) return launch_gemm<T, STA_MX8_GEGLU>(p, ps, q, qs, out, out_s, bias, col_scale, M, N, K, ldo, st);
  return launch_gemm<T, GL_ALL>(p, ps, q, qs, out, out_s, bias, col_scale, M, N, K, ldo, st);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int sta_mx8_quant_rows(const void* x, void* xq, void* xs, long rows, int K, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !xq || !xs) return sta_fail(STA_E_ARG, "null pointer");
  if (rows <= 0 || K <= 0) return sta_fail(STA_E_ARG, "rows=%ld K=%d", rows, K);
  if (K % 32) return sta_fail(STA_E_UNSUP, "K=%d unsupported (K %% 32 == 0)", K);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_UNSUP, "dtype %d", dtype);
  if (!aligned16(x) || !aligned16(xq)) return sta_fail(STA_E_ARG, "x and xq must be 16-byte aligned");
  const long nblk = rows * (long)(K / 32);
  const dim3 grid((unsigned)((nblk + 255) / 256));
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<mx8_quant_kernel<T>>("mx8_quant_rows launch", grid, dim3(256), 0, (hipStream_t)stream, (const typename Vec<T>::v8*)x,
                                           (u32x4*)xq, (uint8_t*)xs, nblk);
  });
}

extern "C" int sta_mx8_gemm(const void* p, const void* ps, const void* q, const void* qs, void* out, void* out_scale, const void* bias,
                            const float* col_scale, long M, int N, int K, long ldo, int flags, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!p || !ps || !q || !qs || !out) return sta_fail(STA_E_ARG, "null pointer");
  if (M <= 0 || N <= 0 || K <= 0) return sta_fail(STA_E_ARG, "M=%ld N=%d K=%d", M, N, K);
  if (K % 32) return sta_fail(STA_E_UNSUP, "K=%d unsupported (K %% 32 == 0)", K);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_UNSUP, "dtype %d", dtype);
  if (flags & ~GL_ALL) return sta_fail(STA_E_ARG, "flags %d", flags);
  if (!aligned16(p) || !aligned16(q)) return sta_fail(STA_E_ARG, "P and Q must be 16-byte aligned");
  if (flags & STA_MX8_GEGLU) {
    if (N % 64) return sta_fail(STA_E_UNSUP, "GEGLU needs N %% 64 == 0 (N=%d)", N);
    if (col_scale) return sta_fail(STA_E_ARG, "GEGLU takes no col_scale");
    if (ldo < N / 2 || (ldo & 3)) return sta_fail(STA_E_ARG, "ldo=%ld (GEGLU output is [M][N/2], ldo %% 4 == 0)", ldo);
    if ((flags & STA_MX8_MX_OUT) && (!out_scale || ldo != N / 2)) return sta_fail(STA_E_ARG, "MXFP8 output needs out_scale and ldo == N/2");
  } else {
    if (flags & STA_MX8_MX_OUT) return sta_fail(STA_E_UNSUP, "MXFP8 output only behind the GEGLU epilogue");
    if (ldo < N) return sta_fail(STA_E_ARG, "ldo=%ld < N=%d", ldo, N);
  }
  if (!aligned16(out)) return sta_fail(STA_E_ARG, "out must be 16-byte aligned");
  return sta_by_dtype(dtype, [&](auto tag) {
    return launch_gemm_flags<decltype(tag)>(flags, p, ps, q, qs, out, out_scale, bias, col_scale, M, N, K, ldo, (hipStream_t)stream);
  });
}
