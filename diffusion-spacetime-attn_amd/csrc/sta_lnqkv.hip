// sta_lnqkv.hip — the front end of the block's self-attention at SD-v1 level 0 (C = 320) as ONE pass:
//
//     s = x + bias;  y = norm1(s);  q|k = y [Wq * scale * log2 e; Wk]^T;  V^T = Wv y^T        attention.py:175-180 behind :270
//
// Row-major this is sta_add_layernorm (reads x, writes y) + two library GEMMs that read y back (0.67 + 1.01 + 0.67 GB per call at
// 524 288 rows); here y never exists in HBM: the pass reads x once and writes q|k [R][2C] row-major and V^T [C][R] — what
// sta_selfattn_fwd* reads — 1.34 GB in all.
//
// LayerNorm: one wave per row, lane = 8-channel chunk — the row helpers of csrc/sta_trunk_dev.h and the lane assignment of
// csrc/sta_unet.hip::add_layernorm_kernel (bit-identical y). A wave owns 32 rows per pass as two 16-row items; the normalised
// chunks cross a wave-private LDS tile (the query-fragment tile of sta_trunk_dev.h) into 2 x 10 MFMA operand fragments
// that stay in registers for the whole pass. Item `it` holds the rows 8 (c >> 2) + 4 it + (c & 3), c = 0 .. 15, of the 32: in the
// V part the operands are exchanged (V^T tile = y_frag x wv_frag: a lane's accumulator registers are consecutive ROWS of one
// channel), and with this interleave the two items of a lane are 8 consecutive rows: one 16-byte store into V^T, 64 contiguous
// bytes per channel and wave.
//
// GEMM: rows are the MFMA columns (Out^T = W y^T) for q|k, as in csrc/sta_ffgemm.hip. The packed [Wq'; Wk; Wv] (960 x 320, 600
// fragments of 1 KiB, L2-resident) is streamed through a 2-slot LDS ring by LDS-DMA in 30 sub-chunks of two 16-channel tiles x
// 10 k-steps, one sub-chunk ahead, once per 256-row pass (8 waves x 32 rows). Per sub-chunk a wave issues 40 MFMAs behind 20
// operand reads (each serves both of its items) and stores 2 x 16 bytes per lane. q|k tiles use the row permutation of
// pack_w1_kernel, so a lane finishes 8 consecutive channels of a row.
//
// Roofline: MFMA (2 * 320 * 960 flop per row = 614 kFLOP against 640 + 1920 bytes: 240 flop/B, the ridge of this chip is ~310) —
// close to balanced; HBM floor 1.34 GB, MFMA floor 322 GFLOP per call.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sta_xattn.h"
#include "sta_unet.h"
#include "sta_internal.h"
#include "sta_xattn_dev.h"
#include "sta_wring_dev.h"
#include "sta_trunk_dev.h"

namespace {

constexpr int LQ_C = 320;
constexpr int LQ_NKS = LQ_C / 32;              // 10 k-steps
constexpr int LQ_NSC_QK = 2 * LQ_C / 32;       // 20 sub-chunks of q|k (32 output channels each)
constexpr int LQ_NSC = 3 * LQ_C / 32;          // 30 sub-chunks in all (the last 10: V)
constexpr int LQ_SC_FR = 2 * LQ_NKS;           // 20 fragments per sub-chunk
constexpr int LQ_NW = 8;
using LqRing = WRing<LQ_NW, LQ_SC_FR>;         // 3 LDS-DMA instructions per wave per sub-chunk (4 padding copies), 24 KiB per slot
constexpr int LQ_SLOT = LqRing::SLOT;
constexpr int LQ_TILE = (LQ_C / 8) * QFRAG_CHUNK;      // a wave's query-fragment tile of one 16-row item (sta_trunk_dev.h): 10 880 bytes
constexpr int LQ_LDS = 2 * LQ_SLOT + LQ_NW * LQ_TILE;

// [Wq'; Wk] [2C][C] and Wv [C][C] -> [sub-chunk sc][t][k-step f] fragments. q|k (sc < 20): lane (g, c) holds
// Wqk[32 sc + 8 (c >> 2) + 4 t + (c & 3)][32 f + 8 g .. + 7]; V: Wv[32 (sc - 20) + 16 t + c][32 f + 8 g .. + 7]
template <typename T>
__global__ __launch_bounds__(64) void pack_wqkv_kernel(const T* __restrict__ wqk, const T* __restrict__ wv, T* __restrict__ packed) {
  const int fr = blockIdx.x;                   // (sc * 2 + t) * NKS + f
  const int f = fr % LQ_NKS, t = (fr / LQ_NKS) & 1, sc = fr / (2 * LQ_NKS);
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  const T* src = sc < LQ_NSC_QK ? wqk + (size_t)(32 * sc + 8 * (c >> 2) + 4 * t + (c & 3)) * LQ_C      // row frag_sigma(2 sc + t, c), spelled out
                                : wv + (size_t)(32 * (sc - LQ_NSC_QK) + 16 * t + c) * LQ_C;
  const typename Tr<T>::V8 x = *(const typename Tr<T>::V8*)(src + 32 * f + 8 * g);
  *(typename Tr<T>::V8*)(packed + (size_t)fr * (FRAG / 2) + lane * 8) = x;
}

struct LQ {
  const void* x;        // [R][C]
  const void* bias;     // [C] or null
  const void* gamma;
  const void* beta;
  const char* w;        // packed [Wq'; Wk; Wv]
  void* s;              // [R][C] or null
  void* y;              // [R][C] or null (tests)
  void* qk;             // [R][2C]
  void* vt;             // [C][R]
  long R;
  int C;
  float eps;
};

template <typename T>
__global__ __launch_bounds__(64 * LQ_NW, 2) void ln_qkv_kernel(const LQ p) {
  using V8 = typename Tr<T>::V8;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  char* ring = smem;
  char* tile = smem + 2 * LQ_SLOT + wv * LQ_TILE;
  const int C = p.C;
  const bool on = lane < LQ_C / 8;
  const unsigned lane16 = (unsigned)lane * 16u;
  const __amdgpu_buffer_rsrc_t w_srd = make_srd(p.w, (unsigned)(LQ_NSC * LQ_SC_FR * FRAG));
  auto stage = [&](int sc, int slot) __attribute__((always_inline)) {
    LqRing::stage(w_srd, ring + slot * LQ_SLOT, 0u, sc * LQ_SC_FR, wv, lane16);
  };
  const unsigned xbytes = (unsigned)((size_t)p.R * LQ_C * sizeof(T));
  const __amdgpu_buffer_rsrc_t x_srd = make_srd(p.x, xbytes);
  const __amdgpu_buffer_rsrc_t s_srd = make_srd(p.s, p.s ? xbytes : 0u);
  const __amdgpu_buffer_rsrc_t y_srd = make_srd(p.y, p.y ? xbytes : 0u);
  const __amdgpu_buffer_rsrc_t qk_srd = make_srd(p.qk, 2u * xbytes);
  const __amdgpu_buffer_rsrc_t vt_srd = make_srd(p.vt, xbytes);
  V8 bs = {}, gm = {}, bt = {};
  if (on) {
    if (p.bias) bs = ((const V8*)p.bias)[lane];
    gm = ((const V8*)p.gamma)[lane];
    bt = ((const V8*)p.beta)[lane];
  }
  const long nblk = (p.R + 32 * LQ_NW - 1) / (32 * LQ_NW);
  const char* lbase = ring + lane * 16;
  stage(0, 0);
  for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const long row0 = (blk * LQ_NW + wv) * 32;            // this wave's 32 rows; R % 16 == 0
    V8 b[2][LQ_NKS];
    // ---- LayerNorm of the wave's 32 rows -> operand fragments in registers
    V8 raw[2][16];
    unsigned xo[2][16];                                   // byte offset of (row, this lane's chunk); past the descriptor: loads 0, stores dropped
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const long row = row0 + 8 * (c >> 2) + 4 * it + (c & 3);
        xo[it][c] = (on && row < p.R) ? (unsigned)(row * LQ_C * (long)sizeof(T)) + lane16 : SRD_DROP;
        raw[it][c] = srd_load16<V8>(x_srd, xo[it][c], 0);
      }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {                       // four rows at a time: their reductions interleave
        float v[4][8];
        float sum[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const V8 a = raw[it][4 * j + r];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[r][e] = (float)a[e];
          if (p.bias) {      // (ln_add8, written out: through the helper this kernel allocates its registers differently)
#pragma unroll
            for (int e = 0; e < 8; ++e) v[r][e] += (float)bs[e];
          }
          if (p.s) {   // the residual stream continues in the activation dtype: normalise what is stored
            const V8 o = ln_round8<T>(v[r]);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), s_srd, xo[it][4 * j + r], 0, 0);
          }
          const float t = ln_sum8(0.f, v[r]);
          sum[r] = on ? t : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float mean = ln_mean(sum[r], C);
          float q = 0.f;
          if (on) q = ln_sq8(q, v[r], mean);
          const float rstd = ln_rstd(q, C, p.eps);
          V8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (T)ln_affine(v[r][e], mean, rstd, (float)gm[e], (float)bt[e]);
          if (on) *(V8*)(tile + qfrag_tile_at(lane, 4 * j + r)) = o;
          if (p.y) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), y_srd, xo[it][4 * j + r], 0, 0);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own tile: written by 40 lanes, read by 64
#pragma unroll
      for (int f = 0; f < LQ_NKS; ++f) b[it][f] = *(const V8*)(tile + qfrag_tile_at(4 * f + g, c16));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // ... before the next item overwrites it
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the sub-chunk 0 DMA, the s / y stores and the previous pass's last stores
    // ---- q|k (KIND 0) and V^T (KIND 1) against the streamed weight
    auto sub = [&](auto kind_tag, auto slot_tag, const int sc) __attribute__((always_inline)) {
      constexpr int KIND = decltype(kind_tag)::value;
      constexpr int SLOT = decltype(slot_tag)::value;
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");    // this sub-chunk's DMA landed; the previous epilogue's two stores may fly
      __builtin_amdgcn_s_barrier();
      stage(sc + 1 < LQ_NSC ? sc + 1 : 0, SLOT ^ 1);      // next sub-chunk (sub-chunk 0 of the next pass behind the last one)
      const V8* fr = (const V8*)(lbase + SLOT * LQ_SLOT);
      V8 wa[2][LQ_NKS];
#pragma unroll
      for (int f = 0; f < LQ_NKS; ++f) {
        wa[0][f] = fr[f * 64];
        wa[1][f] = fr[(LQ_NKS + f) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
      f32x4 a00 = {0.f, 0.f, 0.f, 0.f}, a01 = a00, a10 = a00, a11 = a00;      // [t][item]
#pragma unroll
      for (int f = 0; f < LQ_NKS; ++f) {
        if constexpr (KIND == 0) {
          a00 = Tr<T>::mfma(wa[0][f], b[0][f], a00);
          a01 = Tr<T>::mfma(wa[0][f], b[1][f], a01);
          a10 = Tr<T>::mfma(wa[1][f], b[0][f], a10);
          a11 = Tr<T>::mfma(wa[1][f], b[1][f], a11);
        } else {
          a00 = Tr<T>::mfma(b[0][f], wa[0][f], a00);
          a01 = Tr<T>::mfma(b[1][f], wa[0][f], a01);
          a10 = Tr<T>::mfma(b[0][f], wa[1][f], a10);
          a11 = Tr<T>::mfma(b[1][f], wa[1][f], a11);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      // ALWAYS two stores per sub-chunk (rows past R: an offset the descriptor drops): the counted vmcnt above relies on it
      if constexpr (KIND == 0) {
        // lane (g, c): tiles t = 0, 1, registers r -> channels 32 sc + 8 g + 4 t + r of the item's row c
        const f32x4 acc[2][2] = {{a00, a01}, {a10, a11}};
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const long row = row0 + 8 * (c16 >> 2) + 4 * it + (c16 & 3);
          V8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (T)acc[e >> 2][it][e & 3];
          const unsigned qo = row < p.R ? (unsigned)(row * (2 * LQ_C) * (long)sizeof(T)) + (unsigned)(32 * sc + 8 * g) * (unsigned)sizeof(T) : SRD_DROP;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), qk_srd, qo, 0, 0);
        }
      } else {
        // lane (g, c): tile t, item it, register r -> channel 32 (sc - 20) + 16 t + c of row 8 g + 4 it + r: 8 consecutive rows
        const f32x4 acc[2][2] = {{a00, a01}, {a10, a11}};
        const long rowb = row0 + 8 * g;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const long ch = 32 * (sc - LQ_NSC_QK) + 16 * t + c16;
          V8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (T)acc[t][e >> 2][e & 3];
          const unsigned vo = rowb < p.R ? (unsigned)((ch * p.R + rowb) * (long)sizeof(T)) : SRD_DROP;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), vt_srd, vo, 0, 0);
        }
      }
    };
    for (int sp = 0; sp < LQ_NSC_QK; sp += 2) {
      sub(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, sp);
      sub(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, sp + 1);
    }
    for (int sp = LQ_NSC_QK; sp < LQ_NSC; sp += 2) {
      sub(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, sp);
      sub(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{}, sp + 1);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

extern "C" {

size_t sta_ln_qkv_packed_w_bytes(int C) {
  return C == LQ_C ? (size_t)LQ_NSC * LQ_SC_FR * FRAG : 0;
}

int sta_ln_qkv_pack_w(const void* wqk, const void* wv, void* packed, int C, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!wqk || !wv || !packed) return sta_fail(STA_E_ARG, "null pointer");
  if (sta_ln_qkv_packed_w_bytes(C) == 0) return sta_fail(STA_E_UNSUP, "fused norm1 + q/k/v projection: C = 320 only (C=%d)", C);
  hipStream_t st = (hipStream_t)stream;
  const unsigned nfr = LQ_NSC * LQ_SC_FR;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<pack_wqkv_kernel<T>>("pack_wqkv launch", dim3(nfr), dim3(64), 0, st, (const T*)wqk, (const T*)wv, (T*)packed);
  });
}

int sta_ln_qkv(const void* x, const void* bias, const void* gamma, const void* beta, const void* packed_w, void* s, void* y_dbg,
               void* qk, void* vt, long R, int C, float eps, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !gamma || !beta || !packed_w || !qk || !vt) return sta_fail(STA_E_ARG, "null pointer");
  if (sta_ln_qkv_packed_w_bytes(C) == 0) return sta_fail(STA_E_UNSUP, "fused norm1 + q/k/v projection: C = 320 only (C=%d)", C);
  if (R <= 0 || R % 16) return sta_fail(STA_E_ARG, "ln_qkv: R=%ld (need a positive multiple of 16 rows)", R);
  if ((size_t)R * 2 * C * 2 >= 0xfffffff0ull) return sta_fail(STA_E_UNSUP, "ln_qkv: the q|k output must stay below 4 GiB (R=%ld)", R);
  LQ p{x, bias, gamma, beta, (const char*)packed_w, s, y_dbg, qk, vt, R, C, eps};
  const long nblk = (R + 32 * LQ_NW - 1) / (32 * LQ_NW);
  const unsigned grid = (unsigned)(nblk < 256 ? nblk : 256);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    return sta_launch_lds<ln_qkv_kernel<decltype(tag)>>("ln_qkv launch", LQ_LDS, dim3(grid), dim3(64 * LQ_NW), LQ_LDS, st, p);
  });
}

}  // extern "C"
