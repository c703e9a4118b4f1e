// sta_ffgemm.hip — the first half of the block's feed-forward at SD-v1 level 0 (C = 320, inner = 1280) and level 1 (C = 640,
// inner = 2560) as ONE pass:
//
//     h = (y W_v^T + b_v) * gelu(y W_g^T + b_g)          GEGLU.forward (attention.py:42-45) inside FeedForward (:48-69), called at :299
//
// with y = norm3(x) read in QUERY-FRAGMENT order (what sta_to_out_ln_ofrag / sta_add_layernorm_qfrag write). Row-major, this is
// a library GEMM that writes the [R][2 * inner] projection (1.34 GB at 32 images at level 0, at 131072 rows at level 1) followed by
// the GEGLU pass that reads it back and writes [R][inner]: here the projection never exists in HBM — the accumulators of a value
// tile pair and of its gate tile pair meet in registers and leave as 8 finished channels per lane.
//
// Rows are the MFMA columns: Out^T = W' y^T. B operand = one 1-KiB fragment of y per k-step (lane (g, c): channels 32 s + 8 g .. + 7
// of row c), 2 x C / 32 of them per wave (32 rows) held for a whole pass; A operand = proj.weight [2 * inner][C] re-laid out once
// per model in sub-chunks of 40 fragments = {value tiles 2v, 2v+1; gate tiles 2v, 2v+1} x 10 k-steps, rows permuted
// (sigma(2v + t, rho) = 32 v + 8 (rho >> 2) + 4 t + (rho & 3)) so that a lane's two value tiles are 8 CONSECUTIVE channels.
// The weight (1.6 MB | 6.6 MB) is streamed through a 2-slot LDS ring by LDS-DMA, one 40-KiB sub-chunk ahead, once per 256-row pass
// (8 waves x 32 rows; L2-resident). Per sub-chunk a wave issues 80 MFMAs behind 40 operand reads (each serves both of its
// 16-row items); behind a tile pair's last sub-chunk it finishes 2 x 8 channels per lane with the exact-erf GELU of csrc/sta_unet.hip.
//
// Level 0: a tile pair is ONE sub-chunk (all 10 k-steps), 40 of them; its operands are read in one group of 2 x 10 fragments.
// Level 1: a whole {pair, pair} x 20 k-steps sub-chunk is 80 KiB and does not fit beside a second ring slot, so K is streamed in
// halves: 160 sub-chunks, the eight accumulators live across the two halves of a tile pair and the epilogue runs behind the second.
// The operands are read in quarters of a tile pair (2 x 5 fragments) — with halves the kernel spills. Register budget there:
// 160 (y) + 32 (accumulators) + 40 (operands) + addressing = 255 of the 256 two waves per SIMD leave: the build refuses a toolchain
// that spills it (sta/lib.py::NO_SPILL_KERNELS), and h leaves row-major only (no register for the fragment-order select, and
// nothing reads fragment-order h at C = 640).
//
// Roofline: MFMA. Level 0: 2 * 320 * 2560 flop per row = 1.64 MFLOP against 640 + 2560 bytes: 512 flop/B. Level 1: 2 * 640 * 5120
// flop per row = 6.55 MFLOP against 1280 + 5120 bytes: 1024 flop/B.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sta_xattn.h"
#include "sta_unet.h"
#include "sta_internal.h"
#include "sta_xattn_dev.h"
#include "sta_wring_dev.h"
#include "sta_rows_dev.h"

namespace {

// The shape of the GEGLU projection pass at C = 320 | 640
template <int C_>
struct FfShape {
  static_assert(C_ == 320 || C_ == 640, "SD-v1 level 0 or level 1");
  static constexpr int C = C_, INNER = 4 * C;
  static constexpr int NKS = C / 32;                 // 10 | 20 k-steps
  static constexpr int NH = C / 320;                 // parts of K a tile pair's weight is streamed in: 1 | 2
  static constexpr int HKS = NKS / NH;               // 10 k-steps per sub-chunk
  static constexpr int RG = NH == 1 ? HKS : HKS / 2; // k-steps per operand read group: 10 | 5
  static constexpr int NTP = INNER / 32;             // 40 | 80 tile pairs (a pair of value tiles + its pair of gate tiles each)
  static constexpr int NSC = NH * NTP;               // 40 | 160 sub-chunks: tile pair v, K part hf -> NH v + hf
  static constexpr int SC_FR = 4 * HKS;              // 40 fragments per sub-chunk
  static constexpr int NW = 8;
  using Ring = WRing<NW, SC_FR>;                     // 5 LDS-DMA instructions per wave per sub-chunk, 40 KiB per slot
  static constexpr int SLOT = Ring::SLOT;
  static constexpr int TAB = 2 * INNER * 2;          // bias (value | gate) as 16-bit behind the ring: 5 | 10 KiB
  static constexpr int LDS = 2 * SLOT + TAB;         // 85 | 90 KiB
  static_assert(Ring::PER * NW == SC_FR, "the ring of this kernel has no spare positions");
  static constexpr const char* TAG = C == 320 ? "" : " (c640)";    // host: how an error names the level-1 entry points
};
// what the second half (level 0 only) shares with the first
constexpr int FF_C = 320, FF_INNER = FfShape<FF_C>::INNER, FF_NKS = FfShape<FF_C>::NKS, FF_NW = FfShape<FF_C>::NW;

// Exact-erf GELU, the formula of csrc/sta_unet.hip::gelu_erf (Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 on erf) with the
// constants folded and the sign handled without a select — gelu(g) = max(g, 0) - |g| * (0.5 * (1 - erf(|g| / sqrt 2))):
// a reciprocal, an exp2 and 11 plain vector instructions per value instead of 16 (|g| is an operand modifier): this kernel's
// vector-issue port is as loaded as its matrix pipe. Max |difference| to the fp64 GELU on [-12, 12]: 5.2e-7.
__device__ __forceinline__ float ff_gelu_erf(float g) {
  const float a = fabsf(g);
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f * 0.70710678118654752f, a, 1.0f));
  float p = __builtin_fmaf(0.5f * 1.061405429f, t, 0.5f * -1.453152027f);
  p = __builtin_fmaf(p, t, 0.5f * 1.421413741f);
  p = __builtin_fmaf(p, t, 0.5f * -0.284496736f);
  p = __builtin_fmaf(p, t, 0.5f * 0.254829592f);
  const float e = (p * t) * __builtin_amdgcn_exp2f((-0.5f * 1.4426950408889634f) * g * g);      // 0.5 * (1 - erf(|g| / sqrt 2))
  return __builtin_fmaf(-a, e, fmaxf(g, 0.f));
}

// proj.weight [2 * inner][C] (rows 0 .. inner-1: value, inner ..: gate) -> [tile pair v][K part hf][part][t][k-step f] fragments:
// lane (g, c) holds W[part * inner + frag_sigma(2 v + t, c)][32 (HKS hf + f) + 8 g .. + 7]
template <typename T, int C>
__global__ __launch_bounds__(64) void pack_w1_kernel(const T* __restrict__ w, T* __restrict__ packed) {
  using S = FfShape<C>;
  const int fr = blockIdx.x;                   // (((v * NH + hf) * 2 + part) * 2 + t) * HKS + f
  const int f = fr % S::HKS, t = (fr / S::HKS) & 1, part = (fr / (2 * S::HKS)) & 1, hf = (fr / (4 * S::HKS)) % S::NH, v = fr / (4 * S::HKS * S::NH);
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  const int row = part * S::INNER + frag_sigma(2 * v + t, c);
  const typename Tr<T>::V8 x = *(const typename Tr<T>::V8*)(w + (size_t)row * C + 32 * (S::HKS * hf + f) + 8 * g);
  *(typename Tr<T>::V8*)(packed + (size_t)fr * (FRAG / 2) + lane * 8) = x;
}

struct FF {
  const char* y;        // norm3 output, query-fragment order [R / 16][C / 32][1 KiB]
  const char* w;        // packed proj.weight
  const void* bias;     // [2 * inner] or null
  void* h;              // [R][inner] row-major, or fragment order (h_frag)
  long R;
  int h_frag;           // C = 320 only. 1: h leaves as [R / 16][inner / 32] fragments of 1 KiB (lane (g, c): channels 32 s + 8 g .. + 7 of row c) for sta_ff_out_res_hfrag
};

// THE counted-wait invariant of this kernel. vmcnt counts a wave's own memory instructions in issue order, so the waits in front
// of the barrier name "this sub-chunk's DMA" only because the number of instructions issued behind it is the same in every wave
// and on every path:
//   - EVERY wave issues five copies per sub-chunk (8 waves x 5 are the 40 fragments exactly: `stage` has no spare positions);
//   - the epilogue issues ALWAYS two stores per tile pair (rows past R: an offset the descriptor drops), row-major or fragment order.
// Hence vmcnt(2) in front of a tile pair's first sub-chunk (the previous tile pair's two stores may fly) and vmcnt(0) in front of
// a later K part (a sub-chunk that is not the tile pair's last has no epilogue, nothing was issued behind its successor's DMA).
template <typename T, int C>
__global__ __launch_bounds__(64 * FfShape<C>::NW, 2) void ff_geglu_qfrag_kernel(const FF p) {
  using S = FfShape<C>;
  using V8 = typename Tr<T>::V8;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  char* ring = smem;
  T* tab = (T*)(smem + 2 * S::SLOT);
  for (int i = threadIdx.x; i < 2 * S::INNER; i += 64 * S::NW) tab[i] = p.bias ? ((const T*)p.bias)[i] : (T)0.0f;
  __syncthreads();
  const __amdgpu_buffer_rsrc_t w_srd = make_srd(p.w, (unsigned)(S::NSC * S::SC_FR * FRAG));
  const unsigned lane16 = (unsigned)lane * 16u;
  // S::Ring::stage spelled out without its clamp of the spare positions: this ring has none (the static_assert of FfShape), and the
  // shared loop would add five scalar selects per sub-chunk here
  auto stage = [&](int sc, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < S::Ring::PER; ++i) {
      const int f = wv + S::NW * i;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_srd, (__attribute__((address_space(3))) void*)(ring + slot * S::SLOT + f * FRAG), 16, lane16,
                                               (unsigned)((sc * S::SC_FR + f) * FRAG), 0, 0);
    }
  };
  const __amdgpu_buffer_rsrc_t y_srd = make_srd(p.y, (unsigned)((size_t)p.R * C * sizeof(T)));
  const __amdgpu_buffer_rsrc_t h_srd = make_srd(p.h, (unsigned)((size_t)p.R * S::INNER * sizeof(T)));
  const long nblk = (p.R + 32 * S::NW - 1) / (32 * S::NW);
  const char* lbase = ring + lane * 16;
  stage(0, 0);
  for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const long row0 = (blk * S::NW + wv) * 32;            // this wave's two 16-row items; R % 16 == 0
    V8 b[2][S::NKS];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const long r0 = row0 + 16 * it;
      const unsigned vo = r0 < p.R ? (unsigned)(r0 * C * (long)sizeof(T)) + lane16 : SRD_DROP;
#pragma unroll
      for (int f = 0; f < S::NKS; ++f) b[it][f] = srd_load16<V8>(y_srd, vo, 1024u * f);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // y fragments + the sub-chunk 0 DMA (+ the previous pass's last stores)
    f32x4 acc[2][2][2];                                     // [part][t][item], across the K parts of a tile pair
    auto sub = [&](auto slot_tag, auto part_tag, const int v) __attribute__((always_inline)) {
      constexpr int SLOT = decltype(slot_tag)::value;       // the ring slot this sub-chunk landed in
      constexpr int HF = decltype(part_tag)::value;         // the K part: sub-chunk NH v + HF
      const int sc = S::NH * v + HF;
      if constexpr (HF == 0) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");      // this sub-chunk's DMA landed (the invariant above)
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      stage(sc + 1 < S::NSC ? sc + 1 : 0, SLOT ^ 1);        // next sub-chunk (sub-chunk 0 of the next pass behind the last one)
      const V8* fr = (const V8*)(lbase + SLOT * S::SLOT);
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        f32x4 a00, a01, a10, a11;
        if constexpr (HF == 0) { a00 = f32x4{0.f, 0.f, 0.f, 0.f}; a01 = a00; a10 = a00; a11 = a00; }
        else { a00 = acc[part][0][0]; a01 = acc[part][0][1]; a10 = acc[part][1][0]; a11 = acc[part][1][1]; }
#pragma unroll
        for (int q = 0; q < S::HKS / S::RG; ++q) {
          V8 wa[2][S::RG];
#pragma unroll
          for (int f = 0; f < S::RG; ++f) {
            wa[0][f] = fr[((part * 2 + 0) * S::HKS + S::RG * q + f) * 64];
            wa[1][f] = fr[((part * 2 + 1) * S::HKS + S::RG * q + f) * 64];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int f = 0; f < S::RG; ++f) {
            const int k = S::HKS * HF + S::RG * q + f;
            a00 = Tr<T>::mfma(wa[0][f], b[0][k], a00);
            a01 = Tr<T>::mfma(wa[0][f], b[1][k], a01);
            a10 = Tr<T>::mfma(wa[1][f], b[0][k], a10);
            a11 = Tr<T>::mfma(wa[1][f], b[1][k], a11);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        acc[part][0][0] = a00; acc[part][0][1] = a01; acc[part][1][0] = a10; acc[part][1][1] = a11;
      }
      if constexpr (HF == S::NH - 1) {
        // lane (g, c): tiles t = 0, 1, registers r -> channels 32 v + 8 g + 4 t + r of row c: 8 consecutive channels per item
        const V8 bv = *(const V8*)(tab + 32 * v + 8 * g), bg = *(const V8*)(tab + S::INNER + 32 * v + 8 * g);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const long row = row0 + 16 * it + c16;
          V8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float val = acc[0][e >> 2][it][e & 3] + (float)bv[e];
            const float gate = acc[1][e >> 2][it][e & 3] + (float)bg[e];
            o[e] = (T)(val * ff_gelu_erf(gate));
          }
          // Fragment order (level 0 only: the level-1 instance has no register for the select): the lane's 8 channels ARE lane
          // 16 g + c of fragment `v` of the item's group — one contiguous KiB per store
          bool h_frag = false;
          if constexpr (S::NH == 1) h_frag = p.h_frag;
          const unsigned ho = row0 + 16 * it >= p.R ? SRD_DROP
                            : h_frag ? (unsigned)((row0 + 16 * it) * S::INNER * (long)sizeof(T)) + (unsigned)v * (unsigned)FRAG + lane16
                                     : (unsigned)(row * S::INNER * (long)sizeof(T)) + (unsigned)(32 * v + 8 * g) * (unsigned)sizeof(T);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), h_srd, ho, 0, 0);
        }
      }
    };
    constexpr std::integral_constant<int, 0> _0{};
    constexpr std::integral_constant<int, 1> _1{};
    if constexpr (S::NH == 1) {                             // one sub-chunk per tile pair: the slot alternates with the tile pair
      for (int sp = 0; sp < S::NTP; sp += 2) {
        sub(_0, _0, sp);
        sub(_1, _0, sp + 1);
      }
    } else {                                                // two: the slot is the K half
      for (int v = 0; v < S::NTP; ++v) {
        sub(_0, _0, v);
        sub(_1, _1, v);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// -------------------------------------------------------------------------------------------------------------------------------
// The second half: out = x + h W2^T + b2   (FeedForward's output Linear, attention.py:66-69, + the block's last residual, :299),
// h read in the fragment order the kernel above writes. Same structure as csrc/sta_rowgemm.hip (a wave owns 16 rows and all 20
// output row tiles; the weight streamed through a 2-slot LDS ring in chunks of two row tiles x 10 k-steps), with the reduction
// dimension (1280) walked in four k-chunks of 320: the ten B fragments of the NEXT k-chunk are requested during the last two weight
// chunks of the current one. Roofline: HBM (2560 + 640 + 640 bytes per row against 2 * 1280 * 320 flop: 213 flop/B).
// -------------------------------------------------------------------------------------------------------------------------------
constexpr int F2_NKC = FF_INNER / FF_C;        // 4 k-chunks of 320
constexpr int F2_NRT = FF_C / 16;              // 20 output row tiles
constexpr int F2_NCH = F2_NRT / 2;             // 10 weight chunks (two row tiles) per k-chunk
constexpr int F2_CH_FR = 2 * FF_NKS;           // 20 fragments per chunk
using F2Ring = WRing<FF_NW, F2_CH_FR>;         // 3 LDS-DMA instructions per wave per chunk (4 padding copies), 24 KiB per slot
constexpr int F2_SLOT = F2Ring::SLOT;
constexpr int F2_LDS = 2 * F2_SLOT + FF_C * 2;

// net[2].weight [C][inner] -> [k-chunk kc][chunk v][t][k-step f] fragments: lane (g, c) holds
// W[32 v + 8 (c >> 2) + 4 t + (c & 3)][320 kc + 32 f + 8 g .. + 7]
template <typename T>
__global__ __launch_bounds__(64) void pack_w2_kernel(const T* __restrict__ w, T* __restrict__ packed) {
  const int fr = blockIdx.x;                   // ((kc * NCH + v) * 2 + t) * NKS + f
  const int f = fr % FF_NKS, t = (fr / FF_NKS) & 1, v = (fr / (2 * FF_NKS)) % F2_NCH, kc = fr / (2 * FF_NKS * F2_NCH);
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  const int row = 32 * v + 8 * (c >> 2) + 4 * t + (c & 3);     // frag_sigma(2 v + t, c), spelled out
  const typename Tr<T>::V8 x = *(const typename Tr<T>::V8*)(w + (size_t)row * FF_INNER + FF_C * kc + 32 * f + 8 * g);
  *(typename Tr<T>::V8*)(packed + (size_t)fr * (FRAG / 2) + lane * 8) = x;
}

struct F2 {
  const char* h;        // fragment order [R / 16][40][1 KiB]
  const char* w;        // packed net[2].weight
  const void* bias;     // [C] or null
  const void* x;        // [R][C] residual
  void* out;            // [R][C]
  long R;
};

template <typename T>
__global__ __launch_bounds__(64 * FF_NW, 2) void ff_out_res_hfrag_kernel(const F2 p) {
  using V8 = typename Tr<T>::V8;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  char* ring = smem;
  T* tab = (T*)(smem + 2 * F2_SLOT);
  for (int i = threadIdx.x; i < FF_C; i += 64 * FF_NW) tab[i] = p.bias ? ((const T*)p.bias)[i] : (T)0.0f;
  const __amdgpu_buffer_rsrc_t w_srd = make_srd(p.w, (unsigned)(F2_NKC * F2_NCH * F2_CH_FR * FRAG));
  const unsigned lane16 = (unsigned)lane * 16u;
  auto stage = [&](int chunk, int slot) __attribute__((always_inline)) {      // chunk = kc * NCH + ch, 0 .. 39
    F2Ring::stage(w_srd, ring + slot * F2_SLOT, 0u, chunk * F2_CH_FR, wv, lane16);
  };
  const __amdgpu_buffer_rsrc_t h_srd = make_srd(p.h, (unsigned)((size_t)p.R * FF_INNER * sizeof(T)));
  const long nblk = (p.R + 16 * FF_NW - 1) / (16 * FF_NW);
  auto h_off = [&](long blk) -> unsigned {
    const long row0 = (blk * FF_NW + wv) * 16;
    return (blk < nblk && row0 < p.R) ? (unsigned)(row0 * FF_INNER * (long)sizeof(T)) + lane16 : SRD_DROP;
  };
  long blk = blockIdx.x;
  V8 b[FF_NKS], bn[FF_NKS];
  stage(0, 0);
  {
    const unsigned vo = h_off(blk);
#pragma unroll
    for (int f = 0; f < FF_NKS; ++f) b[f] = srd_load16<V8>(h_srd, vo, 1024u * f);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const char* lbase = ring + lane * 16;
  for (; blk < nblk; blk += gridDim.x) {
    f32x4 acc[F2_NRT];
#pragma unroll
    for (int u = 0; u < F2_NRT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < F2_NKC; ++kc) {
      auto chunk = [&](auto ch_tag) __attribute__((always_inline)) {
        constexpr int CH = decltype(ch_tag)::value;
        constexpr int SLOT = CH & 1;
        // VMEM operations younger than this chunk's DMA that may stay in flight: the previous pass's 10 stores (chunk 0 of k-chunk 0),
        // the next k-chunk's ten B fragments (chunk 9: requested during chunk 8, behind that chunk's DMA)
        if constexpr (CH == 0) { if (kc == 0) asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        else if constexpr (CH == F2_NCH - 1) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        stage((kc * F2_NCH + CH + 1) % (F2_NKC * F2_NCH), SLOT ^ 1);
        if constexpr (CH == F2_NCH - 2) {      // B fragments of the next k-chunk (of the next pass behind the last one)
          const bool last = kc == F2_NKC - 1;
          const unsigned vo = h_off(last ? blk + gridDim.x : blk);
          const unsigned so = last ? 0u : (unsigned)(kc + 1) * (unsigned)(FF_NKS * FRAG);
#pragma unroll
          for (int f = 0; f < FF_NKS; ++f) bn[f] = srd_load16<V8>(h_srd, vo, so + 1024u * f);
        }
        const V8* fr = (const V8*)(lbase + SLOT * F2_SLOT);
        f32x4 a0 = acc[2 * CH], a1 = acc[2 * CH + 1];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          V8 wa[2][FF_NKS / 2];
#pragma unroll
          for (int f = 0; f < FF_NKS / 2; ++f) {
            wa[0][f] = fr[(half * (FF_NKS / 2) + f) * 64];
            wa[1][f] = fr[(FF_NKS + half * (FF_NKS / 2) + f) * 64];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int f = 0; f < FF_NKS / 2; ++f) {
            a0 = Tr<T>::mfma(wa[0][f], b[half * (FF_NKS / 2) + f], a0);
            a1 = Tr<T>::mfma(wa[1][f], b[half * (FF_NKS / 2) + f], a1);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        acc[2 * CH] = a0;
        acc[2 * CH + 1] = a1;
      };
      sta_static_for<F2_NCH>(chunk);
#pragma unroll
      for (int f = 0; f < FF_NKS; ++f) b[f] = bn[f];
    }
    // ---- epilogue: + bias + residual; ALWAYS ten stores (rows past R dropped by the descriptor): the counted vmcnt relies on it
    const long row0 = (blk * FF_NW + wv) * 16;
    const long row = row0 + c16;
    const bool ok = row0 < p.R;
    const T* xr = (const T*)p.x + (ok ? row : 0) * FF_C + 8 * g;
    const __amdgpu_buffer_rsrc_t o_srd = make_srd(p.out, (unsigned)((size_t)p.R * FF_C * sizeof(T)));
#pragma unroll
    for (int v = 0; v < F2_NCH; ++v) {
      const V8 xv = *(const V8*)(xr + 32 * v);
      const V8 bs = *(const V8*)(tab + 32 * v + 8 * g);
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (T)(acc[2 * v + (e >> 2)][e & 3] + (float)bs[e] + (float)xv[e]);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), o_srd,
                                             ok ? (unsigned)(row * FF_C * (long)sizeof(T)) + (unsigned)(32 * v + 8 * g) * (unsigned)sizeof(T) : SRD_DROP, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The host side of the GEGLU projection pass at shape C: what the sta_ff_geglu_* (C = 320) and sta_ff_geglu_c640_* entry points
// share. `name` / `what`: the texts by which an entry point's errors name it.
template <int C>
size_t ff_geglu_packed_bytes(int c, int inner) {
  using S = FfShape<C>;
  return (c == C && inner == S::INNER) ? (size_t)S::NSC * S::SC_FR * FRAG : 0;
}

template <int C>
int ff_geglu_pack(const char* what, const void* w, void* packed, int c, int inner, int dtype, void* stream) {
  using S = FfShape<C>;
  g_sta_err[0] = 0;
  if (!w || !packed) return sta_fail(STA_E_ARG, "null pointer");
  if (ff_geglu_packed_bytes<C>(c, inner) == 0) return sta_fail(STA_E_UNSUP, "fused GEGLU projection%s: C = %d, inner = %d only (C=%d inner=%d)", S::TAG, C, S::INNER, c, inner);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return sta_launch<pack_w1_kernel<T, C>>(what, dim3(S::NSC * S::SC_FR), dim3(64), 0, st, (const T*)w, (T*)packed);
  });
}

template <int C>
int ff_geglu_launch(const char* name, const char* what, const void* y_qfrag, const void* packed_w, const void* bias, void* h, long R,
                    int c, int inner, int h_frag, int max_workgroups, int dtype, void* stream) {
  using S = FfShape<C>;
  g_sta_err[0] = 0;
  if (!y_qfrag || !packed_w || !h) return sta_fail(STA_E_ARG, "null pointer");
  if (ff_geglu_packed_bytes<C>(c, inner) == 0) return sta_fail(STA_E_UNSUP, "fused GEGLU projection%s: C = %d, inner = %d only (C=%d inner=%d)", S::TAG, C, S::INNER, c, inner);
  if (R <= 0 || R % 16) return sta_fail(STA_E_ARG, "%s: R=%ld (need a positive multiple of 16 rows)", name, R);
  if ((size_t)R * inner * 2 >= 0xfffffff0ull) return sta_fail(STA_E_UNSUP, "activations must stay below 4 GiB (R=%ld)", R);
  if (max_workgroups < 0) return sta_fail(STA_E_ARG, "%s: max_workgroups=%d", name, max_workgroups);
  FF p{(const char*)y_qfrag, (const char*)packed_w, bias, h, R, h_frag};
  const long nblk = (R + 32 * S::NW - 1) / (32 * S::NW);
  const long cap = max_workgroups > 0 && max_workgroups < 256 ? max_workgroups : 256;
  const unsigned grid = (unsigned)(nblk < cap ? nblk : cap);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto t) {
    return sta_launch_lds<ff_geglu_qfrag_kernel<decltype(t), C>>(what, S::LDS, dim3(grid), dim3(64 * S::NW), S::LDS, st, p);
  });
}

}  // namespace

extern "C" {

size_t sta_ff_out_packed_w_bytes(int C, int inner) {
  return (C == FF_C && inner == FF_INNER) ? (size_t)F2_NKC * F2_NCH * F2_CH_FR * FRAG : 0;
}

int sta_ff_out_pack_w(const void* w, void* packed, int C, int inner, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!w || !packed) return sta_fail(STA_E_ARG, "null pointer");
  if (sta_ff_out_packed_w_bytes(C, inner) == 0) return sta_fail(STA_E_UNSUP, "fused feed-forward output: C = 320, inner = 1280 only (C=%d inner=%d)", C, inner);
  hipStream_t st = (hipStream_t)stream;
  const unsigned nfr = F2_NKC * F2_NCH * F2_CH_FR;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<pack_w2_kernel<T>>("pack_w2 launch", dim3(nfr), dim3(64), 0, st, (const T*)w, (T*)packed);
  });
}

int sta_ff_out_res_hfrag(const void* h_frag, const void* packed_w, const void* bias, const void* x, void* out, long R, int C, int inner,
                         int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!h_frag || !packed_w || !x || !out) return sta_fail(STA_E_ARG, "null pointer");
  if (sta_ff_out_packed_w_bytes(C, inner) == 0) return sta_fail(STA_E_UNSUP, "fused feed-forward output: C = 320, inner = 1280 only (C=%d inner=%d)", C, inner);
  if (R <= 0 || R % 16) return sta_fail(STA_E_ARG, "ff_out_res_hfrag: R=%ld (need a positive multiple of 16 rows)", R);
  if ((size_t)R * inner * 2 >= 0xfffffff0ull) return sta_fail(STA_E_UNSUP, "activations must stay below 4 GiB (R=%ld)", R);
  F2 p{(const char*)h_frag, (const char*)packed_w, bias, x, out, R};
  const long nblk = (R + 16 * FF_NW - 1) / (16 * FF_NW);
  const unsigned grid = (unsigned)(nblk < 256 ? nblk : 256);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    return sta_launch_lds<ff_out_res_hfrag_kernel<decltype(tag)>>("ff_out_res_hfrag launch", F2_LDS, dim3(grid), dim3(64 * FF_NW), F2_LDS, st, p);
  });
}

size_t sta_ff_geglu_packed_w_bytes(int C, int inner) { return ff_geglu_packed_bytes<320>(C, inner); }
int sta_ff_geglu_pack_w(const void* w, void* packed, int C, int inner, int dtype, void* stream) {
  return ff_geglu_pack<320>("pack_w1 launch", w, packed, C, inner, dtype, stream);
}
int sta_ff_geglu_qfrag(const void* y_qfrag, const void* packed_w, const void* bias, void* h, long R, int C, int inner, int h_frag,
                       int dtype, void* stream) {
  return ff_geglu_launch<320>("ff_geglu_qfrag", "ff_geglu_qfrag launch", y_qfrag, packed_w, bias, h, R, C, inner, h_frag ? 1 : 0, 0, dtype, stream);
}

size_t sta_ff_geglu_c640_packed_w_bytes(int C, int inner) { return ff_geglu_packed_bytes<640>(C, inner); }
int sta_ff_geglu_c640_pack_w(const void* w, void* packed, int C, int inner, int dtype, void* stream) {
  return ff_geglu_pack<640>("pack_w1_c640 launch", w, packed, C, inner, dtype, stream);
}
int sta_ff_geglu_c640_qfrag(const void* y_qfrag, const void* packed_w, const void* bias, void* h, long R, int C, int inner,
                            int max_workgroups, int dtype, void* stream) {
  return ff_geglu_launch<640>("ff_geglu_c640_qfrag", "ff_geglu_c640_qfrag launch", y_qfrag, packed_w, bias, h, R, C, inner, 0, max_workgroups, dtype, stream);
}

}  // extern "C"

// The tail of a SpatialTransformer (the output Linear above + proj_out as one GEMM), built with this translation unit
#include "sta_rowstail.hip"
