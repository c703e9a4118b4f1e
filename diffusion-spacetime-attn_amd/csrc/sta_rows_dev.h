// sta_rows_dev.h — the skeleton of the row passes whose wave holds 320 of a row's output channels: sta_rows640.hip (rows640_kernel,
// at the end of sta_rowgemm.hip) and sta_rowstail.hip (rows_tail_kernel, at the end of sta_ffgemm.hip). What the two share is here
// once; each keeps its own B-operand schedule (where A comes from, how far ahead, in which index width) and its own epilogue.
//
// The skeleton. Rows are the MFMA columns. Persistent workgroups of 8 waves; a wave owns 32 rows (two 16-row items) x 320 output
// channels = 2 x 20 accumulator tiles (160 registers), and every weight fragment it reads from LDS serves both items.
//   C = 640: 4 row groups x 2 column halves, 128 rows per pass, 40 fragments (40 KiB) per k-step; half h reads fragments 20 h .. + 19.
//   C = 320: 8 row groups, no column halves, 256 rows per pass, 20 fragments (20 KiB) per k-step.
//   A operand = the weight [C][K], re-laid out once per model (rows_pack_kernel): fragment (k-step f, row tile u) at [f][u], lane
//               (g, c) holding W[frag_sigma(u, c)][32 f + 8 g .. + 7] — a lane's tile pair 2v | 2v + 1 is 8 CONSECUTIVE output
//               channels. Streamed through the 2-slot LDS ring (sta_wring_dev.h) one k-step ahead.
//   B operand = 16 bytes per lane and (item, k-step) straight from the activations, requested two k-steps ahead into one of four
//               register sets.
// These kernels sit at 234 - 256 VGPRs for two waves per SIMD (sta/lib.py::NO_SPILL_KERNELS): the helpers below are forced inline,
// and sharing more than they do (the epilogue loop) changes the schedule of some instantiation (profiles/rows_one_core.md).
//
// THE counted-wait invariant of both kernels. vmcnt counts a wave's own memory instructions in issue order; the waits in front of
// the barriers name "this k-step's DMA" only because every wave issues the same instructions on every path:
//   - per k-step Ring::PER LDS-DMA copies (the spare positions of C = 320 copy too) and, behind them, the two B loads of k-step + 2
//     (of the next pass's first two k-steps behind the last two; rows past R or no next pass: an offset the descriptor drops);
//   - per pass the loads and NST stores of the kernel's epilogue, a fixed number each, dropped the same way for rows past R.
// Hence vmcnt(2) in front of a k-step (the two B loads issued behind its DMA may fly) and vmcnt(NST) in front of a pass's first
// (the previous epilogue's stores may fly; its loads, the B loads and the DMA of k-step 0 are all older than those). NST is the
// one number a kernel states for itself.
#ifndef STA_ROWS_DEV_H
#define STA_ROWS_DEV_H
#include "sta_xattn_dev.h"  // Tr<T>, f32x4; through it sta_internal.h (host helpers) and sta_wring_dev.h (WRing, frag_sigma)

namespace {

template <int C_>
struct RowsShape {
  static_assert(C_ == 320 || C_ == 640, "SD-v1 level 0 or level 1");
  static constexpr int C = C_;
  static constexpr int NW = 8;
  static constexpr int NH = C / 320;                 // column halves: 1 | 2
  static constexpr int NG = NW / NH;                 // row groups of 32 rows: 8 | 4
  static constexpr int ROWS = 32 * NG;               // rows per workgroup pass: 256 | 128
  static constexpr int NRT = C / 16;                 // output row tiles = the fragments of one k-step: 20 | 40
  static constexpr int HT = 20;                      // tiles per wave (320 channels)
  static constexpr int NTP = HT / 2;                 // tile pairs per wave
  static constexpr int QF = 5;                       // operand fragments read per group (a quarter of a wave's tiles)
  using Ring = WRing<NW, NRT>;                       // 3 (4 padding copies) | 5 LDS-DMA instructions per wave per k-step
  static constexpr int SLOT = Ring::SLOT;            // 24 | 40 KiB
};

// W [C][K] -> [k-step f][row tile u] fragments, nrt = C / 16 row tiles: lane (g, c) holds W[frag_sigma(u, c)][32 f + 8 g .. + 7]
template <typename T>
__global__ __launch_bounds__(64) void rows_pack_kernel(const T* __restrict__ w, T* __restrict__ packed, int K, int nrt) {
  const int fr = blockIdx.x;                   // f * nrt + u
  const int f = fr / nrt, u = fr % nrt;
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  const typename Tr<T>::V8 x = *(const typename Tr<T>::V8*)(w + (size_t)frag_sigma(u, c) * K + 32 * f + 8 * g);
  *(typename Tr<T>::V8*)(packed + (size_t)fr * (FRAG / 2) + lane * 8) = x;
}

// the dtype check (`bad`: the entry point's code for it) and the launch of both *_pack_w entry points; shapes are theirs to refuse
inline int rows_pack_w(const char* what, const void* w, void* packed, int C, int K, int dtype, int bad, void* stream) {
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(bad, "dtype %d", dtype);
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<rows_pack_kernel<T>>(what, dim3((K / 32) * (C / 16)), dim3(64), 0, (hipStream_t)stream, (const T*)w, (T*)packed, K, C / 16);
  });
}

// The refusals the two entry points share, in the order both test them: 0 or sta_fail's code. `a_row` = bytes of a row of the
// widest operand (32-bit buffer offsets); `unsup` = what the entry point answers where the library, not the caller, sets the limit.
inline int rows_refuse(const char* name, long R, size_t a_row, int max_workgroups, int dtype, int unsup) {
  if (R <= 0 || R % 16) return sta_fail(STA_E_ARG, "%s: R=%ld (need a positive multiple of 16 rows)", name, R);
  if ((size_t)R * a_row >= 0xfffffff0ull) return sta_fail(unsup, "activations must stay below 4 GiB (R=%ld)", R);
  if (max_workgroups < 0) return sta_fail(STA_E_ARG, "%s: max_workgroups=%d", name, max_workgroups);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(unsup, "dtype %d", dtype);
  return 0;
}

// the persistent grid: one workgroup per pass of `rows` rows, at most one per CU (256) or max_workgroups if that is smaller
inline unsigned rows_grid(long R, long rows, int max_workgroups) {
  const long nblk = (R + rows - 1) / rows;
  const long cap = max_workgroups > 0 && max_workgroups < 256 ? max_workgroups : 256;
  return (unsigned)(nblk < cap ? nblk : cap);
}

// The lane id again, opaque to hipcc: what is derived from it (table, exchange and row offsets) is then computed where it is used
// and not kept in registers across the MFMA loop, which has none to spare (rows640_kernel's LN instance spills otherwise).
__device__ __forceinline__ int rows_opaque_lane(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

// One k-step of a wave: its HT weight fragments from `fr` (this lane's 16 bytes of fragment 0 in the landed slot) in groups of QF,
// each fragment against the B operands of both items.
template <typename T, int HT, int QF>
__device__ __forceinline__ void rows_mfma_step(const typename Tr<T>::V8* fr, typename Tr<T>::V8 b0, typename Tr<T>::V8 b1, f32x4 (&acc)[2][HT]) {
#pragma unroll
  for (int q = 0; q < HT / QF; ++q) {
    typename Tr<T>::V8 wa[QF];
#pragma unroll
    for (int t = 0; t < QF; ++t) wa[t] = fr[(QF * q + t) * 64];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < QF; ++t) {
      acc[0][QF * q + t] = Tr<T>::mfma(wa[t], b0, acc[0][QF * q + t]);
      acc[1][QF * q + t] = Tr<T>::mfma(wa[t], b1, acc[1][QF * q + t]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace
#endif
