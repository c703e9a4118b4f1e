// sta_wring_dev.h — the device-side pieces the streamed-weight passes share (sta_rowgemm.hip, sta_ffgemm.hip, sta_lnqkv.hip,
// sta_gemm.hip, sta_conv.hip; sta_rows_dev.h builds the skeleton of sta_rows640.hip and sta_rowstail.hip on them): the 2-slot LDS
// weight ring, the row permutation of their packed weights, the wave reduction of
// the LayerNorm kernels, the DPP row sum of the statistics epilogues, the dropped buffer offset and a compile-time loop. gfx950 only. Needs nothing but the HIP runtime, so
// the glue kernels (sta_unet.hip, sta_unet_bwd.hip) take wave_sum from here too.
#ifndef STA_WRING_DEV_H
#define STA_WRING_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

namespace {

constexpr int FRAG = 1024;  // bytes of one operand fragment (64 lanes x 16 B)

// A buffer offset no descriptor of this library covers: every descriptor is built with num_records <= 0xfffffff0 (the host
// wrappers refuse larger tensors), and the raw-buffer bounds check compares offset + size against num_records — a load at
// SRD_DROP returns zeros, a store is dropped. It is the predicate for rows / pixels past the end where the NUMBER of memory
// instructions must not depend on the data (counted s_waitcnt vmcnt(n)).
constexpr unsigned SRD_DROP = 0xfffffff0u;

// Row of the weight held by lane row `rho` (0 .. 15) of packed row tile `u`: the accumulators of tiles 2v | 2v + 1 in lane
// (g, c) are then the 8 CONSECUTIVE output channels 32 v + 8 g .. + 7 of row c (16-byte epilogue accesses).
__host__ __device__ constexpr int frag_sigma(int u, int rho) { return 32 * (u >> 1) + 8 * (rho >> 2) + 4 * (u & 1) + (rho & 3); }

// Sum over the 64 lanes of a wave, result in every lane. ONE butterfly for every LayerNorm in the library: kernels that promise
// bit-identical row statistics (sta_lnqkv.hip against sta_unet.hip::add_layernorm_kernel) get them by calling the same function
// (the wave-per-row kernels through ln_mean / ln_rstd of sta_trunk_dev.h).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Sum over the 16 lanes of a DPP row (lanes 16 g .. 16 g + 15), result in every lane: xor 1, xor 2, half-row mirror, row mirror. The
// epilogues that accumulate a consumer GroupNorm's statistics (sta_conv.hip, sta_gemm.hip, sta_encode.hip, sta_rowstail.hip) fold the
// 16 rows / pixels of an MFMA column group with it.
__device__ __forceinline__ float row16_sum(float x) {
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xf, 0xf, true));   // row_half_mirror
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xf, 0xf, true));   // row_mirror
  return x;
}

// f(integral_constant<int, 0>{}), ..., f(integral_constant<int, N - 1>{}) in this order: a loop whose index is a constant expression
template <typename F, int... I>
__device__ __forceinline__ void sta_static_for_seq(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void sta_static_for(F&& f) {
  sta_static_for_seq(f, std::make_integer_sequence<int, N>{});
}

// The weight ring: a packed weight (1-KiB fragments in lane order) streamed chunk by chunk through two LDS slots by LDS-DMA, one
// chunk ahead of the MFMAs. NW waves share the NFR fragments of a chunk round-robin (wave wv: fragments wv, wv + NW, ...).
//
// The invariant every user's counted `s_waitcnt vmcnt(n)` rests on: EVERY wave issues exactly PER copies per chunk, whatever wv
// is. vmcnt counts a wave's own outstanding memory instructions in issue order, so "wait until at most n are in flight" names
// this chunk's DMA only if the number of instructions issued behind it is the same in every wave and on every path. Where
// NW does not divide NFR the spare positions f >= NFR therefore still copy — fragment 0 again, into the slot's padding
// [NFR * FRAG, SLOT) that no MFMA operand read touches — and the slot is PER * NW fragments, not NFR.
template <int NW, int NFR>
struct WRing {
  static constexpr int PER = (NFR + NW - 1) / NW;   // LDS-DMA instructions per wave per chunk
  static constexpr int SLOT = PER * NW * FRAG;      // bytes of one ring slot
  // The chunk that starts `src` bytes + `first` fragments into the weight behind `srd` -> the slot at `slot`; lane16 = lane * 16
  // (the buffer form keeps the per-lane part of the address in ONE register, the fragment is a scalar offset). A caller gives the
  // chunk's position in ONE of the two units and 0 in the other — the row passes count fragments (signed: (first + f) * FRAG),
  // sta_gemm.hip / sta_conv.hip bytes (unsigned: src + f * FRAG); hipcc selects different scalar code for the two spellings, and each
  // kernel keeps the one it was tuned and measured with. The same holds for the select of the spare positions: written for every
  // position, hipcc emits a scalar compare + select even where i alone shows that the position is never spare. STATIC_SPARE
  // leaves the select to the positions that can be spare. The row passes of sta_rows_dev.h were tuned and measured that way and
  // pass `true`; every other user was tuned with the plain form, and turning the flag on there changes hot machine code: it
  // wants its own measurement (profiles/rows_one_core.md).
  template <bool STATIC_SPARE = false>
  static __device__ __forceinline__ void stage(__amdgpu_buffer_rsrc_t srd, char* slot, unsigned src, int first, int wv, unsigned lane16) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int f = wv + NW * i;
      const int fs = (STATIC_SPARE && (i + 1) * NW <= NFR) || f < NFR ? f : 0;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (__attribute__((address_space(3))) void*)(slot + f * FRAG), 16, lane16,
                                               src + (unsigned)((first + fs) * FRAG), 0, 0);
    }
  }
};

}  // namespace
#endif
