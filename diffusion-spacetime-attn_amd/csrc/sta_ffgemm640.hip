// sta_ffgemm640.hip — the first half of the block's feed-forward at SD-v1 level 1 (C = 640, inner = 2560) as ONE pass:
//
//     h = (y W_v^T + b_v) * gelu(y W_g^T + b_g)          GEGLU.forward (attention.py:42-45) inside FeedForward (:48-69), called at :299
//
// the level-0 pass of csrc/sta_ffgemm.hip (ff_geglu_qfrag_kernel) at twice the reduction length. Row-major, this is a library GEMM
// that writes the [R][5120] projection (1.34 GB at 131072 rows) followed by the GEGLU pass that reads it back and writes [R][2560];
// here the projection never exists in HBM. The level-0 kernel keeps its instructions: this is a kernel of its own beside it.
//
// Rows are the MFMA columns: Out^T = W' y^T. B operand = one 1-KiB fragment of y per k-step, 2 x 20 of them per wave (32 rows,
// 160 VGPRs) held for a whole 256-row pass. A operand = proj.weight [5120][640] re-laid out once per model: 160 sub-chunks of 40
// fragments = {value tiles 2v, 2v+1; gate tiles 2v, 2v+1} x ONE HALF of K (10 k-steps), rows permuted by frag_sigma so that a
// lane's two value tiles are 8 consecutive channels. (A whole {pair, pair} x 20 k-steps sub-chunk is 80 KiB and does not fit beside
// a second ring slot.) The eight accumulators live across the two halves of a tile pair; the level-0 epilogue (bias, exact-erf
// GELU, one rounding, two 16-byte stores) runs behind the second half. Per sub-chunk a wave issues 80 MFMAs behind 40 operand
// reads, as at level 0; the operands are read in quarters of a tile pair (2 x 5 fragments) — with halves the kernel spills.
//
// Register budget: 160 (y) + 32 (accumulators) + 40 (operands) + addressing = 255 of the 256 two waves per SIMD leave: the build
// refuses a toolchain that spills it (sta/lib.py::NO_SPILL_KERNELS).
//
// Roofline: MFMA (2 * 640 * 5120 flop per row = 6.55 MFLOP against 1280 + 5120 bytes: 1024 flop/B).
//
// Not a translation unit of its own: sta_ffgemm.hip includes this file at its end (sta/lib.py::INCLUDED_SOURCES) — same flags
// (-ffinite-math-only), same pass through the hazard lint, and ff_gelu_erf is that file's.

namespace {

constexpr int G6_C = 640, G6_INNER = 2560;
constexpr int G6_NKS = G6_C / 32;              // 20 k-steps
constexpr int G6_HKS = G6_NKS / 2;             // 10 per sub-chunk (one half of K)
constexpr int G6_QKS = G6_HKS / 2;             // 5 per operand read group
constexpr int G6_NTP = G6_INNER / 32;          // 80 tile pairs (a pair of value tiles + its pair of gate tiles each)
constexpr int G6_NSC = 2 * G6_NTP;             // 160 sub-chunks: tile pair v, K half hf -> 2 v + hf
constexpr int G6_SC_FR = 4 * G6_HKS;           // 40 fragments per sub-chunk
constexpr int G6_NW = 8;
using G6Ring = WRing<G6_NW, G6_SC_FR>;         // 5 LDS-DMA instructions per wave per sub-chunk, 40 KiB per slot, no spare positions
constexpr int G6_SLOT = G6Ring::SLOT;
constexpr int G6_TAB = 2 * G6_INNER * 2;       // bias (value | gate) as 16-bit behind the ring: 10 KiB
constexpr int G6_LDS = 2 * G6_SLOT + G6_TAB;   // 90 KiB
static_assert(G6Ring::PER * G6_NW == G6_SC_FR, "the ring of this kernel has no spare positions");

// proj.weight [2 * inner][C] (rows 0 .. inner-1: value, inner ..: gate) -> [tile pair v][K half hf][part][t][k-step f] fragments:
// lane (g, c) holds W[part * inner + 32 v + 8 (c >> 2) + 4 t + (c & 3)][32 (10 hf + f) + 8 g .. + 7]
template <typename T>
__global__ __launch_bounds__(64) void pack_w1_c640_kernel(const T* __restrict__ w, T* __restrict__ packed) {
  const int fr = blockIdx.x;                   // (((v * 2 + hf) * 2 + part) * 2 + t) * HKS + f
  const int f = fr % G6_HKS, t = (fr / G6_HKS) & 1, part = (fr / (2 * G6_HKS)) & 1, hf = (fr / (4 * G6_HKS)) & 1, v = fr / (8 * G6_HKS);
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  const int row = part * G6_INNER + frag_sigma(2 * v + t, c);
  const typename Tr<T>::V8 x = *(const typename Tr<T>::V8*)(w + (size_t)row * G6_C + 32 * (G6_HKS * hf + f) + 8 * g);
  *(typename Tr<T>::V8*)(packed + (size_t)fr * (FRAG / 2) + lane * 8) = x;
}

struct G6 {
  const char* y;        // norm3 output, query-fragment order [R / 16][20][1 KiB]
  const char* w;        // packed proj.weight
  const void* bias;     // [2 * inner] or null
  void* h;              // [R][inner] row-major
  long R;
};

template <typename T>
__global__ __launch_bounds__(64 * G6_NW, 2) void ff_geglu_c640_qfrag_kernel(const G6 p) {
  using V8 = typename Tr<T>::V8;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  char* ring = smem;
  T* tab = (T*)(smem + 2 * G6_SLOT);
  for (int i = threadIdx.x; i < 2 * G6_INNER; i += 64 * G6_NW) tab[i] = p.bias ? ((const T*)p.bias)[i] : (T)0.0f;
  __syncthreads();
  const __amdgpu_buffer_rsrc_t w_srd = make_srd(p.w, (unsigned)(G6_NSC * G6_SC_FR * FRAG));
  const unsigned lane16 = (unsigned)lane * 16u;
  // 8 waves x 5 copies are the 40 fragments exactly: EVERY wave issues five copies per sub-chunk (the counted waits below)
  auto stage = [&](int sc, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < G6Ring::PER; ++i) {
      const int f = wv + G6_NW * i;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_srd, (__attribute__((address_space(3))) void*)(ring + slot * G6_SLOT + f * FRAG), 16, lane16,
                                               (unsigned)((sc * G6_SC_FR + f) * FRAG), 0, 0);
    }
  };
  const __amdgpu_buffer_rsrc_t y_srd = make_srd(p.y, (unsigned)((size_t)p.R * G6_C * sizeof(T)));
  const __amdgpu_buffer_rsrc_t h_srd = make_srd(p.h, (unsigned)((size_t)p.R * G6_INNER * sizeof(T)));
  const long nblk = (p.R + 32 * G6_NW - 1) / (32 * G6_NW);
  const char* lbase = ring + lane * 16;
  stage(0, 0);
  for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const long row0 = (blk * G6_NW + wv) * 32;            // this wave's two 16-row items; R % 16 == 0
    V8 b[2][G6_NKS];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const long r0 = row0 + 16 * it;
      const unsigned vo = r0 < p.R ? (unsigned)(r0 * G6_C * (long)sizeof(T)) + lane16 : SRD_DROP;
#pragma unroll
      for (int f = 0; f < G6_NKS; ++f) b[it][f] = srd_load16<V8>(y_srd, vo, 1024u * f);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // y fragments + the sub-chunk 0 DMA (+ the previous pass's last stores)
    f32x4 acc[2][2][2];                                     // [part][t][item], across the two K halves of a tile pair
    auto sub = [&](auto half_tag, const int v) __attribute__((always_inline)) {
      constexpr int HF = decltype(half_tag)::value;         // the K half, and the ring slot: sub-chunk 2 v + HF
      const int sc = 2 * v + HF;
      // This sub-chunk's DMA landed. Behind it in issue order: the previous tile pair's two stores in front of a first half
      // (they may fly), nothing in front of a second half (a first half has no epilogue).
      if constexpr (HF == 0) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      stage(sc + 1 < G6_NSC ? sc + 1 : 0, HF ^ 1);          // next sub-chunk (sub-chunk 0 of the next pass behind the last one)
      const V8* fr = (const V8*)(lbase + HF * G6_SLOT);
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        f32x4 a00, a01, a10, a11;
        if constexpr (HF == 0) { a00 = f32x4{0.f, 0.f, 0.f, 0.f}; a01 = a00; a10 = a00; a11 = a00; }
        else { a00 = acc[part][0][0]; a01 = acc[part][0][1]; a10 = acc[part][1][0]; a11 = acc[part][1][1]; }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          V8 wa[2][G6_QKS];
#pragma unroll
          for (int f = 0; f < G6_QKS; ++f) {
            wa[0][f] = fr[((part * 2 + 0) * G6_HKS + G6_QKS * q + f) * 64];
            wa[1][f] = fr[((part * 2 + 1) * G6_HKS + G6_QKS * q + f) * 64];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int f = 0; f < G6_QKS; ++f) {
            constexpr int K0 = G6_HKS * HF;
            const int k = K0 + G6_QKS * q + f;
            a00 = Tr<T>::mfma(wa[0][f], b[0][k], a00);
            a01 = Tr<T>::mfma(wa[0][f], b[1][k], a01);
            a10 = Tr<T>::mfma(wa[1][f], b[0][k], a10);
            a11 = Tr<T>::mfma(wa[1][f], b[1][k], a11);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        acc[part][0][0] = a00; acc[part][0][1] = a01; acc[part][1][0] = a10; acc[part][1][1] = a11;
      }
      if constexpr (HF == 1) {
        // lane (g, c): tiles t = 0, 1, registers r -> channels 32 v + 8 g + 4 t + r of row c: 8 consecutive channels per item
        const V8 bv = *(const V8*)(tab + 32 * v + 8 * g), bg = *(const V8*)(tab + G6_INNER + 32 * v + 8 * g);
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
          // ALWAYS two stores per tile pair (rows past R: an offset the descriptor drops): the counted vmcnt above relies on it
          const unsigned ho = row0 + 16 * it >= p.R ? SRD_DROP
                            : (unsigned)(row * G6_INNER * (long)sizeof(T)) + (unsigned)(32 * v + 8 * g) * (unsigned)sizeof(T);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), h_srd, ho, 0, 0);
        }
      }
    };
    for (int v = 0; v < G6_NTP; ++v) {
      sub(std::integral_constant<int, 0>{}, v);
      sub(std::integral_constant<int, 1>{}, v);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

extern "C" {

size_t sta_ff_geglu_c640_packed_w_bytes(int C, int inner) {
  return (C == G6_C && inner == G6_INNER) ? (size_t)G6_NSC * G6_SC_FR * FRAG : 0;
}

int sta_ff_geglu_c640_pack_w(const void* w, void* packed, int C, int inner, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!w || !packed) return sta_fail(STA_E_ARG, "null pointer");
  if (sta_ff_geglu_c640_packed_w_bytes(C, inner) == 0) return sta_fail(STA_E_UNSUP, "fused GEGLU projection (c640): C = 640, inner = 2560 only (C=%d inner=%d)", C, inner);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<pack_w1_c640_kernel<T>>("pack_w1_c640 launch", dim3(G6_NSC * G6_SC_FR), dim3(64), 0, st, (const T*)w, (T*)packed);
  });
}

int sta_ff_geglu_c640_qfrag(const void* y_qfrag, const void* packed_w, const void* bias, void* h, long R, int C, int inner,
                            int max_workgroups, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!y_qfrag || !packed_w || !h) return sta_fail(STA_E_ARG, "null pointer");
  if (sta_ff_geglu_c640_packed_w_bytes(C, inner) == 0) return sta_fail(STA_E_UNSUP, "fused GEGLU projection (c640): C = 640, inner = 2560 only (C=%d inner=%d)", C, inner);
  if (R <= 0 || R % 16) return sta_fail(STA_E_ARG, "ff_geglu_c640_qfrag: R=%ld (need a positive multiple of 16 rows)", R);
  if ((size_t)R * inner * 2 >= 0xfffffff0ull) return sta_fail(STA_E_UNSUP, "activations must stay below 4 GiB (R=%ld)", R);
  if (max_workgroups < 0) return sta_fail(STA_E_ARG, "ff_geglu_c640_qfrag: max_workgroups=%d", max_workgroups);
  G6 p{(const char*)y_qfrag, (const char*)packed_w, bias, h, R};
  const long nblk = (R + 32 * G6_NW - 1) / (32 * G6_NW);
  const long cap = max_workgroups > 0 && max_workgroups < 256 ? max_workgroups : 256;
  const unsigned grid = (unsigned)(nblk < cap ? nblk : cap);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    return sta_launch_lds<ff_geglu_c640_qfrag_kernel<decltype(tag)>>("ff_geglu_c640_qfrag launch", G6_LDS, dim3(grid), dim3(64 * G6_NW), G6_LDS, st, p);
  });
}

}  // extern "C"
