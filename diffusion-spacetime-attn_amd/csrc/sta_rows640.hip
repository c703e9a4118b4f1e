// sta_rows640.hip — the output Linears of a transformer block at SD-v1 level 1 (C = 640) with the residual add, and for the two
// attention outputs the LayerNorm that follows, as ONE pass over row-major activations:
//
//     s = x + A W^T + b ;  y = LayerNorm(s)          K = 640:  attn1.to_out + residual + norm2, attn2.to_out + residual + norm3
//     s = x + A W^T + b                              K = 2560: ff.net[2] + the block's last residual
//
// Row-major, each site is a library GEMM that writes [R][640] and a glue pass (sta_add_layernorm_qfrag / an elementwise add) that
// reads it back: here the Linear's result never exists in HBM. Not a translation unit of its own: #included at the end of
// sta_rowgemm.hip (sta/lib.py::INCLUDED_SOURCES), whose headers, flags and hazard lint it shares.
//
// Rows are the MFMA columns, as in sta_rowgemm.hip, but one wave cannot hold a whole 640-channel output row of its pixels (the level-0
// kernel's 80 accumulator registers would be 160 for ONE 16-row item, with nothing left to amortise an operand read over): a
// workgroup of 8 waves is 4 row groups of 32 rows x 2 column halves of 320 channels. A wave keeps 2 items x 20 accumulator tiles
// (160 registers); every weight fragment it reads from LDS serves both items.
//   A operand = W [640][K] re-laid out once per model (rows640_pack_kernel): fragment (k-step f, row tile u) at [f][u], lane (g, c)
//               holding W[frag_sigma(u, c)][32 f + 8 g .. + 7] — a lane's tile pair 2v | 2v + 1 is 8 CONSECUTIVE output channels.
//               Streamed through the 2-slot LDS ring one k-step (40 fragments = 40 KiB) ahead; half h reads fragments 20 h .. + 19.
//   B operand = read straight from row-major A: lane (g, c) = the 16 bytes of row c at channel 32 f + 8 g, requested two k-steps
//               ahead into one of four register sets (no re-layout pass; a row's 128-byte line serves two k-steps).
// LayerNorm: a row's 640 channels live in the two waves of a row group. Each reduces its half over its 4 lane rows, the pair
// exchanges the row sums through LDS, then the sums of squared deviations (the two-pass order of every LayerNorm here, on the
// ROUNDED s). Both waves add the same two numbers, so they normalise with the same mean and rstd.
//
// Roofline. K = 640: 4 x 1280 bytes per row against 2 * 640 * 640 flop: 160 flop/B — HBM. K = 2560: 5120 + 3 x 1280 bytes against
// 3.28 MFLOP: 366 flop/B — between the two limits.

namespace {

constexpr int R6_C = 640;                      // output channels
constexpr int R6_NRT = R6_C / 16;              // 40 output row tiles = the fragments of one k-step
constexpr int R6_HT = R6_NRT / 2;              // 20 tiles per column half
constexpr int R6_NTP = R6_HT / 2;              // 10 tile pairs per column half
constexpr int R6_QF = 5;                       // operand fragments read per group (a quarter of a half)
constexpr int R6_NW = 8;                       // waves: 4 row groups x 2 column halves
constexpr int R6_ROWS = 128;                   // rows per workgroup pass
using R6Ring = WRing<R6_NW, R6_NRT>;           // 5 LDS-DMA instructions per wave per k-step, 40 KiB per slot
static_assert(R6Ring::PER * R6_NW == R6_NRT, "the ring of this kernel has no spare positions");
constexpr int R6_SLOT = R6Ring::SLOT;
constexpr int R6_TAB = 3 * R6_C * 2;           // bias | gamma | beta as 16-bit, behind the ring
constexpr int R6_XCH = 2 * R6_NW * 2 * 16 * 4; // row sums | sums of squared deviations: [wave][item][row] fp32
constexpr int R6_LDS = 2 * R6_SLOT + R6_TAB + R6_XCH;

// W [640][K] -> [k-step f][row tile u] fragments: lane (g, c) holds W[frag_sigma(u, c)][32 f + 8 g .. + 7]
template <typename T>
__global__ __launch_bounds__(64) void rows640_pack_kernel(const T* __restrict__ w, T* __restrict__ packed, int K) {
  const int fr = blockIdx.x;                   // f * 40 + u
  const int f = fr / R6_NRT, u = fr % R6_NRT;
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  const typename Tr<T>::V8 x = *(const typename Tr<T>::V8*)(w + (size_t)frag_sigma(u, c) * K + 32 * f + 8 * g);
  *(typename Tr<T>::V8*)(packed + (size_t)fr * (FRAG / 2) + lane * 8) = x;
}

struct R6 {
  const char* a;        // [R][K] row-major
  const char* w;        // packed weight
  const void* bias;     // [640] or null
  const void* gamma;    // LN only
  const void* beta;
  const void* x;        // [R][640] residual stream
  void* s;              // [R][640] x + A W^T + bias
  void* y;              // [R][640] LayerNorm(s) (LN only)
  long R;
  float eps;
  int y_qfrag;          // 1: y leaves in QUERY-fragment order ([R / 16][20][1 KiB])
};

// THE counted-wait invariant of this kernel. vmcnt counts a wave's own memory instructions in issue order; the waits in front of
// the barriers name "this k-step's DMA" only because every wave issues the same instructions on every path:
//   - per k-step five LDS-DMA copies (8 waves x 5 are the 40 fragments exactly) and, behind them, the two B loads of k-step + 2
//     (of the next pass's first two k-steps behind the last two; rows past R or no next pass: an offset the descriptor drops);
//   - per pass 20 residual loads and NST = 20 | 40 (LN) stores, dropped the same way for rows past R.
// Hence vmcnt(2) in front of a k-step (the two B loads issued behind its DMA may fly) and vmcnt(NST) in front of a pass's first
// (the previous epilogue's stores may fly; its loads, the B loads and the DMA of k-step 0 are all older than those).
template <typename T, int K, bool LN>
__global__ __launch_bounds__(64 * R6_NW, 2) void rows640_kernel(const R6 p) {
  using V8 = typename Tr<T>::V8;
  constexpr int NKS = K / 32;
  static_assert(NKS % 4 == 0, "k-steps are walked four at a time");
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rg = wv >> 1, hf = wv & 1;
  const int g = lane >> 4, c16 = lane & 15;
  char* ring = smem;
  T* tab = (T*)(smem + 2 * R6_SLOT);
  float* xch = (float*)(smem + 2 * R6_SLOT + R6_TAB);
  for (int i = threadIdx.x; i < R6_C; i += 64 * R6_NW) {
    tab[i] = p.bias ? ((const T*)p.bias)[i] : (T)0.0f;
    if constexpr (LN) {
      tab[R6_C + i] = ((const T*)p.gamma)[i];
      tab[2 * R6_C + i] = ((const T*)p.beta)[i];
    }
  }
  const __amdgpu_buffer_rsrc_t w_srd = make_srd(p.w, (unsigned)(NKS * R6_NRT * FRAG));
  const unsigned lane16 = (unsigned)lane * 16u;
  auto stage = [&](int ks, int slot) __attribute__((always_inline)) {      // the fragments of k-step `ks` into ring slot `slot`
#pragma unroll
    for (int i = 0; i < R6Ring::PER; ++i) {
      const int f = wv + R6_NW * i;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_srd, (__attribute__((address_space(3))) void*)(ring + slot * R6_SLOT + f * FRAG), 16, lane16,
                                               (unsigned)((ks * R6_NRT + f) * FRAG), 0, 0);
    }
  };
  // (tensors of 4 GiB and above are refused by the host wrapper: 32-bit buffer offsets)
  const __amdgpu_buffer_rsrc_t a_srd = make_srd(p.a, (unsigned)((size_t)p.R * K * sizeof(T)));
  const unsigned cbytes = (unsigned)((size_t)p.R * R6_C * sizeof(T));
  const __amdgpu_buffer_rsrc_t x_srd = make_srd(p.x, cbytes), s_srd = make_srd(p.s, cbytes), y_srd = make_srd(LN ? p.y : p.s, cbytes);
  const long nblk = (p.R + R6_ROWS - 1) / R6_ROWS;
  // lane (g, c) of item `it` of pass `blk`: byte offset of its 16 bytes of k-step 0 in A; R % 16 == 0: an item exists whole or not at all
  auto a_off = [&](long blk, int it) -> unsigned {
    const long r0 = (blk * 4 + rg) * 32 + 16 * it;
    return (blk < nblk && r0 < p.R) ? (unsigned)((r0 + c16) * (K * (long)sizeof(T))) + (unsigned)g * 16u : SRD_DROP;
  };
  long blk = blockIdx.x;
  V8 b[4][2];                                  // B operands of k-steps ks % 4, both items
  unsigned vo[2] = {a_off(blk, 0), a_off(blk, 1)};
  stage(0, 0);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int it = 0; it < 2; ++it) b[j][it] = srd_load16<V8>(a_srd, vo[it], 64u * j);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                             // tables + k-step 0 visible
  const char* lbase = ring + hf * (R6_HT * FRAG) + lane * 16;
  for (; blk < nblk; blk += gridDim.x) {
    const unsigned vn[2] = {a_off(blk + gridDim.x, 0), a_off(blk + gridDim.x, 1)};
    f32x4 acc[2][R6_HT];
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int t = 0; t < R6_HT; ++t) acc[it][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kg = 0; kg < NKS / 4; ++kg) {
      auto step = [&](auto j_tag) __attribute__((always_inline)) {
        constexpr int J = decltype(j_tag)::value;
        constexpr int SLOT = J & 1;
        const int ks = 4 * kg + J;
        if constexpr (J == 0) {                // the invariant above
          if (kg == 0) { if constexpr (LN) asm volatile("s_waitcnt vmcnt(40)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); }
          else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        __builtin_amdgcn_s_barrier();          // k-step ks landed for every wave; everyone is done with the other slot
        stage(ks + 1 < NKS ? ks + 1 : 0, SLOT ^ 1);      // the next k-step (k-step 0 of the next pass behind the last one)
        if constexpr (J < 2) {
#pragma unroll
          for (int it = 0; it < 2; ++it) b[J + 2][it] = srd_load16<V8>(a_srd, vo[it], 64u * (unsigned)(ks + 2));
        } else {                               // behind the pass's last two k-steps: the next pass's first two
          const bool last = kg == NKS / 4 - 1;
          const unsigned so = last ? 64u * (J - 2) : 64u * (unsigned)(ks + 2);
#pragma unroll
          for (int it = 0; it < 2; ++it) b[J - 2][it] = srd_load16<V8>(a_srd, last ? vn[it] : vo[it], so);
        }
        const V8* fr = (const V8*)(lbase + SLOT * R6_SLOT);
#pragma unroll
        for (int q = 0; q < R6_HT / R6_QF; ++q) {
          V8 wa[R6_QF];
#pragma unroll
          for (int t = 0; t < R6_QF; ++t) wa[t] = fr[(R6_QF * q + t) * 64];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int t = 0; t < R6_QF; ++t) {
            acc[0][R6_QF * q + t] = Tr<T>::mfma(wa[t], b[J][0], acc[0][R6_QF * q + t]);
            acc[1][R6_QF * q + t] = Tr<T>::mfma(wa[t], b[J][1], acc[1][R6_QF * q + t]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      sta_static_for<4>(step);
    }
    vo[0] = vn[0];
    vo[1] = vn[1];
    // ---- epilogue: + bias + residual, the new residual stream, LayerNorm. ALWAYS 20 loads and NST stores ---------------------
    const long rbase = (blk * 4 + rg) * 32;    // wave-uniform
    // the lane's coordinates again, opaque to hipcc: what the epilogue derives from them (table, exchange and row offsets) is then
    // computed here and not kept in registers across the MFMA loop, which has none to spare (the LN instance spills otherwise)
    int le = lane;
    asm volatile("" : "+v"(le));
    const int ge = le >> 4, ce = le & 15;
    constexpr int XG = LN ? 5 : 10;            // residual loads in flight per item (LN: the statistics need the registers)
    V8 xv[XG];
    unsigned ro[2];                            // lane (g, c) of item `it`: byte offset of channels 320 hf + 8 g .. + 7 of row c in [R][640]
    float sum[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const long r0 = rbase + 16 * it;
      ro[it] = r0 < p.R ? (unsigned)((r0 + ce) * (R6_C * (long)sizeof(T))) + (unsigned)(320 * hf + 8 * ge) * (unsigned)sizeof(T) : SRD_DROP;
      float sm = 0.f;
#pragma unroll
      for (int v = 0; v < R6_NTP; ++v) {
        if (v % XG == 0) {                     // the residual of the next XG tile pairs
#pragma unroll
          for (int i = 0; i < XG; ++i) xv[i] = srd_load16<V8>(x_srd, ro[it], 64u * (v + i));
        }
        const V8 bs = *(const V8*)(tab + 320 * hf + 32 * v + 8 * ge);
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = acc[it][2 * v + (e >> 2)][e & 3] + (float)bs[e] + (float)xv[v % XG][e];
          o[e] = (T)t;                         // the residual stream continues in the activation dtype: normalise what is stored
          const float r = (float)o[e];
          acc[it][2 * v + (e >> 2)][e & 3] = r;
          sm += r;
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), s_srd, ro[it], 64u * v, 0);
        __builtin_amdgcn_sched_barrier(0);     // one tile pair at a time: hipcc otherwise hoists every table read to the top
      }
      sum[it] = sm;
    }
    if constexpr (LN) {
      // a row's other 320 channels are in wave wv ^ 1: row sums, then sums of squared deviations, through LDS. Every wave reaches
      // both barriers in every pass, whether its rows exist or not.
      float mean[2], rstd[2];
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        sum[it] = bfly_sum(sum[it]);
        if (ge == 0) xch[(wv * 2 + it) * 16 + ce] = sum[it];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        mean[it] = (sum[it] + xch[((wv ^ 1) * 2 + it) * 16 + ce]) * (1.0f / R6_C);
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < R6_HT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d = acc[it][t][r] - mean[it];
            q += d * d;
          }
        sum[it] = bfly_sum(q);
        if (ge == 0) xch[R6_NW * 2 * 16 + (wv * 2 + it) * 16 + ce] = sum[it];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const unsigned ystep = p.y_qfrag ? (unsigned)FRAG : 64u;
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        rstd[it] = rsqrtf((sum[it] + xch[R6_NW * 2 * 16 + ((wv ^ 1) * 2 + it) * 16 + ce]) * (1.0f / R6_C) + p.eps);
        const long r0 = rbase + 16 * it;
        // query-fragment order: tile pair v of half hf IS fragment 10 hf + v of the item's 16-row group, lane 16 g + c
        const unsigned yo = r0 >= p.R ? SRD_DROP
                          : p.y_qfrag ? (unsigned)(r0 * (R6_C * (long)sizeof(T))) + (unsigned)(R6_NTP * hf) * (unsigned)FRAG + (unsigned)le * 16u : ro[it];
#pragma unroll
        for (int v = 0; v < R6_NTP; ++v) {
          const V8 gm = *(const V8*)(tab + R6_C + 320 * hf + 32 * v + 8 * ge), bt = *(const V8*)(tab + 2 * R6_C + 320 * hf + 32 * v + 8 * ge);
          V8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (T)((acc[it][2 * v + (e >> 2)][e & 3] - mean[it]) * rstd[it] * (float)gm[e] + (float)bt[e]);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), y_srd, yo, ystep * v, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the trailing DMA of "k-step 0 of the next pass" must not outlive the workgroup
}

const char* rows640_refusal(int C, int K) {
  return (C == R6_C && (K == 640 || K == 2560)) ? nullptr : "Linear + residual (+ LayerNorm) at C = 640: 640 output channels, K = 640 or 2560 only (C=%d K=%d)";
}

}  // namespace

extern "C" {

size_t sta_rows_c640_packed_w_bytes(int C, int K) { return rows640_refusal(C, K) ? 0 : (size_t)R6_C * K * 2; }

int sta_rows_c640_pack_w(const void* w, void* packed, int C, int K, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!w || !packed) return sta_fail(STA_E_ARG, "null pointer");
  if (const char* why = rows640_refusal(C, K)) return sta_fail(STA_E_ARG, why, C, K);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_ARG, "dtype %d", dtype);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<rows640_pack_kernel<T>>("pack_rows640 launch", dim3((K / 32) * R6_NRT), dim3(64), 0, st, (const T*)w, (T*)packed, K);
  });
}

int sta_rows_c640(const void* a, const void* packed_w, const void* bias, const void* x, const void* gamma, const void* beta, void* s,
                  void* y, long R, int C, int K, float eps, int y_qfrag, int max_workgroups, int dtype, void* stream) {
  g_sta_err[0] = 0;
  // (every refusal of this entry point is STA_E_ARG: nothing is launched, the reason is in sta_last_error)
  if (const char* why = rows640_refusal(C, K)) return sta_fail(STA_E_ARG, why, C, K);
  const bool ln = K == 640;
  if (!a || !packed_w || !x || !s || (ln && (!gamma || !beta || !y))) return sta_fail(STA_E_ARG, "null pointer");
  if (!ln && (gamma || beta || y)) return sta_fail(STA_E_ARG, "rows_c640: K = 2560 has no LayerNorm (gamma, beta and y must be null)");
  if (R <= 0 || R % 16) return sta_fail(STA_E_ARG, "rows_c640: R=%ld (need a positive multiple of 16 rows)", R);
  if ((size_t)R * K * 2 >= 0xfffffff0ull) return sta_fail(STA_E_ARG, "activations must stay below 4 GiB (R=%ld)", R);
  if (max_workgroups < 0) return sta_fail(STA_E_ARG, "rows_c640: max_workgroups=%d", max_workgroups);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_ARG, "dtype %d", dtype);
  R6 p{(const char*)a, (const char*)packed_w, bias, gamma, beta, x, s, y, R, eps, y_qfrag ? 1 : 0};
  const long nblk = (R + R6_ROWS - 1) / R6_ROWS;
  const long cap = max_workgroups > 0 && max_workgroups < 256 ? max_workgroups : 256;     // one persistent workgroup per CU
  const unsigned grid = (unsigned)(nblk < cap ? nblk : cap);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (ln) return sta_launch_lds<rows640_kernel<T, 640, true>>("rows_c640 (ln) launch", R6_LDS, dim3(grid), dim3(64 * R6_NW), R6_LDS, st, p);
    return sta_launch_lds<rows640_kernel<T, 2560, false>>("rows_c640 launch", R6_LDS, dim3(grid), dim3(64 * R6_NW), R6_LDS, st, p);
  });
}

}  // extern "C"
