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
// kernel's 80 accumulator registers would be 160 for ONE 16-row item, with nothing left to amortise an operand read over): the
// skeleton is that of csrc/sta_rows_dev.h at C = 640 (RowsShape<640>: 4 row groups x 2 column halves, W packed by rows_pack_kernel),
// with its counted-wait invariant.
//   B operand = read straight from row-major A: lane (g, c) = the 16 bytes of row c at channel 32 f + 8 g (no re-layout pass; a
//               row's 128-byte line serves two k-steps).
// LayerNorm: a row's 640 channels live in the two waves of a row group. Each reduces its half over its 4 lane rows, the pair
// exchanges the row sums through LDS, then the sums of squared deviations (the two-pass order of every LayerNorm here, on the
// ROUNDED s). Both waves add the same two numbers, so they normalise with the same mean and rstd.
//
// Roofline. K = 640: 4 x 1280 bytes per row against 2 * 640 * 640 flop: 160 flop/B — HBM. K = 2560: 5120 + 3 x 1280 bytes against
// 3.28 MFLOP: 366 flop/B — between the two limits.

namespace {

struct S6 : RowsShape<640> {
  static_assert(Ring::PER * NW == NRT, "the ring of this kernel has no spare positions");
  static constexpr int TAB = 3 * C * 2;               // bias | gamma | beta as 16-bit, behind the ring
  static constexpr int XCH = 2 * NW * 2 * 16 * 4;     // row sums | sums of squared deviations: [wave][item][row] fp32
  static constexpr int LDS = 2 * SLOT + TAB + XCH;
};

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

// The counted-wait invariant of sta_rows_dev.h with this kernel's numbers: five LDS-DMA copies per k-step (8 waves x 5 are the 40
// fragments exactly); per pass 20 residual loads and NST = 20 | 40 (LN) stores.
template <typename T, int K, bool LN>
__global__ __launch_bounds__(64 * S6::NW, 2) void rows640_kernel(const R6 p) {
  using V8 = typename Tr<T>::V8;
  constexpr int NKS = K / 32;
  static_assert(NKS % 4 == 0, "k-steps are walked four at a time");
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rg = wv >> 1, hf = wv & 1;
  const int g = lane >> 4, c16 = lane & 15;
  char* ring = smem;
  T* tab = (T*)(smem + 2 * S6::SLOT);
  float* xch = (float*)(smem + 2 * S6::SLOT + S6::TAB);
  for (int i = threadIdx.x; i < S6::C; i += 64 * S6::NW) {
    tab[i] = p.bias ? ((const T*)p.bias)[i] : (T)0.0f;
    if constexpr (LN) {
      tab[S6::C + i] = ((const T*)p.gamma)[i];
      tab[2 * S6::C + i] = ((const T*)p.beta)[i];
    }
  }
  const __amdgpu_buffer_rsrc_t w_srd = make_srd(p.w, (unsigned)(NKS * S6::NRT * FRAG));
  const unsigned lane16 = (unsigned)lane * 16u;
  auto stage = [&](int ks, int slot) __attribute__((always_inline)) {      // the fragments of k-step `ks` into ring slot `slot`
    S6::Ring::stage<true>(w_srd, ring + slot * S6::SLOT, 0u, ks * S6::NRT, wv, lane16);
  };
  // (tensors of 4 GiB and above are refused by the host wrapper: 32-bit buffer offsets)
  const __amdgpu_buffer_rsrc_t a_srd = make_srd(p.a, (unsigned)((size_t)p.R * K * sizeof(T)));
  const unsigned cbytes = (unsigned)((size_t)p.R * S6::C * sizeof(T));
  const __amdgpu_buffer_rsrc_t x_srd = make_srd(p.x, cbytes), s_srd = make_srd(p.s, cbytes), y_srd = make_srd(LN ? p.y : p.s, cbytes);
  const long nblk = (p.R + S6::ROWS - 1) / S6::ROWS;
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
  const char* lbase = ring + hf * (S6::HT * FRAG) + lane * 16;
  for (; blk < nblk; blk += gridDim.x) {
    const unsigned vn[2] = {a_off(blk + gridDim.x, 0), a_off(blk + gridDim.x, 1)};
    f32x4 acc[2][S6::HT];
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int t = 0; t < S6::HT; ++t) acc[it][t] = f32x4{0.f, 0.f, 0.f, 0.f};
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
        rows_mfma_step<T, S6::HT, S6::QF>((const V8*)(lbase + SLOT * S6::SLOT), b[J][0], b[J][1], acc);
      };
      sta_static_for<4>(step);
    }
    vo[0] = vn[0];
    vo[1] = vn[1];
    // ---- epilogue: + bias + residual, the new residual stream, LayerNorm. ALWAYS 20 loads and NST stores ---------------------
    const long rbase = (blk * 4 + rg) * 32;    // wave-uniform
    const int le = rows_opaque_lane(lane), ge = le >> 4, ce = le & 15;       // (the epilogue's offsets are derived here, not across the MFMA loop)
    constexpr int XG = LN ? 5 : 10;            // residual loads in flight per item (LN: the statistics need the registers)
    V8 xv[XG];
    unsigned ro[2];                            // lane (g, c) of item `it`: byte offset of channels 320 hf + 8 g .. + 7 of row c in [R][640]
    float sum[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const long r0 = rbase + 16 * it;
      ro[it] = r0 < p.R ? (unsigned)((r0 + ce) * (S6::C * (long)sizeof(T))) + (unsigned)(320 * hf + 8 * ge) * (unsigned)sizeof(T) : SRD_DROP;
      float sm = 0.f;
#pragma unroll
      for (int v = 0; v < S6::NTP; ++v) {
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
        mean[it] = (sum[it] + xch[((wv ^ 1) * 2 + it) * 16 + ce]) * (1.0f / S6::C);
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < S6::HT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d = acc[it][t][r] - mean[it];
            q += d * d;
          }
        sum[it] = bfly_sum(q);
        if (ge == 0) xch[S6::NW * 2 * 16 + (wv * 2 + it) * 16 + ce] = sum[it];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const unsigned ystep = p.y_qfrag ? (unsigned)FRAG : 64u;
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        rstd[it] = rsqrtf((sum[it] + xch[S6::NW * 2 * 16 + ((wv ^ 1) * 2 + it) * 16 + ce]) * (1.0f / S6::C) + p.eps);
        const long r0 = rbase + 16 * it;
        // query-fragment order: tile pair v of half hf IS fragment 10 hf + v of the item's 16-row group, lane 16 g + c
        const unsigned yo = r0 >= p.R ? SRD_DROP
                          : p.y_qfrag ? (unsigned)(r0 * (S6::C * (long)sizeof(T))) + (unsigned)(S6::NTP * hf) * (unsigned)FRAG + (unsigned)le * 16u : ro[it];
#pragma unroll
        for (int v = 0; v < S6::NTP; ++v) {
          const V8 gm = *(const V8*)(tab + S6::C + 320 * hf + 32 * v + 8 * ge), bt = *(const V8*)(tab + 2 * S6::C + 320 * hf + 32 * v + 8 * ge);
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
  return (C == S6::C && (K == 640 || K == 2560)) ? nullptr : "Linear + residual (+ LayerNorm) at C = 640: 640 output channels, K = 640 or 2560 only (C=%d K=%d)";
}

}  // namespace

extern "C" {

size_t sta_rows_c640_packed_w_bytes(int C, int K) { return rows640_refusal(C, K) ? 0 : (size_t)S6::C * K * 2; }

int sta_rows_c640_pack_w(const void* w, void* packed, int C, int K, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!w || !packed) return sta_fail(STA_E_ARG, "null pointer");
  if (const char* why = rows640_refusal(C, K)) return sta_fail(STA_E_ARG, why, C, K);
  return rows_pack_w("pack_rows640 launch", w, packed, C, K, dtype, STA_E_ARG, stream);
}

int sta_rows_c640(const void* a, const void* packed_w, const void* bias, const void* x, const void* gamma, const void* beta, void* s,
                  void* y, long R, int C, int K, float eps, int y_qfrag, int max_workgroups, int dtype, void* stream) {
  g_sta_err[0] = 0;
  // (every refusal of this entry point is STA_E_ARG: nothing is launched, the reason is in sta_last_error)
  if (const char* why = rows640_refusal(C, K)) return sta_fail(STA_E_ARG, why, C, K);
  const bool ln = K == 640;
  if (!a || !packed_w || !x || !s || (ln && (!gamma || !beta || !y))) return sta_fail(STA_E_ARG, "null pointer");
  if (!ln && (gamma || beta || y)) return sta_fail(STA_E_ARG, "rows_c640: K = 2560 has no LayerNorm (gamma, beta and y must be null)");
  if (const int rc = rows_refuse("rows_c640", R, (size_t)K * 2, max_workgroups, dtype, STA_E_ARG)) return rc;
  R6 p{(const char*)a, (const char*)packed_w, bias, gamma, beta, x, s, y, R, eps, y_qfrag ? 1 : 0};
  const unsigned grid = rows_grid(R, S6::ROWS, max_workgroups);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (ln) return sta_launch_lds<rows640_kernel<T, 640, true>>("rows_c640 (ln) launch", S6::LDS, dim3(grid), dim3(64 * S6::NW), S6::LDS, st, p);
    return sta_launch_lds<rows640_kernel<T, 2560, false>>("rows_c640 launch", S6::LDS, dim3(grid), dim3(64 * S6::NW), S6::LDS, st, p);
  });
}

}  // extern "C"
