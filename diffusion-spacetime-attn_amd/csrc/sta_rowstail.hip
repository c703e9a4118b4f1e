// sta_rowstail.hip — the tail of a SpatialTransformer at SD-v1 level 0 (C = 320) and level 1 (C = 640) as ONE pass:
//
//     x3  = x2 + h W2^T + b2            ff.net[2] + the block's last residual      (attention.py:299; x2 = residual stream, h = GEGLU output)
//     out = x3 Wp^T + bp + x_in         proj_out (1x1 conv) + the transformer's residual   (attention.py:346)
//
// x3 has no other reader, and between the two Linear maps there are only additions, so the pair is one GEMM over a longer K:
//
//     out = [h | x2] [W' | Wp]^T + b' + x_in,      W' = Wp W2  (C x inner),   b' = Wp b2 + bp
//
// W' and b' depend on frozen weights only (sta.fused.ff_tail_weights builds them once per model, products in fp32, W' rounded once).
// Against ff_out_res_hfrag / rows640_kernel<T, 2560, false> followed by gemm_rows_kernel, x3 is neither written nor read back and
// proj_out is no launch of its own. The per-image, per-channel sums the next GroupNorm needs leave in the epilogue, as they do from
// gemm_rows_kernel today.
//
// Structure: the skeleton of csrc/sta_rows_dev.h (RowsShape<C>, the weight [W' | Wp] [C][inner + C] packed by rows_pack_kernel) with
// its counted-wait invariant.
//   C = 640: 100 k-steps (80 of h, 20 of x2).
//   C = 320: 50 k-steps (40 of h, 10 of x2); the weight is streamed once per 256 rows.
//   B operand = x2 and (C = 640) h are row-major: lane (g, c) = the 16 bytes of row c at channel 32 f + 8 g. At C = 320 h arrives in
//               the fragment order sta_ff_geglu_qfrag(h_frag = 1) writes: one coalesced 1-KiB load per (item, k-step). The source
//               switches from h to x2 at k-step inner / 32.
// 50 k-steps are no multiple of the four register sets: at C = 320 the last two k-steps of a pass (sets 0 and 1) request the next
// pass's first two BEHIND their own MFMAs, into the sets they just released, so that every pass starts with set 0; those loads land
// under the epilogue.
//
// Roofline, level 0: 2 * 1600 * 320 flop per row against 2560 + 3 x 640 bytes: 229 flop/B; level 1: 4.1 MFLOP against 5120 + 3 x 1280
// bytes: 457 flop/B — both between the two limits.
//
// Not a translation unit of its own: #included at the end of sta_ffgemm.hip (sta/lib.py::INCLUDED_SOURCES), whose headers, flags
// (-ffinite-math-only) and hazard lint it shares.

namespace {

template <int C_>
struct TailShape : RowsShape<C_> {
  using RowsShape<C_>::C;
  using RowsShape<C_>::SLOT;
  static constexpr int INNER = 4 * C, K = INNER + C;
  static constexpr int NKS_H = INNER / 32;           // k-steps that read h: 40 | 80
  static constexpr int NKS = K / 32;                 // 50 | 100
  static constexpr bool HFRAG = C == 320;            // h in fragment order
  static constexpr unsigned HSTEP = HFRAG ? (unsigned)FRAG : 64u;      // bytes from one k-step of h to the next, per lane
  static constexpr int TAB = C * 4;                  // b' in fp32, behind the ring
  static constexpr int LDS = 2 * SLOT + TAB;
  static_assert(NKS % 2 == 0 && NKS_H % 2 == 0, "the ring slot of k-step 0 is slot 0 in every pass");
};

struct RT {
  const char* h;        // [R][inner] row-major (C = 640) or fragment order [R / 16][inner / 32][1 KiB] (C = 320)
  const char* x2;       // [R][C] residual stream in front of the feed-forward
  const char* w;        // packed [W' | Wp]
  const float* bias;    // b' [C] fp32 or null
  const void* xin;      // [R][C] the transformer's input (row view of NHWC)
  void* out;            // [R][C]
  float* stats;         // null, or [R / rows_img + 1][rows_img / 32][C][2] fp32: per (image, 32-row slot) sums / sums of squares of the stored values
  long R;
  unsigned rows_img;
};

// The counted-wait invariant of sta_rows_dev.h with this kernel's numbers: per pass 20 residual loads, 20 stores and, with
// statistics, 10 more stores (lanes that hold no piece: a dropped offset): NST = 20 | 30.
template <typename T, int C>
__global__ __launch_bounds__(64 * TailShape<C>::NW, 2) void rows_tail_kernel(const RT p) {
  using S = TailShape<C>;
  using V8 = typename Tr<T>::V8;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rg = wv / S::NH, hf = wv % S::NH;
  char* ring = smem;
  float* tab = (float*)(smem + 2 * S::SLOT);
  for (int i = threadIdx.x; i < C; i += 64 * S::NW) tab[i] = p.bias ? p.bias[i] : 0.f;
  const __amdgpu_buffer_rsrc_t w_srd = make_srd(p.w, (unsigned)(S::NKS * S::NRT * FRAG));
  const unsigned lane16 = (unsigned)lane * 16u;
  auto stage = [&](int ks, int slot) __attribute__((always_inline)) {      // the fragments of k-step `ks` into ring slot `slot`
    S::Ring::template stage<true>(w_srd, ring + slot * S::SLOT, 0u, ks * S::NRT, wv, lane16);
  };
  // (tensors of 4 GiB and above are refused by the host wrapper: 32-bit buffer offsets)
  const unsigned cbytes = (unsigned)((size_t)p.R * C * sizeof(T));
  const __amdgpu_buffer_rsrc_t h_srd = make_srd(p.h, (unsigned)((size_t)p.R * S::INNER * sizeof(T)));
  const __amdgpu_buffer_rsrc_t x2_srd = make_srd(p.x2, cbytes), xin_srd = make_srd(p.xin, cbytes), out_srd = make_srd(p.out, cbytes);
  // (rows are counted in 32 bits: R * inner * 2 < 4 GiB, and a 64-bit compare would take a register pair in every lane)
  const int R = (int)p.R, nblk = (R + S::ROWS - 1) / S::ROWS;
  // lane `ln` = (g, c) of item `it` of pass `blk`: byte offset of its 16 bytes of k-step 0 in h / in x2; R % 16 == 0: an item exists
  // whole or not at all. (The callers inside the pass loop hand in a copy of the lane id that is opaque to hipcc: the lane's
  // coordinates are then derived where they are used and hold no register across the MFMA loop, which has none to spare.)
  auto h_off = [&](int blk, int it, int ln) -> unsigned {
    const int r0 = (blk * S::NG + rg) * 32 + 16 * it;
    const bool ok = (blk < nblk) & (r0 < R);               // (no short circuit: a select, not a branch around the load)
    if constexpr (S::HFRAG) return ok ? (unsigned)r0 * (unsigned)(S::INNER * sizeof(T)) + (unsigned)ln * 16u : SRD_DROP;
    else return ok ? (unsigned)(r0 + (ln & 15)) * (unsigned)(S::INNER * sizeof(T)) + (unsigned)(ln >> 4) * 16u : SRD_DROP;
  };
  auto x_off = [&](int blk, int it, int ln) -> unsigned {
    const int r0 = (blk * S::NG + rg) * 32 + 16 * it;
    return ((blk < nblk) & (r0 < R)) ? (unsigned)(r0 + (ln & 15)) * (unsigned)(C * sizeof(T)) + (unsigned)(ln >> 4) * 16u : SRD_DROP;
  };
  V8 b[4][2];                                  // B operands of four consecutive k-steps, both items
  stage(0, 0);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int it = 0; it < 2; ++it) b[j][it] = srd_load16<V8>(h_srd, h_off(blockIdx.x, it, lane), S::HSTEP * j);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                             // table + k-step 0 visible
  const char* lbase = ring + hf * (S::HT * FRAG) + lane * 16;

  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int lp = rows_opaque_lane(lane);
    const unsigned vh[2] = {h_off(blk, 0, lp), h_off(blk, 1, lp)}, vx[2] = {x_off(blk, 0, lp), x_off(blk, 1, lp)};
    unsigned vn[2] = {0u, 0u};                  // the next pass's (C = 320: derived where they are used, no register across the loop)
    if constexpr (S::NKS % 4 == 0) { vn[0] = h_off(blk + gridDim.x, 0, lp); vn[1] = h_off(blk + gridDim.x, 1, lp); }
    f32x4 acc[2][S::HT];
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int t = 0; t < S::HT; ++t) acc[it][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto step = [&](auto j_tag, auto tail_tag, const int ks) __attribute__((always_inline)) {
      constexpr int J = decltype(j_tag)::value;            // the register set of this k-step: ks % 4
      constexpr bool TAIL = decltype(tail_tag)::value;     // one of the two k-steps behind the last whole group of four (C = 320)
      constexpr int SLOT = J & 1;
      if constexpr (J == 0) {                              // the invariant above
        if (ks == 0) { if (p.stats) asm volatile("s_waitcnt vmcnt(30)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); }
        else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      __builtin_amdgcn_s_barrier();            // k-step ks landed for every wave; everyone is done with the other slot
      stage(ks + 1 < S::NKS ? ks + 1 : 0, SLOT ^ 1);       // the next k-step (k-step 0 of the next pass behind the last one)
      if constexpr (!TAIL) {
        // the B operands of k-step ks + 2: of h, of x2 from k-step NKS_H on, of the next pass's h behind the last two
        const int kn = ks + 2;
        const bool nxt = S::NKS % 4 == 0 && kn >= S::NKS, xs = !nxt && kn >= S::NKS_H;
        const unsigned so = nxt ? S::HSTEP * (unsigned)(kn - S::NKS) : xs ? 64u * (unsigned)(kn - S::NKS_H) : S::HSTEP * (unsigned)kn;
        const __amdgpu_buffer_rsrc_t srd = xs ? x2_srd : h_srd;
#pragma unroll
        for (int it = 0; it < 2; ++it) b[(J + 2) & 3][it] = srd_load16<V8>(srd, nxt ? vn[it] : xs ? vx[it] : vh[it], so);
      }
      rows_mfma_step<T, S::HT, S::QF>((const V8*)(lbase + SLOT * S::SLOT), b[J][0], b[J][1], acc);
      if constexpr (TAIL) {                    // k-step J of the next pass into the set this k-step is done with: still two loads behind the DMA
        const int lt = rows_opaque_lane(lane);
#pragma unroll
        for (int it = 0; it < 2; ++it) b[J][it] = srd_load16<V8>(h_srd, h_off(blk + gridDim.x, it, lt), S::HSTEP * (unsigned)J);
      }
    };
    constexpr std::false_type whole{};
    constexpr std::true_type tail{};
    constexpr std::integral_constant<int, 0> _0{};
    constexpr std::integral_constant<int, 1> _1{};
    constexpr std::integral_constant<int, 2> _2{};
    constexpr std::integral_constant<int, 3> _3{};
    int ks = 0;
    for (; ks + 4 <= S::NKS; ks += 4) {
      step(_0, whole, ks);
      step(_1, whole, ks + 1);
      step(_2, whole, ks + 2);
      step(_3, whole, ks + 3);
    }
    if constexpr (S::NKS % 4 == 2) {
      step(_0, tail, ks);
      step(_1, tail, ks + 1);
    }
    // ---- epilogue: + b' + x_in, 16-byte stores. ALWAYS 20 loads and 20 stores ---------------------------------------------------
    const int rbase = (blk * S::NG + rg) * 32;             // wave-uniform
    const int le = rows_opaque_lane(lane), ge = le >> 4, ce = le & 15;       // (the epilogue's offsets are derived here, not across the MFMA loop)
    constexpr int XG = 10;                     // residual loads in flight per item
    V8 xv[XG];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int r0 = rbase + 16 * it;
      // lane (g, c) of item `it`: byte offset of channels 320 hf + 8 g .. + 7 of row c in [R][C]
      const unsigned ro = r0 < R ? (unsigned)(r0 + ce) * (unsigned)(C * sizeof(T)) + (unsigned)(320 * hf + 8 * ge) * (unsigned)sizeof(T) : SRD_DROP;
#pragma unroll
      for (int v = 0; v < S::NTP; ++v) {
        if (v % XG == 0) {                     // the residual of the next XG tile pairs
#pragma unroll
          for (int i = 0; i < XG; ++i) xv[i] = srd_load16<V8>(xin_srd, ro, 64u * (v + i));
        }
        const f32x4 b0 = *(const f32x4*)(tab + 320 * hf + 32 * v + 8 * ge), b1 = *(const f32x4*)(tab + 320 * hf + 32 * v + 8 * ge + 4);
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = acc[it][2 * v + (e >> 2)][e & 3] + (e < 4 ? b0[e & 3] : b1[e & 3]) + (float)xv[v % XG][e];
          o[e] = (T)t;
          acc[it][2 * v + (e >> 2)][e & 3] = (float)o[e];          // the statistics are those of the stored values
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), out_srd, ro, 64u * v, 0);
        __builtin_amdgcn_sched_barrier(0);     // one tile pair at a time: hipcc otherwise hoists every table read to the top
      }
    }
    if (p.stats) {
      // Per-image, per-channel sums of this wave's 32 rows into ITS slot of the image (fixed order, no atomics): the two items in
      // registers, the 16 rows of an item across the DPP row. rows_img % ROWS == 0: a pass lies inside one image. Lane (g, c) holds
      // 8 channels = 16 floats (sum, sum of squares interleaved); lanes c = 0 .. 3 store one 16-byte piece each. ALWAYS 10 stores.
      const bool live = rbase < R, two = rbase + 16 < R;       // (a wave past R writes the spare image; it adds nothing anywhere)
      const unsigned slots = p.rows_img / 32u, r0w = (unsigned)rbase;
      const unsigned n_img = (unsigned)R / p.rows_img, img = live ? r0w / p.rows_img : n_img;
      const unsigned slot = live ? (r0w - img * p.rows_img) / 32u : (unsigned)rg;
      const __amdgpu_buffer_rsrc_t st_srd = make_srd(p.stats, (n_img + 1u) * slots * (unsigned)(C * 8));
      const unsigned so = ce < 4 ? ((img * slots + slot) * (unsigned)C + (unsigned)(320 * hf + 8 * ge)) * 8u + 16u * (unsigned)ce : SRD_DROP;
#pragma unroll
      for (int v = 0; v < S::NTP; ++v) {
        float s[8], q[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float a0 = acc[0][2 * v + (e >> 2)][e & 3], a1 = two ? acc[1][2 * v + (e >> 2)][e & 3] : 0.f;
          s[e] = row16_sum(a0 + a1);
          q[e] = row16_sum(a0 * a0 + a1 * a1);
        }
        f32x4 o = {s[0], q[0], s[1], q[1]};
#pragma unroll
        for (int j = 1; j < 4; ++j)
          if (ce == j) o = f32x4{s[2 * j], q[2 * j], s[2 * j + 1], q[2 * j + 1]};
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), st_srd, so, 256u * v, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the trailing DMA of "k-step 0 of the next pass" must not outlive the workgroup
}

template <int C>
bool tail_is(int c, int inner) { return c == C && inner == TailShape<C>::INNER; }

const char* const TAIL_SHAPES = "feed-forward output + proj_out: C = 320 with inner = 1280 or C = 640 with inner = 2560 only (C=%d inner=%d)";

}  // namespace

extern "C" {

size_t sta_ff_tail_packed_w_bytes(int C, int inner) {
  return (tail_is<320>(C, inner) || tail_is<640>(C, inner)) ? (size_t)C * (inner + C) * 2 : 0;
}

int sta_ff_tail_pack_w(const void* wcat, void* packed, int C, int inner, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!wcat || !packed) return sta_fail(STA_E_ARG, "null pointer");
  if (sta_ff_tail_packed_w_bytes(C, inner) == 0) return sta_fail(STA_E_UNSUP, TAIL_SHAPES, C, inner);
  return rows_pack_w("pack_rows_tail launch", wcat, packed, C, inner + C, dtype, STA_E_UNSUP, stream);
}

int sta_ff_tail(const void* h, const void* x2, const void* packed_w, const float* bias, const void* x_in, void* out, float* stats,
                long rows_per_image, long R, int C, int inner, int max_workgroups, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (sta_ff_tail_packed_w_bytes(C, inner) == 0) return sta_fail(STA_E_UNSUP, TAIL_SHAPES, C, inner);
  if (!h || !x2 || !packed_w || !x_in || !out) return sta_fail(STA_E_ARG, "null pointer");
  if (const int rc = rows_refuse("ff_tail", R, (size_t)inner * 2, max_workgroups, dtype, STA_E_UNSUP)) return rc;
  const long rows = C == 320 ? TailShape<320>::ROWS : TailShape<640>::ROWS;
  if (stats && (rows_per_image <= 0 || rows_per_image % rows || R % rows_per_image))
    return sta_fail(STA_E_ARG, "ff_tail: rows_per_image=%ld (statistics need a multiple of the pass height %ld that divides R=%ld)", rows_per_image, rows, R);
  RT p{(const char*)h, (const char*)x2, (const char*)packed_w, bias, x_in, out, stats, R, stats ? (unsigned)rows_per_image : 0u};
  const unsigned grid = rows_grid(R, rows, max_workgroups);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (C == 320) return sta_launch_lds<rows_tail_kernel<T, 320>>("ff_tail (c320) launch", TailShape<320>::LDS, dim3(grid), dim3(512), TailShape<320>::LDS, st, p);
    return sta_launch_lds<rows_tail_kernel<T, 640>>("ff_tail (c640) launch", TailShape<640>::LDS, dim3(grid), dim3(512), TailShape<640>::LDS, st, p);
  });
}

}  // extern "C"
