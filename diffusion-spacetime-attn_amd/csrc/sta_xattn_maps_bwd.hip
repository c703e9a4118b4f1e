// sta_xattn_maps_bwd.hip — backward of the token-map readout (sta_xattn_token_maps, sta_xattn.hip) w.r.t. q for MI355X
// (gfx950 / CDNA4); C-ABI in include/sta_xattn.h (sta_xattn_token_maps_bwd). MFMA operand conventions: sta_xattn.hip.
// Not a translation unit of its own: sta_xattn_bwd.hip includes this file at its end (sta/lib.py::INCLUDED_SOURCES).
//
// The readout is out[r][p] = (1/heads) sum_h o_{r,h}[p], o_{r,h}[p] = sum_m w_r[m] P_h[p][m], P_h = softmax_m(scale q_h[p] . K_{c_r,h}[m]).
// With G = dmaps (the gradient w.r.t. the non-accumulated map), per head and per context c a q row attends:
//   dS_h[p][m] = (1/heads) P_h[p][m] sum_{r : c_r = c} G[r][p] (w_r[m] - o_{r,h}[p])
//   dq_h[p]    = scale sum_c sum_m dS_h[p][m] K_{c,h}[m]
// No dK and no dw: the prompts and the key weights are constants of the optimisation, as in sta_xattn_bwd.
//
// One wave owns a (16-pixel tile, q row, head, image) and walks the contexts that row attends, in ascending order: S^T = K Q^T
// from the KQ fragments exactly as the forward readout, softmax once per context, then the readouts of that context in register
// groups of MAPS_BWD_RB (their key weights are 20 registers per lane and readout): o_{r,h} needs the butterfly over the four lane
// rows right away — the forward defers it to the end, here it is a factor of dS — and the bracket sum_r G (w_r - o_r) is added up
// per key. The dS^T accumulators of two key tiles are then already the B operand of dq^T += KP dS^T (the packed image's backward
// part [VQ | KP], pv_key slot order: the hand-over of sta_xattn_bwd.hip). Heads are independent here, so they are a grid dimension:
// 16 tiles x 2 rows x 8 heads per image at N = 256 instead of 32 waves, with no sum across waves. No LDS, no atomics, no workspace;
// every dq element has one writer and one summation order (contexts ascending, readouts in the order the host lists them), so the
// result is bit-reproducible and independent of n_img. A row no readout names is written as zeros by its own waves.
//
// 16-bit range: dS is rounded to the activation type before the MFMA, and G of a layout energy is tiny (or huge under a loss
// scale), so the per-pixel factor max_r |G[r][p]| is taken out of the bracket — the MFMA column of a pixel is linear in it — and
// multiplied back, with scale / heads, onto the fp32 dq^T accumulators: what is rounded is P times a bracket of order one.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sta_xattn.h"
#include "sta_internal.h"
#include "sta_xattn_dev.h"

namespace {

constexpr int MAPS_BWD_RB = 2;             // readouts whose key weights are in registers at a time
struct MapBwdWork {
  int n;                                   // contexts some readout names, ascending
  int ctx[STA_MAX_READOUTS];               // context of item i
  int first[STA_MAX_READOUTS];             // its readouts are rd[first .. first + cnt)
  int cnt[STA_MAX_READOUTS];
  unsigned char rd[STA_MAX_READOUTS];      // readout indices, grouped by context
};
struct MapBwdParams {
  const void* q;         // [n_img][2][N][C]
  const char* packed;    // fragment image, image-major
  const float* w;        // [n_img][R][M]
  const float* dmaps;    // [n_img][R][N]
  void* dq;              // [n_img][2][N][C]
  int N, C, H, d, M, K, R;
  float sl2e, fac;       // scale * log2(e); scale / heads
  MapBwdWork wk;
};

template <typename T, int NDT>
__global__ __launch_bounds__(64) void xattn_token_maps_bwd_kernel(const MapBwdParams p) {
  using V8 = typename Tr<T>::V8;
  constexpr int NKS = nks_of(NDT);
  constexpr int NKF = NKT * NKS, NFWD = fwd_frags(NDT);
  const int lane = threadIdx.x, g = lane >> 4, c16 = lane & 15;
  const int img = blockIdx.y;
  const int h = blockIdx.x % p.H, rest = blockIdx.x / p.H;
  const int row = rest & 1, tile = rest >> 1;
  const int N = p.N, d = p.d, M = p.M, R = p.R;
  const int px = tile * 16 + c16;
  const bool valid = px < N;

  const unsigned row_bytes = (unsigned)p.C * (unsigned)sizeof(T);
  const size_t plane = (size_t)N * row_bytes;
  const __amdgpu_buffer_rsrc_t q_srd = make_srd((const char*)p.q + ((size_t)2 * img + row) * plane, (unsigned)plane);
  const unsigned ctx_bytes = (unsigned)p.H * all_frags(NDT) * FRAG;
  const char* img_packed = p.packed + (size_t)img * (p.K + 2) * ctx_bytes;
  const unsigned koff = (unsigned)h * all_frags(NDT) * FRAG;

  // the B operand of S^T is the same for every context of the row: 16 B per lane at head-dim offset 32 s + 8 g of the pixel's head
  // row; pixels >= N and offsets >= d are pushed out of the descriptor's range -> read as 0
  const unsigned qbase = valid ? (unsigned)px * row_bytes + (unsigned)(h * d + 8 * g) * (unsigned)sizeof(T) : SRD_DROP;
  V8 qf[NKS];
#pragma unroll
  for (int s = 0; s < NKS; ++s) qf[s] = srd_load16<V8>(q_srd, (32 * s + 8 * g < d) ? qbase : SRD_DROP, 64u * s);

  // the pixel's gradient column (clamped address, predicate on the value) and its largest magnitude over this row's readouts
  const float* dm = p.dmaps + (size_t)img * R * N + (valid ? px : 0);
  float gmax = 0.f;
  for (int i = 0; i < p.wk.n; ++i) {
    if ((p.wk.ctx[i] == 0) != (row == 0)) continue;
    for (int k = 0; k < p.wk.cnt[i]; ++k) gmax = fmaxf(gmax, fabsf(dm[(size_t)p.wk.rd[p.wk.first[i] + k] * N]));
  }
  gmax = valid ? gmax : 0.f;
  const float ginv = gmax > 0.f ? 1.0f / gmax : 0.f;

  f32x4 dq[NDT];
#pragma unroll
  for (int u = 0; u < NDT; ++u) dq[u] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int i = 0; i < p.wk.n; ++i) {
    const int cc = p.wk.ctx[i];
    if ((cc == 0) != (row == 0)) continue;          // context 0 is attended by the uncond row, every other one by the cond row
    const int first = p.wk.first[i], cnt = p.wk.cnt[i];
    const __amdgpu_buffer_rsrc_t kv_srd = make_srd(img_packed + (size_t)cc * ctx_bytes, ctx_bytes);
    f32x4 st[NKT];
    {
      V8 ka[NKF];
#pragma unroll
      for (int f = 0; f < NKF; ++f) ka[f] = srd_load16<V8>(kv_srd, lane * 16, koff + f * FRAG);
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NKS; ++s) st[t] = Tr<T>::mfma(ka[t * NKS + s], qf[s], st[t]);
      }
    }
    const float inv = softmax_keys_fast(st, g, M, p.sl2e);       // st = exp2(..) (0 for key >= M), P = st * inv

    // bracket[m] = sum_r (G[r][p] / gmax) (w_r[m] - o_r), the readouts of this context MAPS_BWD_RB at a time
    f32x4 br[NKT];
#pragma unroll
    for (int t = 0; t < NKT; ++t) br[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < cnt; k0 += MAPS_BWD_RB) {
      float wr[MAPS_BWD_RB][NKT][4], gj[MAPS_BWD_RB];
#pragma unroll
      for (int j = 0; j < MAPS_BWD_RB; ++j) {
        const bool live = k0 + j < cnt;
        const int r = p.wk.rd[first + (live ? k0 + j : k0)];
        const float* wrow = p.w + ((size_t)img * R + r) * M;
        const float gr = dm[(size_t)r * N];
        gj[j] = live ? gr * ginv : 0.f;
#pragma unroll
        for (int t = 0; t < NKT; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int key = 16 * t + 4 * g + e;
            const float x = wrow[min(key, M - 1)];
            wr[j][t][e] = (live && key < M) ? x : 0.f;
          }
      }
#pragma unroll
      for (int j = 0; j < MAPS_BWD_RB; ++j) {
        float s4[NKT];
#pragma unroll
        for (int t = 0; t < NKT; ++t)
          s4[t] = (wr[j][t][0] * st[t][0] + wr[j][t][1] * st[t][1]) + (wr[j][t][2] * st[t][2] + wr[j][t][3] * st[t][3]);
        const float o = bfly_sum(((s4[0] + s4[1]) + (s4[2] + s4[3])) + s4[4]) * inv;
#pragma unroll
        for (int t = 0; t < NKT; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) br[t][e] = __builtin_fmaf(gj[j], wr[j][t][e] - o, br[t][e]);
      }
    }
    V8 pb[NPS];
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) st[t][e] = st[t][e] * inv * br[t][e];            // padded keys: st == 0
    tiles_to_b<T>(st, pb);
#pragma unroll
    for (int u = 0; u < NDT; ++u) {
      V8 kp[NPS];
#pragma unroll
      for (int s = 0; s < NPS; ++s) kp[s] = srd_load16<V8>(kv_srd, lane * 16, koff + (unsigned)(NFWD + NKF + s * NDT + u) * FRAG);
#pragma unroll
      for (int s = 0; s < NPS; ++s) dq[u] = Tr<T>::mfma(kp[s], pb[s], dq[u]);
    }
  }

  const float back = gmax * p.fac;
#pragma unroll
  for (int u = 0; u < NDT; ++u) dq[u] = dq[u] * back;
  T* obase = (T*)((char*)p.dq + ((size_t)2 * img + row) * plane) + (size_t)(valid ? px : 0) * p.C + h * d;
  if (valid) store_row16<T, NDT>(obase, dq, g, d);
}

}  // namespace

extern "C" {

int sta_xattn_token_maps_bwd(const void* q, const void* packed, const int32_t* sel_ctx, const float* w, const float* dmaps, void* dq,
                             int n_img, int N, int C, int heads, int M, int K, int R, float scale, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!q || !packed || !sel_ctx || !w || !dmaps || !dq) return sta_fail(STA_E_ARG, "null pointer");
  if ((((uintptr_t)q | (uintptr_t)packed | (uintptr_t)dq) & 15) || (((uintptr_t)w | (uintptr_t)dmaps) & 3))
    return sta_fail(STA_E_ARG, "misaligned pointer (q, packed, dq: 16 bytes; w, dmaps: 4 bytes)");
  if (n_img < 1 || n_img > 65535) return sta_fail(STA_E_ARG, "n_img=%d", n_img);
  if (int rc = check_shape(N, C, heads, M, K)) return rc;
  if (R < 1 || R > STA_MAX_READOUTS) return sta_fail(STA_E_ARG, "R=%d readouts (1..%d)", R, STA_MAX_READOUTS);
  for (int r = 0; r < R; ++r)
    if (sel_ctx[r] < 0 || sel_ctx[r] >= K + 2) return sta_fail(STA_E_ARG, "sel_ctx[%d]=%d names no context (K+2=%d)", r, (int)sel_ctx[r], K + 2);
  const int d = C / heads, ndt = (d + 15) / 16;
  // what one buffer descriptor of the kernel spans: a [N][C] plane of q, the fragments of one context
  if ((size_t)N * C * 2 >= (1ull << 32) || (size_t)heads * all_frags(ndt) * FRAG >= (1ull << 32))
    return sta_fail(STA_E_UNSUP, "N=%d C=%d heads=%d beyond a 4 GiB buffer range", N, C, heads);
  MapBwdParams p{};
  p.q = q; p.packed = (const char*)packed; p.w = w; p.dmaps = dmaps; p.dq = dq;
  p.N = N; p.C = C; p.H = heads; p.d = d; p.M = M; p.K = K; p.R = R;
  p.sl2e = scale * 1.4426950408889634f; p.fac = scale / (float)heads;
  // one item per context somebody reads, contexts ascending, a context's readouts in the caller's order
  int filled = 0;
  for (int c = 0; c < K + 2; ++c) {
    int cur = -1;
    for (int r = 0; r < R; ++r) {
      if (sel_ctx[r] != c) continue;
      if (cur < 0) { cur = p.wk.n++; p.wk.ctx[cur] = c; p.wk.first[cur] = filled; }
      p.wk.rd[filled++] = (unsigned char)r;
      p.wk.cnt[cur]++;
    }
  }
  const long tiles = ((long)N + 15) / 16;
  if (tiles * 2 * heads > 0x7fffffffL) return sta_fail(STA_E_UNSUP, "N=%d: too many pixel tiles for one launch", N);
  const dim3 grid((unsigned)(tiles * 2 * heads), n_img);
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const char* const what = "token maps backward launch";
    const hipStream_t st = (hipStream_t)stream;
    switch (ndt) {
      case 1: return sta_launch<xattn_token_maps_bwd_kernel<T, 1>>(what, grid, dim3(64), 0, st, p);
      case 2: return sta_launch<xattn_token_maps_bwd_kernel<T, 2>>(what, grid, dim3(64), 0, st, p);
      case 3: return sta_launch<xattn_token_maps_bwd_kernel<T, 3>>(what, grid, dim3(64), 0, st, p);
      case 4: return sta_launch<xattn_token_maps_bwd_kernel<T, 4>>(what, grid, dim3(64), 0, st, p);
      case 5: return sta_launch<xattn_token_maps_bwd_kernel<T, 5>>(what, grid, dim3(64), 0, st, p);
      case 6: return sta_launch<xattn_token_maps_bwd_kernel<T, 6>>(what, grid, dim3(64), 0, st, p);
      case 7: return sta_launch<xattn_token_maps_bwd_kernel<T, 7>>(what, grid, dim3(64), 0, st, p);
      case 8: return sta_launch<xattn_token_maps_bwd_kernel<T, 8>>(what, grid, dim3(64), 0, st, p);
      case 9: return sta_launch<xattn_token_maps_bwd_kernel<T, 9>>(what, grid, dim3(64), 0, st, p);
      case 10: return sta_launch<xattn_token_maps_bwd_kernel<T, 10>>(what, grid, dim3(64), 0, st, p);
    }
    return sta_fail(STA_E_UNSUP, "head dim %d unsupported", d);
  });
}

}  // extern "C"
