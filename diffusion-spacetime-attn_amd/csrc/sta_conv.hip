// sta_conv.hip — the 3x3, stride-1, padding-1 convolutions of the UNet's ResBlocks / Upsample layers on NHWC activations as an
// implicit GEMM on gfx950 MFMAs (reference: ResBlock in_layers / out_layers and Upsample.conv, openaimodel.py:163-275, :91-120;
// called once per ResBlock half inside UNetModel.forward :710-743). These convolutions are ~45 % of a UNet call's GPU time through
// the library kernels (17 - 27 % of the MFMA peak at the UNet's shapes); this is the same operation laid out for this chip.
//
//   out[b][y][x][o] = sum_{ky, kx, i} w[o][i][ky][kx] * in[b][y + ky - 1][x + kx - 1][i]          (zero outside the image)
//
// Pixels are the MFMA columns: Out^T[o][px] = sum over (tap, 32-channel step) of W_tap[o][i] . X_tap^T[i][px]  (v_mfma_f32_16x16x32).
//   * A workgroup (8 waves) owns an output tile of 256 pixels (8 rows x 32 columns, 16 x 16 for 16-pixel-wide images, or two whole
//     8 x 8 images = 128 pixels) and 160 output channels (128 for the VAE decoder's 128 / 256 / 512); a wave owns 64 of the pixels
//     (four 16-pixel row segments) and 80 (64) of the channels: 20 (16) accumulator tiles.
//   * The input tile WITH its one-pixel halo ((8+2) x (32+2) pixels x 32 channels = 21.25 KiB per channel step) is copied to LDS
//     once per channel step by LDS-DMA with per-lane source addresses (pixels outside the image read a page of zeros), double
//     buffered; all nine taps read their B operands from it: one ds_read_b128 per (tap, pixel segment), with the four 16-byte
//     channel chunks of a pixel stored at slot g ^ 2 ((p >> 2) & 1) so that the read is bank-conflict-free at every tap offset.
//   * The weights are re-laid out once per model into 1-KiB A-operand fragments [part][channel step][ky][kx][tile] and streamed
//     through a 2-slot LDS ring, one kernel row (3 taps x 10 tiles = 30 KiB) per step; a step is 60 MFMAs per wave behind
//     27 operand reads (those of tap kx + 1 requested before the MFMAs of tap kx), one barrier per step, the next step's DMA issued
//     behind the first tap's MFMAs (at the barrier every wave would pay its issue cost with the matrix pipe idle).
//   * Workgroups are persistent; the (tile, part) -> workgroup map keeps the parts of one pixel tile on one XCD (shared L2).
//   * `up2`: the input is the nearest-neighbour 2x upsampling of a half-resolution tensor (Upsample.forward, :107-120): the
//     halo copy reads pixel (y >> 1, x >> 1) of the small tensor, so the upsampled tensor never exists in HBM.
//   * SUB (sta_conv3x3_up2_nhwc): the same `up2` convolution as four 2x2 convolutions of the small tensor, one per output phase
//     (a, b) = (row, column parity): out[2y + a][2x + b] = sum_{u, v in {0, 1}} W'_ab[u][v] . in[y + u + a - 1][x + v + b - 1] with
//     W'_ab[u][v] = sum_{ky in R_a(u), kx in R_b(v)} w[ky][kx], R_0 = ({0}, {1, 2}), R_1 = ({0, 1}, {2}) — 16 instead of 36
//     multiply-adds per small pixel. Tiles are those of the SMALL tensor, the halo tile is its plain (non-up2) halo tile, tap (u, v)
//     of phase (a, b) reads where 3x3 tap (u + a, v + b) reads; an item is (tile, part, phase), a step one whole channel step
//     (4 taps x 2 NTW tiles = 40 KiB per ring slot at NTW = 5, 80 MFMAs per wave per barrier).
//   * Epilogue: + bias + residual tensor (ResBlock's `skip_connection(x) + out_layers(h)`), and — `stats` — the partial sums / sums of
//     squares per output channel of the values it stores: the statistics of the GroupNorm that consumes the result.
//   * The input gradient of this convolution is the same convolution with the weight's channel axes exchanged and its taps mirrored:
//     the tracked epochs run forward and backward on this kernel (sta.fused.Conv3x3Fn).
//
// Roofline: MFMA (2 * 9 * Cin * Cout flop per pixel against 2 (Cin + Cout) bytes: 1440 flop/B at 320 -> 320).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "sta_xattn.h"
#include "sta_unet.h"
#include "sta_internal.h"
#include "sta_xattn_dev.h"
#include "sta_wring_dev.h"

namespace {

constexpr int CV_NW = 8;
// NTW = row tiles (16 output channels) per wave: 5 (a workgroup owns 160 channels: the UNet's 320 / 640 / 1280) or 4 (128 channels:
// the VAE decoder's 128 / 256 / 512)
constexpr int cv_part(int ntw) { return 32 * ntw; }                       // output channels per workgroup
constexpr int cv_nt(int ntw) { return 2 * ntw; }                          // row tiles per part
constexpr int cv_wfr(int ntw) { return 3 * cv_nt(ntw); }                  // 30 / 24 weight fragments per step (one kernel row)
template <int NTW> using CvRing = WRing<CV_NW, cv_wfr(NTW)>;              // 4 / 3 weight DMAs per wave per step, 32 / 24 KiB per slot
// Tile geometries. GEO 0: 8 rows x 32 columns; GEO 1: 16 x 16 (16-pixel-wide images): 256 pixels, four 16-pixel segments per wave.
// GEO 2: TWO whole 8 x 8 images (the UNet's lowest level): 128 pixels, two segments (four image rows) per wave — at 64 images x 1280
// channels that is 256 work items, one per CU, where 256-pixel tiles would leave half of the chip idle. The halo tile is stored at a
// row pitch that keeps the chunk swizzle separable (see seg_e below): 36 / 20 / 16 pixels. XPW = input DMA pieces (16 pixels each)
// per wave per channel step; NQ = pixel segments per wave.
constexpr int cv_tr(int geo) { return geo == 0 ? 8 : geo == 1 ? 16 : 8; }
constexpr int cv_tc(int geo) { return geo == 0 ? 32 : geo == 1 ? 16 : 8; }
constexpr int cv_pitch(int geo) { return geo == 0 ? 36 : geo == 1 ? 20 : 16; }
constexpr int cv_npx(int geo) { return geo == 2 ? 2 * 10 * 16 : (cv_tr(geo) + 2) * cv_pitch(geo); }    // 360 / 360 / 320 pixels
constexpr int cv_nq(int geo) { return geo == 2 ? 2 : 4; }
constexpr int cv_xpw(int geo) { return (cv_npx(geo) + 16 * CV_NW - 1) / (16 * CV_NW); }                   // 3
constexpr int cv_xbuf(int geo) { return cv_xpw(geo) * CV_NW * FRAG; }                                      // 24 KiB
template <int NTW, int GEO> constexpr int cv_lds = 2 * CvRing<NTW>::SLOT + 2 * cv_xbuf(GEO);              // 112 / 96 KiB
template <int NTW> using CvSubRing = WRing<CV_NW, 4 * cv_nt(NTW)>;        // SUB: 5 / 4 weight DMAs per wave per step, 40 / 32 KiB per slot
template <int NTW, int GEO> constexpr int cv_sub_lds = 2 * CvSubRing<NTW>::SLOT + 2 * cv_xbuf(GEO);      // 128 / 112 KiB
#ifndef CV_STAGE_AFTER_TAP
#define CV_STAGE_AFTER_TAP 0                  // the next step's DMA is issued behind the MFMAs of this tap (not right behind the barrier,
#endif                                        // where every wave of the workgroup would pay the issue cost with the matrix pipe idle)

// conv weight (o, i, ky, kx) at o*so + i*si + ky*sy + kx*sx -> fragments [part][kc][ky][kx][tile t]: lane (g, c) holds
// W[16 nt part + 16 t + c][32 kc + 8 g .. + 7][ky][kx]      (nt = 10 or 8 row tiles per part)
template <typename T>
__global__ __launch_bounds__(64) void pack_conv_w_kernel(const T* __restrict__ w, long so, long si, long sy, long sx, T* __restrict__ packed,
                                                         int nkc, int nt) {
  const int fr = blockIdx.x;                   // (((part * nkc + kc) * 3 + ky) * 3 + kx) * nt + t
  const int t = fr % nt, kx = (fr / nt) % 3, ky = (fr / (3 * nt)) % 3, kc = (fr / (9 * nt)) % nkc, part = fr / (9 * nt * nkc);
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  const T* src = w + (size_t)(16 * nt * part + 16 * t + c) * so + (size_t)(32 * kc + 8 * g) * si + ky * sy + kx * sx;
  typename Tr<T>::V8 x;
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = src[j * si];
  *(typename Tr<T>::V8*)(packed + (size_t)fr * (FRAG / 2) + lane * 8) = x;
}

// SUB: the pre-summed 2x2 taps of the four output phases -> fragments [phase 2a + b][part][kc][u][v][tile t], lane (g, c) as above.
// W'_ab[u][v] is summed in fp32 over ky in R_a(u) (outer loop, ascending), kx in R_b(v) (inner loop, ascending) and rounded ONCE
// (sta.fused.subpixel_weights restates exactly this order).
template <typename T>
__global__ __launch_bounds__(64) void pack_conv_up2_w_kernel(const T* __restrict__ w, long so, long si, long sy, long sx, T* __restrict__ packed,
                                                             int nkc, int nt, int parts) {
  const int fr = blockIdx.x;                   // ((((phase * parts + part) * nkc + kc) * 2 + u) * 2 + v) * nt + t
  const int t = fr % nt, v = (fr / nt) % 2, u = (fr / (2 * nt)) % 2, kc = (fr / (4 * nt)) % nkc;
  const int pp = fr / (4 * nt * nkc), part = pp % parts, ph = pp / parts, a = ph >> 1, b = ph & 1;
  const int ky0 = a ? 2 * u : u, ky1 = a ? 1 + u : 2 * u;       // R_a(u) = [ky0, ky1]: a = 0: {0}, {1, 2}; a = 1: {0, 1}, {2}
  const int kx0 = b ? 2 * v : v, kx1 = b ? 1 + v : 2 * v;
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  const T* src = w + (size_t)(16 * nt * part + 16 * t + c) * so + (size_t)(32 * kc + 8 * g) * si;
  typename Tr<T>::V8 x;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float s = 0.f;
    for (int ky = ky0; ky <= ky1; ++ky)
      for (int kx = kx0; kx <= kx1; ++kx) s += (float)src[j * si + ky * sy + kx * sx];
    x[j] = (T)s;
  }
  *(typename Tr<T>::V8*)(packed + (size_t)fr * (FRAG / 2) + lane * 8) = x;
}

struct CV {
  const char* x;        // [B][Hs][Ws][Cin] (Hs = H >> up2)
  const char* w;        // packed weights
  const char* zeros;    // >= 2 * Cin bytes of zeros
  void* out;            // [B][H][W][Cout]
  const void* bias;     // [Cout] or null
  const void* res;      // [B][H][W][Cout] or null: out = conv + bias + res
  float* stats;         // null, or [B + 1][stats_slots][Cout][2] fp32: per (image, slot) partial sums / sums of squares of the STORED values
  int stats_slots;
  int B, H, W, Cin, Cout, up2;  // (SUB: H, W are those of x, up2 = 0, out is [B][2 H][2 W][Cout])
  int parts, tiles_x, tiles_per_img, items, xcd_map;
};

// SUB: what is not read inside the MFMA loop (tile decode, halo addresses, epilogue) re-reads the launch arguments from the kernel
// argument segment where it needs them, so that they do not occupy SGPRs across the loop (the instantiations are built free of
// spills). These helpers are functions, not lambdas of the kernel, so that the plain instantiations do not see them at all.
__device__ __forceinline__ CV cv_fresh_args() {
  typedef const __attribute__((address_space(4))) unsigned* KP;
  KP k = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  static_assert(sizeof(CV) % 4 == 0, "CV is a sequence of dwords");
  union { CV c; unsigned u[sizeof(CV) / 4]; } r;
#pragma unroll
  for (unsigned i = 0; i < sizeof(CV) / 4; ++i) r.u[i] = k[i];
  return r.c;
}
// SUB: in_ptr of the kernel for the small tensor itself (no up2 shift), from freshly read arguments; the lane's halo position is made
// opaque so that nothing of it is hoisted out of the item loop into SGPR lane masks
template <typename T, int GEO>
__device__ __forceinline__ const char* cv_sub_in_ptr(int lane, int tile, int pc) {
  constexpr int TR = cv_tr(GEO), TC = cv_tc(GEO), TWH = TC + 2, PITCH = cv_pitch(GEO), NPX = cv_npx(GEO);
  const CV a = cv_fresh_args();
  int pp = 16 * pc + (lane >> 2);
  asm volatile("" : "+v"(pp));
  const int chunk = (lane & 3) ^ (((pp >> 2) & 1) << 1);
  int b, y, x, hx;
  if (GEO == 2) {
    const int im = pp / (10 * PITCH), rem = pp - im * (10 * PITCH);
    const int hy = rem / PITCH;
    hx = rem - hy * PITCH;
    b = 2 * tile + im; y = hy - 1; x = hx - 1;
  } else {
    b = tile / a.tiles_per_img;
    const int tt = tile - b * a.tiles_per_img;
    const int ty = tt / a.tiles_x, tx = tt - ty * a.tiles_x;
    const int hy = pp / PITCH;
    hx = pp - hy * PITCH;
    y = ty * TR - 1 + hy; x = tx * TC - 1 + hx;
  }
  const bool ok = pp < NPX && hx < TWH && y >= 0 && y < a.H && x >= 0 && x < a.W && b < a.B;
  const size_t px = ((size_t)b * a.H + y) * a.W + x;
  return ok ? a.x + px * (size_t)a.Cin * sizeof(T) + chunk * 16 : a.zeros + chunk * 16;
}
// the launch arguments a piece of the kernel works from: p itself, or (SUB) the copy it has just re-read
template <bool SUB> struct CvArgs {};
template <> struct CvArgs<true> { CV v; };
__device__ __forceinline__ const CV& cv_pick(const CvArgs<false>&, const CV& p) { return p; }
__device__ __forceinline__ const CV& cv_pick(const CvArgs<true>& f, const CV&) { return f.v; }

template <typename T, int GEO, int NTW, bool SUB = false>
__global__ __launch_bounds__(64 * CV_NW, 1) void conv3x3_nhwc_kernel(const CV p) {
  using V8 = typename Tr<T>::V8;
  using V4 = typename Tr<T>::V4;
  using Ring = std::conditional_t<SUB, CvSubRing<NTW>, CvRing<NTW>>;
  constexpr int CV_PART = cv_part(NTW), CV_NT = cv_nt(NTW), CV_WFR = SUB ? 4 * CV_NT : cv_wfr(NTW), CV_WSLOT = Ring::SLOT;
  // halo tile: (TR + 2) rows of TC + 2 pixels at a pitch that is a multiple of 4: the chunk swizzle ((pixel index >> 2) & 1) << 1 of pixel
  // (row, xx) is then ((row * (PITCH / 4) + (xx >> 2)) & 1) << 1 — separable in row and column, so a lane needs 12 operand addresses
  // instead of 36 (PITCH / 4 odd: bit 5 of the address flips on odd kernel rows; even: it does not depend on the row at all)
  constexpr int TR = cv_tr(GEO), TC = cv_tc(GEO), TWH = TC + 2, PITCH = cv_pitch(GEO), NPX = cv_npx(GEO), XPW = cv_xpw(GEO), CV_XBUF = cv_xbuf(GEO), NQ = cv_nq(GEO);
  constexpr bool ROW_FLIPS = (PITCH / 4) % 2 == 1;
  static_assert(PITCH % 4 == 0 && PITCH >= TWH, "halo tile geometry");
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int pq = wv & 3, ch = wv >> 2;                     // pixel quarter (4 row segments), channel half (5 row tiles)
  char* xring = smem;                                      // input buffers first: their operand reads then fit ds_read's 16-bit offset field
  char* wring = smem + 2 * CV_XBUF;
  const int nkc = p.Cin >> 5;
  const int Hs = p.H >> p.up2, Ws = p.W >> p.up2;
  const __amdgpu_buffer_rsrc_t w_srd = make_srd(p.w, (unsigned)((size_t)p.parts * nkc * (SUB ? 16 : 9) * CV_NT * FRAG));
  const unsigned lane16 = (unsigned)lane * 16u;

  // item -> (tile, part): the parts of a pixel tile run back to back on ONE XCD (workgroup id % 8), so the input tile is fetched
  // from HBM once per XCD-L2 and the weight stream of a part is shared by the XCD's CUs walking the channel steps together
  // (tile counts that are not a multiple of 8 — small batches — take the plain order). SUB: `part` is 4 (channel part) + phase, the
  // four phases of a part back to back
  auto item_tile = [&](int it, int& tile, int& part) {
    CvArgs<SUB> fresh;
    if constexpr (SUB) fresh.v = cv_fresh_args();
    const CV& a = cv_pick(fresh, p);
    const int nsub = SUB ? 4 * a.parts : a.parts;
    if (a.xcd_map) {
      const int j = it >> 3;
      tile = (j / nsub) * 8 + (it & 7);
      part = j % nsub;
    } else {
      tile = it / nsub;
      part = it - tile * nsub;
    }
  };
  // per-lane source pointer of input piece `pc` (pixels 16 pc .. + 15 of the halo tile, this lane: pixel 16 pc + (lane >> 2), LDS slot
  // lane & 3) at channel step 0
  auto in_ptr = [&](int tile, int pc) -> const char* {
    const int pp = 16 * pc + (lane >> 2);
    const int chunk = (lane & 3) ^ (((pp >> 2) & 1) << 1);
    int b, y, x, hx;
    if (GEO == 2) {                                        // image 2 tile + pp / 160, halo row (pp % 160) / 16
      const int im = pp / (10 * PITCH), rem = pp - im * (10 * PITCH);
      const int hy = rem / PITCH;
      hx = rem - hy * PITCH;
      b = 2 * tile + im; y = hy - 1; x = hx - 1;
    } else {
      b = tile / p.tiles_per_img;
      const int tt = tile - b * p.tiles_per_img;
      const int ty = tt / p.tiles_x, tx = tt - ty * p.tiles_x;
      const int hy = pp / PITCH;
      hx = pp - hy * PITCH;
      y = ty * TR - 1 + hy; x = tx * TC - 1 + hx;
    }
    const bool ok = pp < NPX && hx < TWH && y >= 0 && y < p.H && x >= 0 && x < p.W && b < p.B;
    const size_t px = ((size_t)b * Hs + (y >> p.up2)) * Ws + (x >> p.up2);
    return ok ? p.x + px * (size_t)p.Cin * sizeof(T) + chunk * 16 : p.zeros + chunk * 16;
  };
  auto stage_w = [&](int part, int kc, int ky, int slot) __attribute__((always_inline)) {
    Ring::stage(w_srd, wring + slot * CV_WSLOT, (unsigned)(((part * nkc + kc) * 3 + ky) * CV_WFR) * (unsigned)FRAG, 0, wv, lane16);
  };
  auto stage_w_sub = [&](int sub, int kc, int slot) __attribute__((always_inline)) {      // sub = 4 part + phase -> image [phase][part][kc]
    Ring::stage(w_srd, wring + slot * CV_WSLOT, (unsigned)((((sub & 3) * p.parts + (sub >> 2)) * nkc + kc) * CV_WFR) * (unsigned)FRAG, 0, wv, lane16);
  };
  auto stage_x = [&](const char* src, int pc, int buf) __attribute__((always_inline)) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)(xring + buf * CV_XBUF + pc * FRAG), 16, 0, 0);
  };

  // this wave's NQ pixel segments: segment index gi = 4 pq + q -> (row, first column) inside the tile (GEO 2: image pq >> 1, rows
  // 4 (pq & 1) + 2 q and the next, lane c -> (row + (c >> 3), c & 7)). Byte offset inside an input buffer of this lane's B operand chunk for tap (ky, kx):
  // seg_e[q][kx] + ky * PITCH * 64, bit 5 flipped when ky is odd and ROW_FLIPS
  auto seg_rc = [&](int q, int& ry, int& x0) {             // first halo row / column of the segment's lane-0 pixel at tap (0, 0)
    const int gi = 4 * pq + q;
    if (GEO == 0) { ry = gi >> 1; x0 = (gi & 1) * 16 + c16; }
    else if (GEO == 1) { ry = gi; x0 = c16; }
    else { ry = 10 * (pq >> 1) + 4 * (pq & 1) + 2 * q + (c16 >> 3); x0 = c16 & 7; }
  };
  unsigned seg_e[NQ][3];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    int ry, x0;
    seg_rc(q, ry, x0);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = x0 + kx;
      seg_e[q][kx] = (unsigned)((ry * PITCH + xx) * 64 + ((g ^ (((ry * (PITCH / 4) + (xx >> 2)) & 1) << 1)) << 4));
    }
  }

  int it = blockIdx.x;
  if (it >= (SUB ? cv_fresh_args().items : p.items)) return;
  int tile, part;
  item_tile(it, tile, part);
  const char* xp[XPW];                                     // this wave's input pieces (wv, wv + 8, ...) of the NEXT channel step
#pragma unroll
  for (int i = 0; i < XPW; ++i) {
    if constexpr (SUB) xp[i] = cv_sub_in_ptr<T, GEO>(lane, tile, wv + CV_NW * i);
    else xp[i] = in_ptr(tile, wv + CV_NW * i);
  }
  // prologue: kernel row 0 of channel step 0 (SUB: the four taps of channel step 0) and the whole input tile of channel step 0
  if constexpr (SUB) stage_w_sub(part, 0, 0);
  else stage_w(part, 0, 0, 0);
#pragma unroll
  for (int i = 0; i < XPW; ++i) { stage_x(xp[i], wv + CV_NW * i, 0); xp[i] += 64; }

  const size_t obytes = (size_t)p.B * p.H * p.W * p.Cout * sizeof(T);      // (SUB builds its descriptors in the epilogue)
  const __amdgpu_buffer_rsrc_t o_srd0 = make_srd(p.out, (unsigned)(obytes < 0xfffffff0ull ? obytes : 0xfffffff0ull));
  const __amdgpu_buffer_rsrc_t r_srd0 = make_srd(p.res ? p.res : p.out, (unsigned)(obytes < 0xfffffff0ull ? obytes : 0xfffffff0ull));
  bool first_of_tile = false;                              // the step that follows an epilogue: 4 NTW stores are younger than its DMAs

  while (true) {
    f32x4 acc[NQ][NTW];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int t = 0; t < NTW; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    int nit = it + gridDim.x, ntile = 0, npart = 0;
    bool more = false;                                     // (SUB finds the next item where it needs it: nothing of it is live across the loop)
    if constexpr (!SUB) {
      more = nit < p.items;
      if (more) item_tile(nit, ntile, npart);
    }

    if constexpr (SUB) {
      // phase (a, b) of this item: tap (u, v) reads where 3x3 tap (u + a, v + b) reads — the existing seg_e[q][kx], row offset and odd-row flip
      const int pa = (part >> 1) & 1, pb = part & 1;
      unsigned tap_e[4][NQ];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
          for (int q = 0; q < NQ; ++q) {                   // = seg_e[q][v + pb] (recomputed: a run-time index would put seg_e in scratch)
            int ry, x0;
            seg_rc(q, ry, x0);
            const int ky = u + pa, xx = x0 + v + pb;
            const unsigned e = (unsigned)((ry * PITCH + xx) * 64 + ((g ^ (((ry * (PITCH / 4) + (xx >> 2)) & 1) << 1)) << 4));
            tap_e[2 * u + v][q] = (ROW_FLIPS ? e ^ ((unsigned)(ky & 1) << 5) : e) + (unsigned)(ky * PITCH * 64);
          }
      // one step = the four taps of one channel step; buffers and slots alternate with the channel step (compile-time: two per trip)
      auto step = [&](auto xb_tag, const int kc) __attribute__((always_inline)) {
        constexpr int XB = decltype(xb_tag)::value, WS = XB;
        if (first_of_tile) {                               // the epilogue's stores (and statistics stores) are younger than this step's DMAs
          if (cv_fresh_args().stats) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NQ * NTW + 2 * NTW) : "memory");
          else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NQ * NTW) : "memory");
        } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        first_of_tile = false;
        __builtin_amdgcn_s_barrier();
        // the next channel step's taps and input tile (the next item's first, behind this item's last)
        auto stage_next = [&]() __attribute__((always_inline)) {
          const bool last_kc = kc + 1 == nkc;
          if (last_kc) {
            more = nit < cv_fresh_args().items;
            if (more) item_tile(nit, ntile, npart);
          }
          if (!last_kc) stage_w_sub(part, kc + 1, WS ^ 1);
          else if (more) stage_w_sub(npart, 0, WS ^ 1);
          if (!last_kc || more) {
#pragma unroll
            for (int i = 0; i < XPW; ++i) {
              if (last_kc) xp[i] = cv_sub_in_ptr<T, GEO>(lane, ntile, wv + CV_NW * i);
              stage_x(xp[i], wv + CV_NW * i, XB ^ 1);
              xp[i] += 64;
            }
          }
        };
        const char* xb = xring + XB * CV_XBUF;
        const V8* wf = (const V8*)(wring + WS * CV_WSLOT + lane * 16) + (NTW * ch) * 64;
        V8 a[NTW], b[NQ];
        auto load_tap = [&](int tp, V8 (&aa)[NTW], V8 (&bb)[NQ]) __attribute__((always_inline)) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) bb[q] = *(const V8*)(xb + tap_e[tp][q]);
#pragma unroll
          for (int t = 0; t < NTW; ++t) aa[t] = wf[(tp * CV_NT + t) * 64];
        };
        load_tap(0, a, b);
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
          V8 an[NTW], bn[NQ];
          if (tp < 3) load_tap(tp + 1, an, bn);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int t = 0; t < NTW; ++t)
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q][t] = Tr<T>::mfma(a[t], b[q], acc[q][t]);
          __builtin_amdgcn_sched_barrier(0);
          if (tp == 0) {
            stage_next();
            __builtin_amdgcn_sched_barrier(0);
          }
          if (tp < 3) {
#pragma unroll
            for (int t = 0; t < NTW; ++t) a[t] = an[t];
#pragma unroll
            for (int q = 0; q < NQ; ++q) b[q] = bn[q];
          }
        }
      };
      for (int kc = 0; kc < nkc; kc += 2) {
        step(std::integral_constant<int, 0>{}, kc);
        step(std::integral_constant<int, 1>{}, kc + 1);
      }
    } else {
    // one step = one kernel row (3 taps) of one channel step. Slots are compile-time: two channel steps (6 steps) per trip.
    auto step = [&](auto xb_tag, auto ws_tag, auto ky_tag, const int kc) __attribute__((always_inline)) {
      constexpr int XB = decltype(xb_tag)::value, WS = decltype(ws_tag)::value, KY = decltype(ky_tag)::value;
      if (first_of_tile) {                                 // the epilogue's stores (and statistics atomics) are younger than this step's DMAs
        if (p.stats) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NQ * NTW + 2 * NTW) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NQ * NTW) : "memory");
      } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      first_of_tile = false;
      __builtin_amdgcn_s_barrier();
      // the next step's kernel row, and one piece of the next channel step's input tile
      auto stage_next = [&]() __attribute__((always_inline)) {
        const bool last_kc = kc + 1 == nkc;
        if (KY < 2) stage_w(part, kc, KY + 1, WS ^ 1);
        else if (!last_kc) stage_w(part, kc + 1, 0, WS ^ 1);
        else if (more) stage_w(npart, 0, 0, WS ^ 1);
        if (!last_kc || more) {
#pragma unroll
          for (int i = KY; i < XPW; i += 3) {              // pieces KY, KY + 3 of this wave: one or two per step
            if (last_kc) xp[i] = in_ptr(ntile, wv + CV_NW * i);
            stage_x(xp[i], wv + CV_NW * i, XB ^ 1);
            xp[i] += 64;
          }
        }
      };
      if (CV_STAGE_AFTER_TAP < 0) stage_next();
      const char* xb = xring + XB * CV_XBUF;
      const V8* wf = (const V8*)(wring + WS * CV_WSLOT + lane * 16) + (NTW * ch) * 64;
      // operands of tap kx + 1 are requested before the 20 MFMAs of tap kx (two register sets)
      V8 a[NTW], b[NQ];
      auto load_tap = [&](int kx, V8 (&aa)[NTW], V8 (&bb)[NQ]) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) bb[q] = *(const V8*)(xb + KY * PITCH * 64 + ((KY & 1) && ROW_FLIPS ? seg_e[q][kx] ^ 32u : seg_e[q][kx]));
#pragma unroll
        for (int t = 0; t < NTW; ++t) aa[t] = wf[(kx * CV_NT + t) * 64];
      };
      load_tap(0, a, b);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        V8 an[NTW], bn[NQ];
        if (kx < 2) load_tap(kx + 1, an, bn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
          for (int q = 0; q < NQ; ++q) acc[q][t] = Tr<T>::mfma(a[t], b[q], acc[q][t]);
        __builtin_amdgcn_sched_barrier(0);
        if (kx == CV_STAGE_AFTER_TAP) {
          stage_next();
          __builtin_amdgcn_sched_barrier(0);
        }
        if (kx < 2) {
#pragma unroll
          for (int t = 0; t < NTW; ++t) a[t] = an[t];
#pragma unroll
          for (int q = 0; q < NQ; ++q) b[q] = bn[q];
        }
      }
    };
    for (int kc = 0; kc < nkc; kc += 2) {
      using I0 = std::integral_constant<int, 0>;
      using I1 = std::integral_constant<int, 1>;
      using I2 = std::integral_constant<int, 2>;
      step(I0{}, I0{}, I0{}, kc);
      step(I0{}, I1{}, I1{}, kc);
      step(I0{}, I0{}, I2{}, kc);
      step(I1{}, I1{}, I0{}, kc + 1);
      step(I1{}, I0{}, I1{}, kc + 1);
      step(I1{}, I1{}, I2{}, kc + 1);
    }
    }
    // epilogue: lane (g, c) of tile t holds output channels 16 t + 4 g .. + 3 of pixel c (+ bias, + the residual tensor):
    // ALWAYS NQ * NTW stores of 8 bytes, issued behind every load of the epilogue
    {
      CvArgs<SUB> fresh;
      if constexpr (SUB) fresh.v = cv_fresh_args();
      const CV& e = cv_pick(fresh, p);
      const int b = GEO == 2 ? 2 * tile + (pq >> 1) : tile / e.tiles_per_img, tt = GEO == 2 ? 0 : tile - b * e.tiles_per_img;
      const int cpart = SUB ? part >> 2 : part;            // SUB: pixel (row, col) of the tile is output pixel (2 row + a, 2 col + b)
      const int ty = tt / e.tiles_x, tx = tt - ty * e.tiles_x;
      typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
      const int OH = SUB ? 2 * e.H : e.H, OW = SUB ? 2 * e.W : e.W;
      __amdgpu_buffer_rsrc_t o_srd, r_srd;
      if constexpr (SUB) {
        const size_t obytes = (size_t)e.B * OH * OW * e.Cout * sizeof(T);
        o_srd = make_srd(e.out, (unsigned)(obytes < 0xfffffff0ull ? obytes : 0xfffffff0ull));
        r_srd = make_srd(e.res ? e.res : e.out, (unsigned)(obytes < 0xfffffff0ull ? obytes : 0xfffffff0ull));
      } else { o_srd = o_srd0; r_srd = r_srd0; }
      float bs[NTW][4];
#pragma unroll
      for (int t = 0; t < NTW; ++t) {
        V4 bv = {};
        if (e.bias) bv = *(const V4*)((const T*)e.bias + cpart * CV_PART + ch * (16 * NTW) + 16 * t + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) bs[t][r] = (float)bv[r];
      }
      float ssum[NTW][4], ssq[NTW][4];                     // GroupNorm statistics of the stored values, per output channel
#pragma unroll
      for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) { ssum[t][r] = 0.f; ssq[t][r] = 0.f; }
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        int ry, x0;
        seg_rc(q, ry, x0);
        if (GEO == 2) ry -= 10 * (pq >> 1);
        size_t px;
        if constexpr (SUB) px = ((size_t)b * OH + 2 * (ty * TR + ry) + ((part >> 1) & 1)) * OW + 2 * (tx * TC + x0) + (part & 1);
        else px = ((size_t)b * e.H + ty * TR + ry) * e.W + tx * TC + x0;
        const bool img_ok = b < e.B;                       // (GEO 2: the second image of the last tile of an odd batch does not exist)
        const unsigned base = (unsigned)((px * e.Cout + cpart * CV_PART + ch * (16 * NTW) + 4 * g) * sizeof(T));
        V4 rv[NTW];
        if (e.res) {
#pragma unroll
          for (int t = 0; t < NTW; ++t)
            rv[t] = __builtin_bit_cast(V4, __builtin_amdgcn_raw_buffer_load_b64(r_srd, img_ok ? base + (unsigned)(16 * t * sizeof(T)) : SRD_DROP, 0, 0));
        }
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
          V4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (T)(acc[q][t][r] + bs[t][r] + (e.res ? (float)rv[t][r] : 0.f));
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), o_srd, img_ok ? base + (unsigned)(16 * t * sizeof(T)) : SRD_DROP, 0, 0);
          if (e.stats) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float v = img_ok ? (float)o[r] : 0.f;
              ssum[t][r] += v;
              ssq[t][r] += v * v;
            }
          }
        }
      }
      // the consumer's GroupNorm statistics from here (sta_stats_finalize -> sta_groupnorm_silu_nhwc_cstats): sum over the wave's 16 pixel
      // lanes, then lane c16 == 0 stores the wave's partial sums of its 4 x NTW channels into the slot (tile of the image, pixel quarter)
      // — plain stores, no atomics (2.6 M atomics per level-0 convolution cost 18 % of it), ALWAYS 2 NTW store instructions per wave
      if (e.stats) {
        const int slot0 = GEO == 2 ? (pq & 1) : tt * 4 + pq;
        const int slot = SUB ? 4 * slot0 + (part & 3) : slot0;                 // SUB: the four phases of a (tile, pixel quarter)
        const int bb = b < e.B ? b : e.B;                  // a nonexistent image (GEO 2, odd batch) writes the spare image slot
        float* dst = e.stats + (((size_t)bb * e.stats_slots + slot) * e.Cout + cpart * CV_PART + ch * (16 * NTW) + 4 * g) * 2;
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
          f32x4 lo, hi;
          lo[0] = row16_sum(ssum[t][0]); lo[1] = row16_sum(ssq[t][0]); lo[2] = row16_sum(ssum[t][1]); lo[3] = row16_sum(ssq[t][1]);
          hi[0] = row16_sum(ssum[t][2]); hi[1] = row16_sum(ssq[t][2]); hi[2] = row16_sum(ssum[t][3]); hi[3] = row16_sum(ssq[t][3]);
          if (c16 == 0) {
            *(f32x4*)(dst + 32 * t) = lo;
            *(f32x4*)(dst + 32 * t + 4) = hi;
          }
        }
      }
    }
    if constexpr (SUB) {
      more = nit < cv_fresh_args().items;
      if (more) item_tile(nit, ntile, npart);
    }
    if (!more) break;
    it = nit; tile = ntile; part = npart;
    first_of_tile = true;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

int conv_geo(int H, int W) {                  // tile geometry of an H x W image, -1: none
  if (W % 32 == 0 && H % 8 == 0) return 0;
  if (W == 16 && H % 16 == 0) return 1;
  if (W == 8 && H == 8) return 2;
  return -1;
}

template <typename T, int GEO, int NTW>
int conv_launch(const CV& p, unsigned grid, hipStream_t st) {
  return sta_launch_lds<conv3x3_nhwc_kernel<T, GEO, NTW>>("conv3x3_nhwc launch", cv_lds<NTW, GEO>, dim3(grid), dim3(64 * CV_NW), cv_lds<NTW, GEO>, st, p);
}

template <typename T, int GEO, int NTW>
int conv_up2_launch(const CV& p, unsigned grid, hipStream_t st) {
  return sta_launch_lds<conv3x3_nhwc_kernel<T, GEO, NTW, true>>("conv3x3_up2_nhwc launch", cv_sub_lds<NTW, GEO>, dim3(grid), dim3(64 * CV_NW),
                                                                cv_sub_lds<NTW, GEO>, st, p);
}

}  // namespace

extern "C" {

static int conv_ntw(int Cout) { return Cout > 0 && Cout % 160 == 0 ? 5 : (Cout > 0 && Cout % 128 == 0 ? 4 : 0); }

int sta_conv3x3_nhwc_supported(int B, int H, int W, int Cin, int Cout) {
  if (B <= 0 || conv_geo(H, W) < 0) return 0;
  if (Cin <= 0 || Cin % 64 || conv_ntw(Cout) == 0) return 0;
  if ((size_t)B * H * W * (size_t)Cout * 2 >= 0xfffffff0ull) return 0;
  return 1;
}

int sta_conv3x3_stats_slots(int H, int W) {
  const int geo = conv_geo(H, W);
  return geo < 0 ? 0 : geo == 2 ? 2 : 4 * (H / cv_tr(geo)) * (W / cv_tc(geo));
}

size_t sta_conv3x3_packed_w_bytes(int Cin, int Cout) {
  return (Cin > 0 && Cin % 64 == 0 && conv_ntw(Cout)) ? (size_t)Cout * Cin * 9 * 2 : 0;
}

int sta_conv3x3_pack_w(const void* w, long so, long si, long sy, long sx, void* packed, int Cin, int Cout, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!w || !packed) return sta_fail(STA_E_ARG, "null pointer");
  if (sta_conv3x3_packed_w_bytes(Cin, Cout) == 0)
    return sta_fail(STA_E_UNSUP, "conv3x3: Cin %% 64 == 0 and Cout %% 160 == 0 or Cout %% 128 == 0 (Cin=%d Cout=%d)", Cin, Cout);
  hipStream_t st = (hipStream_t)stream;
  const int nkc = Cin / 32, nt = cv_nt(conv_ntw(Cout));
  const unsigned nfr = (unsigned)(Cout / (16 * nt)) * nkc * 9 * nt;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<pack_conv_w_kernel<T>>("pack_conv_w launch", dim3(nfr), dim3(64), 0, st, (const T*)w, so, si, sy, sx, (T*)packed, nkc, nt);
  });
}

int sta_conv3x3_nhwc(const void* x, const void* packed_w, const void* zeros, const void* bias, const void* res, void* out, float* stats, int B,
                     int H, int W, int Cin, int Cout, int up2, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !packed_w || !zeros || !out) return sta_fail(STA_E_ARG, "null pointer");
  if (!sta_conv3x3_nhwc_supported(B, H, W, Cin, Cout))
    return sta_fail(STA_E_UNSUP, "conv3x3_nhwc: unsupported geometry B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W, Cin, Cout);
  if (up2 && (H % 2 || W % 2)) return sta_fail(STA_E_ARG, "conv3x3_nhwc: up2 needs even H, W");
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_UNSUP, "dtype %d", dtype);
  const int geo = conv_geo(H, W), ntw = conv_ntw(Cout);
  const int tr = cv_tr(geo), tc = cv_tc(geo);
  CV p{(const char*)x, (const char*)packed_w, (const char*)zeros, out, bias, res, stats, 0, B, H, W, Cin, Cout, up2 ? 1 : 0,
       Cout / cv_part(ntw), W / tc, (H / tr) * (W / tc), 0, 0};
  p.stats_slots = geo == 2 ? 2 : 4 * p.tiles_per_img;
  const long tiles = geo == 2 ? (B + 1) / 2 : (long)B * p.tiles_per_img;
  const long items = tiles * p.parts;
  if (items >= (1l << 30)) return sta_fail(STA_E_UNSUP, "conv3x3_nhwc: too many tiles");
  p.items = (int)items;
  p.xcd_map = tiles % 8 == 0;
  const unsigned grid = (unsigned)(p.items < 256 ? p.items : 256);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (geo == 0) return ntw == 5 ? conv_launch<T, 0, 5>(p, grid, st) : conv_launch<T, 0, 4>(p, grid, st);
    if (geo == 1) return ntw == 5 ? conv_launch<T, 1, 5>(p, grid, st) : conv_launch<T, 1, 4>(p, grid, st);
    return ntw == 5 ? conv_launch<T, 2, 5>(p, grid, st) : conv_launch<T, 2, 4>(p, grid, st);
  });
}

// The `up2` convolution as four 2x2 sub-pixel convolutions of the half-resolution tensor (SUB). H, W: the OUTPUT size, as for
// sta_conv3x3_nhwc with up2 = 1; the tile geometry is that of the H / 2 x W / 2 input.
int sta_conv3x3_up2_nhwc_supported(int B, int H, int W, int Cin, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2 || conv_geo(H / 2, W / 2) < 0) return 0;
  if (Cin <= 0 || Cin % 64 || conv_ntw(Cout) == 0) return 0;
  if ((size_t)B * H * W * (size_t)Cout * 2 >= 0xfffffff0ull) return 0;
  return 1;
}

int sta_conv3x3_up2_stats_slots(int H, int W) {
  return (H <= 0 || W <= 0 || H % 2 || W % 2) ? 0 : 4 * sta_conv3x3_stats_slots(H / 2, W / 2);
}

size_t sta_conv3x3_up2_packed_w_bytes(int Cin, int Cout) {
  return (Cin > 0 && Cin % 64 == 0 && conv_ntw(Cout)) ? (size_t)Cout * Cin * 16 * 2 : 0;
}

int sta_conv3x3_up2_pack_w(const void* w, long so, long si, long sy, long sx, void* packed, int Cin, int Cout, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!w || !packed) return sta_fail(STA_E_ARG, "null pointer");
  if (sta_conv3x3_up2_packed_w_bytes(Cin, Cout) == 0)
    return sta_fail(STA_E_UNSUP, "conv3x3_up2: Cin %% 64 == 0 and Cout %% 160 == 0 or Cout %% 128 == 0 (Cin=%d Cout=%d)", Cin, Cout);
  hipStream_t st = (hipStream_t)stream;
  const int nkc = Cin / 32, nt = cv_nt(conv_ntw(Cout)), parts = Cout / (16 * nt);
  const unsigned nfr = 4u * parts * nkc * 4 * nt;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<pack_conv_up2_w_kernel<T>>("pack_conv_up2_w launch", dim3(nfr), dim3(64), 0, st, (const T*)w, so, si, sy, sx, (T*)packed, nkc, nt,
                                                 parts);
  });
}

int sta_conv3x3_up2_nhwc(const void* x, const void* packed_w, const void* zeros, const void* bias, const void* res, void* out, float* stats, int B,
                         int H, int W, int Cin, int Cout, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !packed_w || !zeros || !out) return sta_fail(STA_E_ARG, "null pointer");
  if (!sta_conv3x3_up2_nhwc_supported(B, H, W, Cin, Cout))
    return sta_fail(STA_E_UNSUP, "conv3x3_up2_nhwc: unsupported geometry B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W, Cin, Cout);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_UNSUP, "dtype %d", dtype);
  const int Hs = H / 2, Ws = W / 2;
  const int geo = conv_geo(Hs, Ws), ntw = conv_ntw(Cout);
  const int tr = cv_tr(geo), tc = cv_tc(geo);
  CV p{(const char*)x, (const char*)packed_w, (const char*)zeros, out, bias, res, stats, 0, B, Hs, Ws, Cin, Cout, 0,
       Cout / cv_part(ntw), Ws / tc, (Hs / tr) * (Ws / tc), 0, 0};
  p.stats_slots = sta_conv3x3_up2_stats_slots(H, W);
  const long tiles = geo == 2 ? (B + 1) / 2 : (long)B * p.tiles_per_img;
  const long items = tiles * p.parts * 4;                  // (tile, part, phase)
  if (items >= (1l << 30)) return sta_fail(STA_E_UNSUP, "conv3x3_up2_nhwc: too many tiles");
  p.items = (int)items;
  p.xcd_map = tiles % 8 == 0;
  const unsigned grid = (unsigned)(p.items < 256 ? p.items : 256);
  hipStream_t st = (hipStream_t)stream;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (geo == 0) return ntw == 5 ? conv_up2_launch<T, 0, 5>(p, grid, st) : conv_up2_launch<T, 0, 4>(p, grid, st);
    if (geo == 1) return ntw == 5 ? conv_up2_launch<T, 1, 5>(p, grid, st) : conv_up2_launch<T, 1, 4>(p, grid, st);
    return ntw == 5 ? conv_up2_launch<T, 2, 5>(p, grid, st) : conv_up2_launch<T, 2, 4>(p, grid, st);
  });
}

}  // extern "C"
