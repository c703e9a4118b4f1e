// sta_encode.hip — the image end of img2img on gfx950: the VAE encoder's stride-2 downsampling convolution on NHWC activations and
// the one elementwise pass from the encoder's output to the first UNet call's input. C-ABI in include/sta_unet.h.
//
// 1. sta_conv3x3_s2_nhwc — Downsample (reference ldm/modules/diffusionmodules/model.py:60-79: F.pad(x, (0, 1, 0, 1)) + 3x3 conv,
//    stride 2) without the padded copy:
//
//      out[b][y][x][o] = bias[o] + sum_{ky, kx, i} w[o][i][ky][kx] * in[b][2y + ky][2x + kx][i]      (in = 0 at row >= H or col >= W)
//
//    Implicit GEMM on v_mfma_f32_16x16x32 with pixels as the MFMA columns, as in sta_conv.hip. A workgroup (4 waves) owns an output
//    tile of 8 rows x 16 columns and 128 output channels (one part of sta_conv3x3_pack_w's weight image, reused as is); a wave owns 4
//    output rows (4 16-pixel segments) x 64 channels: 16 accumulator tiles, every B operand read from LDS feeds 4 MFMAs.
//    The tile's input footprint (17 rows x 33 columns) is copied to LDS once per 32-channel step by LDS-DMA with per-lane source
//    addresses, double buffered; pixels at row >= H or column >= W (the bottom / right pad — top and left are never outside) read a
//    page of zeros, so no padded tensor is ever written. Each input row is stored as two planes, its 17 even columns then its 16 odd
//    columns: the 16 pixels a tap reads for one output segment (input columns 2x + kx) are then 16 CONSECUTIVE plane pixels
//    (kx = 0: even plane from 0, kx = 1: odd plane, kx = 2: even plane from 1), and the 16-byte channel chunks of a pixel sit at slot
//    g ^ 2 ((p >> 2) & 1), the chunk swizzle of sta_conv.hip. The weights are read per lane straight from the packed 1-KiB fragments
//    (L2-resident: at most 4.7 MB), one kernel row ahead of the MFMAs that use them.
//    Epilogue: + bias, 8-byte stores, and (stats) the per-channel partial sums / sums of squares of the stored values in fixed slots
//    (sta_conv3x3_s2_stats_slots per image) for sta_stats_finalize: the statistics of the next ResnetBlock's norm1.
//    Roofline per output pixel: 2 * 9 * Cin * Cout flop against ~2 (4 Cin + Cout) bytes: 230 flop/B at 128 channels (HBM-bound below
//    the ridge), MFMA-bound at 256 and 512 by that roofline. Measured (16 images, fp16, profiles/img2img_throughput.json): 0.30 - 0.37 of
//    the bound at every supported shape, 2.1 - 3.6 x faster than F.pad + the library convolution; what limits it below the bound is not
//    measured (candidates: the per-lane A-operand loads, which both waves of a channel half issue for the same fragments, and the
//    compiler's wait for them inside each kernel row).
//
// 2. sta_vae_encode_step — per latent pixel, in fp32: quant_conv (8x8 1x1 + bias), the posterior's mean / clamped logvar, its sample
//    z0 = scale_factor (mean + exp(logvar / 2) n_post) (DiagonalGaussianDistribution.sample + get_first_stage_encoding), and DDIM's
//    stochastic_encode x = sqrt_a z0 + sqrt_1ma n_enc; writes x (the sampler state), optionally z0, and the 16-bit CFG input pair.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sta_xattn.h"
#include "sta_unet.h"
#include "sta_internal.h"
#include "sta_xattn_dev.h"
#include "sta_wring_dev.h"      // row16_sum
#include "sta_encode_dev.h"     // the per-pixel arithmetic of part 2: shared with the canvas form in sta_window.hip

namespace {

constexpr int S2_NW = 4;                                      // waves per workgroup
constexpr int S2_TR = 8, S2_TC = 16;                          // output tile: 8 rows x 16 columns
constexpr int S2_IR = 2 * S2_TR + 1;                          // 17 input rows
constexpr int S2_EC = S2_TC + 1;                              // 17 even input columns at LDS columns 0 .. 16
constexpr int S2_OC0 = 18;                                    // 16 odd input columns at LDS columns 18 .. 33
constexpr int S2_PITCH = 36;                                  // LDS pixels per input row: a multiple of 4, so the chunk swizzle of
                                                              // pixel (r, col) is (r & 1) ^ ((col >> 2) & 1): separable
constexpr int S2_NPX = S2_IR * S2_PITCH;                      // 612
constexpr int S2_XPW = (S2_NPX + 16 * S2_NW - 1) / (16 * S2_NW);   // 10 DMA pieces (16 pixels x 64 B) per wave per channel step
constexpr int S2_XBUF = S2_XPW * S2_NW * FRAG;                // 40 KiB
constexpr int S2_LDS = 2 * S2_XBUF;                           // 80 KiB: two workgroups per CU
constexpr int S2_PART = 128, S2_NT = 8;                       // output channels / 16-channel row tiles per workgroup
constexpr int S2_TW = 4, S2_QW = 4;                           // row tiles, pixel segments per wave

struct S2 {
  const char* x;        // [B][H][W][Cin]
  const char* w;        // sta_conv3x3_pack_w image (128-channel parts)
  const char* zeros;    // >= 2 * Cin bytes of zeros
  void* out;            // [B][H / 2][W / 2][Cout]
  const void* bias;     // [Cout] or null
  float* stats;         // null, or [B + 1][stats_slots][Cout][2]
  int B, H, W, Cin, Cout, Ho, Wo, parts, tiles_x, tiles_per_img, stats_slots;
};

// LDS byte offset of channel chunk g of the pixel at column col of an even input row (odd rows: bit 5 flipped; the chunk swizzle of
// sta_conv.hip: chunk g of LDS pixel P sits at slot g ^ 2 ((P >> 2) & 1))
__device__ __forceinline__ unsigned col_off(int col, int g) { return (unsigned)(col * 64 + ((g ^ (((col >> 2) & 1) << 1)) << 4)); }

template <typename T>
__global__ __launch_bounds__(64 * S2_NW, 2) void conv3x3_s2_nhwc_kernel(const S2 p) {
  using V8 = typename Tr<T>::V8;
  using V4 = typename Tr<T>::V4;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int ph = wv & 1, chh = wv >> 1;                    // output rows 4 ph .. + 3 of the tile, row tiles 4 chh .. + 3 of the part
  const int part = blockIdx.x % p.parts, tile = blockIdx.x / p.parts;
  const int b = tile / p.tiles_per_img, tt = tile - b * p.tiles_per_img;
  const int ty = tt / p.tiles_x, tx = tt - ty * p.tiles_x;
  const int nkc = p.Cin >> 5;
  const int y0 = 2 * S2_TR * ty, x0 = 2 * S2_TC * tx;      // first input row / column of the footprint

  // this wave's DMA pieces wv, wv + 4, ...: lane -> tile pixel 16 pc + (lane >> 2), LDS slot lane & 3 (source chunk slot ^ swizzle)
  const char* xp[S2_XPW];
#pragma unroll
  for (int i = 0; i < S2_XPW; ++i) {
    const int pp = 16 * (wv + S2_NW * i) + (lane >> 2);
    const int chunk = (lane & 3) ^ (((pp >> 2) & 1) << 1);
    const int r = pp / S2_PITCH, j = pp - r * S2_PITCH;
    const bool col_ok = j < S2_EC || (j >= S2_OC0 && j < S2_OC0 + S2_TC);
    const int y = y0 + r, x = x0 + (j < S2_EC ? 2 * j : 2 * (j - S2_OC0) + 1);
    const bool ok = pp < S2_NPX && col_ok && y < p.H && x < p.W;
    xp[i] = ok ? p.x + (((size_t)b * p.H + y) * p.W + x) * (size_t)p.Cin * sizeof(T) + chunk * 16 : p.zeros + chunk * 16;
  }
  auto stage_x = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < S2_XPW; ++i) {
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)xp[i],
                                       (__attribute__((address_space(3))) void*)(smem + buf * S2_XBUF + (wv + S2_NW * i) * FRAG), 16, 0, 0);
      xp[i] += 64;                                         // next 32-channel step (the zero page is 2 Cin bytes long)
    }
  };
  // A operands of kernel row ky at channel step kc: fragment (((part nkc + kc) 3 + ky) 3 + kx) 8 + t, this lane's 16 bytes
  const char* wbase = p.w + (size_t)part * nkc * 9 * S2_NT * FRAG + (size_t)(S2_TW * chh) * FRAG + lane * 16;
  auto load_row = [&](V8 (&a)[3][S2_TW], int kc, int ky) __attribute__((always_inline)) {
    const char* src = wbase + (size_t)((kc * 3 + ky) * 3) * S2_NT * FRAG;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int t = 0; t < S2_TW; ++t) a[kx][t] = *(const V8*)(src + (kx * S2_NT + t) * FRAG);
  };

  f32x4 acc[S2_QW][S2_TW];
#pragma unroll
  for (int q = 0; q < S2_QW; ++q)
#pragma unroll
    for (int t = 0; t < S2_TW; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's B operand (pixel c16 of a segment, chunk g) at tap kx: even plane from column 0 / odd plane / even plane from column 1
  const unsigned boff[3] = {col_off(c16, g), col_off(S2_OC0 + c16, g), col_off(c16 + 1, g)};

  V8 a[3][S2_TW];
  stage_x(0);
  load_row(a, 0, 0);
  for (int kc = 0; kc < nkc; ++kc) {
    __builtin_amdgcn_s_waitcnt(0);                         // this wave's DMA of step kc has landed ...
    __syncthreads();                                       // ... and every wave's; every wave is done reading the other buffer
    const char* xb = smem + (kc & 1) * S2_XBUF + 8 * ph * S2_PITCH * 64;   // this wave's first input row
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      // the next kernel row's A operands (after the last row: row 0 of the last step again, never used), then — behind the first of
      // them, so that waiting for kernel row 1 does not wait for it — the next step's input tile
      V8 an[3][S2_TW];
      load_row(an, ky < 2 ? kc : (kc + 1 < nkc ? kc + 1 : kc), ky < 2 ? ky + 1 : 0);
      if (ky == 0 && kc + 1 < nkc) stage_x((kc + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        V8 bq[S2_QW];
#pragma unroll
        for (int q = 0; q < S2_QW; ++q)                    // input row 8 ph + 2 q + ky of the tile: output row 4 ph + q at this tap
          bq[q] = *(const V8*)(xb + (2 * q + ky) * S2_PITCH * 64 + ((ky & 1) ? boff[kx] ^ 32u : boff[kx]));
#pragma unroll
        for (int t = 0; t < S2_TW; ++t)
#pragma unroll
          for (int q = 0; q < S2_QW; ++q) acc[q][t] = Tr<T>::mfma(a[kx][t], bq[q], acc[q][t]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int t = 0; t < S2_TW; ++t) a[kx][t] = an[kx][t];
    }
  }

  // epilogue: lane (g, c) of tile t holds output channels 16 t + 4 g .. + 3 of pixel c of the segment
  const int ch0 = part * S2_PART + 16 * S2_TW * chh + 4 * g;
  float bs[S2_TW][4];
#pragma unroll
  for (int t = 0; t < S2_TW; ++t) {
    V4 bv = {};
    if (p.bias) bv = *(const V4*)((const T*)p.bias + ch0 + 16 * t);
#pragma unroll
    for (int r = 0; r < 4; ++r) bs[t][r] = (float)bv[r];
  }
  float ssum[S2_TW][4], ssq[S2_TW][4];
#pragma unroll
  for (int t = 0; t < S2_TW; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) { ssum[t][r] = 0.f; ssq[t][r] = 0.f; }
#pragma unroll
  for (int q = 0; q < S2_QW; ++q) {
    const int oy = S2_TR * ty + 4 * ph + q, ox = S2_TC * tx + c16;
    T* dst = (T*)p.out + (((size_t)b * p.Ho + oy) * p.Wo + ox) * p.Cout + ch0;
#pragma unroll
    for (int t = 0; t < S2_TW; ++t) {
      V4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (T)(acc[q][t][r] + bs[t][r]);
      *(V4*)(dst + 16 * t) = o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = (float)o[r];
        ssum[t][r] += v;
        ssq[t][r] += v * v;
      }
    }
  }
  if (p.stats) {                                           // slot (tile of the image, pixel half): plain stores, no atomics
    float* dst = p.stats + (((size_t)b * p.stats_slots + 2 * tt + ph) * p.Cout + ch0) * 2;
#pragma unroll
    for (int t = 0; t < S2_TW; ++t) {
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

// ------------------------------------------------------------------------------------------------ encoder output -> first UNet input
template <typename T>
__global__ __launch_bounds__(256) void vae_encode_step_kernel(const T* __restrict__ h, const float* __restrict__ qw, const float* __restrict__ qb,
                                                              const float* __restrict__ n_post, const float* __restrict__ n_enc,
                                                              float* __restrict__ x, float* __restrict__ z0, T* __restrict__ xin, long npx,
                                                              long hw, float scale_factor, float sqrt_a, float sqrt_1ma) {
  using V8 = typename V8T<T>::type;
  QuantConv q;
  quant_conv_load(q, qw, qb);
  const long stride = (long)gridDim.x * 256;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < npx; v += stride) {
    const long img = v / hw, pix = v - img * hw;
    float mo[8];
    quant_moments<T>(q, ((const V8*)h)[v], mo);            // the 8 channels of one NHWC pixel: one 16-byte load
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long idx = (img * 4 + c) * hw + pix;
      float zz;
      const float xx = encode1(mo[c], mo[4 + c], n_post[idx], n_enc[idx], scale_factor, sqrt_a, sqrt_1ma, zz);
      x[idx] = xx;
      if (z0) z0[idx] = zz;
      if (xin) {
        xin[((2 * img) * 4 + c) * hw + pix] = (T)xx;
        xin[((2 * img + 1) * 4 + c) * hw + pix] = (T)xx;
      }
    }
  }
}

}  // namespace

extern "C" {

int sta_conv3x3_s2_nhwc_supported(int B, int H, int W, int Cin, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || H % (2 * S2_TR) || W % (2 * S2_TC)) return 0;
  // the weight image of sta_conv3x3_pack_w in 128-channel parts (Cout % 160 == 0 packs 160-channel parts)
  // Downsample keeps the channel count: Cin == Cout, in 128-channel parts of sta_conv3x3_pack_w's image (Cout % 160 == 0 packs 160-channel
  // parts); the SD-v1 encoder's 128 / 256 / 512 (faster than F.pad + the library convolution at all of them: profiles/img2img_throughput.json)
  if (Cin != Cout || Cin <= 0 || Cin % S2_PART || Cin % 160 == 0) return 0;
  if ((size_t)B * H * W * (size_t)Cin * 2 >= 0xfffffff0ull) return 0;
  if ((size_t)B * (H / 2) * (W / 2) * (size_t)(Cout / S2_PART) / (S2_TR * S2_TC) >= (1ull << 31)) return 0;
  return 1;
}

int sta_conv3x3_s2_stats_slots(int H, int W) {
  if (H <= 0 || W <= 0 || H % (2 * S2_TR) || W % (2 * S2_TC)) return 0;
  return 2 * (H / (2 * S2_TR)) * (W / (2 * S2_TC));
}

int sta_conv3x3_s2_nhwc(const void* x, const void* packed_w, const void* zeros, const void* bias, void* out, float* stats, int B, int H, int W,
                        int Cin, int Cout, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!x || !packed_w || !zeros || !out) return sta_fail(STA_E_ARG, "null pointer");
  if (!sta_conv3x3_s2_nhwc_supported(B, H, W, Cin, Cout))
    return sta_fail(STA_E_UNSUP, "conv3x3_s2_nhwc: unsupported geometry B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W, Cin, Cout);
  S2 p{(const char*)x, (const char*)packed_w, (const char*)zeros, out, bias, stats, B, H, W, Cin, Cout, H / 2, W / 2, Cout / S2_PART,
       (W / 2) / S2_TC, 0, 0};
  p.tiles_per_img = ((H / 2) / S2_TR) * p.tiles_x;
  p.stats_slots = 2 * p.tiles_per_img;
  const unsigned grid = (unsigned)((long)B * p.tiles_per_img * p.parts);
  return sta_by_dtype(dtype, [&](auto tag) {
    return sta_launch_lds<conv3x3_s2_nhwc_kernel<decltype(tag)>>("conv3x3_s2_nhwc", S2_LDS, dim3(grid), dim3(64 * S2_NW), S2_LDS,
                                                                 (hipStream_t)stream, p);
  });
}

int sta_vae_encode_step(const void* h, const float* quant_w, const float* quant_b, const float* n_post, const float* n_enc, float* x, float* z0,
                        void* xin, long B, long hw, float scale_factor, float sqrt_a, float sqrt_1ma, int dtype, void* stream) {
  g_sta_err[0] = 0;
  if (!h || !quant_w || !quant_b || !n_post || !n_enc || !x) return sta_fail(STA_E_ARG, "null pointer");
  if (B <= 0 || hw <= 0) return sta_fail(STA_E_ARG, "vae_encode_step: B=%ld hw=%ld", B, hw);
  if (((uintptr_t)h & 15) != 0) return sta_fail(STA_E_ARG, "vae_encode_step: h must be 16-byte aligned");
  const long npx = B * hw;
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<vae_encode_step_kernel<T>>("vae_encode_step", dim3(sta_grid_for(npx)), dim3(256), 0, (hipStream_t)stream, (const T*)h, quant_w,
                                                 quant_b, n_post, n_enc, x, z0, (T*)xin, npx, hw, scale_factor, sqrt_a, sqrt_1ma);
  });
}

}  // extern "C"
