// sta_clip.hip — the image front end of the CLIP fidelity loss (gfx950): from the clamped decoder output straight to the
// ViT-B/32 patch rows, and back. C-ABI in include/sta_unet.h (sta_clip_views / sta_clip_views_bwd).
//
// A view is a 224 x 224 image that is never stored: the forward writes it as [49][3072] patch rows ((c, dy, dx) columns, the
// column order of visual.conv1.weight.view(width, 3072)), the backward reads the gradient of those rows.
//   global view (box = whole image):  AvgPool2d(p)(Upsample(x7 nearest)(x)), p = 7 H / 224 = H / 32. Output pixel Y covers the
//     upsampled rows [Y p, Y p + p), source row r covers [7 r, 7 r + 7): the weight of r in Y is the length of the overlap, an
//     integer, and the pixel is sum(wy wx x) / p^2 over at most (ceil(p / 7) + 1)^2 source pixels. No 7H x 7W intermediate.
//   crop view: bilinear resize of x[:, y1:y2, x1:x2] to 224^2, align_corners = False, source index clamped inside the box.
// Forward: one lane per 8 consecutive output columns of one patch row (one 16-byte store; a wave writes 1 KiB contiguous).
// Backward: a gather with one lane per source pixel (all three channels: the index arithmetic is shared), which sums the few
// output pixels the source pixel feeds, over the views of its image. dimg is written exactly once per element: no memset, no
// atomics, the same bits on every run. All arithmetic in fp32.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sta_xattn.h"
#include "sta_unet.h"
#include "sta_internal.h"

namespace {

constexpr int VIEW = 224;            // side of a view
constexpr int PATCH = 32;            // ViT-B/32
constexpr int GRID = VIEW / PATCH;   // 7 patches per side
constexpr int ROWS = GRID * GRID;    // 49 patch rows per view
constexpr int COLS = 3 * PATCH * PATCH;   // 3072
constexpr long VIEW_ELEMS = (long)ROWS * COLS;

struct Box {
  int img, y1, y2, x1, x2;
};

// The table is validated on the host before every launch; the clamp here only makes sure that a table that changed on the
// device afterwards cannot send a load outside `img`.
__device__ __forceinline__ Box load_box(const int* __restrict__ boxes, int v, int H, int W) {
  Box b;
  b.img = boxes[5 * v];
  b.y1 = min(max(boxes[5 * v + 1], 0), H - 2);
  b.y2 = min(max(boxes[5 * v + 2], b.y1 + 2), H);
  b.x1 = min(max(boxes[5 * v + 3], 0), W - 2);
  b.x2 = min(max(boxes[5 * v + 4], b.x1 + 2), W);
  return b;
}

__device__ __forceinline__ bool is_global(const Box& b, int H, int W) { return b.y1 == 0 && b.y2 == H && b.x1 == 0 && b.x2 == W; }

// bilinear source of output index o for a source extent n: rows i0, i1 (inside [0, n)) and the weight l of i1
__device__ __forceinline__ void bilinear_src(int o, int n, float scale, int& i0, int& i1, float& l) {
  float f = scale * ((float)o + 0.5f) - 0.5f;
  f = f < 0.f ? 0.f : f;
  i0 = min((int)f, n - 1);
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  l = f - (float)i0;
}

// the weight of source index s in output index o (0 almost everywhere)
__device__ __forceinline__ float bilinear_weight(int o, int s, int n, float scale) {
  int i0, i1;
  float l;
  bilinear_src(o, n, scale, i0, i1, l);
  return (i0 == s ? 1.f - l : 0.f) + (i1 == s ? l : 0.f);
}

// length of [7 s, 7 s + 7) n [o p, o p + p)
__device__ __forceinline__ int pool_weight(int o, int s, int p) { return min(7 * s + 7, o * p + p) - max(7 * s, o * p); }

template <typename T>
__global__ __launch_bounds__(256) void clip_views_kernel(const float* __restrict__ img, const int* __restrict__ boxes,
                                                         T* __restrict__ out, int B, int H, int W, int p) {
  using V8 = typename V8T<T>::type;
  const int v = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;      // which 8 elements of the view's [49][3072]
  if (t >= ROWS * (COLS / 8)) return;
  const Box bx = load_box(boxes, v, H, W);
  if ((unsigned)bx.img >= (unsigned)B) return;
  const int row = t / (COLS / 8), col8 = t - row * (COLS / 8);
  const int c = col8 >> 7, dy = (col8 & 127) >> 2, dx0 = (col8 & 3) * 8;
  const int Y = (row / GRID) * PATCH + dy, X0 = (row % GRID) * PATCH + dx0;
  const float* __restrict__ src = img + ((long)bx.img * 3 + c) * H * W;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (is_global(bx, H, W)) {
    const int r0 = (Y * p) / 7, r1 = (Y * p + p - 1) / 7;
    for (int r = r0; r <= r1; ++r) {
      const float wy = (float)pool_weight(Y, r, p);
      const float* __restrict__ line = src + (long)r * W;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int X = X0 + j, c0 = (X * p) / 7, c1 = (X * p + p - 1) / 7;
        float h = 0.f;
        for (int cc = c0; cc <= c1; ++cc) h += (float)pool_weight(X, cc, p) * line[cc];
        acc[j] += wy * h;
      }
    }
    const float area = (float)(p * p);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] / area;
  } else {
    const int h = bx.y2 - bx.y1, w = bx.x2 - bx.x1;
    const float sy = (float)h / (float)VIEW, sx = (float)w / (float)VIEW;
    int y0, y1;
    float ly;
    bilinear_src(Y, h, sy, y0, y1, ly);
    const float* __restrict__ la = src + (long)(bx.y1 + y0) * W + bx.x1;
    const float* __restrict__ lb = src + (long)(bx.y1 + y1) * W + bx.x1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int x0, x1;
      float lx;
      bilinear_src(X0 + j, w, sx, x0, x1, lx);
      acc[j] = (1.f - ly) * ((1.f - lx) * la[x0] + lx * la[x1]) + ly * ((1.f - lx) * lb[x0] + lx * lb[x1]);
    }
  }
  V8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (T)acc[j];
  ((V8*)(out + (long)v * VIEW_ELEMS))[t] = o;
}

__device__ __forceinline__ long patch_offset(int Y, int X) {
  return (long)((Y >> 5) * GRID + (X >> 5)) * COLS + (Y & 31) * PATCH + (X & 31);
}

// grid (H W / 256, B): a block lies inside one image, so the image and its range of views are wave-uniform.
template <typename T>
__global__ __launch_bounds__(256) void clip_views_bwd_kernel(const T* __restrict__ dout, const int* __restrict__ boxes,
                                                             float* __restrict__ dimg, int H, int W, int n_views, int p) {
  const int b = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= H * W) return;
  const int r = pix / W, cx = pix - r * W;
  // boxes are grouped by image (checked on the host): first view with image >= b by bisection
  int lo = 0, hi = n_views;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (boxes[5 * mid] < b) lo = mid + 1; else hi = mid;
  }
  float g[3] = {0.f, 0.f, 0.f};
  for (int v = lo; v < n_views && boxes[5 * v] == b; ++v) {
    const Box bx = load_box(boxes, v, H, W);
    const T* __restrict__ d = dout + (long)v * VIEW_ELEMS;
    if (is_global(bx, H, W)) {
      const int Ya = (7 * r) / p, Yb = min((7 * r + 6) / p, VIEW - 1);
      const int Xa = (7 * cx) / p, Xb = min((7 * cx + 6) / p, VIEW - 1);
      float s[3] = {0.f, 0.f, 0.f};
      for (int Y = Ya; Y <= Yb; ++Y) {
        const int wy = pool_weight(Y, r, p);
        for (int X = Xa; X <= Xb; ++X) {
          const float wgt = (float)(wy * pool_weight(X, cx, p));
          const long off = patch_offset(Y, X);
#pragma unroll
          for (int c = 0; c < 3; ++c) s[c] += wgt * (float)d[off + c * (PATCH * PATCH)];
        }
      }
      const float area = (float)(p * p);
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] += s[c] / area;
    } else {
      if (r < bx.y1 || r >= bx.y2 || cx < bx.x1 || cx >= bx.x2) continue;
      const int h = bx.y2 - bx.y1, w = bx.x2 - bx.x1, rr = r - bx.y1, rc = cx - bx.x1;
      const float sy = (float)h / (float)VIEW, sx = (float)w / (float)VIEW;
      // an output index o reads source s when its source coordinate lies in [s - 1, s + 1); one index of slack on both sides
      const int Ya = max((int)floorf(((float)rr - 0.5f) / sy - 0.5f) - 1, 0);
      const int Yb = min((int)ceilf(((float)rr + 1.5f) / sy - 0.5f) + 1, VIEW - 1);
      const int Xa = max((int)floorf(((float)rc - 0.5f) / sx - 0.5f) - 1, 0);
      const int Xb = min((int)ceilf(((float)rc + 1.5f) / sx - 0.5f) + 1, VIEW - 1);
      for (int Y = Ya; Y <= Yb; ++Y) {
        const float wy = bilinear_weight(Y, rr, h, sy);
        if (wy == 0.f) continue;
        for (int X = Xa; X <= Xb; ++X) {
          const float wx = bilinear_weight(X, rc, w, sx);
          if (wx == 0.f) continue;
          const long off = patch_offset(Y, X);
#pragma unroll
          for (int c = 0; c < 3; ++c) g[c] += wy * wx * (float)d[off + c * (PATCH * PATCH)];
        }
      }
    }
  }
  float* __restrict__ o = dimg + (long)b * 3 * H * W + pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(long)c * H * W] = g[c];
}

// The shape rules of both entry points (include/sta_unet.h). `grouped`: the backward also needs the views of an image adjacent.
int check_views(const char* what, const int* boxes_host, int B, int H, int W, int n_views, int dtype, bool grouped) {
  if (B <= 0 || n_views <= 0) return sta_fail(STA_E_ARG, "%s: B=%d n_views=%d", what, B, n_views);
  if (H != W || H % 32 || H < 256 || H > 1024)
    return sta_fail(STA_E_UNSUP, "%s: image %dx%d (need H == W, a multiple of 32, 256 <= H <= 1024)", what, H, W);
  if ((long)n_views * VIEW_ELEMS >= (1L << 31)) return sta_fail(STA_E_UNSUP, "%s: %d views: the patch rows pass 2^31 elements", what, n_views);
  if (dtype != STA_BF16 && dtype != STA_F16) return sta_fail(STA_E_UNSUP, "%s: dtype %d", what, dtype);
  for (int v = 0; v < n_views; ++v) {
    const int* q = boxes_host + 5 * v;
    if (q[0] < 0 || q[0] >= B) return sta_fail(STA_E_ARG, "%s: view %d names image %d of %d", what, v, q[0], B);
    if (q[1] < 0 || q[2] > H || q[3] < 0 || q[4] > W || q[2] - q[1] < 2 || q[4] - q[3] < 2)
      return sta_fail(STA_E_ARG, "%s: view %d box [%d:%d, %d:%d] (need at least 2x2 inside %dx%d)", what, v, q[1], q[2], q[3], q[4], H, W);
    if (grouped && v && q[0] < q[-5]) return sta_fail(STA_E_ARG, "%s: view %d: boxes must be grouped by image, in image order", what, v);
  }
  return 0;
}

}  // namespace

extern "C" {

int sta_clip_views(const float* img, const int* boxes, const int* boxes_host, void* out, int B, int H, int W, int n_views, int out_dtype,
                   void* stream) {
  g_sta_err[0] = 0;
  if (!img || !boxes || !boxes_host || !out) return sta_fail(STA_E_ARG, "null pointer");
  if (((uintptr_t)out & 15) != 0) return sta_fail(STA_E_ARG, "clip_views: out must be 16-byte aligned");
  if (const int rc = check_views("clip_views", boxes_host, B, H, W, n_views, out_dtype, false)) return rc;
  const dim3 grid((ROWS * (COLS / 8) + 255) / 256, n_views);
  return sta_by_dtype(out_dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<clip_views_kernel<T>>("clip_views", grid, dim3(256), 0, (hipStream_t)stream, img, boxes, (T*)out, B, H, W, H / 32);
  });
}

int sta_clip_views_bwd(const void* dout, const int* boxes, const int* boxes_host, float* dimg, int B, int H, int W, int n_views, int dtype,
                       void* stream) {
  g_sta_err[0] = 0;
  if (!dout || !boxes || !boxes_host || !dimg) return sta_fail(STA_E_ARG, "null pointer");
  if (const int rc = check_views("clip_views_bwd", boxes_host, B, H, W, n_views, dtype, true)) return rc;
  const dim3 grid(H * W / 256, B);
  return sta_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return sta_launch<clip_views_bwd_kernel<T>>("clip_views_bwd", grid, dim3(256), 0, (hipStream_t)stream, (const T*)dout, boxes, dimg, H, W,
                                                n_views, H / 32);
  });
}

}  // extern "C"
