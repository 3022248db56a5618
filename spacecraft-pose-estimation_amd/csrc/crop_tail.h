// The crop tail of the image decoders: crop_warp_kernel (crop.hip) of a frame that is never written.  jpeg_decode.hip and
// png_decode.hip each end in a kernel that takes crop.hip's source position and bilinear tap (bilinear_fixed.h) and fetches every tap
// from what the decoder holds -- sample planes, or an unfiltered plane and a palette.  Shared: the windows, the predicate, the body.
#pragma once
#include "bilinear_fixed.h"

namespace scpose {

// The windows of up to kRoiChunk images travel in the kernel arguments: the host has them (api.cpp checks each against the frame),
// and the workspace keeps the size scpose_*_decode_workspace_bytes() states.  Image img0 + blockIdx.y has rois.v[blockIdx.y].
constexpr int kRoiChunk = 128;
struct RoiChunk { int32_t v[kRoiChunk][4]; };      // x, y, w, h
// roi_host: host int32 [n][4].  launch(rois, img0, count) once per chunk, in order.
template <class Launch>
inline void for_each_roi_chunk(const int32_t* roi_host, int n, Launch&& launch) {
  for (int img0 = 0; img0 < n; img0 += kRoiChunk) {
    const int count = n - img0 < kRoiChunk ? n - img0 : kRoiChunk;
    RoiChunk rois{};
    memcpy(rois.v, roi_host + (size_t)img0 * 4, (size_t)count * 4 * sizeof(int32_t));
    launch(rois, img0, count);
  }
}

constexpr int kCropThreads = 256;        // the workgroup of a kernel that calls crop_tail; its grid for `count` images:
inline dim3 crop_tail_grid(int oh, int ow, int count) {
  const int64_t groups = ((int64_t)oh * ow + kCropThreads - 1) / kCropThreads;
  return dim3((unsigned)(groups < 4096 ? groups : 4096), (unsigned)count);
}

// A tap counts when it lies inside the h x w frame (BORDER_CONSTANT: 0 outside) and inside the image's window (rx, ry, rw, rh): the window bounds
// what is in memory -- the stored part of the frame, the transformed blocks, the unfiltered rows.
__device__ __forceinline__ bool in_window(long long xx, long long yy, int h, int w, int rx, int ry, int rw, int rh) {
  return yy >= 0 && yy < h && xx >= 0 && xx < w && yy >= ry && yy < ry + rh && xx >= rx && xx < rx + rw;
}
struct Rgb { int32_t r, g, b; };

// One image's crop, oh x ow x 3 at `out`, by the workgroups blockIdx.x of the grid: px(x, y) -> Rgb is pixel (x, y) of the h x w
// frame, asked only where in_window holds; m: the image's inverse map.  gray: r == g == b for every pixel, one blend serves all three.
template <class PixelAt>
__device__ __forceinline__ void crop_tail(PixelAt px, int h, int w, bool gray, int bgr, const double* __restrict__ m, const int32_t* roi,
                                          int oh, int ow, uint8_t* __restrict__ out) {
  const int32_t rx = roi[0], ry = roi[1], rw = roi[2], rh = roi[3];
  const int64_t total = (int64_t)oh * ow;
  for (int64_t pix = (int64_t)blockIdx.x * kCropThreads + threadIdx.x; pix < total; pix += (int64_t)gridDim.x * kCropThreads) {
    const AffineSource p = affine_source(m, (int)(pix % ow), (int)(pix / ow));
    const BilinearTap bil(p.a, p.b);
    Rgb t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long yy = p.y0 + (j >> 1), xx = p.x0 + (j & 1);
      t[j] = in_window(xx, yy, h, w, rx, ry, rw, rh) ? px((int32_t)xx, (int32_t)yy) : Rgb{0, 0, 0};
    }
    const uint8_t r = bil(t[0].r, t[1].r, t[2].r, t[3].r);
    const uint8_t g = gray ? r : bil(t[0].g, t[1].g, t[2].g, t[3].g), b = gray ? r : bil(t[0].b, t[1].b, t[2].b, t[3].b);
    out[pix * 3] = bgr ? b : r;
    out[pix * 3 + 1] = g;
    out[pix * 3 + 2] = bgr ? r : b;
  }
}

}  // namespace scpose
