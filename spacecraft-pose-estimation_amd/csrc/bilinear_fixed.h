// The project's one definition of "OpenCV-style bilinear" for uint8 images (3.4 imgwarp.cpp: remapBilinear with
// FixedPtCast<int, uchar, 15>): a source position in 1/32 px (INTER_BITS = 5) splits into the pixel (X >> 5, saturated
// to int16 as OpenCV stores it) and the 5-bit fraction X & 31; the four integer weights (32-a)(32-b)*32 ... a*b*32 sum to
// 2^15; the pixel is (sum of taps * weights + 2^14) >> 15.  How a kernel arrives at the 1/32-px coordinates is its own
// business (affine_source below, for crop.hip and crop_tail.h: an affine map in 1/1024 px; events.hip: a float64 distortion map); the tap is shared.
// utils/transforms.py:warp_affine_bilinear is the NumPy restatement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace scpose {

// cv::saturate_cast<int>(double): cvRound (to nearest even) + clamp to int32
__device__ __forceinline__ long long sat_round_int32(double v) {
  v = rint(v);
  return (long long)(v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v));
}

// cv::saturate_cast<short> of a pixel index
__device__ __forceinline__ long long sat_int16(long long v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// cv::warpAffine's source position of output pixel (x, y) under the inverse map m[6] (3.4 imgwarp.cpp: WarpAffineInvoker): the
// map in 1/1024 px, the two roundings kept apart, then 1/32 px; the pixel (x0, y0) of the first tap and the fractions (a, b).
// crop.hip and crop_tail.h sample at exactly these positions.
struct AffineSource {
  long long x0, y0;
  int a, b;
};
__device__ __forceinline__ AffineSource affine_source(const double* __restrict__ m, int x, int y) {
#pragma clang fp contract(off)
  const double xs = (double)x, ys = (double)y;
  const long long X = (sat_round_int32((m[1] * ys + m[2]) * 1024.0) + 16 + sat_round_int32(m[0] * xs * 1024.0)) >> 5;
  const long long Y = (sat_round_int32((m[4] * ys + m[5]) * 1024.0) + 16 + sat_round_int32(m[3] * xs * 1024.0)) >> 5;
  return {sat_int16(X >> 5), sat_int16(Y >> 5), (int)(X & 31), (int)(Y & 31)};
}

struct BilinearTap {
  int w00, w01, w10, w11;
  // a, b: the 5-bit fractions (X & 31, Y & 31) of the source position
  __device__ __forceinline__ BilinearTap(int a, int b)
      : w00((32 - a) * (32 - b) * 32), w01(a * (32 - b) * 32), w10((32 - a) * b * 32), w11(a * b * 32) {}
  // s00 = source(y0, x0), s01 = source(y0, x0 + 1), s10 = source(y0 + 1, x0), s11 = source(y0 + 1, x0 + 1); taps outside the image are 0
  __device__ __forceinline__ uint8_t operator()(int s00, int s01, int s10, int s11) const {
    const int v = (s00 * w00 + s01 * w01 + s10 * w10 + s11 * w11 + 16384) >> 15;
    return (uint8_t)(v > 255 ? 255 : v);
  }
};

}  // namespace scpose
