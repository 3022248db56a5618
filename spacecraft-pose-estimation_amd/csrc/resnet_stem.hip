// ResNet stem for gfx950, one kernel: Conv2d(3 -> 64, 7x7, stride 2, padding 3) + folded BN + ReLU + MaxPool2d(3, stride 2, padding 1)
// (pose_resnet's conv1 / bn1 / relu / maxpool): uint8 NHWC or float32 NCHW input -> blocked 16-bit 64 x H/4 x W/4.  The
// 64 x H/2 x W/2 convolution result never reaches HBM.
//
// One 256-thread workgroup per tile of 4 x 8 pooled pixels:
//   stage  the 23 x 39 x 3 input patch as normalised 16-bit values in LDS -- uint8 through a 3 x 256 table of
//          ((u / 255 - mean) / std) rounded to the 16-bit type, float32 rounded -- exactly the operand stem_fused.hip forms for
//          its first layer, so "x" means the same thing in both stems; pixels outside the image are 0 (the convolution's padding);
//   conv   the 9 x 17 convolution pixels under the tile's pool windows, as an implicit GEMM on v_mfma_f32_16x16x32: M = 64 output
//          channels (4 tiles), N = 153 pixels (10 tiles of 16, shared among the 4 waves), K = 147 = (7 x 7 taps) x 3 channels padded
//          to 160 = 5 k-steps (the padding slots read a zero word; their weights are zero too), f32 accumulation.  The weights
//          (20 A fragments) stay in registers.  + bias, ReLU, ONE rounding to the 16-bit type, into LDS;
//   pool   thread (pooled pixel, 8-channel plane) takes the maximum of its 3 x 3 window and stores one 16-byte vector.
// The pool runs on the rounded values: rounding is monotone, so max(round(v)) == round(max(v)) and the f32 value is never stored.
// A window that hangs over the map's border ignores the missing positions (MaxPool2d pads with -inf, not with zeros): convolution
// pixels outside the H/2 x W/2 map are written as -inf.  Behind the ReLU every real value is >= 0 and every window contains its
// centre, so zeros would give the same maximum; -inf is what the module does and costs nothing.
#include "common.h"
#include "conv_device.h"

namespace scpose {

namespace {
constexpr int kPH = 4, kPW = 8;                    // pooled tile
constexpr int kCH = 2 * kPH + 1, kCW = 2 * kPW + 1;  // convolution pixels under it: 9 x 17
constexpr int kIH = 2 * (kCH - 1) + 7, kIW = 2 * (kCW - 1) + 7;   // input patch: 23 x 39
constexpr int kCPix = kCH * kCW;                   // 153
constexpr int kPTiles = (kCPix + 15) / 16;         // 10
constexpr int kInElems = 3 * kIH * kIW;            // 2691; element kInElems is the zero word of the K padding
constexpr int kK = 147, kKSteps = 5;
}

struct ResnetStemLaunch {
  const void* in;
  const void* w;          // [4 Cout tiles][5 k-steps][64 lanes][8] 16-bit A fragments
  const float* bias;      // [64], natural order
  const float* mean_std;  // [6] (uint8 input)
  void* out;
  int32_t N, H, W, Hc, Wc, Hp, Wp, tiles_x, tiles_y;
};

template <int DT, int FMT>
__global__ __launch_bounds__(256) void resnet_stem_kernel(const ResnetStemLaunch p) {
  typedef typename DtOf<DT>::type T;
  typedef typename FragOf<T>::type Frag;
  __shared__ __attribute__((aligned(16))) uint16_t in16[kInElems + 5];
  __shared__ __attribute__((aligned(16))) uint16_t conv16[8 * kPTiles * 16 * 8];   // [plane][pixel slot][8]
  __shared__ uint16_t lut[768];
  __shared__ uint16_t koff[kKSteps * 32];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tiles_img = p.tiles_x * p.tiles_y;
  const int n = blockIdx.x / tiles_img, tr = blockIdx.x - n * tiles_img;
  const int py0 = (tr / p.tiles_x) * kPH, px0 = (tr % p.tiles_x) * kPW;
  const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;      // first convolution pixel of the tile (may be -1)
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;      // first input pixel of the patch

  if constexpr (FMT == SCPOSE_IN_U8_NHWC) {
    // ToTensor: u/255 ; Normalize: (t - mean)/std (torchvision's op order), rounded once to the 16-bit operand type
    for (int e = tid; e < 768; e += 256) {
      const int c = e >> 8;
      lut[e] = to_bits<T>(((float)(e & 255) / 255.0f - p.mean_std[c]) / p.mean_std[3 + c]);
    }
  }
  for (int k = tid; k < kKSteps * 32; k += 256) {   // k = (ky * 7 + kx) * 3 + c -> offset inside the patch
    const int tap = k / 3, c = k - 3 * tap, ky = tap / 7, kx = tap - 7 * ky;
    koff[k] = (uint16_t)(k < kK ? c * (kIH * kIW) + ky * kIW + kx : 0);
  }
  if (tid < 5) in16[kInElems + tid] = 0;
  if constexpr (FMT == SCPOSE_IN_U8_NHWC) __syncthreads();
  for (int e = tid; e < kInElems; e += 256) {
    const int c = e / (kIH * kIW), r = e - c * (kIH * kIW), y = r / kIW, x = r - y * kIW;
    const int gy = iy0 + y, gx = ix0 + x;
    uint16_t v = 0;
    if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
      if constexpr (FMT == SCPOSE_IN_U8_NHWC)
        v = lut[c * 256 + static_cast<const uint8_t*>(p.in)[(((size_t)n * p.H + gy) * p.W + gx) * 3 + c]];
      else
        v = to_bits<T>(static_cast<const float*>(p.in)[(((size_t)n * 3 + c) * p.H + gy) * p.W + gx]);
    }
    in16[e] = v;
  }

  // weights: 4 Cout tiles x 5 k-steps of A fragments, in registers for the whole tile
  uint4 a[4][kKSteps];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < kKSteps; ++s) a[r][s] = static_cast<const uint4*>(p.w)[(r * kKSteps + s) * 64 + lane];
  __syncthreads();

  const int q = lane >> 4;
  const uint16_t ninf = DT == 0 ? 0xff80u : 0xfc00u;   // -inf in bf16 / f16
  for (int pt = wv; pt < kPTiles; pt += 4) {
    const int pix = pt * 16 + (lane & 15);
    const bool real = pix < kCPix;
    const int cyl = real ? pix / kCW : 0, cxl = real ? pix - (pix / kCW) * kCW : 0;
    const int base = 2 * cyl * kIW + 2 * cxl;
    f32x4 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < kKSteps; ++s) {
      uint32_t d[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k0 = s * 32 + q * 8 + 2 * j;
        const uint32_t lo = in16[k0 < kK ? base + koff[k0] : kInElems];
        const uint32_t hi = in16[k0 + 1 < kK ? base + koff[k0 + 1] : kInElems];
        d[j] = lo | (hi << 16);
      }
      const Frag b = __builtin_bit_cast(Frag, make_uint4(d[0], d[1], d[2], d[3]));
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = mfma16<T>(__builtin_bit_cast(Frag, a[r][s]), b, acc[r]);
    }
    if (real) {
      const int cy = cy0 + cyl, cx = cx0 + cxl;
      const bool inmap = cy >= 0 && cy < p.Hc && cx >= 0 && cx < p.Wc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = r * 16 + 4 * q;
        uint2 ov;
        if (inmap) {
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) { v[j] = acc[r][j] + p.bias[co + j]; v[j] = v[j] > 0.f ? v[j] : 0.f; }
          ov.x = pack2<T>(v[0], v[1]); ov.y = pack2<T>(v[2], v[3]);
        } else {
          ov.x = ov.y = (uint32_t)ninf | ((uint32_t)ninf << 16);
        }
        *reinterpret_cast<uint2*>(&conv16[((co >> 3) * (kPTiles * 16) + pix) * 8 + (co & 4)]) = ov;
      }
    }
  }
  __syncthreads();

  // pool: thread = (pooled pixel, plane)
  const int pp = tid & 31, plane = tid >> 5;
  const int ppy = pp / kPW, ppx = pp - ppy * kPW;
  const int py = py0 + ppy, px = px0 + ppx;
  if (py >= p.Hp || px >= p.Wp) return;
  float m[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] = -__builtin_inff();
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int pix = (2 * ppy + dy) * kCW + 2 * ppx + dx;
      const uint4 v = *reinterpret_cast<const uint4*>(&conv16[(plane * (kPTiles * 16) + pix) * 8]);
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        m[2 * j] = fmaxf(m[2 * j], from_bits<T>((uint16_t)(d[j] & 0xffffu)));
        m[2 * j + 1] = fmaxf(m[2 * j + 1], from_bits<T>((uint16_t)(d[j] >> 16)));
      }
    }
  uint4 o;   // (the maxima are values of the 16-bit type already: the conversion back is exact)
  o.x = pack2<T>(m[0], m[1]); o.y = pack2<T>(m[2], m[3]); o.z = pack2<T>(m[4], m[5]); o.w = pack2<T>(m[6], m[7]);
  static_cast<uint4*>(p.out)[(((size_t)n * 8 + plane) * p.Hp + py) * p.Wp + px] = o;
}

// w: folded f32 [64][3][7][7], b: [64]
void resnet_stem_pack(const float* w, int dtype, std::vector<uint16_t>* pw) {
  pw->assign((size_t)4 * kKSteps * 64 * 8, 0);
  for (int r = 0; r < 4; ++r)
    for (int s = 0; s < kKSteps; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int co = r * 16 + (lane & 15), k = s * 32 + (lane >> 4) * 8 + j;
          if (k >= kK) continue;
          const int tap = k / 3, c = k - 3 * tap;
          (*pw)[(((size_t)r * kKSteps + s) * 64 + lane) * 8 + j] = host_f32_to_16(w[((size_t)co * 3 + c) * 49 + tap], dtype);
        }
}

int32_t resnet_stem_launch(const void* in, int in_fmt, const void* w, const float* bias, const float* mean_std, int N, int H, int W,
                           int dtype, void* out, hipStream_t stream) {
  SCP_REQUIRE(in && w && bias && out, "resnet stem: null argument");
  SCP_REQUIRE(N > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, "resnet stem: N=%d H=%d W=%d (H, W multiples of 4)", N, H, W);
  SCP_REQUIRE(in_fmt == SCPOSE_IN_F32_NCHW || in_fmt == SCPOSE_IN_U8_NHWC, "resnet stem: input format %d", in_fmt);
  SCP_REQUIRE(in_fmt == SCPOSE_IN_F32_NCHW || mean_std, "resnet stem: u8 input needs mean/std");
  ResnetStemLaunch L{};
  L.in = in; L.w = w; L.bias = bias; L.mean_std = mean_std; L.out = out;
  L.N = N; L.H = H; L.W = W; L.Hc = H / 2; L.Wc = W / 2; L.Hp = H / 4; L.Wp = W / 4;
  L.tiles_x = (L.Wp + kPW - 1) / kPW; L.tiles_y = (L.Hp + kPH - 1) / kPH;
  const long long grid = (long long)N * L.tiles_x * L.tiles_y;
  SCP_REQUIRE(grid < (1ll << 31), "resnet stem: %lld tiles exceed the grid", grid);
  const bool bf = dtype == SCPOSE_DT_BF16;
#define RSTEM(DT, FMT) resnet_stem_kernel<DT, FMT><<<dim3((unsigned)grid), 256, 0, stream>>>(L)
  if (in_fmt == SCPOSE_IN_U8_NHWC) { if (bf) RSTEM(0, SCPOSE_IN_U8_NHWC); else RSTEM(1, SCPOSE_IN_U8_NHWC); }
  else { if (bf) RSTEM(0, SCPOSE_IN_F32_NCHW); else RSTEM(1, SCPOSE_IN_F32_NCHW); }
#undef RSTEM
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
