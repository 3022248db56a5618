// Area resize of uint8 frames for shrinking (cv2.resize INTER_AREA as restated in resize_area.py), then OpenCV's 8-bit gray rule:
// (F, H, W, C) -> (F, h, w, C) or (F, h, w), C = 1 or 3.  The emulator's input (dvs_emulator.hip) comes out of here.
//
// The host builds one table per axis and this file only applies them.  A table has one record of five words per output index:
// first source index, tap count, and the weights of the first, the inner and the last tap (the taps of an output index are
// consecutive source indices, and all inner taps share one weight).  Two rules:
//   weighted  h = ((0 + p0 a0) + p1 a1) + ... along a source row in tap order, v = b0 h0, then + b1 h1, ... down the rows; every
//             multiply and every add is one float32 rounding (__fmul_rn / __fadd_rn, and the file is built with contraction off);
//   box       integer sums of count_x x count_y pixels; 2 x 2: (s + 2) >> 2, else float32(s) * inv_area.
// Both end in round-half-to-even, saturated to 0 .. 255.
//
// One block owns a strip of kRows output rows x `tw` output columns (tw <= 256), one thread per column with all its channels.  It
// walks the strip's source rows once, top to bottom.  A row's segment under the strip is fetched with 16-byte loads from the
// 16-byte boundary below its first byte and laid into LDS (4 KiB per pass, two buffers, one barrier per pass); each thread sums its
// own taps out of LDS into the row's horizontal value, which stays in its registers and is added into the vertical sum of the output
// row -- and of the next one too when the two share a fractional boundary row, so inside a strip no row is fetched twice.  A 16-byte
// window that would reach outside the source batch is fetched byte by byte inside it.  No atomics, no workspace traffic but the
// tables.  Indexing is 32-bit inside a frame (the host checks H W C < 2^31) and 64-bit for the frame's offset.
#include "common.h"
#include <type_traits>

namespace scpose {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = 8;                    // output rows of one strip
constexpr int kPass = kThreads * 16;        // bytes fetched per pass
constexpr int kStep = kPass - 16;           // bytes a pass advances: a multiple of 3 and of 16, so a pixel never straddles two passes
constexpr int kRec = 5;                     // words per table record
static_assert(kStep % 3 == 0 && kStep % 16 == 0, "a pass must advance by whole pixels and whole 16-byte windows");

struct Tap {
  int first, count;
  float w_first, w_mid, w_last;
};

__device__ __forceinline__ Tap load_tap(const int32_t* tab, int d) {
  const int32_t* r = tab + (size_t)d * kRec;
  Tap t;
  t.first = r[0]; t.count = r[1];
  t.w_first = __int_as_float(r[2]); t.w_mid = __int_as_float(r[3]); t.w_last = __int_as_float(r[4]);
  return t;
}

__device__ __forceinline__ float tap_weight(const Tap t, int k) { return k == 0 ? t.w_first : (k == t.count - 1 ? t.w_last : t.w_mid); }

__device__ __forceinline__ int round_u8(float v) {
  const float r = rintf(v);                 // half to even
  return r <= 0.0f ? 0 : (r >= 255.0f ? 255 : (int)r);
}

// sixteen source bytes at p, or those of them that lie inside [lo, hi): the rest are never read and count as 0
__device__ __forceinline__ uint4 fetch16(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4*>(p);
  uint32_t v[4] = {0, 0, 0, 0};
  for (int i = 0; i < 16; ++i)
    if (p + i >= lo && p + i < hi) v[i >> 2] |= (uint32_t)p[i] << ((i & 3) * 8);
  return make_uint4(v[0], v[1], v[2], v[3]);
}

template <int C, bool BOX>
__global__ __launch_bounds__(kThreads) void resize_area_kernel(const uint8_t* __restrict__ src, int F, int H, int W, uint8_t* __restrict__ dst,
                                                               int h, int w, int gray, int r_plane, const int32_t* __restrict__ xtab,
                                                               const int32_t* __restrict__ ytab, int tw, int strips_x, int strips_y,
                                                               int shift2x2, float inv_area) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][kPass];
  const int t = threadIdx.x;
  int b = blockIdx.x;
  const int sx = b % strips_x; b /= strips_x;
  const int sy = b % strips_y;
  const int f = b / strips_y;
  const int x0 = sx * tw, x1 = min(x0 + tw, w);                 // the strip's output columns
  const int d0 = sy * kRows, d1 = min(d0 + kRows, h);           // and rows
  const int x = x0 + t;
  const bool mine = t < tw && x < x1;
  Tap tx = load_tap(xtab, mine ? x : x0);                       // a thread without a column has no taps
  if (!mine) tx.count = 0;
  const Tap t_lo = load_tap(xtab, x0), t_hi = load_tap(xtab, x1 - 1);
  const int seg0 = t_lo.first;                                  // source pixels [seg0, seg1) lie under the strip
  const int seg_bytes = (t_hi.first + t_hi.count - seg0) * C;
  const uint8_t* lo = src;
  const uint8_t* hi = src + (size_t)F * H * W * C;
  const uint8_t* frame = src + (size_t)f * H * W * C;

  typedef typename std::conditional<BOX, int, float>::type Acc;
  Acc hv[C], acc[C];
  int staged = -1, pass_no = 0;
  for (int d = d0; d < d1; ++d) {
    const Tap ty = load_tap(ytab, d);
    for (int k = 0; k < ty.count; ++k) {
      const int row = ty.first + k;
      if (row != staged) {                                      // block-uniform: a boundary row shared with the row above is not fetched again
        staged = row;
        const uint8_t* g = frame + ((uint32_t)row * (uint32_t)W + (uint32_t)seg0) * (uint32_t)C;
        const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 15);
        const uint8_t* ga = g - mis;
        const int total = seg_bytes + mis;
        for (int c = 0; c < C; ++c) hv[c] = 0;
        int tap = 0;
        for (int base = 0; base < total; base += kStep, ++pass_no) {
          uint8_t* buf = lds[pass_no & 1];
          if (base + t * 16 < total) *reinterpret_cast<uint4*>(buf + t * 16) = fetch16(ga + base + t * 16, lo, hi);
          __syncthreads();       // one barrier per pass: the buffer written next is the one every thread left two passes ago
          while (tap < tx.count) {
            const int pb = (tx.first - seg0 + tap) * C;         // the tap's byte in the segment
            if (pb >= base + kStep) break;
            const uint8_t* q = buf + (pb - base + mis);
            if (BOX) {
              for (int c = 0; c < C; ++c) hv[c] += q[c];
            } else {
              const float a = tap_weight(tx, tap);
              for (int c = 0; c < C; ++c) hv[c] = __fadd_rn(hv[c], __fmul_rn((float)q[c], a));
            }
            ++tap;
          }
        }
      }
      if (BOX) {
        for (int c = 0; c < C; ++c) acc[c] = k == 0 ? hv[c] : acc[c] + hv[c];
      } else {
        const float bw = tap_weight(ty, k);
        for (int c = 0; c < C; ++c) acc[c] = k == 0 ? __fmul_rn(bw, hv[c]) : __fadd_rn(acc[c], __fmul_rn(bw, hv[c]));
      }
    }
    if (!mine) continue;
    int px[C];
    for (int c = 0; c < C; ++c) {
      if (BOX) px[c] = shift2x2 ? ((int)acc[c] + 2) >> 2 : round_u8(__fmul_rn((float)acc[c], inv_area));
      else px[c] = round_u8(acc[c]);
    }
    const size_t o = ((size_t)f * h + d) * w + x;
    if (C == 1) {
      dst[o] = (uint8_t)px[0];
    } else if (gray) {
      dst[o] = (uint8_t)((4899 * px[r_plane] + 9617 * px[1] + 1868 * px[2 - r_plane] + 8192) >> 14);
    } else {
      for (int c = 0; c < C; ++c) dst[o * C + c] = (uint8_t)px[c];
    }
  }
}

}  // namespace

size_t resize_area_workspace_bytes(int h, int w) {
  Carve c{nullptr};
  c.take<int32_t>((size_t)w * kRec);
  c.take<int32_t>((size_t)h * kRec);
  return c.bytes();
}

// xtab_host / ytab_host: w / h records, checked by the caller (api.cpp); uploaded into the workspace on `stream`
int32_t resize_area_launch(const uint8_t* src, int F, int H, int W, int C, uint8_t* dst, int h, int w, int gray, int bgr, int box,
                           const int32_t* xtab_host, const int32_t* ytab_host, uint8_t* ws, hipStream_t stream) {
  Carve c{ws};
  int32_t* xtab = c.take<int32_t>((size_t)w * kRec);
  int32_t* ytab = c.take<int32_t>((size_t)h * kRec);
  SCP_CHECK_HIP(hipMemcpyAsync(xtab, xtab_host, (size_t)w * kRec * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  SCP_CHECK_HIP(hipMemcpyAsync(ytab, ytab_host, (size_t)h * kRec * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  const int strips_x = (w + kThreads - 1) / kThreads;
  const int tw = (w + strips_x - 1) / strips_x;                 // equal strips: 640 columns are 3 x 214, not 256 + 256 + 128
  const int strips_y = (h + kRows - 1) / kRows;
  const int64_t blocks = (int64_t)strips_x * strips_y * F;
  SCP_REQUIRE(blocks < ((int64_t)1 << 31), "resize_area: %lld blocks: split the batch", (long long)blocks);
  const int cx = xtab_host[1], cy = ytab_host[1];
  const int shift2x2 = box && cx == 2 && cy == 2;
  const float inv_area = 1.0f / (float)(cx * cy);
  const dim3 grid((unsigned)blocks), block(kThreads);
  const int r_plane = bgr ? 2 : 0;
#define SCP_RESIZE(CH, BOX)                                                                                                          \
  hipLaunchKernelGGL((resize_area_kernel<CH, BOX>), grid, block, 0, stream, src, F, H, W, dst, h, w, gray, r_plane, xtab, ytab, tw, \
                     strips_x, strips_y, shift2x2, inv_area)
  if (C == 1) { if (box) SCP_RESIZE(1, true); else SCP_RESIZE(1, false); }
  else        { if (box) SCP_RESIZE(3, true); else SCP_RESIZE(3, false); }
#undef SCP_RESIZE
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
