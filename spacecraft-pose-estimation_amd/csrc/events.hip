// Event stream -> event frames on the device (stage 0 of the reference's event pipeline).
//
// Replaces v2e/convert_aedats.py: `e2v.py --dvs_exposure duration 10000 --dvs_vid_full_scale 2` (v2ecore/renderer.py:
// render_events_to_frames, accumulate_event_frame; v2ecore/v2e_utils.py: hist2d_numba_seq) followed by cv2.undistort of
// every frame.  Three kernels:
//   events_frame_bounds_kernel  per frame the slice [searchsorted(t, start_k, left), searchsorted(t, start_k+1, right)) of the
//                               time-sorted stream (int64 ticks compared as float64, exact below 2^53), end clamped to n - 1:
//                               the reference never draws the last event of a stream
//   events_accumulate_kernel    one workgroup per (frame, band of rows): scans the frame's CONTIGUOUS slice, counts the events
//                               of its band into int32 counters in LDS (no global atomic anywhere; integer adds commute, so
//                               the result is bitwise deterministic), clips to [-fs, fs] AFTER the sum, looks the gray value
//                               up in the host-built table and stores it (3 equal channels, and / or a 1-byte plane)
//   events_undistort_kernel     cv2.undistort(img, K, dist): per output pixel the source position through the forward
//                               distortion model (float64, same model as pnp.hip), X = round_half_even(map * 32), the
//                               fixed-point bilinear tap of bilinear_fixed.h on the gray plane, border 0.  The map does not
//                               depend on the frame: a thread computes it once for its pixels and walks the frames.
// Equal addresses inside a wave (hot pixels) are summed with ballots before the LDS add, see peel below.
// tests/event_render_restated.py is the NumPy restatement; both kernels are bit-exact against it.
#include "common.h"
#include "bilinear_fixed.h"

#pragma clang fp contract(off)

namespace scpose {

constexpr int kEvThreads = 1024;
constexpr int kEvLutBytes = 256;                              // static LDS: the gray table, 2 * fs + 1 <= 255 entries
constexpr int kEvLdsBytes = 160 * 1024 - kEvLutBytes;         // dynamic LDS: the band's counters
constexpr int kEvLdsInts = kEvLdsBytes / 4;

int events_max_width() { return kEvLdsInts; }

__global__ __launch_bounds__(256) void events_frame_bounds_kernel(const int64_t* __restrict__ t, int64_t n,
                                                                  const double* __restrict__ starts, int F,
                                                                  int64_t* __restrict__ bounds) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= F) return;
  const double s = starts[k], e = starts[k + 1];
  int64_t lo = 0, hi = n;
  while (lo < hi) {                      // first i with t[i] >= s
    const int64_t mid = (lo + hi) >> 1;
    if ((double)t[mid] < s) lo = mid + 1; else hi = mid;
  }
  const int64_t b0 = lo;
  lo = 0; hi = n;
  while (lo < hi) {                      // first i with t[i] > e
    const int64_t mid = (lo + hi) >> 1;
    if ((double)t[mid] <= e) lo = mid + 1; else hi = mid;
  }
  bounds[2 * k] = b0;
  bounds[2 * k + 1] = lo < n - 1 ? lo : n - 1;
}

struct U32x3 { uint32_t a, b, c; };

// four gray pixels as the 12 bytes of four RGB pixels with equal channels: one store
__device__ __forceinline__ U32x3 gray4_to_rgb(uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3) {
  U32x3 o;
  o.a = g0 * 0x010101u | (g1 << 24);
  o.b = g1 * 0x0101u | (g2 << 16) | (g2 << 24);
  o.c = g2 | (g3 * 0x01010100u);
  return o;
}

template <bool FOLD>
__global__ __launch_bounds__(kEvThreads) void events_accumulate_kernel(
    const int32_t* __restrict__ ex, const int32_t* __restrict__ ey, const void* __restrict__ ep, int p_bytes,
    const int64_t* __restrict__ bounds, int H, int W, int band_rows, int fs, const uint8_t* __restrict__ lut,
    uint8_t* __restrict__ plane, uint8_t* __restrict__ rgb, int vec) {
  extern __shared__ __attribute__((aligned(16))) int cnt[];
  __shared__ uint8_t s_lut[kEvLutBytes];
  const int tid = threadIdx.x, lane = tid & 63;
  const int f = blockIdx.y;
  const int r0 = blockIdx.x * band_rows;
  const int r1 = r0 + band_rows < H ? r0 + band_rows : H;
  const int npx = (r1 - r0) * W;
  for (int i = tid; i < npx; i += kEvThreads) cnt[i] = 0;
  if (tid < 2 * fs + 1) s_lut[tid] = lut[tid];
  __syncthreads();

  const int64_t b0 = bounds[2 * f], b1 = bounds[2 * f + 1];
  // every lane of a wave runs the same number of iterations: the ballots below need the whole wave
  for (int64_t base = b0 + (tid - lane); base < b1; base += kEvThreads) {
    const int64_t i = base + lane;
    bool valid = i < b1;
    int addr = 0, val = 1;
    if (valid) {
      const int yy = ey[i];
      valid = yy >= r0 && yy < r1;
      if (valid) {                                         // x (and p) are read for the band's own events only
        const int xx = ex[i];
        valid = xx >= 0 && xx < W;
        addr = (yy - r0) * W + xx;
        if (!FOLD) {
          const int pv = p_bytes == 1 ? (int)static_cast<const int8_t*>(ep)[i] : static_cast<const int32_t*>(ep)[i];
          val = pv == 1 ? 1 : -1;                          // the reference: ON is p == 1, everything else is OFF
        }
      }
    }
    // Peel: the lanes that hit the address of the first remaining lane are summed with a ballot and added once, so that a
    // hot pixel costs one LDS add per wave and not one per event.  Always two rounds (a hot pixel that holds most of a
    // wave is missed by both only when neither leader is hot), up to four while a round finds four lanes or more.
    unsigned long long rem = __ballot(valid);
    const unsigned long long on = FOLD ? ~0ull : __ballot(val > 0);
#pragma unroll 1
    for (int it = 0; it < 4 && rem; ++it) {
      const int lead = __ffsll((long long)rem) - 1;
      const int a0 = __builtin_amdgcn_readlane(addr, lead);
      const bool hit = valid && addr == a0;
      const unsigned long long mm = __ballot(hit);
      const int sum = FOLD ? __popcll(mm) : __popcll(mm & on) - __popcll(mm & ~on);
      if (lane == lead && sum != 0) atomicAdd(&cnt[a0], sum);
      valid = valid && !hit;
      rem &= ~mm;
      if (it >= 1 && __popcll(mm) < 4) break;
    }
    if (valid) atomicAdd(&cnt[addr], val);
  }
  __syncthreads();

  const size_t pix0 = (size_t)f * H * W + (size_t)r0 * W;      // first pixel of the band in the output
  auto gray = [&](int c) -> uint32_t {
    c = c < -fs ? -fs : (c > fs ? fs : c);                      // clip after the sum
    return s_lut[c + fs];
  };
  if (vec) {                                                    // W % 4 == 0 and 4-byte aligned outputs: 4 pixels per thread
    for (int i = tid * 4; i < npx; i += kEvThreads * 4) {
      const int4 c = *reinterpret_cast<const int4*>(cnt + i);
      const uint32_t g0 = gray(c.x), g1 = gray(c.y), g2 = gray(c.z), g3 = gray(c.w);
      if (plane) *reinterpret_cast<uint32_t*>(plane + pix0 + i) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
      if (rgb) *reinterpret_cast<U32x3*>(rgb + (pix0 + i) * 3) = gray4_to_rgb(g0, g1, g2, g3);
    }
  } else {
    for (int i = tid; i < npx; i += kEvThreads) {
      const uint8_t g = (uint8_t)gray(cnt[i]);
      if (plane) plane[pix0 + i] = g;
      if (rgb) { uint8_t* o = rgb + (pix0 + i) * 3; o[0] = g; o[1] = g; o[2] = g; }
    }
  }
}

// PX consecutive pixels of a row per thread (4: W % 4 == 0 and aligned output, one 12-byte store per frame; else 1)
template <int PX>
__global__ __launch_bounds__(256) void events_undistort_kernel(const uint8_t* __restrict__ plane, int F, int H, int W,
                                                               const double* __restrict__ K, const double* __restrict__ dist,
                                                               uint8_t* __restrict__ out, int frames_per_group) {
  const int npix = H * W;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= npix / PX) return;
  const int pix = q * PX;
  const int v = pix / W, u0 = pix - v * W;
  const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
  const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
  int off[PX][4];          // byte offsets of the four taps inside a gray plane, -1 outside the frame
  int fa[PX], fb[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    // forward distortion model, new camera matrix = K (cv2.undistort's default); the order of operations is the restatement's
    const double xn = ((double)(u0 + j) - cx) / fx, yn = ((double)v - cy) / fy;
    const double r2 = xn * xn + yn * yn;
    const double cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
    const double xd = xn * cd + p1 * 2 * xn * yn + p2 * (r2 + 2 * xn * xn);
    const double yd = yn * cd + p1 * (r2 + 2 * yn * yn) + p2 * 2 * xn * yn;
    const double mx = fx * xd + cx, my = fy * yd + cy;
    const long long X = sat_round_int32(mx * 32.0), Y = sat_round_int32(my * 32.0);
    const long long x0 = sat_int16(X >> 5), y0 = sat_int16(Y >> 5);
    fa[j] = (int)(X & 31); fb[j] = (int)(Y & 31);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long yy = y0 + (k >> 1), xx = x0 + (k & 1);
      off[j][k] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (int)(yy * W + xx) : -1;
    }
  }
  const int f0 = blockIdx.y * frames_per_group;
  const int f1 = f0 + frames_per_group < F ? f0 + frames_per_group : F;
  for (int f = f0; f < f1; ++f) {
    const uint8_t* src = plane + (size_t)f * npix;
    uint32_t g[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      int s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = off[j][k] >= 0 ? (int)src[off[j][k]] : 0;
      g[j] = BilinearTap(fa[j], fb[j])(s[0], s[1], s[2], s[3]);
    }
    uint8_t* o = out + ((size_t)f * npix + pix) * 3;
    if (PX == 4) {
      *reinterpret_cast<U32x3*>(o) = gray4_to_rgb(g[0], g[1], g[2], g[3]);
    } else {
      o[0] = (uint8_t)g[0]; o[1] = (uint8_t)g[0]; o[2] = (uint8_t)g[0];
    }
  }
}

int32_t events_frame_bounds_launch(const int64_t* t, int64_t n, const double* starts, int F, int64_t* bounds,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(events_frame_bounds_kernel, dim3((F + 255) / 256), dim3(256), 0, stream, t, n, starts, F, bounds);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

template <bool FOLD>
static int32_t accumulate_launch(const int32_t* x, const int32_t* y, const void* p, int p_bytes, const int64_t* bounds, int F,
                                 int H, int W, int fs, const uint8_t* lut, uint8_t* plane, uint8_t* rgb, int vec,
                                 hipStream_t stream) {
  // rows per band: as many as the LDS holds; with few frames, more and smaller bands so that the chip has work (the extra
  // passes over the y column are cheap then)
  int nb = (H + kEvLdsInts / W - 1) / (kEvLdsInts / W);
  if ((long long)F * nb < 512) { const int want = (512 + F - 1) / F; nb = want < H ? (want > nb ? want : nb) : H; }
  const int rows = (H + nb - 1) / nb;
  nb = (H + rows - 1) / rows;
  const size_t lds = (size_t)rows * W * sizeof(int);
  static LdsOptIn memo;
  if (lds > 64 * 1024) {
    const int32_t rc = lds_opt_in(reinterpret_cast<const void*>(&events_accumulate_kernel<FOLD>), kEvLdsBytes, &memo);
    if (rc != SCPOSE_OK) return rc;
  }
  const size_t fstride = (size_t)H * W;
  for (int f0 = 0; f0 < F; f0 += 32768) {                       // gridDim.y limit
    const int nf = F - f0 < 32768 ? F - f0 : 32768;
    hipLaunchKernelGGL(events_accumulate_kernel<FOLD>, dim3(nb, nf), dim3(kEvThreads), lds, stream, x, y, p, p_bytes,
                       bounds + 2 * (size_t)f0, H, W, rows, fs, lut, plane ? plane + f0 * fstride : nullptr,
                       rgb ? rgb + f0 * fstride * 3 : nullptr, vec);
    SCP_CHECK_HIP(hipGetLastError());
  }
  return SCPOSE_OK;
}

int32_t events_render_launch(const int32_t* x, const int32_t* y, const void* p, int p_bytes, const int64_t* bounds, int F,
                             int H, int W, int fs, int fold, const uint8_t* lut, const double* K, const double* dist,
                             uint8_t* frames, uint8_t* distorted, uint8_t* workspace, hipStream_t stream) {
  const bool undist = K != nullptr;
  auto al4 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; };
  const int vec = (W % 4 == 0) && al4(frames) && al4(distorted) && al4(workspace);
  uint8_t* plane = undist ? workspace : nullptr;
  uint8_t* rgb = undist ? distorted : frames;
  const int32_t rc = fold ? accumulate_launch<true>(x, y, p, p_bytes, bounds, F, H, W, fs, lut, plane, rgb, vec, stream)
                          : accumulate_launch<false>(x, y, p, p_bytes, bounds, F, H, W, fs, lut, plane, rgb, vec, stream);
  if (rc != SCPOSE_OK) return rc;
  const size_t fbytes = (size_t)H * W * 3;
  if (!undist) {
    if (distorted) SCP_CHECK_HIP(hipMemcpyAsync(distorted, frames, (size_t)F * fbytes, hipMemcpyDeviceToDevice, stream));
    return SCPOSE_OK;
  }
  const int px = vec ? 4 : 1;
  const int bx = (H * W / px + 255) / 256;
  int groups = (2048 + bx - 1) / bx;                            // enough workgroups for the chip; the rest of F is walked
  if (groups > F) groups = F;
  const int fpg = (F + groups - 1) / groups;
  groups = (F + fpg - 1) / fpg;
  if (vec) hipLaunchKernelGGL(events_undistort_kernel<4>, dim3(bx, groups), dim3(256), 0, stream, plane, F, H, W, K, dist, frames, fpg);
  else hipLaunchKernelGGL(events_undistort_kernel<1>, dim3(bx, groups), dim3(256), 0, stream, plane, F, H, W, K, dist, frames, fpg);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
