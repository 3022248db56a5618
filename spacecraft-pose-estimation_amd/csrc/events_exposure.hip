// COUNT and AREA_COUNT exposure of the event renderer: the [begin, end) bounds of every frame, on the device.
//
// The reference's renderer (v2e/v2ecore/renderer.py: render_events_to_frames, compute_area_counts) ends a frame
//   COUNT N          every N events: frame k = [kN, (k+1)N)
//   AREA_COUNT M D   at the first event e >= s whose D x D area has received M events within [s, e], every area counter
//                    starting at zero at s; frame = [s, e), and e opens the next frame
// and writes a frame only while its end is < n - 1.  The histogram of every frame is events.hip's, unchanged: these kernels
// only produce the int64 (F, 2) bounds that scpose_events_render takes.
//
// AREA_COUNT without the serial scan.  g[j] = index of the M-th occurrence of area(j) counting j itself as the first (no such
// occurrence: n - 1, which no written frame can end at).  Along one area's occurrences g does not decrease, so min_{i >= s}
// g[i] is attained at the first occurrence of every area at or after s: it is exactly the reference's trigger e(s).  So
//   area_id_kernel      per event its area (Python floor division and negative wraparound on the (1 + W // D) x (1 + H // D)
//                       grid); a coordinate off that grid sets the status word (a plain store of 1: no order to race on)
//   rs_*                stable LSD radix sort of (area, index), 8 bits per pass: per-tile digit counts in LDS, one exclusive
//                       sum scan (scan_device.h) of the digit-major (digit, tile) table, a scatter whose in-tile ranks come from
//                       ballots -- stable, no global atomic, so the permutation is the same on every run
//   area_g_kernel       g from the sorted order: the M-th occurrence of area(j) is M - 1 places further in j's run
//   scan_* (min, REV)   next[s] = suffix minimum of g, clamped to n - 1 (an absorbing node): the same device-wide scan
//   area_double_kernel  J_l = next^(2^l): L doubling passes, 2^L > the frame-count bound (n - 2) / (M - 1)
//   area_count_kernel   one thread: F = the number of chain steps from 0 that stay below n - 1, found with the tables top
//                       down (and the chain's nodes every 2^L steps, when L had to be capped)
//   area_expand_kernel  frame k in parallel: s_k = next^k(0) from the bits of k, bounds = [s_k, next[s_k])
// Every output is an integer and every step is a fixed function of the input: two runs are bitwise equal.
// tests/event_exposure_restated.py restates both the serial loop and this suffix-minimum form.
#include "common.h"
#include "scan_device.h"

namespace scpose {

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kScanThreads, "the scan bodies of scan_device.h run in the workgroups of this file");
constexpr int kTileItems = 16;
constexpr int kTile = kThreads * kTileItems;   // 4096 elements per tile of the radix sort
constexpr int kRadix = 256;
constexpr int kMaxLevels = 31;

// ------------------------------------------------------------------------------------------------ device-wide int32 scan
// scan_device.h's three passes over a length the host knows
template <int OP, bool REV>
__global__ __launch_bounds__(kThreads) void scan_reduce_kernel(const int32_t* __restrict__ in, int64_t len,
                                                               int32_t* __restrict__ aggr) {
  __shared__ int32_t s[kThreads];
  scan_tile_reduce<OP, REV>(in, len, aggr, s);
}

template <int OP>
__global__ __launch_bounds__(kThreads) void scan_aggr_kernel(int32_t* __restrict__ aggr, int64_t nb) {
  __shared__ int32_t s[kThreads];
  scan_aggregates<OP>(aggr, nb, s);
}

template <int OP, bool REV, bool EXCL>
__global__ __launch_bounds__(kThreads) void scan_apply_kernel(const int32_t* in, int32_t* out, int64_t len,
                                                              const int32_t* __restrict__ aggr) {
  __shared__ int32_t s[kThreads];
  scan_tile_apply<OP, REV, EXCL>(in, out, len, aggr, s);
}

template <int OP, bool REV, bool EXCL>
int32_t scan_launch(const int32_t* in, int32_t* out, int64_t len, int32_t* aggr, hipStream_t stream) {
  if (len == 0) return SCPOSE_OK;
  const int64_t nb = (len + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL((scan_reduce_kernel<OP, REV>), dim3((unsigned)nb), dim3(kThreads), 0, stream, in, len, aggr);
  hipLaunchKernelGGL((scan_aggr_kernel<OP>), dim3(1), dim3(kThreads), 0, stream, aggr, nb);
  hipLaunchKernelGGL((scan_apply_kernel<OP, REV, EXCL>), dim3((unsigned)nb), dim3(kThreads), 0, stream, in, out, len, aggr);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

// ------------------------------------------------------------------------------------------------ stable LSD radix sort
// a tile is 16 rounds of 256 consecutive elements; thread (wave w, lane l) holds element round * 256 + w * 64 + l
__global__ __launch_bounds__(kThreads) void rs_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift, int64_t nt,
                                                           int32_t* __restrict__ hist) {
  __shared__ int32_t h[kRadix];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kTile;
  for (int r = 0; r < kTileItems; ++r) {
    const int64_t i = base + r * kThreads + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & (kRadix - 1)], 1);   // LDS; integer adds commute
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * nt + blockIdx.x] = h[threadIdx.x];      // digit-major: one exclusive scan gives the offsets
}

// vals_in == nullptr: the value of element i is i (the first pass)
__global__ __launch_bounds__(kThreads) void rs_scatter_kernel(const uint32_t* __restrict__ keys_in, const int32_t* __restrict__ vals_in,
                                                              int64_t n, int shift, int64_t nt, const int32_t* __restrict__ offs,
                                                              uint32_t* __restrict__ keys_out, int32_t* __restrict__ vals_out) {
  __shared__ int32_t s_run[kRadix];
  __shared__ int32_t s_cnt[kThreads / 64][kRadix];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  s_run[tid] = offs[(int64_t)tid * nt + blockIdx.x];
  for (int q = 0; q < kThreads / 64; ++q) s_cnt[q][tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const unsigned long long lt = (1ull << lane) - 1;
  for (int r = 0; r < kTileItems; ++r) {
    const int64_t i = base + r * kThreads + tid;
    const bool valid = i < n;
    const uint32_t key = valid ? keys_in[i] : 0u;
    const int d = (int)((key >> shift) & (kRadix - 1));
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const int rank = __popcll(peers & lt);
    if (valid && rank == 0) s_cnt[w][d] = __popcll(peers);
    __syncthreads();
    if (valid) {
      int32_t pos = s_run[d] + rank;
      for (int q = 0; q < w; ++q) pos += s_cnt[q][d];
      keys_out[pos] = key;
      vals_out[pos] = vals_in ? vals_in[i] : (int32_t)i;
    }
    __syncthreads();
    int32_t add = 0;
    for (int q = 0; q < kThreads / 64; ++q) { add += s_cnt[q][tid]; s_cnt[q][tid] = 0; }
    s_run[tid] += add;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ AREA_COUNT
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t d) {
  const int64_t q = a / d;
  return (a % d != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(kThreads) void area_id_kernel(const int32_t* __restrict__ x, const int32_t* __restrict__ y, int64_t n,
                                                           int D, int nw, int nh, uint32_t* __restrict__ key,
                                                           int64_t* __restrict__ count_status) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    int64_t qx = floor_div(x[i], D), qy = floor_div(y[i], D);
    const bool ok = qx >= -nw && qx < nw && qy >= -nh && qy < nh;      // the indices area_counts[qx, qy] accepts
    if (!ok) {
      count_status[1] = 1;
      qx = 0; qy = 0;
    }
    if (qx < 0) qx += nw;
    if (qy < 0) qy += nh;
    key[i] = (uint32_t)(qx * nh + qy);
  }
}

// skeys / sidx nullptr: one area only, the sorted order is the identity
__global__ __launch_bounds__(kThreads) void area_g_kernel(const uint32_t* __restrict__ skeys, const int32_t* __restrict__ sidx,
                                                          int64_t n, int64_t m1, int32_t* __restrict__ g) {
  const int32_t last = (int32_t)(n - 1);
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < n; q += stride) {
    const int64_t q2 = q + m1;
    int32_t v = last;
    if (q2 < n && (!skeys || skeys[q2] == skeys[q])) {
      const int32_t e = sidx ? sidx[q2] : (int32_t)q2;
      v = e < last ? e : last;
    }
    g[sidx ? sidx[q] : q] = v;
  }
}

__global__ __launch_bounds__(kThreads) void area_double_kernel(const int32_t* __restrict__ jin, int64_t n, int32_t* __restrict__ jout) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < n; s += stride) jout[s] = jin[jin[s]];
}

// one thread.  count_status[1] (0 or the out-of-grid flag) was written before; [0] <- F
__global__ void area_count_kernel(const int32_t* __restrict__ tables, int64_t n, int L, int64_t capacity, int32_t* __restrict__ tops,
                                  int64_t tops_cap, int64_t* __restrict__ count_status) {
  if (threadIdx.x != 0) return;
  int64_t status = count_status[1];
  int64_t cnt = 0;
  if (n >= 2 && status == 0) {
    const int32_t last = (int32_t)(n - 1);
    int32_t cur = 0;
    int64_t ti = 0;
    tops[0] = 0;
    const int32_t* JL = tables + (int64_t)L * n;
    while (JL[cur] < last) {                 // only when L had to be capped below the frame-count bound
      cur = JL[cur];
      cnt += (int64_t)1 << L;
      if (++ti >= tops_cap) { status = 2; break; }
      tops[ti] = cur;
    }
    for (int l = L - 1; l >= 0 && status == 0; --l) {
      const int32_t nx = tables[(int64_t)l * n + cur];
      if (nx < last) { cur = nx; cnt += (int64_t)1 << l; }
    }
    if (cnt > capacity) status = 2;
  }
  count_status[0] = status == 0 ? cnt : 0;
  count_status[1] = status;
}

__global__ __launch_bounds__(kThreads) void area_expand_kernel(const int32_t* __restrict__ tables, int64_t n, int L,
                                                               const int32_t* __restrict__ tops,
                                                               const int64_t* __restrict__ count_status, int64_t* __restrict__ bounds) {
  const int64_t F = count_status[0];
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < F; k += stride) {
    int32_t cur = tops[k >> L];
    for (int l = L - 1; l >= 0; --l)
      if ((k >> l) & 1) cur = tables[(int64_t)l * n + cur];
    bounds[2 * k] = cur;
    bounds[2 * k + 1] = tables[cur];
  }
}

// ------------------------------------------------------------------------------------------------ COUNT, names
__global__ __launch_bounds__(kThreads) void count_bounds_kernel(int64_t N, int64_t F, int64_t* __restrict__ bounds) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < F; k += stride) {
    bounds[2 * k] = k * N;
    bounds[2 * k + 1] = (k + 1) * N;
  }
}

// the reference's frame time (ts[start] + ts[end]) / 2: an int64 sum, then float64
__global__ __launch_bounds__(kThreads) void bounds_mid_kernel(const int64_t* __restrict__ t, const int64_t* __restrict__ bounds,
                                                              int64_t F, double* __restrict__ mids) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < F; k += stride)
    mids[k] = (double)(t[bounds[2 * k]] + t[bounds[2 * k + 1]]) / 2.0;
}

unsigned grid_for(int64_t items) {
  int64_t b = (items + kThreads - 1) / kThreads;
  if (b > 65536) b = 65536;
  return (unsigned)(b < 1 ? 1 : b);
}

struct AreaPlan {
  int64_t nt, tops_cap;
  int nw, nh, passes, L;
  uint32_t *k0, *k1;                       // sort keys, ping and pong
  int32_t *v0, *v1, *hist, *aggr, *tables, *tops;
  size_t bytes;
};

// ws == nullptr: the sizes only
AreaPlan area_plan(int64_t n, int64_t M, int D, int h, int w, uint8_t* ws) {
  AreaPlan p{};
  p.nw = 1 + w / D;
  p.nh = 1 + h / D;
  const int64_t areas = (int64_t)p.nw * p.nh;
  int bits = 0;
  while (bits < 32 && (((int64_t)1 << bits) < areas)) ++bits;
  p.passes = (bits + 7) / 8;
  p.nt = (n + kTile - 1) / kTile;
  const int64_t scan_len = n > (int64_t)kRadix * p.nt ? n : (int64_t)kRadix * p.nt;
  const int64_t fcap = n >= 2 ? (n - 2) / (M - 1) : 0;
  int L = 0;
  while (L < kMaxLevels && ((int64_t)1 << L) <= fcap) ++L;        // 2^L > every possible frame count: no top walk
  // the tables take (L + 1) * 4n bytes: above 32 GiB keep fewer levels and walk the top level (one node every 2^L frames)
  while (L > 8 && (double)(L + 1) * 4.0 * (double)n > 34359738368.0) --L;
  p.L = L;
  p.tops_cap = (fcap >> L) + 2;
  Carve c{ws};
  p.k0 = c.take<uint32_t>(n);
  p.k1 = c.take<uint32_t>(n);
  p.v0 = c.take<int32_t>(n);
  p.v1 = c.take<int32_t>(n);
  p.hist = c.take<int32_t>(kRadix * p.nt);
  p.aggr = c.take<int32_t>((scan_len + kScanTile - 1) / kScanTile + 1);
  p.tables = c.take<int32_t>((L + 1) * n);
  p.tops = c.take<int32_t>(p.tops_cap);
  p.bytes = c.bytes();
  return p;
}

}  // namespace

size_t events_area_workspace_bytes(int64_t n, int64_t M, int D, int h, int w) { return area_plan(n, M, D, h, w, nullptr).bytes; }

int32_t events_area_bounds_launch(const int32_t* x, const int32_t* y, int64_t n, int64_t M, int D, int h, int w, int64_t* bounds,
                                  int64_t capacity, int64_t* count_status, uint8_t* ws, hipStream_t stream) {
  const AreaPlan p = area_plan(n, M, D, h, w, ws);
  uint32_t *k0 = p.k0, *k1 = p.k1;
  int32_t *v0 = p.v0, *v1 = p.v1, *hist = p.hist, *aggr = p.aggr, *tables = p.tables, *tops = p.tops;
  SCP_CHECK_HIP(hipMemsetAsync(count_status, 0, 2 * sizeof(int64_t), stream));
  if (n > 0)
    hipLaunchKernelGGL(area_id_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, x, y, n, D, p.nw, p.nh, k0, count_status);
  if (n >= 2) {
    // stable sort of (area, index): keys k0 -> k1 -> k0 ..., values implicit in the first pass
    const uint32_t* kin = k0;
    const int32_t* vin = nullptr;
    for (int pass = 0; pass < p.passes; ++pass) {
      uint32_t* kout = (pass & 1) ? k0 : k1;
      int32_t* vout = (pass & 1) ? v0 : v1;
      hipLaunchKernelGGL(rs_hist_kernel, dim3((unsigned)p.nt), dim3(kThreads), 0, stream, kin, n, 8 * pass, p.nt, hist);
      const int32_t rc = scan_launch<0, false, true>(hist, hist, (int64_t)kRadix * p.nt, aggr, stream);
      if (rc != SCPOSE_OK) return rc;
      hipLaunchKernelGGL(rs_scatter_kernel, dim3((unsigned)p.nt), dim3(kThreads), 0, stream, kin, vin, n, 8 * pass, p.nt, hist,
                         kout, vout);
      kin = kout;
      vin = vout;
    }
    hipLaunchKernelGGL(area_g_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, p.passes ? kin : nullptr,
                       p.passes ? vin : nullptr, n, M - 1 < n ? M - 1 : n, tables);
    const int32_t rc = scan_launch<1, true, false>(tables, tables, n, aggr, stream);     // next = suffix min of g
    if (rc != SCPOSE_OK) return rc;
    for (int l = 1; l <= p.L; ++l)
      hipLaunchKernelGGL(area_double_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, tables + (int64_t)(l - 1) * n, n,
                         tables + (int64_t)l * n);
  }
  hipLaunchKernelGGL(area_count_kernel, dim3(1), dim3(64), 0, stream, tables, n, p.L, capacity, tops, p.tops_cap, count_status);
  if (n >= 2 && capacity > 0)
    hipLaunchKernelGGL(area_expand_kernel, dim3(grid_for(capacity)), dim3(kThreads), 0, stream, tables, n, p.L, tops, count_status,
                       bounds);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t events_count_bounds_launch(int64_t N, int64_t F, int64_t* bounds, hipStream_t stream) {
  if (F == 0) return SCPOSE_OK;
  hipLaunchKernelGGL(count_bounds_kernel, dim3(grid_for(F)), dim3(kThreads), 0, stream, N, F, bounds);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t events_bounds_midpoints_launch(const int64_t* t, const int64_t* bounds, int64_t F, double* mids, hipStream_t stream) {
  if (F == 0) return SCPOSE_OK;
  hipLaunchKernelGGL(bounds_mid_kernel, dim3(grid_for(F)), dim3(kThreads), 0, stream, t, bounds, F, mids);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
