// The records of an AEDAT-2.0 file -> (t, x, y, p) on the device: the binary reader next to the text reader (events_csv.hip), and
// the inverse of aedat2_pack_kernel (events_write.hip).
//
// A record is two big-endian 32-bit words, (address, time stamp).  Under the DAVIS layout (jAER) a record with bit 31 set is an
// APS / IMU sample and one with bit 31 clear and bit 10 set a special event: both are dropped and counted; under the V2E layout
// (the reference's AEDat2Output, scpose_events_aedat2_pack) every record is a polarity event and bit 31 belongs to y.  The kept
// events are compacted in file order.  The time stamp word u is a uint32 that rolls over: record i carries
// wraps_i = #{ 1 <= j <= i : u[j-1] > u[j] and u[j-1] - u[j] > 2^31 } full roll-overs, counted over ALL records.
//
// A workgroup owns one tile of kScanTile = 4096 records; thread T takes records k * 256 + T of the tile, k = 0 .. 15, so that a
// wave's load is 512 consecutive bytes and a wave's stores of one k go to consecutive rows.  One (k, wave) pair is a GROUP of 64
// consecutive records: a ballot gives the keep and wrap masks of a group, popcounts of the masks below a lane its position in it.
//   aedat2_count_kernel   per tile: kept / wrap / other counts (ballots, summed over the four waves through LDS), and of the
//                         tile's last kept record the time stamp word and the wraps inside the tile up to it
//   aedat2_scan_kernel    one workgroup, scan_device.h: int64 row offsets and int64 wrap carries of the tiles (tile-count scan),
//                         the total of the other counts, the last tile before b that keeps an event (exclusive min-scan of -b)
//                         and from it the final time stamp of the last kept event before tile b; count_status
//   aedat2_unpack_kernel  the tile again: the 64 group counts (keep | wrap << 16) go through one block scan, then every kept
//                         lane decodes its record and stores the row at tile offset + group offset + rank in the group
// The columns are written without atomics.  The two order-independent integers that only this last pass knows, the RANGE bit and
// n_backward, reach count_status through one integer atomicOr / atomicAdd per workgroup that has something to add.
// No floating point but the optional division of the time stamps (one IEEE float64 division per record); integer work on fixed
// positions: two runs on the same bytes are bitwise equal.  Traffic: 8 + 8 bytes read and at most 17 written per record.
#include "common.h"
#include "scan_device.h"

namespace scpose {

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kScanThreads, "the scan bodies of scan_device.h run in the workgroups of this file");
constexpr int kWaves = kThreads / 64;
constexpr int kGroups = kScanItems * kWaves;         // 64 groups of 64 records per tile
static_assert(kGroups <= kThreads, "one thread per group in the block scan");
static_assert(kScanTile < (1 << 16), "keep and wrap counts of a tile share one int32");
constexpr int64_t kNoTime = INT64_MIN;               // "no kept event before": below every time stamp

inline int64_t tiles_of(int64_t n) { return (n + kScanTile - 1) / kScanTile; }

__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

struct Flags {
  bool keep, other, wrap;
};

// record j (all 64 lanes of a wave call this with consecutive j): one 8-byte load, both words swapped in registers.  The time
// stamp word before it comes from the lane below; lane 0 reads it again from memory.
__device__ __forceinline__ Flags load_record(const uint2* __restrict__ rec, int64_t n, int64_t j, int layout, uint32_t& a, uint32_t& u) {
  const bool in = j < n;
  uint2 v = make_uint2(0u, 0u);
  if (in) v = rec[j];
  a = bswap32(v.x);
  u = bswap32(v.y);
  uint32_t before = (uint32_t)__shfl_up((int)u, 1, 64);
  if ((threadIdx.x & 63) == 0) before = (in && j > 0) ? bswap32(rec[j - 1].y) : u;
  Flags f;
  f.wrap = in && before > u && before - u > 0x80000000u;
  f.other = in && layout == SCPOSE_AEDAT2_LAYOUT_DAVIS && (a >> 31) != 0;
  const bool special = layout == SCPOSE_AEDAT2_LAYOUT_DAVIS && ((a >> 10) & 1u) != 0;
  f.keep = in && !f.other && !special;
  return f;
}

__device__ __forceinline__ int64_t final_time(uint32_t u, int64_t wraps, int unwrap, double t_div) {
  int64_t t = unwrap ? (int64_t)u + (wraps << 32) : (int64_t)(int32_t)u;
  if (t_div != 0.0) t = (int64_t)((double)t / t_div);
  return t;
}

__device__ __forceinline__ int top_lane(unsigned long long m) { return 63 - __clzll((long long)m); }

__global__ __launch_bounds__(kThreads) void aedat2_count_kernel(const uint2* __restrict__ rec, int64_t n, int layout,
                                                                int32_t* __restrict__ tile_keep, int32_t* __restrict__ tile_wrap,
                                                                int32_t* __restrict__ tile_other, int32_t* __restrict__ tile_last,
                                                                uint32_t* __restrict__ last_u, int32_t* __restrict__ last_wraps) {
  __shared__ int32_t s_cnt[kWaves][4];               // kept, wraps, others, in-tile index of the wave's last kept record
  __shared__ uint32_t s_u[kWaves];
  __shared__ int32_t s_upto[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  int32_t nk = 0, nw = 0, no = 0, last = -1;
  uint32_t ul = 0, wrapbits = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    uint32_t a, u;
    const Flags f = load_record(rec, n, base + k * kThreads + threadIdx.x, layout, a, u);
    const unsigned long long km = __ballot(f.keep), wm = __ballot(f.wrap), om = __ballot(f.other);
    nk += __popcll(km);
    nw += __popcll(wm);
    no += __popcll(om);
    const uint32_t utop = (uint32_t)__shfl((int)u, km ? top_lane(km) : 0, 64);
    if (km) {
      last = k * kThreads + wave * 64 + top_lane(km);
      ul = utop;
    }
    wrapbits |= (uint32_t)f.wrap << k;
  }
  if (lane == 0) {
    s_cnt[wave][0] = nk;
    s_cnt[wave][1] = nw;
    s_cnt[wave][2] = no;
    s_cnt[wave][3] = last;
    s_u[wave] = ul;
  }
  __syncthreads();
  int32_t li = -1;                                   // the tile's last kept record
#pragma unroll
  for (int v = 0; v < kWaves; ++v) li = s_cnt[v][3] > li ? s_cnt[v][3] : li;
  int32_t upto = 0;                                  // wraps of the tile at or before it
#pragma unroll
  for (int k = 0; k < kScanItems; ++k)
    upto += __popcll(__ballot(((wrapbits >> k) & 1u) != 0 && k * kThreads + (int)threadIdx.x <= li));
  if (lane == 0) s_upto[wave] = upto;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t k3[3] = {0, 0, 0}, w3 = 0;
    uint32_t u3 = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
      k3[0] += s_cnt[v][0];
      k3[1] += s_cnt[v][1];
      k3[2] += s_cnt[v][2];
      w3 += s_upto[v];
      if (s_cnt[v][3] == li) u3 = s_u[v];
    }
    tile_keep[blockIdx.x] = k3[0];
    tile_wrap[blockIdx.x] = k3[1];
    tile_other[blockIdx.x] = k3[2];
    tile_last[blockIdx.x] = li >= 0 ? -(int32_t)blockIdx.x : INT_MAX;      // min-scanned: the last tile with a kept event
    last_u[blockIdx.x] = u3;
    last_wraps[blockIdx.x] = w3;
  }
}

// one workgroup.  prev_t serves the sum of the other counts as scratch before it is filled.
__global__ __launch_bounds__(kThreads) void aedat2_scan_kernel(const int32_t* tile_keep, const int32_t* tile_wrap, const int32_t* tile_other,
                                                               int32_t* tile_last, const uint32_t* last_u, const int32_t* last_wraps,
                                                               int64_t nb, int64_t n, int unwrap, double t_div, int64_t capacity,
                                                               int64_t* tile_off, int64_t* wrap_off, int64_t* prev_t,
                                                               int64_t* __restrict__ count_status) {
  __shared__ int32_t sc[kThreads];
  // a step sums at most 256 * 4096 flags: fits int32
  const int64_t others = scan_tile_counts(tile_other, nb, prev_t, sc);
  const int64_t kept = scan_tile_counts(tile_keep, nb, tile_off, sc);
  const int64_t wraps = scan_tile_counts(tile_wrap, nb, wrap_off, sc);
  scan_aggregates<1>(tile_last, nb, sc);
  __syncthreads();                                   // wrap_off and tile_last of other threads
  for (int64_t b = threadIdx.x; b < nb; b += kThreads) {
    const int32_t m = tile_last[b];
    int64_t pt = kNoTime;
    if (m != INT_MAX) {
      const int64_t j = -(int64_t)m;
      pt = final_time(last_u[j], wrap_off[j] + last_wraps[j], unwrap, t_div);
    }
    prev_t[b] = pt;
  }
  if (threadIdx.x == 0) {
    const bool full = kept > capacity;
    count_status[0] = full ? 0 : kept;
    count_status[1] = full ? SCPOSE_AEDAT2_READ_CAPACITY : 0;
    count_status[2] = others;
    count_status[3] = n - kept - others;             // a record is kept, other or special
    count_status[4] = wraps;
    count_status[5] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void aedat2_unpack_kernel(const uint2* __restrict__ rec, int64_t n, int32_t h, int32_t w, int layout,
                                                                 int flip_x, int flip_y, int unwrap, double t_div,
                                                                 const int64_t* __restrict__ tile_off, const int64_t* __restrict__ wrap_off,
                                                                 const int64_t* __restrict__ prev_t, int64_t* __restrict__ t_out,
                                                                 int32_t* __restrict__ x_out, int32_t* __restrict__ y_out,
                                                                 int8_t* __restrict__ p_out, int64_t capacity, int64_t* count_status) {
  __shared__ int32_t sc[kThreads];
  __shared__ int32_t s_cnt[kGroups];                 // kept | wraps << 16 of a group, then everything before the group
  __shared__ int64_t s_last[kGroups];                // final time of the group's last kept event
  __shared__ int64_t s_prev[kGroups];                // final time of the last kept event before the group
  __shared__ int32_t s_red[kWaves][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  uint32_t a[kScanItems];
  int64_t tv[kScanItems];                            // the time stamp word, then the final time
  uint32_t keepbits = 0, wrapbits = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    uint32_t u;
    const Flags f = load_record(rec, n, base + k * kThreads + threadIdx.x, layout, a[k], u);
    tv[k] = (int64_t)u;
    keepbits |= (uint32_t)f.keep << k;
    wrapbits |= (uint32_t)f.wrap << k;
    const unsigned long long km = __ballot(f.keep), wm = __ballot(f.wrap);
    if (lane == 0) s_cnt[k * kWaves + wave] = __popcll(km) | (__popcll(wm) << 16);
  }
  __syncthreads();
  const int32_t mine = threadIdx.x < kGroups ? s_cnt[threadIdx.x] : 0;
  const int32_t inc = block_inclusive_scan<0>(mine, sc);                   // neither half exceeds 4096: no carry between them
  if (threadIdx.x < kGroups) s_cnt[threadIdx.x] = inc - mine;
  __syncthreads();
  const int64_t row0 = tile_off[blockIdx.x], wraps0 = wrap_off[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int g = k * kWaves + wave;
    const unsigned long long km = __ballot(((keepbits >> k) & 1u) != 0), wm = __ballot(((wrapbits >> k) & 1u) != 0);
    tv[k] = final_time((uint32_t)tv[k], wraps0 + (s_cnt[g] >> 16) + __popcll(wm & upto), unwrap, t_div);
    const int64_t tl = __shfl(tv[k], km ? top_lane(km) : 0, 64);
    if (lane == 0) s_last[g] = km ? tl : kNoTime;
  }
  __syncthreads();
  if (threadIdx.x < kGroups) {
    int q = (int)threadIdx.x - 1;
    while (q >= 0 && s_last[q] == kNoTime) --q;
    s_prev[threadIdx.x] = q >= 0 ? s_last[q] : prev_t[blockIdx.x];
  }
  __syncthreads();
  int32_t nback = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int g = k * kWaves + wave;
    const bool keep = ((keepbits >> k) & 1u) != 0;
    const unsigned long long km = __ballot(keep);
    const unsigned long long m = km & below;
    int64_t tp = __shfl(tv[k], m ? top_lane(m) : lane, 64);
    if (!m) tp = s_prev[g];
    nback += __popcll(__ballot(keep && tv[k] < tp));
    if (keep) {
      const int32_t xf = (int32_t)((a[k] >> 12) & 0x3ffu);
      const int32_t yf = (int32_t)(layout == SCPOSE_AEDAT2_LAYOUT_DAVIS ? (a[k] >> 22) & 0x1ffu : a[k] >> 22);
      if (xf >= w || yf >= h) bad = true;
      const int64_t row = row0 + (s_cnt[g] & 0xffff) + __popcll(m);
      if (row < capacity) {
        t_out[row] = tv[k];
        x_out[row] = flip_x ? w - 1 - xf : xf;
        y_out[row] = flip_y ? h - 1 - yf : yf;
        p_out[row] = (int8_t)((a[k] >> 11) & 1u);
      }
    }
  }
  const bool wave_bad = __ballot(bad) != 0;
  if (lane == 0) {
    s_red[wave][0] = nback;
    s_red[wave][1] = wave_bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t nb = 0, flag = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
      nb += s_red[v][0];
      flag |= s_red[v][1];
    }
    unsigned long long* st = reinterpret_cast<unsigned long long*>(count_status);
    if (flag) atomicOr(st + 1, (unsigned long long)SCPOSE_AEDAT2_READ_RANGE);
    if (nb) atomicAdd(st + 5, (unsigned long long)nb);
  }
}

struct ReadPlan {
  int64_t nb;
  int32_t *tile_keep, *tile_wrap, *tile_other, *tile_last, *last_wraps;
  uint32_t* last_u;
  int64_t *tile_off, *wrap_off, *prev_t;
  size_t bytes;
};

ReadPlan read_plan(int64_t n, uint8_t* wsp) {
  ReadPlan p{};
  p.nb = tiles_of(n);
  const size_t cnt = (size_t)(p.nb > 0 ? p.nb : 1);  // never an empty workspace
  Carve c{wsp};
  p.tile_keep = c.take<int32_t>(cnt);
  p.tile_wrap = c.take<int32_t>(cnt);
  p.tile_other = c.take<int32_t>(cnt);
  p.tile_last = c.take<int32_t>(cnt);
  p.last_wraps = c.take<int32_t>(cnt);
  p.last_u = c.take<uint32_t>(cnt);
  p.tile_off = c.take<int64_t>(cnt);
  p.wrap_off = c.take<int64_t>(cnt);
  p.prev_t = c.take<int64_t>(cnt);
  p.bytes = c.bytes();
  return p;
}

}  // namespace

size_t events_aedat2_unpack_workspace_bytes(int64_t n) { return read_plan(n, nullptr).bytes; }

int32_t events_aedat2_unpack_launch(const uint8_t* records, int64_t n, int h, int w, int layout, int flip_x, int flip_y, int unwrap,
                                    double t_div, int64_t* t, int32_t* x, int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status,
                                    uint8_t* wsp, hipStream_t stream) {
  const ReadPlan pl = read_plan(n, wsp);
  const uint2* rec = reinterpret_cast<const uint2*>(records);
  if (pl.nb > 0)
    hipLaunchKernelGGL(aedat2_count_kernel, dim3((unsigned)pl.nb), dim3(kThreads), 0, stream, rec, n, layout, pl.tile_keep, pl.tile_wrap,
                       pl.tile_other, pl.tile_last, pl.last_u, pl.last_wraps);
  // n == 0: no tiles, the scan still writes count_status
  hipLaunchKernelGGL(aedat2_scan_kernel, dim3(1), dim3(kThreads), 0, stream, pl.tile_keep, pl.tile_wrap, pl.tile_other, pl.tile_last,
                     pl.last_u, pl.last_wraps, pl.nb, n, unwrap, t_div, capacity, pl.tile_off, pl.wrap_off, pl.prev_t, count_status);
  if (pl.nb > 0)
    hipLaunchKernelGGL(aedat2_unpack_kernel, dim3((unsigned)pl.nb), dim3(kThreads), 0, stream, rec, n, h, w, layout, flip_x, flip_y,
                       unwrap, t_div, pl.tile_off, pl.wrap_off, pl.prev_t, t, x, y, p, capacity, count_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
