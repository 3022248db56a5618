// (t, x, y, p) on the device -> the bytes of an event file: the writers behind the text reader (events_csv.hip) and the emulator.
//
// Text.  A row is `t SEP a SEP b SEP p '\n'` with (a, b) = (x, y), or (y, x) with swap_xy; every value as C's "%d" prints it ('-'
// for negatives, no '+', no leading zeros), SEP one byte.  That is what `"%d %d %d %d\n" % row` of v2e/v2e.py:write_text gives,
// and it lies inside the grammar csv_parse_kernel accepts, so parse(format(cols)) == cols.  A row takes 8 ... 50 bytes.
//   text_len_kernel    a tile of 256 rows per workgroup, one row per thread: the row's length, the tile's byte sum
//   text_scan_kernel   scan_device.h's tile-count scan: int64 offsets of the tiles (one workgroup, 256 tiles per step),
//                      [n_bytes, 0] -> count_status
//   text_emit_kernel   the same lengths, an in-tile exclusive scan, then every thread renders its row into LDS at its in-tile
//                      offset.  The LDS image is shifted by (tile offset mod 16), so that after one barrier 16-byte pieces of
//                      LDS are 16-byte aligned pieces of the file: the workgroup streams them out with one 16-byte store per
//                      lane and writes the partial first and last piece by the byte.  Nothing is stored at or past `capacity`.
// A value is rendered from its unsigned magnitude (0 - (uint)v for negatives: INT64_MIN and INT32_MIN come out right), digits
// last to first by division by the constant 10 in 32 bits; a 64-bit magnitude of 2^32 or more is first cut into pieces of nine
// digits by division by the constant 10^9.
//
// AEDAT-2.0.  aedat2_pack_kernel writes per event two big-endian 32-bit words, address = xf << 12 | yf << 22 | p << 11 (uint32;
// xf = w - 1 - x, yf = h - 1 - y) and (int32) t, as one 8-byte store per lane.  Flags (x, y or p out of range; t outside
// [0, 2^31)) are OR-ed into the status word, and the index of the first event whose first byte is not '#' goes through an
// integer atomicMin: both are independent of the order.
// Integer work on fixed positions only: two runs on the same columns are bitwise equal.
#include "common.h"
#include "scan_device.h"

namespace scpose {

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kScanThreads, "the scan bodies of scan_device.h run in the workgroups of this file");
constexpr int kTileRows = kThreads;                  // one row per thread
constexpr int kMaxRow = 50;                          // 20 + 11 + 11 + 4 digits and signs, 3 separators, '\n'
constexpr int kStage = kTileRows * kMaxRow + 16;     // the tile's text, shifted by up to 15 bytes

inline int64_t tiles_of(int64_t n) { return (n + kTileRows - 1) / kTileRows; }

__device__ __forceinline__ int digits_u32(uint32_t v) {
  return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
         (v >= 100000000u) + (v >= 1000000000u);
}

__device__ __forceinline__ int digits_u64(uint64_t v) {
  if (v <= 0xffffffffull) return digits_u32((uint32_t)v);
  int d = 10;
  uint64_t p = 10000000000ull;                       // 10^10 ... 10^19 fit 64 bits
  while (d < 20 && v >= p) {
    ++d;
    p *= 10u;
  }
  return d;
}

// a value as sign + magnitude + digit count; the printed length is neg + nd
struct Num32 {
  uint32_t mag;
  int neg, nd;
};
struct Num64 {
  uint64_t mag;
  int neg, nd;
};

__device__ __forceinline__ Num32 num32(int32_t v) {
  Num32 r;
  r.neg = v < 0;
  r.mag = r.neg ? 0u - (uint32_t)v : (uint32_t)v;
  r.nd = digits_u32(r.mag);
  return r;
}

__device__ __forceinline__ Num64 num64(int64_t v) {
  Num64 r;
  r.neg = v < 0;
  r.mag = r.neg ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
  r.nd = digits_u64(r.mag);
  return r;
}

// nd digits of v, the last at s[end - 1]; leading zeros when v has fewer
__device__ __forceinline__ void put_u32(uint8_t* s, int end, uint32_t v, int nd) {
  for (int k = 0; k < nd; ++k) {
    const uint32_t q = v / 10u;
    s[--end] = (uint8_t)('0' + (v - q * 10u));
    v = q;
  }
}

__device__ __forceinline__ int put_num32(uint8_t* s, int pos, const Num32& a) {
  if (a.neg) s[pos++] = '-';
  put_u32(s, pos + a.nd, a.mag, a.nd);
  return pos + a.nd;
}

__device__ __forceinline__ int put_num64(uint8_t* s, int pos, const Num64& a) {
  if (a.neg) s[pos++] = '-';
  const int end = pos + a.nd;
  if (a.mag <= 0xffffffffull) {
    put_u32(s, end, (uint32_t)a.mag, a.nd);
  } else {                                           // 10 ... 20 digits: nine, then nine or fewer, then at most two
    const uint64_t rest = a.mag / 1000000000ull;     // <= 18446744073
    put_u32(s, end, (uint32_t)(a.mag - rest * 1000000000ull), 9);
    if (rest < 1000000000ull) {
      put_u32(s, end - 9, (uint32_t)rest, a.nd - 9);
    } else {
      const uint32_t hi = (uint32_t)(rest / 1000000000ull);
      put_u32(s, end - 9, (uint32_t)(rest - (uint64_t)hi * 1000000000ull), 9);
      put_u32(s, end - 18, hi, a.nd - 18);
    }
  }
  return end;
}

struct Row {
  Num64 t;
  Num32 a, b, p;
  int len;                                           // 0 for a thread past the last row
};

__device__ __forceinline__ Row load_row(const int64_t* __restrict__ t, const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                        const int8_t* __restrict__ p, int64_t i, int64_t n) {
  Row r;
  r.len = 0;
  if (i < n) {
    r.t = num64(t[i]);
    r.a = num32(a[i]);
    r.b = num32(b[i]);
    r.p = num32((int32_t)p[i]);
    r.len = r.t.neg + r.t.nd + r.a.neg + r.a.nd + r.b.neg + r.b.nd + r.p.neg + r.p.nd + 4;
  }
  return r;
}

__global__ __launch_bounds__(kThreads) void text_len_kernel(const int64_t* __restrict__ t, const int32_t* __restrict__ a,
                                                            const int32_t* __restrict__ b, const int8_t* __restrict__ p, int64_t n,
                                                            int32_t* __restrict__ tile_bytes) {
  __shared__ int32_t sc[kThreads];
  const Row r = load_row(t, a, b, p, (int64_t)blockIdx.x * kTileRows + threadIdx.x, n);
  const int32_t inc = block_inclusive_scan<0>(r.len, sc);
  if (threadIdx.x == kThreads - 1) tile_bytes[blockIdx.x] = inc;
}

// one workgroup: tile_off[b] = bytes before tile b; total[0] = bytes of the text; count_status <- [total, 0]
__global__ __launch_bounds__(kThreads) void text_scan_kernel(const int32_t* __restrict__ tile_bytes, int64_t nb,
                                                             int64_t* __restrict__ tile_off, int64_t* __restrict__ total,
                                                             int64_t* __restrict__ count_status) {
  __shared__ int32_t sc[kThreads];
  const int64_t bytes = scan_tile_counts(tile_bytes, nb, tile_off, sc);    // a step sums at most 256 * 256 * 50: fits int32
  if (threadIdx.x == 0) {
    total[0] = bytes;
    count_status[0] = bytes;
    count_status[1] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void text_emit_kernel(const int64_t* __restrict__ t, const int32_t* __restrict__ a,
                                                             const int32_t* __restrict__ b, const int8_t* __restrict__ p, int64_t n,
                                                             uint32_t sep, const int64_t* __restrict__ tile_off,
                                                             const int64_t* __restrict__ total, uint8_t* __restrict__ out,
                                                             int64_t capacity, int64_t* __restrict__ count_status) {
  __shared__ __attribute__((aligned(16))) uint8_t s[kStage];
  __shared__ int32_t sc[kThreads];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    count_status[0] = total[0];
    count_status[1] = total[0] > capacity ? SCPOSE_TEXT_CAPACITY : 0;
  }
  const Row r = load_row(t, a, b, p, (int64_t)blockIdx.x * kTileRows + threadIdx.x, n);
  const int32_t inc = block_inclusive_scan<0>(r.len, sc);
  sc[threadIdx.x] = inc;
  const int64_t base = tile_off[blockIdx.x];
  const int shift = (int)(base & 15);
  if (r.len) {
    int pos = shift + inc - r.len;                   // <= 15 + 255 * 50, and the row ends inside kStage
    pos = put_num64(s, pos, r.t);
    s[pos++] = (uint8_t)sep;
    pos = put_num32(s, pos, r.a);
    s[pos++] = (uint8_t)sep;
    pos = put_num32(s, pos, r.b);
    s[pos++] = (uint8_t)sep;
    pos = put_num32(s, pos, r.p);
    s[pos] = '\n';
  }
  __syncthreads();
  const int tile_len = sc[kThreads - 1];
  // LDS byte i is file byte g0 + i; the tile's text is LDS [shift, shift + tile_len), cut at the capacity
  const int64_t g0 = base - shift;
  const int64_t room = capacity - g0;
  const int vlo = shift;
  const int vhi = (int)(room < (int64_t)(shift + tile_len) ? (room > 0 ? room : 0) : (int64_t)(shift + tile_len));
  for (int c = threadIdx.x; c * 16 < vhi; c += kThreads) {
    const int lo = c * 16, hi = lo + 16;
    if (lo >= vlo && hi <= vhi) {
      *reinterpret_cast<uint4*>(out + g0 + lo) = *reinterpret_cast<const uint4*>(s + lo);
    } else {                                         // the tile's first and last piece
      const int k1 = hi < vhi ? hi : vhi;
      for (int k = lo > vlo ? lo : vlo; k < k1; ++k) out[g0 + k] = s[k];
    }
  }
}

__global__ void aedat2_init_kernel(int64_t n, int64_t* __restrict__ count_status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  count_status[0] = n;
  count_status[1] = 0;
  count_status[2] = n;                               // lead: the minimum over the events that do not start with '#'
}

__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

__global__ __launch_bounds__(kThreads) void aedat2_pack_kernel(const int64_t* __restrict__ t, const int32_t* __restrict__ x,
                                                               const int32_t* __restrict__ y, const int8_t* __restrict__ p, int64_t n,
                                                               int32_t h, int32_t w, uint2* __restrict__ out,
                                                               int64_t* __restrict__ count_status) {
  __shared__ unsigned long long s_first[kThreads / 64];
  __shared__ uint32_t s_flags[kThreads / 64];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  unsigned long long first = ~0ull;
  uint32_t flags = 0;
  if (i < n) {
    const int64_t tv = t[i];
    const int32_t xv = x[i], yv = y[i], pv = p[i];
    if (xv < 0 || xv >= w || yv < 0 || yv >= h || (pv != 0 && pv != 1)) flags |= SCPOSE_AEDAT2_RANGE;
    if (tv < 0 || tv > 2147483647ll) flags |= SCPOSE_AEDAT2_TIME;
    const uint32_t xf = (uint32_t)(w - 1 - xv), yf = (uint32_t)(h - 1 - yv);
    const uint32_t addr = (xf << 12) | (yf << 22) | ((uint32_t)pv << 11);
    out[i] = make_uint2(bswap32(addr), bswap32((uint32_t)tv));
    if ((addr >> 24) != 0x23u) first = (unsigned long long)i;      // the record's first byte in the file
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(first, off, 64);
    first = o < first ? o : first;
    flags |= __shfl_xor(flags, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_first[threadIdx.x >> 6] = first;
    s_flags[threadIdx.x >> 6] = flags;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kThreads / 64; ++k) {
      first = s_first[k] < first ? s_first[k] : first;
      flags |= s_flags[k];
    }
    unsigned long long* st = reinterpret_cast<unsigned long long*>(count_status);
    if (flags) atomicOr(st + 1, (unsigned long long)flags);
    // most workgroups find a smaller index already there and skip the atomic; the minimum is the same either way
    if (first != ~0ull && first < __atomic_load_n(st + 2, __ATOMIC_RELAXED)) atomicMin(st + 2, first);
  }
}

struct TextPlan {
  int64_t nb;
  int64_t* tile_off;
  int32_t* tile_bytes;
  int64_t* total;                                    // 256 bytes
  size_t bytes;
};

TextPlan text_plan(int64_t n, uint8_t* wsp) {
  TextPlan p{};
  p.nb = tiles_of(n);
  Carve c{wsp};
  p.tile_off = c.take<int64_t>(p.nb);
  p.tile_bytes = c.take<int32_t>(p.nb);
  p.total = c.take<int64_t>(32);
  p.bytes = c.bytes();
  return p;
}

}  // namespace

int events_text_tile_rows() { return kTileRows; }
int events_text_scan_rows() { return kTileRows * kScanThreads; }
size_t events_text_workspace_bytes(int64_t n) { return text_plan(n, nullptr).bytes; }

int32_t events_text_measure_launch(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n,
                                   int64_t* count_status, uint8_t* wsp, hipStream_t stream) {
  const TextPlan pl = text_plan(n, wsp);
  if (pl.nb > 0)
    hipLaunchKernelGGL(text_len_kernel, dim3((unsigned)pl.nb), dim3(kThreads), 0, stream, t, x, y, p, n, pl.tile_bytes);
  hipLaunchKernelGGL(text_scan_kernel, dim3(1), dim3(kThreads), 0, stream, pl.tile_bytes, pl.nb, pl.tile_off, pl.total, count_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t events_text_emit_launch(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n, int sep, int swap_xy,
                                uint8_t* out, int64_t capacity, int64_t* count_status, uint8_t* wsp, hipStream_t stream) {
  const TextPlan pl = text_plan(n, wsp);
  // n == 0: one workgroup without rows still writes count_status
  hipLaunchKernelGGL(text_emit_kernel, dim3((unsigned)(pl.nb > 0 ? pl.nb : 1)), dim3(kThreads), 0, stream, t, swap_xy ? y : x,
                     swap_xy ? x : y, p, n, (uint32_t)sep, pl.tile_off, pl.total, out, capacity, count_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t events_aedat2_pack_launch(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n, int h, int w,
                                  uint8_t* out, int64_t* count_status, hipStream_t stream) {
  hipLaunchKernelGGL(aedat2_init_kernel, dim3(1), dim3(64), 0, stream, n, count_status);
  if (n > 0)
    hipLaunchKernelGGL(aedat2_pack_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, t, x, y, p, n,
                       h, w, reinterpret_cast<uint2*>(out), count_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
