// events.csv -> (t, x, y, p) on the device: the text reader in front of the event renderer.
//
// The reference reads the file with pandas.read_csv(header=None, comment='#', sep=',' or whitespace, 4 names) and casts to
// int64 (v2e/e2v.py); event_render.read_events_csv is that call.  These kernels accept the subset of that reader's grammar on
// which a row is a function of its own line plus one flag per column (tests/events_csv_restated.py states it in full), and
// report everything else as "unsupported" in the status word -- never a different answer.  A line whose blanks and fields (the
// part before any '#') take 64 KiB or more is unsupported too: one thread walks a line, and its walk stays bounded.
//
//   line ends   every '\n' and every '\r' ends a line ('\r\n': a line end and an empty line); a line starts at byte 0 and after
//               every line end.  A line is a ROW when its first byte that is not a space / tab is none of '\n', '\r', '#'.
//   csv_count_kernel   a tile of 4096 bytes (+ 256 bytes of halo) goes through LDS; the thread that owns a line end classifies
//                      the line that starts after it; rows per tile
//   csv_scan_kernel    scan_device.h's tile-count scan: int64 offsets of the tiles (one workgroup), the total
//   csv_parse_kernel   the same classification, an in-tile exclusive scan of the per-thread row counts, then the owner of a row
//                      walks its line -- from LDS while it stays inside tile + halo, from global memory past that -- splits
//                      the four fields, converts and stores the row at its final index: file order, no compaction pass, no
//                      atomic in the data path.  Flags (unsupported input, '.' seen in column c, more than 15 digits in
//                      column c) are OR-ed into one workspace word: the OR of a set does not depend on the order.
//   csv_finish_kernel  one thread: [n_rows, status] from the total, the capacity and the flags
// A field with a '.' makes the reference's whole column float64 before the cast; with at most 15 digit characters in every field
// of such a column the float64 is within an ulp of the decimal, which is further than that from any integer it does not equal,
// and every integer of the column is below 2^53: the integer part as written is then the reference's value exactly.  A column
// with a '.' somewhere and a longer field somewhere is unsupported.
// Everything is integer work on fixed positions (the optional time-stamp division is one IEEE float64 division per row): two
// runs on the same bytes are bitwise equal.
#include "common.h"
#include "scan_device.h"

namespace scpose {

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kScanThreads, "the scan bodies of scan_device.h run in the workgroups of this file");
constexpr int kPerThread = 16;
constexpr int kTile = kThreads * kPerThread;   // 4096 bytes of text per workgroup
constexpr int kHalo = 256;                     // bytes after the tile kept in LDS: a line that starts in the tile ends there
constexpr int kStage = kTile + kHalo;

constexpr uint32_t kFlagBad = 1u;              // unsupported input
constexpr int kDotShift = 4;                   // bit (4 + c): a '.' in file column c
constexpr int kLongShift = 8;                  // bit (8 + c): a field of more than 15 digit characters in file column c
constexpr int kMaxFloatDigits = 15;
constexpr int64_t kMaxLine = 65536;            // one thread walks a line: a longer walk (blanks, digits) stops and is unsupported

inline int64_t tiles_of(int64_t n) { return n > 0 ? (n + kTile - 1) / kTile : 1; }

// tile + halo -> LDS, 16 bytes per load; bytes at and past n read as '\n'
__device__ __forceinline__ void stage_tile(const uint8_t* __restrict__ data, int64_t n, int64_t base, uint8_t* s) {
  for (int c = threadIdx.x; c < kStage / 16; c += kThreads) {
    const int64_t o = base + (int64_t)c * 16;
    uint4 v = make_uint4(0x0a0a0a0au, 0x0a0a0a0au, 0x0a0a0a0au, 0x0a0a0a0au);
    if (o + 16 <= n) {
      v = *reinterpret_cast<const uint4*>(data + o);
    } else if (o < n) {
      uint32_t w[4] = {0x0a0a0a0au, 0x0a0a0a0au, 0x0a0a0a0au, 0x0a0a0a0au};
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (o + k < n) w[k >> 2] = (w[k >> 2] & ~(0xffu << (8 * (k & 3)))) | ((uint32_t)data[o + k] << (8 * (k & 3)));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(s + c * 16) = v;
  }
  __syncthreads();
}

struct Reader {
  const uint8_t* s;      // LDS copy of [base, base + kStage)
  const uint8_t* g;
  int64_t base, n;
  __device__ __forceinline__ uint32_t operator()(int64_t p) const {
    const int64_t d = p - base;
    if (d < kStage) return s[d];
    return p < n ? g[p] : (uint32_t)'\n';
  }
};

__device__ __forceinline__ bool is_blank(uint32_t c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ bool is_end(uint32_t c) { return c == '\n' || c == '\r'; }
__device__ __forceinline__ bool is_digit(uint32_t c) { return c - (uint32_t)'0' < 10u; }

// the line that starts at byte `start` (after_cr: the byte before it is '\r'): is it a row?  flags <- what the reference's
// tokenizer does not treat as this grammar does: blanks then '#' (a row of one blank field in comma mode), and after a '\r'
// without '\n' a row that starts with a blank (comma mode) or a line of blanks (whitespace mode)
__device__ __forceinline__ bool line_is_row(const Reader& rd, int64_t start, bool after_cr, bool ws_mode, uint32_t& flags) {
  int64_t p = start;
  const int64_t lim = start + kMaxLine;
  uint32_t c = rd(p);
  while (is_blank(c) && p < lim) c = rd(++p);
  if (p >= lim) {
    flags |= kFlagBad;
    return false;
  }
  const bool lead = p > start;
  if (is_end(c)) {
    if (lead && after_cr && ws_mode) flags |= kFlagBad;
    return false;
  }
  if (c == '#') {
    if (lead) flags |= kFlagBad;
    return false;
  }
  if (lead && after_cr && !ws_mode) flags |= kFlagBad;
  return true;
}

// bit 0: the line at byte 0 (tile 0, thread 0 only); bit k + 1: the line after this thread's byte k
__device__ __forceinline__ uint32_t thread_rows(const Reader& rd, const uint8_t* s, int64_t base, bool ws_mode, uint32_t& flags) {
  uint32_t mask = 0;
  const int64_t mine = base + (int64_t)threadIdx.x * kPerThread;
  if (mine == 0 && line_is_row(rd, 0, false, ws_mode, flags)) mask |= 1u;
  const uint4 v = *reinterpret_cast<const uint4*>(s + threadIdx.x * kPerThread);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    if (is_end(c) && mine + k < rd.n && line_is_row(rd, mine + k + 1, c == '\r', ws_mode, flags)) mask |= 2u << k;
  }
  return mask;
}

__global__ __launch_bounds__(kThreads) void csv_count_kernel(const uint8_t* __restrict__ data, int64_t n, int ws_mode,
                                                             int32_t* __restrict__ tile_rows) {
  __shared__ __attribute__((aligned(16))) uint8_t s[kStage];
  __shared__ int32_t sc[kThreads];
  const int64_t base = (int64_t)blockIdx.x * kTile;
  stage_tile(data, n, base, s);
  const Reader rd{s, data, base, n};
  uint32_t flags = 0;
  const int32_t rows = __popc(thread_rows(rd, s, base, ws_mode != 0, flags));
  const int32_t inc = block_inclusive_scan<0>(rows, sc);
  if (threadIdx.x == kThreads - 1) tile_rows[blockIdx.x] = inc;
}

// one workgroup: tile_off[b] = rows before tile b; total[0] = rows of the file
__global__ __launch_bounds__(kThreads) void csv_scan_kernel(const int32_t* __restrict__ tile_rows, int64_t nb,
                                                            int64_t* __restrict__ tile_off, int64_t* __restrict__ total) {
  __shared__ int32_t sc[kThreads];
  const int64_t rows = scan_tile_counts(tile_rows, nb, tile_off, sc);      // a step sums at most 256 * 4097: fits int32
  if (threadIdx.x == 0) total[0] = rows;
}

// one field: [+-]? digits [. digits] | [+-]? . digits.  p is left on the first byte after it.  The value is the integer part
// with the sign (truncation toward zero).
__device__ __forceinline__ int64_t parse_field(const Reader& rd, int64_t& p, int64_t lim, int col, uint32_t& flags) {
  uint32_t c = rd(p);
  const bool neg = c == '-';
  if (c == '-' || c == '+') c = rd(++p);
  uint64_t acc = 0;
  int digits = 0, significant = 0;
  while (is_digit(c) && p < lim) {
    ++digits;
    if (significant > 0 || c != '0') ++significant;
    acc = acc * 10u + (c - '0');            // wraps only past 19 significant digits, which are flagged below
    c = rd(++p);
  }
  if (c == '.') {
    flags |= 1u << (kDotShift + col);
    c = rd(++p);
    while (is_digit(c) && p < lim) {
      ++digits;
      c = rd(++p);
    }
  }
  if (digits == 0) flags |= kFlagBad;
  if (digits > kMaxFloatDigits) flags |= 1u << (kLongShift + col);
  const uint64_t limit = neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1;
  if (significant > 19 || acc > limit) {
    flags |= kFlagBad;
    acc = 0;
  }
  return neg ? (int64_t)(0 - acc) : (int64_t)acc;
}

__device__ __forceinline__ bool line_done(uint32_t c) { return is_end(c) || c == '#'; }

__global__ __launch_bounds__(kThreads) void csv_parse_kernel(const uint8_t* __restrict__ data, int64_t n, int ws_mode, double t_div,
                                                             const int64_t* __restrict__ tile_off, int64_t capacity,
                                                             int64_t* __restrict__ t, int32_t* __restrict__ c1,
                                                             int32_t* __restrict__ c2, int8_t* __restrict__ pol,
                                                             uint32_t* __restrict__ flags_out) {
  __shared__ __attribute__((aligned(16))) uint8_t s[kStage];
  __shared__ int32_t sc[kThreads];
  const int64_t base = (int64_t)blockIdx.x * kTile;
  stage_tile(data, n, base, s);
  const Reader rd{s, data, base, n};
  const bool ws = ws_mode != 0;
  uint32_t flags = 0;
  uint32_t mask = thread_rows(rd, s, base, ws, flags);
  const int32_t rows = __popc(mask);
  int64_t row = tile_off[blockIdx.x] + block_inclusive_scan<0>(rows, sc) - rows;
  const int64_t mine = base + (int64_t)threadIdx.x * kPerThread;
  while (mask) {
    const int bit = __ffs(mask) - 1;
    mask &= mask - 1;
    int64_t p = bit == 0 ? 0 : mine + bit;      // bit k + 1: the line starts after byte k
    const int64_t lim = p + kMaxLine;
    int64_t v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      uint32_t c = rd(p);
      while (is_blank(c) && p < lim) c = rd(++p);
      v[f] = parse_field(rd, p, lim, f, flags);
      c = rd(p);
      if (f < 3) {
        if (ws) {
          if (!is_blank(c)) flags |= kFlagBad;          // the run is skipped in front of the next field
        } else {
          while (is_blank(c) && p < lim) c = rd(++p);
          if (c != ',') flags |= kFlagBad;
          ++p;
        }
        // a line that ends early must not run into the next one: stop on its end, the row is flagged already
        if (line_done(c)) break;
      } else {
        while (is_blank(c) && p < lim) c = rd(++p);
        if (!line_done(c)) flags |= kFlagBad;
      }
      if (p >= lim) {            // the walk was cut short: whatever was read so far is not the row
        flags |= kFlagBad;
        break;
      }
    }
    if (v[1] != (int32_t)v[1] || v[2] != (int32_t)v[2] || v[3] != (int8_t)v[3]) flags |= kFlagBad;
    if (row < capacity) {
      t[row] = t_div != 0.0 ? (int64_t)((double)v[0] / t_div) : v[0];
      c1[row] = (int32_t)v[1];
      c2[row] = (int32_t)v[2];
      pol[row] = (int8_t)v[3];
    }
    ++row;
  }
  if (flags) atomicOr(flags_out, flags);
}

__global__ void csv_finish_kernel(const int64_t* __restrict__ total, const uint32_t* __restrict__ flags, int64_t capacity,
                                  int64_t* __restrict__ count_status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t f = flags[0];
  int64_t status = 0;
  if ((f & kFlagBad) || ((f >> kDotShift) & (f >> kLongShift) & 0xfu)) status = SCPOSE_CSV_UNSUPPORTED;
  else if (total[0] > capacity) status = SCPOSE_CSV_CAPACITY;
  count_status[0] = status == 0 ? total[0] : 0;
  count_status[1] = status;
}

struct CsvPlan {
  int64_t nb;
  int32_t* tile_rows;
  int64_t *tile_off, *total;                    // total: 256 bytes, the int64 total and the uint32 flags
  size_t bytes;
};

CsvPlan csv_plan(int64_t n_bytes, uint8_t* wsp) {
  CsvPlan p{};
  p.nb = tiles_of(n_bytes);
  Carve c{wsp};
  p.tile_rows = c.take<int32_t>(p.nb);
  p.tile_off = c.take<int64_t>(p.nb);
  p.total = c.take<int64_t>(32);
  p.bytes = c.bytes();
  return p;
}

}  // namespace

size_t events_csv_workspace_bytes(int64_t n_bytes) { return csv_plan(n_bytes, nullptr).bytes; }

int32_t events_csv_parse_launch(const uint8_t* data, int64_t n_bytes, int ws_mode, int swap_xy, double t_div, int64_t* t, int32_t* x,
                                int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status, uint8_t* wsp, hipStream_t stream) {
  const CsvPlan pl = csv_plan(n_bytes, wsp);
  int32_t* tile_rows = pl.tile_rows;
  int64_t *tile_off = pl.tile_off, *total = pl.total;
  uint32_t* flags = reinterpret_cast<uint32_t*>(total + 1);
  SCP_CHECK_HIP(hipMemsetAsync(total, 0, 256, stream));
  hipLaunchKernelGGL(csv_count_kernel, dim3((unsigned)pl.nb), dim3(kThreads), 0, stream, data, n_bytes, ws_mode, tile_rows);
  hipLaunchKernelGGL(csv_scan_kernel, dim3(1), dim3(kThreads), 0, stream, tile_rows, pl.nb, tile_off, total);
  hipLaunchKernelGGL(csv_parse_kernel, dim3((unsigned)pl.nb), dim3(kThreads), 0, stream, data, n_bytes, ws_mode, t_div, tile_off,
                     capacity, t, swap_xy ? y : x, swap_xy ? x : y, p, flags);
  hipLaunchKernelGGL(csv_finish_kernel, dim3(1), dim3(64), 0, stream, total, flags, capacity, count_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
