// Baseline JPEG files -> (N, H, W, 3) uint8 frames on the device: the decoder in front of crop.hip.  The host (jpeg_read.py) walks
// the markers and packs one descriptor per image (tables) and one row per restart segment; everything from the entropy-coded bytes
// to the pixels happens here, in integers, bit for bit what libjpeg's baseline decoder computes (jdhuff.c, jidctint.c's
// jpeg_idct_islow, jdsample.c's h2v2_fancy_upsample, jdcolor.c's ycc_rgb_convert).
//
// A Huffman stream has no entry points.  Every restart segment is cut into subsequences of kS raw bytes; subsequence i owns the
// code words that START inside it.  The state between two code words is (d, blk, k): bits past the start of the subsequence, block
// inside the MCU (it selects the component and so the tables), zig-zag index inside the block.  entry[0] of a segment is (0, 0, 0);
// the true entry[i + 1] is exit(i, entry[i]).  Relaxation finds that fixed point without a sequential walk:
//   jpeg_relax_kernel, launch L = 1 .. max_rounds.  L = 1: every thread decodes its subsequence from (0, 0, 0).  L > 1: only a
//       thread whose entry changed in launch L - 1.  A thread publishes its exit only when it differs from the one it published
//       before.  A slot is one 64-bit word {cur, prev, launch of cur, launch of prev}: a reader that finds "launch of cur == L"
//       met a writer of its own launch and takes prev, so a launch reads exactly what the launch before left (Jacobi) and the
//       number of rounds is a function of the data alone.  An idle workgroup leaves before it loads a table.
//   jpeg_scan_kernel    per image (scan_device.h): exclusive scan of the blocks completed per subsequence, the rounds used, and
//       NOT_CONVERGED when a slot still changed in the last launch.
//   jpeg_write_kernel   the same walk from the converged entries: non-zero coefficients -> coef[block][natural index] (int16, zeroed
//       before), DC differences -> dc[block].  Every store is guarded by the end of the block's own restart segment; a segment
//       that completes another number of blocks than the header implies, a code no table holds and a run past index 63 set CORRUPT.
//   jpeg_dc_kernel      per image and component: inclusive sum of the DC differences in scan order, in place.  The IDCT takes
//       prefix[j] - prefix[start of j's restart segment - 1]: segments are equally long.
//   jpeg_idct_kernel    one thread per block: de-quantise, ISLOW inverse DCT in registers, range limit, 8 x 8 bytes into the
//       component's plane (padded to whole MCUs).
//   jpeg_output_kernel  four pixels per thread: fancy h2v2 chroma upsampling (4:2:0), colour conversion, crop to H x W.
// scpose_jpeg_decode_crop ends differently: it wants the crop_warp of each frame (crop.hip), not the frame.  The passes up to the
// DC sums run on the whole frame as above -- the entropy-coded bytes have no entry points and a DC value needs every block before
// it -- and then
//   jpeg_idct_window_kernel  the same inverse DCT, for the blocks that hold a sample the crop can read (sample_span below)
//   jpeg_crop_kernel         the decoders' shared crop tail (crop_tail.h) over jpeg_pixel(), the arithmetic of jpeg_output_kernel, as
//       its pixel source.  No frame is written; a sample outside the window stays uninitialised and is never read.
// A speculative walk from a wrong state decodes garbage by design: every iteration consumes at least one bit, the walk ends with
// the subsequence (plus one code word) or the segment, zeros are fed past the end of the data, and nothing but the thread's own
// slot and count is written.  No code word starts in the encoder's fill bits (the last min(7, trailing ones) bits of a segment):
// no Huffman code is all ones.  No floating point, no atomics but integer ORs into status; two runs are bitwise equal.
#include "jpeg_common.h"
#include "scan_device.h"
#include "crop_tail.h"

namespace scpose {

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kScanThreads, "the scan bodies of scan_device.h run in the workgroups of this file");
constexpr int kS = SCPOSE_JPEG_SUBSEQ_BYTES;
constexpr int kDesc = SCPOSE_JPEG_DESC_BYTES;
constexpr int kQuantOff = 64, kTablesOff = 448, kSlot = 1424, kSlots = 6;
constexpr int kTableWords = kSlots * kSlot / 4;
static_assert(kTablesOff + kSlots * kSlot <= kDesc, "the tables fit the descriptor");

struct Geo {
  int32_t n, h, w, mode, bpm, ycount, hs, mcus_x, mcus_y, n_mcus, n_blocks, max_subs, pw, ph, pcw, pch;
  int64_t n_bytes, n_rows;
};

Geo make_geo(int n, int h, int w, int mode, int max_subs, int64_t n_bytes, int64_t n_rows) {
  const JpegFrame f = jpeg_frame(h, w, mode);
  Geo g{};
  g.n = n; g.h = h; g.w = w; g.mode = mode; g.max_subs = max_subs; g.n_bytes = n_bytes; g.n_rows = n_rows;
  g.hs = f.hs; g.ycount = f.ycount; g.bpm = f.bpm; g.mcus_x = f.mcus_x; g.mcus_y = f.mcus_y; g.n_mcus = f.n_mcus; g.n_blocks = f.n_blocks;
  g.pw = g.mcus_x * 8 * g.hs; g.ph = g.mcus_y * 8 * g.hs;
  g.pcw = g.mcus_x * 8; g.pch = g.mcus_y * 8;
  return g;
}

// ---- one subsequence: where it lies
struct Sub {
  const uint8_t* p;      // first raw byte of the restart segment
  int32_t len;           // raw bytes of the segment
  int32_t start, end;    // raw bytes [start, end) of the subsequence inside the segment; end may lie past len
  int32_t pad;           // fill bits at the end of the segment
  int32_t seg, ri, next_first;
  bool first, last;
};

__device__ __forceinline__ bool sub_setup(const uint8_t* __restrict__ desc, const int32_t* __restrict__ segs, const uint8_t* __restrict__ data,
                                          const Geo& geo, int img, int g, Sub& s) {
  const int32_t* head = reinterpret_cast<const int32_t*>(desc + (size_t)img * kDesc);
  const int64_t file_off = *reinterpret_cast<const int64_t*>(head);
  const int32_t row0 = head[2], nseg = head[3], nsub = head[4];
  s.ri = head[5];
  if (g >= nsub || nsub > geo.max_subs || nseg < 1 || row0 < 0 || (int64_t)row0 + nseg + 1 > geo.n_rows || s.ri < 1) return false;
  const int32_t* rows = segs + 4 * (size_t)row0;
  int lo = 0, hi = nseg - 1;                           // the last segment whose first subsequence is <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[4 * mid + 2] <= g) lo = mid; else hi = mid - 1;
  }
  const int32_t a = rows[4 * lo], b = rows[4 * lo + 1], i = g - rows[4 * lo + 2];
  s.next_first = rows[4 * lo + 6];
  s.seg = lo;
  const bool ok = a >= 0 && b >= a && file_off >= 0 && file_off + b <= geo.n_bytes && i >= 0 && (int64_t)i * kS < (int64_t)(b - a) + (b == a);
  s.len = ok ? b - a : 0;                              // a row that points outside the bytes: an empty segment (its count is then wrong: CORRUPT)
  s.p = data + (ok ? file_off + a : 0);
  s.first = i == 0;
  s.last = g + 1 >= s.next_first;
  s.start = ok ? i * kS : 0;
  s.end = s.start + kS;
  if (s.start > 0 && s.start < s.len && s.p[s.start] == 0 && s.p[s.start - 1] == 0xFF) ++s.start;   // a stuffed zero: one byte later
  s.pad = 0;
  if (s.len > 0) {
    uint32_t lastb = s.p[s.len - 1];
    if (lastb == 0 && s.len >= 2 && s.p[s.len - 2] == 0xFF) lastb = 0xFF;
    const int t = __builtin_ctz(~lastb);               // trailing ones; ~lastb has bits above bit 7 set
    s.pad = t < 7 ? t : 7;
  }
  return true;
}

// ---- bit reader: MSB first in acc, the stuffed 00 after an FF skipped while refilling, zeros fed past the segment
struct Reader {
  const uint8_t* p;
  int32_t bp, sub_end, len, pad;
  uint64_t acc;
  int32_t nbits, loaded, bound, limit;
  bool ended;
  __device__ __forceinline__ void init(const Sub& s) {
    p = s.p; bp = s.start; sub_end = s.end; len = s.len; pad = s.pad;
    acc = 0; nbits = 0; loaded = 0; bound = INT_MAX; limit = INT_MAX; ended = false;
  }
  __device__ __forceinline__ void refill() {
    while (nbits <= 56) {
      if (bp >= sub_end && bound == INT_MAX) {         // the next subsequence starts at this data bit
        bound = loaded;
        if (limit > loaded) limit = loaded;
      }
      uint32_t c = 0;
      if (bp >= len) {
        if (!ended) {
          ended = true;
          if (bound == INT_MAX) bound = loaded;
          if (limit > loaded - pad) limit = loaded - pad;
        }
      } else {
        c = p[bp++];
        if (c == 0xFF) ++bp;                           // inside a segment an FF is followed by its stuffed 00
      }
      acc |= (uint64_t)c << (56 - nbits);
      nbits += 8;
      loaded += 8;
    }
  }
  __device__ __forceinline__ int32_t at() const { return loaded - nbits; }
  __device__ __forceinline__ void drop(int n) { acc <<= n; nbits -= n; }
};

// state word: d (5 bits) | blk << 5 (3 bits) | k << 8 (6 bits); 0 is the entry of a segment
struct Walk {
  int32_t blk, k, blocks;
  bool bad;
};

// The walk of one subsequence from `entry`.  WRITE: store what the owned code words decode to.
template <bool WRITE>
__device__ __forceinline__ uint32_t walk(const Sub& s, uint32_t entry, const Geo& geo, const uint32_t* tab, Walk& wk, int64_t block0,
                                          int64_t block_end, int16_t* __restrict__ coef, int32_t* __restrict__ dc) {
  const uint16_t* tab16 = reinterpret_cast<const uint16_t*>(tab);
  const uint8_t* tab8 = reinterpret_cast<const uint8_t*>(tab);
  Reader r;
  r.init(s);
  r.refill();
  r.drop((int)(entry & 31u));
  int blk = (int)((entry >> 5) & 7u), k = (int)((entry >> 8) & 63u), blocks = 0;
  bool bad = false;
  for (;;) {
    r.refill();
    if (r.at() >= r.limit) break;
    const uint32_t w = (uint32_t)(r.acc >> 32);
    const int slot = SCP_MCU_COMP_INDEX(blk, geo.ycount) * 2 + (k != 0);
    const uint32_t e = tab16[slot * (kSlot / 2) + (w >> 23)];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (len == 0) {                                    // longer than 9 bits: libjpeg's maxcode / valoffset
      const int32_t* mc = reinterpret_cast<const int32_t*>(tab) + slot * (kSlot / 4) + 256;
      const uint32_t c16 = w >> 16;
      int l = 10;
      while (l <= 16 && (int32_t)(c16 >> (16 - l)) > mc[l]) ++l;
      if (l > 16) {
        bad = true;                                    // no such code: 16 bits, symbol 0
        len = 16; sym = 0;
      } else {
        len = l;
        sym = tab8[slot * kSlot + 1168 + (((int32_t)(c16 >> (16 - l)) + mc[18 + l]) & 255)];
      }
    }
    const int sz = sym & 15, run = k == 0 ? 0 : sym >> 4;
    int32_t v = 0;
    if (sz) {
      v = (int32_t)((w << len) >> (32 - sz));
      if (v < (1 << (sz - 1))) v += 1 - (1 << sz);
    }
    r.drop(len + sz);
    int at = -1;                                       // zig-zag index that receives v
    if (sz) { k += run; at = k; ++k; }
    else if (k == 0) { at = 0; k = 1; }
    else if (run == 15) k += 16;
    else k = 64;
    if (WRITE && at >= 0) {
      const int64_t b = block0 + blocks;
      if (at > 63) bad = true;
      else if (b < block_end) {
        if (at == 0) dc[b] = v;
        else if (v != 0) coef[b * 64 + kZigzag[at]] = (int16_t)v;
      }
    }
    if (k >= 64) {
      k = 0;
      blk = blk + 1 == geo.bpm ? 0 : blk + 1;
      ++blocks;
    }
  }
  wk.blk = blk; wk.k = k; wk.blocks = blocks; wk.bad = bad;
  int d = r.at() - r.bound;
  d = d < 0 ? 0 : (d > 31 ? 31 : d);
  return (uint32_t)d | ((uint32_t)blk << 5) | ((uint32_t)k << 8);
}

__device__ __forceinline__ void load_tables(const uint8_t* __restrict__ desc, int img, uint32_t* tab) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(desc + (size_t)img * kDesc + kTablesOff);
  for (int i = threadIdx.x; i < kTableWords; i += kThreads) tab[i] = src[i];
}

__device__ __forceinline__ unsigned long long slot_load(const unsigned long long* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void slot_store(unsigned long long* p, unsigned long long v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

__global__ __launch_bounds__(kThreads) void jpeg_relax_kernel(const uint8_t* __restrict__ desc, const int32_t* __restrict__ segs,
                                                              const uint8_t* __restrict__ data, Geo geo, int launch,
                                                              unsigned long long* slots, int32_t* __restrict__ counts) {
  __shared__ uint32_t tab[kTableWords];
  const int img = blockIdx.y, g = blockIdx.x * kThreads + threadIdx.x;
  Sub s;
  bool active = sub_setup(desc, segs, data, geo, img, g, s);
  const size_t at = (size_t)img * geo.max_subs + g;
  uint32_t entry = 0;
  if (active && launch > 1) {
    if (s.first) {
      active = false;
    } else {
      const unsigned long long v = slot_load(slots + at - 1);
      const bool mine = (int)((v >> 32) & 255u) == launch;             // written in this very launch: take what was there before
      entry = (uint32_t)(mine ? v >> 16 : v) & 0xffffu;
      active = (int)((mine ? v >> 40 : v >> 32) & 255u) == launch - 1;
    }
  }
  if (!__syncthreads_or(active)) return;
  load_tables(desc, img, tab);
  __syncthreads();
  if (!active) return;
  Walk wk;
  const uint32_t exit_state = walk<false>(s, entry, geo, tab, wk, 0, 0, nullptr, nullptr);
  counts[at] = wk.blocks;
  if (!s.last) {
    const unsigned long long own = slot_load(slots + at);
    const uint32_t cur = (uint32_t)own & 0xffffu;
    if (exit_state != cur)
      slot_store(slots + at, (unsigned long long)exit_state | ((unsigned long long)cur << 16) | ((unsigned long long)launch << 32) |
                                 (((own >> 32) & 255ull) << 40));
  }
}

// one workgroup per image
__global__ __launch_bounds__(kThreads) void jpeg_scan_kernel(const uint8_t* __restrict__ desc, Geo geo, int max_rounds,
                                                             const unsigned long long* __restrict__ slots, int32_t* counts,
                                                             int32_t* __restrict__ totals, int32_t* __restrict__ status) {
  __shared__ int32_t sc[kThreads];
  __shared__ int32_t s_last;
  const int img = blockIdx.x;
  const int32_t* head = reinterpret_cast<const int32_t*>(desc + (size_t)img * kDesc);
  const bool ok = head[4] >= 1 && head[4] <= geo.max_subs;
  const int32_t nsub = ok ? head[4] : 0;
  const size_t base = (size_t)img * geo.max_subs;
  int32_t changed = 0;                                                 // the last launch in which an entry changed
  for (int g = threadIdx.x; g < nsub; g += kThreads) {
    const int32_t c = (int32_t)((slots[base + g] >> 32) & 255u);
    changed = c > changed ? c : changed;
  }
  const int32_t m = block_inclusive_scan<1>(-changed, sc);
  if (threadIdx.x == kThreads - 1) s_last = -m;
  const int32_t total = scan_aggregates<0>(counts + base, nsub, sc);   // a batch's blocks fit int32 (api.cpp)
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t last = s_last;
    const int32_t rounds = last + 1 < max_rounds ? last + 1 : max_rounds;
    totals[img] = total;
    status[img] = (rounds << 8) | (last >= max_rounds ? SCPOSE_JPEG_NOT_CONVERGED : 0) | (ok ? 0 : SCPOSE_JPEG_CORRUPT);
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_write_kernel(const uint8_t* __restrict__ desc, const int32_t* __restrict__ segs,
                                                              const uint8_t* __restrict__ data, Geo geo,
                                                              const unsigned long long* __restrict__ slots,
                                                              const int32_t* __restrict__ prefix, const int32_t* __restrict__ totals,
                                                              int16_t* __restrict__ coef, int32_t* __restrict__ dc, int32_t* status) {
  __shared__ uint32_t tab[kTableWords];
  const int img = blockIdx.y, g = blockIdx.x * kThreads + threadIdx.x;
  Sub s;
  const bool active = sub_setup(desc, segs, data, geo, img, g, s);
  if (!__syncthreads_or(active)) return;
  load_tables(desc, img, tab);
  __syncthreads();
  if (!active) return;
  const size_t base = (size_t)img * geo.max_subs;
  const int32_t nsub = reinterpret_cast<const int32_t*>(desc + (size_t)img * kDesc)[4];
  const uint32_t entry = s.first ? 0u : (uint32_t)slots[base + g - 1] & 0xffffu;
  const int64_t per_seg = (int64_t)s.ri * geo.bpm;
  int64_t b0 = (int64_t)s.seg * per_seg, b1 = b0 + per_seg;
  b0 = b0 < geo.n_blocks ? b0 : geo.n_blocks;
  b1 = b1 < geo.n_blocks ? b1 : geo.n_blocks;
  // blocks of this segment before subsequence g: prefix[g] - prefix[first subsequence of the segment]
  const int32_t* rows = segs + 4 * (size_t)reinterpret_cast<const int32_t*>(desc + (size_t)img * kDesc)[2];
  const int32_t seg_first = rows[4 * s.seg + 2];
  const int64_t img_block0 = (int64_t)img * geo.n_blocks;
  const int64_t before = (int64_t)prefix[base + g] - prefix[base + seg_first];
  Walk wk;
  walk<true>(s, entry, geo, tab, wk, img_block0 + b0 + before, img_block0 + b1, coef, dc);
  bool corrupt = wk.bad;
  if (s.first) {
    const int32_t upto = s.next_first < nsub ? prefix[base + s.next_first] : totals[img];
    if ((int64_t)upto - prefix[base + g] != b1 - b0) corrupt = true;
  }
  if (corrupt) atomicOr(status + img, SCPOSE_JPEG_CORRUPT);
}

// one workgroup per (component, image): dc[] of the component's blocks, in scan order, <- inclusive sums
__global__ __launch_bounds__(kThreads) void jpeg_dc_kernel(Geo geo, int32_t* dc) {
  __shared__ int32_t sc[kThreads];
  const int img = blockIdx.y;
  const McuComp mc = mcu_comp(blockIdx.x, geo.ycount);
  const int32_t total = geo.n_mcus * mc.count;
  int32_t* d = dc + (size_t)img * geo.n_blocks;
  int32_t carry = 0;
  for (int32_t j0 = 0; j0 < total; j0 += kThreads) {
    const int32_t j = j0 + threadIdx.x;
    const int32_t b = j < total ? (j / mc.count) * geo.bpm + mc.first + j % mc.count : 0;
    const int32_t v = j < total ? d[b] : 0;
    const int32_t inc = block_inclusive_scan<0>(v, sc);
    sc[threadIdx.x] = inc;
    __syncthreads();
    const int32_t chunk = sc[kThreads - 1];
    __syncthreads();
    if (j < total) d[b] = carry + inc;
    carry += chunk;
  }
}

// jidctint.c's jpeg_idct_islow (the constants: jpeg_common.h)
template <int SHIFT>
__device__ __forceinline__ void idct_1d(const int32_t (&in)[8], int32_t (&out)[8]) {
  int32_t z2 = in[2], z3 = in[6];
  int32_t z1 = (z2 + z3) * F0541;
  int32_t tmp2 = z1 + z3 * (-F1847);
  int32_t tmp3 = z1 + z2 * F0765;
  z2 = in[0]; z3 = in[4];
  int32_t tmp0 = (z2 + z3) * (1 << 13), tmp1 = (z2 - z3) * (1 << 13);
  const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  int32_t z4 = tmp1 + tmp3;
  const int32_t z5 = (z3 + z4) * F1175;
  tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
  z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  constexpr int32_t half = 1 << (SHIFT - 1);
  out[0] = (tmp10 + tmp3 + half) >> SHIFT;
  out[7] = (tmp10 - tmp3 + half) >> SHIFT;
  out[1] = (tmp11 + tmp2 + half) >> SHIFT;
  out[6] = (tmp11 - tmp2 + half) >> SHIFT;
  out[2] = (tmp12 + tmp1 + half) >> SHIFT;
  out[5] = (tmp12 - tmp1 + half) >> SHIFT;
  out[3] = (tmp13 + tmp0 + half) >> SHIFT;
  out[4] = (tmp13 - tmp0 + half) >> SHIFT;
}

__device__ __forceinline__ uint32_t limit8(int32_t v) {
  v += 128;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The samples [lo, hi] of one axis of a component's plane that the pixels [p0, p0 + len) of that axis read (hi < lo: none).
// Luma, and chroma at 4:4:4 (`half` false): the pixel's own sample.  Chroma at 4:2:0: chroma420() below reads sample p >> 1 and,
// per axis, its neighbour on one side or the other, never one outside the plane of ceil(full / 2) samples -- so one sample more on
// each side, clamped at the plane's edge.  jpeg_read.py: sample_span says the same to the host and the tests.
struct Span {
  int32_t lo, hi;
};
__device__ __forceinline__ Span sample_span(int32_t p0, int32_t len, int32_t full, bool half) {
  if (len <= 0) return {0, -1};
  if (!half) return {p0, p0 + len - 1};
  const int32_t lo = (p0 >> 1) - 1, hi = ((p0 + len - 1) >> 1) + 1, last = ((full + 1) >> 1) - 1;
  return {lo < 0 ? 0 : lo, hi > last ? last : hi};
}

// One thread per block of image `img`.  WINDOW: only a block that holds a sample the pixels of roi = [x0, y0, w, h] read.
template <bool WINDOW>
__device__ __forceinline__ void idct_blocks(const uint8_t* __restrict__ desc, const Geo& geo, const int16_t* __restrict__ coef,
                                            const int32_t* __restrict__ dc, uint8_t* __restrict__ plane_y, uint8_t* __restrict__ plane_c,
                                            int img, const int32_t* roi) {
  __shared__ int32_t q[3][64];
  const int32_t* head = reinterpret_cast<const int32_t*>(desc + (size_t)img * kDesc);
  const uint16_t* qsrc = reinterpret_cast<const uint16_t*>(desc + (size_t)img * kDesc + kQuantOff);
  if (threadIdx.x < 192) q[threadIdx.x >> 6][threadIdx.x & 63] = qsrc[threadIdx.x];
  __syncthreads();
  const int32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= geo.n_blocks) return;
  const int32_t mcu = b / geo.bpm, blk = b - mcu * geo.bpm;
  const McuComp mc = mcu_comp_of_block(blk, geo.ycount);
  const int comp = mc.comp;
  const int32_t mx = mcu % geo.mcus_x, my = mcu / geo.mcus_x;
  const int32_t bx = comp == 0 ? mx * geo.hs + blk % geo.hs : mx, by = comp == 0 ? my * geo.hs + blk / geo.hs : my;   // in the component's plane
  if (WINDOW) {
    const bool half = comp != 0 && geo.mode == SCPOSE_JPEG_420;
    const Span sx = sample_span(roi[0], roi[2], geo.w, half), sy = sample_span(roi[1], roi[3], geo.h, half);
    if (sx.hi < sx.lo || sy.hi < sy.lo || bx < (sx.lo >> 3) || bx > (sx.hi >> 3) || by < (sy.lo >> 3) || by > (sy.hi >> 3)) return;
  }
  const int32_t* d = dc + (size_t)img * geo.n_blocks;
  // the DC value: inclusive sum up to this block minus the sum up to the block before its restart segment
  const int32_t ri = head[5] >= 1 ? head[5] : 1;
  const int32_t seg_mcu = (mcu / ri) * ri;
  int32_t dcv = d[b];
  if (seg_mcu > 0) dcv -= d[(seg_mcu - 1) * geo.bpm + mc.first + mc.count - 1];
  const uint4* src = reinterpret_cast<const uint4*>(coef + ((size_t)img * geo.n_blocks + b) * 64);
  int32_t ws[8][8];                                    // [row][column]
#pragma unroll
  for (int row = 0; row < 8; ++row) {
    const uint4 v = src[row];
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ws[row][2 * c] = (int32_t)(int16_t)(u[c] & 0xffffu) * q[comp][row * 8 + 2 * c];
      ws[row][2 * c + 1] = (int32_t)(int16_t)(u[c] >> 16) * q[comp][row * 8 + 2 * c + 1];
    }
  }
  ws[0][0] = dcv * q[comp][0];
#pragma unroll
  for (int col = 0; col < 8; ++col) {                  // pass 1: columns
    int32_t in[8], out[8];
#pragma unroll
    for (int row = 0; row < 8; ++row) in[row] = ws[row][col];
    idct_1d<13 - 2>(in, out);
#pragma unroll
    for (int row = 0; row < 8; ++row) ws[row][col] = out[row];
  }
  uint8_t* dst;
  int32_t stride;
  if (comp == 0) {
    stride = geo.pw;
    dst = plane_y + ((size_t)img * geo.ph + (size_t)by * 8) * geo.pw + (size_t)bx * 8;
  } else {
    stride = geo.pcw;
    dst = plane_c + (((size_t)(comp - 1) * geo.n + img) * geo.pch + (size_t)by * 8) * geo.pcw + (size_t)bx * 8;
  }
#pragma unroll
  for (int row = 0; row < 8; ++row) {                  // pass 2: rows
    int32_t out[8];
    idct_1d<13 + 2 + 3>(ws[row], out);
    uint2 px;
    px.x = limit8(out[0]) | (limit8(out[1]) << 8) | (limit8(out[2]) << 16) | (limit8(out[3]) << 24);
    px.y = limit8(out[4]) | (limit8(out[5]) << 8) | (limit8(out[6]) << 16) | (limit8(out[7]) << 24);
    *reinterpret_cast<uint2*>(dst + (size_t)row * stride) = px;
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(const uint8_t* __restrict__ desc, Geo geo, const int16_t* __restrict__ coef,
                                                             const int32_t* __restrict__ dc, uint8_t* __restrict__ plane_y,
                                                             uint8_t* __restrict__ plane_c) {
  idct_blocks<false>(desc, geo, coef, dc, plane_y, plane_c, blockIdx.y, nullptr);
}

__global__ __launch_bounds__(kThreads) void jpeg_idct_window_kernel(const uint8_t* __restrict__ desc, Geo geo, const int16_t* __restrict__ coef,
                                                                    const int32_t* __restrict__ dc, uint8_t* __restrict__ plane_y,
                                                                    uint8_t* __restrict__ plane_c, RoiChunk rois, int img0) {
  idct_blocks<true>(desc, geo, coef, dc, plane_y, plane_c, img0 + (int)blockIdx.y, rois.v[blockIdx.y]);
}

__device__ __forceinline__ int32_t clamp255(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// chroma sample of output pixel (x, y) of a 4:2:0 image: jdsample.c's h2v2_fancy_upsample, or replication for planes of <= 2 columns
__device__ __forceinline__ int32_t chroma420(const uint8_t* __restrict__ c, int32_t stride, int32_t dw, int32_t dh, int32_t x, int32_t y) {
  const int32_t cx = x >> 1, cy = y >> 1;
  if (dw <= 2) return c[(size_t)cy * stride + cx];
  int32_t far = (y & 1) ? cy + 1 : cy - 1;
  far = far < 0 ? 0 : (far > dh - 1 ? dh - 1 : far);
  const uint8_t* rn = c + (size_t)cy * stride;
  const uint8_t* rf = c + (size_t)far * stride;
  const int32_t here = 3 * rn[cx] + rf[cx];
  if (x & 1) {
    if (cx == dw - 1) return (4 * here + 7) >> 4;
    return (3 * here + 3 * rn[cx + 1] + rf[cx + 1] + 7) >> 4;
  }
  if (cx == 0) return (4 * here + 8) >> 4;
  return (3 * here + 3 * rn[cx - 1] + rf[cx - 1] + 8) >> 4;
}

// the sample planes of one image; dw x dh: its chroma plane at 4:2:0
struct Planes {
  const uint8_t *y, *cb, *cr;
  int32_t dw, dh;
};
__device__ __forceinline__ Planes image_planes(const Geo& geo, const uint8_t* __restrict__ plane_y, const uint8_t* __restrict__ plane_c, int img) {
  return {plane_y + (size_t)img * geo.ph * geo.pw, plane_c + (size_t)img * geo.pch * geo.pcw,
          plane_c + ((size_t)geo.n + img) * geo.pch * geo.pcw, (geo.w + 1) >> 1, (geo.h + 1) >> 1};
}

// Pixel (x, y) of the frame from the sample planes: what jpeg_output_kernel writes and what a tap of jpeg_crop_kernel is worth.
struct Pixel {
  int32_t y, r, g, b;
};
__device__ __forceinline__ Pixel jpeg_pixel(const Geo& geo, const Planes& p, int32_t x, int32_t y) {
  const int32_t Y = p.y[(size_t)y * geo.pw + x];
  Pixel v{Y, Y, Y, Y};
  if (geo.mode != SCPOSE_JPEG_GRAY) {
    int32_t cb, cr;
    if (geo.mode == SCPOSE_JPEG_420) {
      cb = chroma420(p.cb, geo.pcw, p.dw, p.dh, x, y);
      cr = chroma420(p.cr, geo.pcw, p.dw, p.dh, x, y);
    } else {
      cb = p.cb[(size_t)y * geo.pcw + x];
      cr = p.cr[(size_t)y * geo.pcw + x];
    }
    cb -= 128; cr -= 128;                              // jdcolor.c: SCALEBITS 16, FIX(1.40200), FIX(1.77200), FIX(0.71414), FIX(0.34414)
    v.r = clamp255(Y + ((91881 * cr + 32768) >> 16));
    v.g = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    v.b = clamp255(Y + ((116130 * cb + 32768) >> 16));
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void jpeg_output_kernel(Geo geo, int bgr, const uint8_t* __restrict__ plane_y,
                                                               const uint8_t* __restrict__ plane_c, uint8_t* __restrict__ out,
                                                               uint8_t* __restrict__ y_out) {
  const int32_t x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6), img = blockIdx.z;
  if (x0 >= geo.w || y >= geo.h) return;
  const Planes pl = image_planes(geo, plane_y, plane_c, img);
  uint8_t px[12];
  uint8_t yy[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const Pixel v = jpeg_pixel(geo, pl, x0 + i < geo.w ? x0 + i : geo.w - 1, y);
    yy[i] = (uint8_t)v.y;
    px[3 * i] = (uint8_t)(bgr ? v.b : v.r);
    px[3 * i + 1] = (uint8_t)v.g;
    px[3 * i + 2] = (uint8_t)(bgr ? v.r : v.b);
  }
  const size_t pix = ((size_t)img * geo.h + y) * geo.w + x0;
  if ((geo.w & 3) == 0) {                              // whole quads, 4-byte aligned rows
    uint32_t* o = reinterpret_cast<uint32_t*>(out + pix * 3);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = px[4 * i] | (px[4 * i + 1] << 8) | (px[4 * i + 2] << 16) | ((uint32_t)px[4 * i + 3] << 24);
    if (y_out) *reinterpret_cast<uint32_t*>(y_out + pix) = yy[0] | (yy[1] << 8) | (yy[2] << 16) | ((uint32_t)yy[3] << 24);
  } else {
    for (int i = 0; i < 4 && x0 + i < geo.w; ++i) {
      out[(pix + i) * 3] = px[3 * i];
      out[(pix + i) * 3 + 1] = px[3 * i + 1];
      out[(pix + i) * 3 + 2] = px[3 * i + 2];
      if (y_out) y_out[pix + i] = yy[i];
    }
  }
}

// The crop tail (crop_tail.h) of frame img0 + blockIdx.y, every tap from the sample planes: the window bounds every plane sample
// that is read, and idct_blocks<true> has written exactly those (sample_span).
__global__ __launch_bounds__(kCropThreads) void jpeg_crop_kernel(Geo geo, int bgr, const uint8_t* __restrict__ plane_y,
                                                                 const uint8_t* __restrict__ plane_c, const double* __restrict__ minv,
                                                                 RoiChunk rois, int img0, int oh, int ow, uint8_t* __restrict__ out) {
  const int img = img0 + (int)blockIdx.y;
  const Planes pl = image_planes(geo, plane_y, plane_c, img);
  const auto px = [&](int32_t x, int32_t y) { const Pixel v = jpeg_pixel(geo, pl, x, y); return Rgb{v.r, v.g, v.b}; };
  crop_tail(px, geo.h, geo.w, geo.mode == SCPOSE_JPEG_GRAY, bgr, minv + (size_t)img * 6, rois.v[blockIdx.y], oh, ow,
            out + (size_t)img * ((int64_t)oh * ow) * 3);
}

struct Plan {
  unsigned long long* slots;
  int32_t* dc;
  int16_t* coef;
  size_t zero_bytes;     // slots, dc and coef are one span, zeroed by one memset
  int32_t *counts, *totals;
  uint8_t *plane_y, *plane_c;
  size_t bytes;
};

Plan make_plan(const Geo& g, uint8_t* ws) {
  Plan p{};
  Carve c{ws};
  const size_t subs = (size_t)g.n * g.max_subs, blocks = (size_t)g.n * g.n_blocks;
  p.slots = c.take<unsigned long long>(subs);
  p.dc = c.take<int32_t>(blocks);
  p.coef = c.take<int16_t>(blocks * 64);
  p.zero_bytes = c.bytes();
  p.counts = c.take<int32_t>(subs);
  p.totals = c.take<int32_t>((size_t)g.n);
  p.plane_y = c.take<uint8_t>((size_t)g.n * g.ph * g.pw);
  p.plane_c = c.take<uint8_t>(g.mode == SCPOSE_JPEG_GRAY ? 1 : (size_t)2 * g.n * g.pch * g.pcw);
  p.bytes = c.bytes();
  return p;
}

}  // namespace

size_t jpeg_decode_workspace_bytes(int n, int h, int w, int mode, int max_subs) {
  return make_plan(make_geo(n, h, w, mode, max_subs, 0, 0), nullptr).bytes;
}

namespace {

// memset, relaxation, scan, coefficient write, DC sums: the passes every entry point runs on the whole frame
int32_t launch_entropy_passes(const Geo& g, const Plan& p, const uint8_t* desc, const int32_t* segs, const uint8_t* data, int max_rounds,
                           int32_t* status, uint8_t* ws, hipStream_t stream) {
  SCP_CHECK_HIP(hipMemsetAsync(ws, 0, p.zero_bytes, stream));
  const dim3 subs_grid((unsigned)((g.max_subs + kThreads - 1) / kThreads), (unsigned)g.n);
  for (int launch = 1; launch <= max_rounds; ++launch)
    hipLaunchKernelGGL(jpeg_relax_kernel, subs_grid, dim3(kThreads), 0, stream, desc, segs, data, g, launch, p.slots, p.counts);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)g.n), dim3(kThreads), 0, stream, desc, g, max_rounds, p.slots, p.counts, p.totals, status);
  hipLaunchKernelGGL(jpeg_write_kernel, subs_grid, dim3(kThreads), 0, stream, desc, segs, data, g, p.slots, p.counts, p.totals, p.coef, p.dc,
                     status);
  hipLaunchKernelGGL(jpeg_dc_kernel, dim3(g.mode == SCPOSE_JPEG_GRAY ? 1u : 3u, (unsigned)g.n), dim3(kThreads), 0, stream, g, p.dc);
  return SCPOSE_OK;
}

}  // namespace

int32_t jpeg_decode_launch(const uint8_t* desc, const int32_t* segs, int64_t n_rows, const uint8_t* data, int64_t n_bytes, int n, int h,
                           int w, int mode, int max_subs, int bgr, int max_rounds, uint8_t* out, uint8_t* y_out, int32_t* status,
                           uint8_t* ws, hipStream_t stream) {
  const Geo g = make_geo(n, h, w, mode, max_subs, n_bytes, n_rows);
  const Plan p = make_plan(g, ws);
  if (int32_t rc = launch_entropy_passes(g, p, desc, segs, data, max_rounds, status, ws, stream)) return rc;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((g.n_blocks + kThreads - 1) / kThreads), (unsigned)n), dim3(kThreads), 0, stream, desc, g,
                     p.coef, p.dc, p.plane_y, p.plane_c);
  hipLaunchKernelGGL(jpeg_output_kernel, dim3((unsigned)((w + 255) / 256), (unsigned)((h + 3) / 4), (unsigned)n), dim3(kThreads), 0, stream, g, bgr,
                     p.plane_y, p.plane_c, out, y_out);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t jpeg_decode_crop_launch(const uint8_t* desc, const int32_t* segs, int64_t n_rows, const uint8_t* data, int64_t n_bytes, int n, int h,
                                int w, int mode, int max_subs, int bgr, int max_rounds, const double* minv, const int32_t* roi_host,
                                int out_h, int out_w, uint8_t* crops, int32_t* status, uint8_t* ws, hipStream_t stream) {
  const Geo g = make_geo(n, h, w, mode, max_subs, n_bytes, n_rows);
  const Plan p = make_plan(g, ws);
  if (int32_t rc = launch_entropy_passes(g, p, desc, segs, data, max_rounds, status, ws, stream)) return rc;
  for_each_roi_chunk(roi_host, n, [&](const RoiChunk& rois, int img0, int count) {
    hipLaunchKernelGGL(jpeg_idct_window_kernel, dim3((unsigned)((g.n_blocks + kThreads - 1) / kThreads), (unsigned)count), dim3(kThreads), 0,
                       stream, desc, g, p.coef, p.dc, p.plane_y, p.plane_c, rois, img0);
    hipLaunchKernelGGL(jpeg_crop_kernel, crop_tail_grid(out_h, out_w, count), dim3(kCropThreads), 0, stream, g, bgr, p.plane_y, p.plane_c, minv, rois,
                       img0, out_h, out_w, crops);
  });
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
