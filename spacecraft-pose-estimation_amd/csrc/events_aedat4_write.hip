// (t, x, y, p) on the device -> the event packets of an AEDAT-4.0 recording: the producing direction of
// events_aedat4_read.hip, which states the format.  tests/events_aedat4_write_restated.py says the same in Python.  The host
// (event_write.write_events_aedat4) writes the file header, the IOHeader and the file data table around what this file makes.
//
// What is written:
//   record   int32 streamID, int32 size, `size` payload bytes: the packet's flatbuffer under NONE, one LZ4 frame of it under LZ4.
//   payload  a size-prefixed EventPacket flatbuffer of 48 + 16 * count bytes: uint32 size (of what follows), uint32 root offset 16,
//            "EVTS" at 8, the vtable at 12 (uint16 6, 8, 4, 0), the table at 20 (int32 soffset 8, uint32 uoffset 20), zeros to 44,
//            uint32 count at 44, the structs from 48: int64 t, int16 x, int16 y, uint8 on, 3 zero bytes.  48 keeps every struct on
//            a 16-byte boundary of the payload.  An empty packet is the 48 bytes with count 0.
//   frame    magic 04 22 4D 18, FLG 0x64 (version 01, independent blocks, content checksum, NO content size, no block checksums),
//            BD 0x40 (64 KiB blocks), HC; per block a uint32 size word (bit 31: stored) and the data; the end mark; xxh32 of the
//            flatbuffer.  7 + 8 bytes of framing and 4 per block.
//
// Kernels, all on one stream, one read-back ([bytes, status]) after the last:
//   aedat4w_plan_kernel    one workgroup: checks the boundaries, -> per packet the position and size of its source bytes and its
//                          number of 64 KiB blocks, their scan (scan_device.h), the status word.
//   aedat4w_check_kernel   one thread per event: x, y, p in range, else SCPOSE_AEDAT4_WRITE_RANGE.  It runs BEFORE anything is
//                          stored, and every later kernel returns at once when the status word is set: a refused call stores nothing.
//   aedat4w_pack_kernel    one thread per event: its packet by bisection of the boundaries, the struct as two 8-byte stores; one
//                          thread per packet: the record header, the 48 bytes and the packet's row of the table.  Under NONE the
//                          records go straight to the output and the call ends here.
//   aedat4w_lz4_kernel     the hot path, one wavefront per 64 KiB block, into a slot of the LZ4 bound n + n / 255 + 16.  A greedy
//                          matcher: the 64 lanes load the 4 bytes at 64 consecutive positions, hash them (Fibonacci, 12 bits),
//                          read their candidates from a table of 4096 positions in LDS and then enter their own positions
//                          (atomicMax: the entry is the LATEST position whatever order the lanes are served in, so two runs
//                          agree).  A candidate is verified by comparing its 4 bytes; a ballot picks the first verified position
//                          at or after the end of the last match; the wave extends the match 256 bytes a step (4 per lane,
//                          first differing lane by ballot) up to 5 bytes before the end and emits the sequence: token, literal
//                          length extension, literals, offset, match length extension.  The lanes after a match keep their
//                          candidates, so one round of loads can emit several sequences.  No match starts in the last 12 bytes,
//                          the last 5 are literals, the last sequence ends after its literals.  The source is read only and
//                          lies in another buffer than the output, so no load waits for a store of the wave (the reader's
//                          own_stores_done has no counterpart here).  A block that does not come out smaller is marked stored.
//   aedat4w_sizes_kernel   one workgroup: per packet the positions of its blocks in its frame and the record's size; the records'
//                          positions by two scans (the sizes split at 2^16, so that 256 of them sum within an int32).
//   aedat4w_emit_kernel    one wavefront per block: the size word and the compressed bytes (or the source bytes, when stored) to
//                          their place in the contiguous output; one wavefront per packet: record header, frame header with HC,
//                          end mark and the content checksum (xxh_wave.h).
// The same last four stages frame arbitrary bytes (events_aedat4_frame_launch): `bounds` then cuts a byte string into packets.
// Integer work on fixed positions only: two runs on the same columns are bitwise equal.
#include "common.h"
#include "scan_device.h"
#include "xxh_wave.h"

namespace scpose {

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
static_assert(kThreads == kScanThreads, "the scan bodies of scan_device.h run in the workgroups of this file");
constexpr int kFbHead = 48;                          // flatbuffer bytes before the first struct
constexpr int kRecHead = 8;                          // streamID, size
constexpr int kBlock = 1 << 16;                      // block maximum code 4
constexpr int kSlotCap = kBlock + kBlock / 255 + 16; // the LZ4 bound of one block
constexpr int kSlot = (kSlotCap + 15) & ~15;
constexpr int kHashBits = 12;
constexpr int kHashSize = 1 << kHashBits;
constexpr int kFrameHead = 7, kFrameTail = 8;        // magic FLG BD HC; end mark, content checksum
constexpr uint32_t kFlg = 0x64, kBd = 0x40;
static_assert(kAedat4MaxDecoded / kBlock + 1 <= 128 && 256 * 129 < INT_MAX, "a packet has at most 128 blocks; 256 counts sum in int32");

struct Plan {
  int64_t max_blocks;
  int64_t* src_off;                                  // [np] where the packet's source bytes start
  int64_t* blk_off;                                  // [np] blocks before the packet
  int64_t* off_hi;                                   // [np] scans of the record sizes, split at 2^16
  int64_t* off_lo;
  int64_t* totals;                                   // [0] blocks of all packets
  int32_t* src_size;                                 // [np]
  int32_t* nblk;
  int32_t* size_hi;
  int32_t* size_lo;
  uint32_t* blk_word;                                // [max_blocks] the size word
  int32_t* blk_pos;                                  // [max_blocks] position of the size word in the frame
  uint8_t* staging;                                  // pack under LZ4: the records as NONE would write them
  uint8_t* slots;                                    // [max_blocks][kSlot]
  size_t bytes;
};

inline int64_t records_bytes(int64_t n, int64_t np) { return (kRecHead + kFbHead) * np + 16 * n; }

Plan plan(int64_t src_bytes, int64_t np, int64_t staging_bytes, bool lz4, uint8_t* wsp) {
  Plan p{};
  const size_t cnt = (size_t)(np > 0 ? np : 1);
  p.max_blocks = lz4 ? src_bytes / kBlock + np : 0;
  const size_t nb = (size_t)(p.max_blocks > 0 ? p.max_blocks : 1);
  Carve c{wsp};
  p.src_off = c.take<int64_t>(cnt);
  p.blk_off = c.take<int64_t>(cnt);
  p.off_hi = c.take<int64_t>(cnt);
  p.off_lo = c.take<int64_t>(cnt);
  p.totals = c.take<int64_t>(32);
  p.src_size = c.take<int32_t>(cnt);
  p.nblk = c.take<int32_t>(cnt);
  p.size_hi = c.take<int32_t>(cnt);
  p.size_lo = c.take<int32_t>(cnt);
  p.blk_word = c.take<uint32_t>(nb);
  p.blk_pos = c.take<int32_t>(nb);
  p.staging = c.take<uint8_t>((size_t)staging_bytes);
  p.slots = c.take<uint8_t>(lz4 ? nb * (size_t)kSlot : 0);
  p.bytes = c.bytes();
  return p;
}

// rows != 0: bounds are rows, a packet's source is its flatbuffer inside its record; else bounds are bytes of the caller's string.
// direct != 0 (NONE): the records are the output, their total is checked against the capacity here.
__global__ __launch_bounds__(kThreads) void aedat4w_plan_kernel(const int64_t* __restrict__ bounds, int64_t np, int64_t n, int rows,
                                                                int direct, int64_t capacity, int64_t* src_off, int32_t* src_size,
                                                                int32_t* nblk, int64_t* blk_off, int64_t* totals, int64_t* table,
                                                                int64_t* total_status) {
  __shared__ int32_t sc[kThreads];
  int st = 0;
  if (threadIdx.x == 0 && np > 0 && (bounds[0] != 0 || bounds[np] != n)) st |= SCPOSE_AEDAT4_WRITE_BOUNDS;
  for (int64_t i = threadIdx.x; i < np; i += kThreads) {
    const int64_t lo = bounds[i], c = bounds[i + 1] - lo;
    int64_t size = 0;
    if (c < 0 || lo < 0 || lo > n) st |= SCPOSE_AEDAT4_WRITE_BOUNDS;
    else if (rows ? (c > kAedat4MaxCount || kFbHead + 16 * c > kAedat4MaxDecoded) : c > kAedat4MaxDecoded) st |= SCPOSE_AEDAT4_WRITE_SIZE;
    else size = rows ? kFbHead + 16 * c : c;
    src_off[i] = rows ? (kRecHead + kFbHead) * i + 16 * lo + kRecHead : lo;
    src_size[i] = (int32_t)size;
    nblk[i] = (int32_t)((size + kBlock - 1) / kBlock);
    if (!rows) table[5 * i + 2] = table[5 * i + 3] = table[5 * i + 4] = 0;       // no events to count
  }
  __syncthreads();
  const int64_t blocks = scan_tile_counts(nblk, np, blk_off, sc);
  st = block_or(st, sc);
  if (threadIdx.x == 0) {
    const int64_t total = direct ? (kRecHead + kFbHead) * np + 16 * n : 0;
    if (direct && total > capacity) st |= SCPOSE_AEDAT4_WRITE_CAPACITY;
    totals[0] = blocks;
    total_status[0] = st ? 0 : total;
    total_status[1] = st;
  }
}

__global__ __launch_bounds__(kThreads) void aedat4w_check_kernel(const int32_t* __restrict__ x, const int32_t* __restrict__ y,
                                                                 const int8_t* __restrict__ p, int64_t n, int32_t h, int32_t w,
                                                                 int64_t* total_status) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const int32_t xv = x[i], yv = y[i], pv = p[i];
    bad = xv < 0 || xv >= w || yv < 0 || yv >= h || (pv != 0 && pv != 1);
  }
  if (__ballot(bad) != 0 && (threadIdx.x & (kWave - 1)) == 0)
    atomicOr(reinterpret_cast<unsigned long long*>(total_status) + 1, (unsigned long long)SCPOSE_AEDAT4_WRITE_RANGE);
}

__device__ __forceinline__ void st64(uint8_t* dst, uint32_t a, uint32_t b) { *reinterpret_cast<uint2*>(dst) = make_uint2(a, b); }

// dst: the records (8-byte aligned), the output itself under NONE (direct) or the staging buffer
__global__ __launch_bounds__(kThreads) void aedat4w_pack_kernel(const int64_t* __restrict__ t, const int32_t* __restrict__ x,
                                                                const int32_t* __restrict__ y, const int8_t* __restrict__ p, int64_t n,
                                                                const int64_t* __restrict__ bounds, int64_t np, int32_t stream_id,
                                                                int direct, uint8_t* __restrict__ dst, int64_t* __restrict__ table,
                                                                const int64_t* __restrict__ total_status) {
  if (total_status[1] != 0) return;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) {
    int64_t lo = 0, hi = np;                         // bounds[lo] <= i < bounds[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (bounds[mid] <= i) lo = mid;
      else hi = mid;
    }
    uint8_t* d = dst + (kRecHead + kFbHead) * (lo + 1) + 16 * i;
    const uint64_t tv = (uint64_t)t[i];
    st64(d, (uint32_t)tv, (uint32_t)(tv >> 32));
    st64(d + 8, ((uint32_t)x[i] & 0xFFFFu) | ((uint32_t)y[i] << 16), (uint32_t)p[i]);
  }
  if (i < np) {
    const int64_t lo = bounds[i], c = bounds[i + 1] - lo;
    const int64_t at = (kRecHead + kFbHead) * i + 16 * lo;
    const uint32_t fb = (uint32_t)(kFbHead + 16 * c);
    uint8_t* d = dst + at;
    st64(d, (uint32_t)stream_id, fb);
    st64(d + 8, fb - 4, 16u);
    st64(d + 16, 0x53545645u, 0x00080006u);          // "EVTS"; vtable: 6 bytes, a table of 8
    st64(d + 24, 0x00000004u, 8u);                   // field 0 at 4; the table: soffset back to the vtable
    st64(d + 32, 20u, 0u);                           // uoffset to the vector
    st64(d + 40, 0u, 0u);
    st64(d + 48, 0u, (uint32_t)c);
    if (direct) {
      table[5 * i] = at;
      table[5 * i + 1] = fb;
    }
    table[5 * i + 2] = c;
    table[5 * i + 3] = c ? t[lo] : 0;
    table[5 * i + 4] = c ? t[lo + c - 1] : 0;
  }
}

// the packet of block b: the last one whose blocks start at or before b
__device__ __forceinline__ int64_t packet_of(const int64_t* __restrict__ blk_off, int64_t np, int64_t b) {
  int64_t lo = 0, hi = np;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (blk_off[mid] <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the extension bytes of a length nibble of 15 whose remainder is rem: cnt = rem / 255 + 1 bytes
__device__ __forceinline__ void put_ext(uint8_t* o, int rem, int cnt) {
  for (int k = threadIdx.x; k < cnt; k += kWave) o[k] = (uint8_t)(k < cnt - 1 ? 255 : rem - 255 * (cnt - 1));
}

// n bytes at src as one LZ4 block at dst, by one wavefront -> its size, or -1 when it would pass cap
__device__ int lz4_block(const uint8_t* __restrict__ src, int n, uint8_t* __restrict__ dst, int cap, uint32_t* table) {
  const int lane = threadIdx.x;
  for (int k = lane; k < kHashSize; k += kWave) table[k] = 0;        // position 0: verified like any other candidate
  __syncthreads();
  int anchor = 0, pos = 0, op = 0;
  const int mflimit = n - 12, matchlimit = n - 5;
  while (pos < mflimit) {
    const int base = pos, i = base + lane;
    const bool valid = i < mflimit;
    uint32_t seq = 0, hsh = 0;
    int cand = 0;
    if (valid) {
      seq = ld32(src + i);
      hsh = (seq * 2654435761u) >> (32 - kHashBits);
      cand = (int)table[hsh];
    }
    __syncthreads();                                 // every candidate is read before a position of this round is entered
    if (valid) atomicMax(&table[hsh], (uint32_t)i);
    __syncthreads();
    const bool ok = valid && cand < i && ld32(src + cand) == seq;
    int cur = base;
    for (;;) {
      const unsigned long long m = __ballot(ok && i >= cur);
      if (!m) break;
      const int f = __ffsll((long long)m) - 1;
      const int mpos = base + f, mc = __shfl(cand, f, kWave);
      int len = 4;
      for (;;) {                                     // lane l compares the 4 bytes at len + 4 l
        const int k = len + 4 * lane;
        const int avail = matchlimit - (mpos + k);
        int e = 0;
        if (avail > 0) {
          const uint32_t d = ld32(src + mpos + k) ^ ld32(src + mc + k);
          e = d ? (__ffs((int)d) - 1) >> 3 : 4;
          e = e < avail ? e : avail;
        }
        const unsigned long long stop = __ballot(e < 4);
        if (stop) {
          const int g = __ffsll((long long)stop) - 1;
          len += 4 * g + __shfl(e, g, kWave);
          break;
        }
        len += 4 * kWave;
      }
      const int L = mpos - anchor, M = len - 4, off = mpos - mc;
      const int eL = L >= 15 ? (L - 15) / 255 + 1 : 0, eM = M >= 15 ? (M - 15) / 255 + 1 : 0;
      if (op + 1 + eL + L + 2 + eM > cap) return -1;
      uint8_t* o = dst + op;
      if (lane == 0) o[0] = (uint8_t)(((L < 15 ? L : 15) << 4) | (M < 15 ? M : 15));
      put_ext(o + 1, L - 15, eL);
      o += 1 + eL;
      for (int k = lane; k < L; k += kWave) o[k] = src[anchor + k];
      o += L;
      if (lane == 0) {
        o[0] = (uint8_t)(off & 255);
        o[1] = (uint8_t)(off >> 8);
      }
      put_ext(o + 2, M - 15, eM);
      op += 1 + eL + L + 2 + eM;
      anchor = cur = mpos + len;
      if (cur >= base + kWave) break;
    }
    pos = cur > base + kWave ? cur : base + kWave;
  }
  const int L = n - anchor;
  const int eL = L >= 15 ? (L - 15) / 255 + 1 : 0;
  if (op + 1 + eL + L > cap) return -1;
  uint8_t* o = dst + op;
  if (lane == 0) o[0] = (uint8_t)((L < 15 ? L : 15) << 4);
  put_ext(o + 1, L - 15, eL);
  o += 1 + eL;
  for (int k = lane; k < L; k += kWave) o[k] = src[anchor + k];
  return op + 1 + eL + L;
}

__global__ __launch_bounds__(kWave) void aedat4w_lz4_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off,
                                                            const int32_t* __restrict__ src_size, const int64_t* __restrict__ blk_off,
                                                            const int64_t* __restrict__ totals, int64_t np, uint8_t* __restrict__ slots,
                                                            uint32_t* __restrict__ blk_word, const int64_t* __restrict__ total_status) {
  __shared__ uint32_t table[kHashSize];
  const int64_t b = blockIdx.x;
  if (total_status[1] != 0 || b >= totals[0]) return;
  const int64_t pk = packet_of(blk_off, np, b);
  const int j = (int)(b - blk_off[pk]);
  const int left = src_size[pk] - j * kBlock;
  const int n = left < kBlock ? left : kBlock;
  const int got = lz4_block(src + src_off[pk] + (int64_t)j * kBlock, n, slots + b * kSlot, kSlotCap, table);
  if (threadIdx.x == 0) blk_word[b] = got < 0 || got >= n ? (uint32_t)n | 0x80000000u : (uint32_t)got;
}

__global__ __launch_bounds__(kThreads) void aedat4w_sizes_kernel(const int32_t* __restrict__ nblk, const int64_t* __restrict__ blk_off,
                                                                 const uint32_t* __restrict__ blk_word, int64_t np, int64_t capacity,
                                                                 int32_t* blk_pos, int32_t* size_hi, int32_t* size_lo, int64_t* off_hi,
                                                                 int64_t* off_lo, int64_t* table, int64_t* total_status) {
  __shared__ int32_t sc[kThreads];
  if (total_status[1] != 0) return;
  for (int64_t i = threadIdx.x; i < np; i += kThreads) {
    int32_t pos = kFrameHead;
    const int64_t b0 = blk_off[i];
    for (int j = 0; j < nblk[i]; ++j) {
      blk_pos[b0 + j] = pos;
      pos += 4 + (int32_t)(blk_word[b0 + j] & 0x7FFFFFFFu);
    }
    const int32_t rec = kRecHead + pos + kFrameTail;
    size_hi[i] = rec >> 16;
    size_lo[i] = rec & 0xFFFF;
    table[5 * i + 1] = pos + kFrameTail;
  }
  __syncthreads();
  const int64_t hi = scan_tile_counts(size_hi, np, off_hi, sc);
  const int64_t lo = scan_tile_counts(size_lo, np, off_lo, sc);
  for (int64_t i = threadIdx.x; i < np; i += kThreads) table[5 * i] = (off_hi[i] << 16) + off_lo[i];
  if (threadIdx.x == 0) {
    const int64_t total = (hi << 16) + lo;
    total_status[0] = total > capacity ? 0 : total;
    if (total > capacity) total_status[1] = SCPOSE_AEDAT4_WRITE_CAPACITY;
  }
}

// n bytes, by one wavefront, to a destination of any alignment: bytes up to a 4-byte boundary, words, bytes
__device__ __forceinline__ void copy_wave(uint8_t* dst, const uint8_t* __restrict__ src, int n) {
  const int lane = threadIdx.x;
  int head = (int)((0 - reinterpret_cast<uintptr_t>(dst)) & 3);
  head = head < n ? head : n;
  if (lane < head) dst[lane] = src[lane];
  const int words = (n - head) >> 2;
  for (int k = lane; k < words; k += kWave) *reinterpret_cast<uint32_t*>(dst + head + 4 * k) = ld32(src + head + 4 * k);
  const int done = head + 4 * words;
  if (lane < n - done) dst[done + lane] = src[done + lane];
}

__device__ __forceinline__ void put32(uint8_t* dst, uint32_t v) {
  for (int k = 0; k < 4; ++k) dst[k] = (uint8_t)(v >> (8 * k));
}

// workgroups 0 .. np - 1: what surrounds a packet's blocks; np + b: block b
__global__ __launch_bounds__(kWave) void aedat4w_emit_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off,
                                                             const int32_t* __restrict__ src_size, const int64_t* __restrict__ blk_off,
                                                             const int64_t* __restrict__ totals, int64_t np,
                                                             const uint8_t* __restrict__ slots, const uint32_t* __restrict__ blk_word,
                                                             const int32_t* __restrict__ blk_pos, const int64_t* __restrict__ table,
                                                             int32_t stream_id, uint8_t* __restrict__ out,
                                                             const int64_t* __restrict__ total_status) {
  __shared__ uint32_t sw[256];
  __shared__ uint8_t desc[4];
  if (total_status[1] != 0) return;
  if ((int64_t)blockIdx.x < np) {
    const int64_t pk = blockIdx.x;
    uint8_t* rec = out + table[5 * pk];
    const int32_t frame = (int32_t)table[5 * pk + 1];
    if (threadIdx.x == 0) {
      desc[0] = (uint8_t)kFlg;
      desc[1] = (uint8_t)kBd;
    }
    __syncthreads();
    const uint32_t hc = (xxh32_wave(desc, 2, sw) >> 8) & 0xFFu;
    const uint32_t sum = xxh32_wave(src + src_off[pk], src_size[pk], sw);
    if (threadIdx.x == 0) {
      put32(rec, (uint32_t)stream_id);
      put32(rec + 4, (uint32_t)frame);
      put32(rec + 8, 0x184D2204u);
      rec[12] = (uint8_t)kFlg;
      rec[13] = (uint8_t)kBd;
      rec[14] = (uint8_t)hc;
      put32(rec + kRecHead + frame - 8, 0u);
      put32(rec + kRecHead + frame - 4, sum);
    }
    return;
  }
  const int64_t b = (int64_t)blockIdx.x - np;
  if (b >= totals[0]) return;
  const int64_t pk = packet_of(blk_off, np, b);
  const int j = (int)(b - blk_off[pk]);
  const uint32_t word = blk_word[b];
  uint8_t* d = out + table[5 * pk] + kRecHead + blk_pos[b];
  if (threadIdx.x == 0) put32(d, word);
  copy_wave(d + 4, (word >> 31) ? src + src_off[pk] + (int64_t)j * kBlock : slots + b * kSlot, (int)(word & 0x7FFFFFFFu));
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// the stages after the source bytes exist: compress, place, emit
void frame_stages(const Plan& pl, const uint8_t* src, int64_t np, int stream_id, uint8_t* out, int64_t capacity, int64_t* table,
                  int64_t* total_status, hipStream_t stream) {
  if (pl.max_blocks > 0)
    hipLaunchKernelGGL(aedat4w_lz4_kernel, dim3((unsigned)pl.max_blocks), dim3(kWave), 0, stream, src, pl.src_off, pl.src_size,
                       pl.blk_off, pl.totals, np, pl.slots, pl.blk_word, total_status);
  hipLaunchKernelGGL(aedat4w_sizes_kernel, dim3(1), dim3(kThreads), 0, stream, pl.nblk, pl.blk_off, pl.blk_word, np, capacity,
                     pl.blk_pos, pl.size_hi, pl.size_lo, pl.off_hi, pl.off_lo, table, total_status);
  if (pl.max_blocks + np > 0)
    hipLaunchKernelGGL(aedat4w_emit_kernel, dim3((unsigned)(pl.max_blocks + np)), dim3(kWave), 0, stream, src, pl.src_off, pl.src_size,
                       pl.blk_off, pl.totals, np, pl.slots, pl.blk_word, pl.blk_pos, table, stream_id, out, total_status);
}

}  // namespace

// out_bytes: what the output can need at the most -- every block stored, so the framing on top of the records
Aedat4WriteSizes events_aedat4_pack_sizes(int64_t n, int64_t np, int compression) {
  const int64_t rec = records_bytes(n, np);
  const bool lz4 = compression == SCPOSE_AEDAT4_LZ4;
  const Plan pl = plan(rec, np, lz4 ? rec : 0, lz4, nullptr);
  const int64_t out = lz4 ? rec + (kFrameHead + kFrameTail) * np + 4 * pl.max_blocks : rec;
  return {pl.bytes, (size_t)(out > 16 ? out : 16)};
}

Aedat4WriteSizes events_aedat4_frame_sizes(int64_t n_bytes, int64_t np) {
  const Plan pl = plan(n_bytes, np, 0, true, nullptr);
  const int64_t out = n_bytes + (kRecHead + kFrameHead + kFrameTail) * np + 4 * pl.max_blocks;
  return {pl.bytes, (size_t)(out > 16 ? out : 16)};
}

int32_t events_aedat4_pack_launch(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n, const int64_t* bounds,
                                  int64_t np, int h, int w, int stream_id, int compression, uint8_t* out, int64_t capacity,
                                  int64_t* table, int64_t* total_status, uint8_t* wsp, hipStream_t stream) {
  const int64_t rec = records_bytes(n, np);
  const bool lz4 = compression == SCPOSE_AEDAT4_LZ4;
  const Plan pl = plan(rec, np, lz4 ? rec : 0, lz4, wsp);
  hipLaunchKernelGGL(aedat4w_plan_kernel, dim3(1), dim3(kThreads), 0, stream, bounds, np, n, 1, lz4 ? 0 : 1, capacity, pl.src_off,
                     pl.src_size, pl.nblk, pl.blk_off, pl.totals, table, total_status);
  if (n > 0) hipLaunchKernelGGL(aedat4w_check_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, stream, x, y, p, n, h, w, total_status);
  uint8_t* records = lz4 ? pl.staging : out;
  if (np > 0)
    hipLaunchKernelGGL(aedat4w_pack_kernel, dim3(blocks_of(n > np ? n : np)), dim3(kThreads), 0, stream, t, x, y, p, n, bounds, np,
                       stream_id, lz4 ? 0 : 1, records, table, total_status);
  if (lz4) frame_stages(pl, records, np, stream_id, out, capacity, table, total_status, stream);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t events_aedat4_frame_launch(const uint8_t* src, int64_t n_bytes, const int64_t* bounds, int64_t np, uint8_t* out,
                                   int64_t capacity, int64_t* table, int64_t* total_status, uint8_t* wsp, hipStream_t stream) {
  const Plan pl = plan(n_bytes, np, 0, true, wsp);
  hipLaunchKernelGGL(aedat4w_plan_kernel, dim3(1), dim3(kThreads), 0, stream, bounds, np, n_bytes, 0, 0, capacity, pl.src_off,
                     pl.src_size, pl.nblk, pl.blk_off, pl.totals, table, total_status);
  frame_stages(pl, src, np, 0, out, capacity, table, total_status, stream);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
