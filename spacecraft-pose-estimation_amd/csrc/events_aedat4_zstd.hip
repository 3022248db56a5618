// The ZSTD / ZSTD_HIGH payloads of an AEDAT-4.0 recording -> the packets' flatbuffers in the staging buffer (DESIGN.md section
// 5a.7, "ZSTD"): the Zstandard counterpart of the LZ4 measure / decode pair of events_aedat4_read.hip, under the same output
// contract (per-packet size and status slots, 16-byte-rounded offsets from scan_tile_counts, at most 2^23 - 16 decoded bytes per
// packet), so that the count and unpack steps of that file run unchanged afterwards.  tests/zstd_restated.py says the same in Python.
//
// The format (RFC 8878, no dictionary; all integers little-endian):
//   payload   one or more frames back to back.  Magic 0x184D2A50 .. 5F: a skippable frame, a uint32 size and that many bytes,
//             skipped.  Magic 0xFD2FB528: a Zstandard frame.  Anything else, and a payload without a Zstandard frame: CORRUPT.
//   header    descriptor byte: bits 7..6 FCS flag, 5 single segment, 4 unused (ignored), 3 reserved (must be 0), 2 content
//             checksum, 1..0 dictionary-ID flag.  Unless single segment a window descriptor byte: exponent = b >> 3, mantissa =
//             b & 7, window = (1 << (10 + exponent)) * (8 + mantissa) / 8.  A dictionary ID of 0 / 1 / 2 / 4 bytes (flag 0..3), which
//             must be 0.  Frame_Content_Size of 0 (1 when single segment) / 2 / 4 / 8 bytes (flag 0..3), the 2-byte field + 256.
//             Single segment: window = Frame_Content_Size.
//   blocks    a 3-byte header: bit 0 last, bits 2..1 type (0 Raw, 1 RLE, 2 Compressed, 3 CORRUPT), bits 23..3 size.  No size may
//             exceed min(window, 128 KiB), nor may what a block decodes to.  Raw: `size` bytes.  RLE: one byte, `size` times.
//             Compressed: a literals section, then a sequences section.  After the last block a uint32 when the checksum flag is
//             set: the low 32 bits of XXH64 (seed 0) of the frame's output.
//   literals  byte 0: bits 1..0 type (0 Raw, 1 RLE, 2 Compressed, 3 Treeless), bits 3..2 size format.  Raw / RLE: format 0 or 2: a
//             5-bit size in 1 byte; 1: 12 bits in 2; 3: 20 bits in 3.  Compressed / Treeless: format 0: one stream, 1..3: four
//             streams; regenerated and compressed size of 10 + 10 bits in 3 bytes (formats 0, 1), 14 + 14 in 4 (2), 18 + 18 in
//             5 (3).  Compressed: a Huffman tree description, then the streams; Treeless: the streams, decoded with the table of
//             the last Compressed literals of this frame (none: CORRUPT).  Four streams: a 6-byte jump table (three uint16 sizes,
//             the fourth is the rest); the first three regenerate (size + 3) / 4 bytes each, the fourth the rest.
//   tree      header byte h >= 128: h - 127 weights of 4 bits, high nibble first.  h < 128: h bytes that hold an FSE table
//             description (accuracy <= 6) and a backward bitstream of two interleaved states, which alternate: emit the state's
//             symbol, update the state; when an update asks for more bits than are left, the OTHER state's symbol is the last.
//             Weights w > 0 stand for 2^(w-1); their sum is completed to the next power of two 2^maxbits (maxbits <= 11) by ONE
//             more weight, so the gap must be a power of two.  The decode table has 2^maxbits cells: symbols in order of
//             (weight, symbol) take 2^(w-1) cells each, code length maxbits + 1 - w.
//   streams   backward bitstreams: the highest set bit of the last byte is the end marker (a last byte of 0: CORRUPT), bits are
//             read from there down, zero-padded below the first byte.  A Huffman stream must end exactly at its first bit.
//   FSE       table description, a forward bitstream: 4 bits accuracy - 5, then per symbol a value of `bits` or `bits - 1` bits
//             (bits = highbit(remaining + 1) + 1; the short form when the low bits - 1 bits are below (1 << bits) - 2 - remaining),
//             probability = value - 1 (-1: "less than one", one cell), remaining -= |probability|; a probability of 0 is
//             followed by 2-bit repeat counts of further zeros (3: another count follows).  Ends when remaining is 0, rounded
//             up to a byte.  Table: the -1 symbols take the top cells, the others are spread with step (size >> 1) + (size >> 3)
//             + 3; cell u of symbol s, its x-th (x counted from the probability up): bits = accuracy - highbit(x), baseline =
//             (x << bits) - size.
//   sequences byte 0: 0: none (the section is that byte); < 128: the count; < 255: ((b0 - 128) << 8) + b1; 255: b1 + (b2 << 8) +
//             0x7F00.  A modes byte: bits 7..6 literal lengths, 5..4 offsets, 3..2 match lengths, 1..0 must be 0; mode 0
//             Predefined, 1 RLE (one symbol byte), 2 FSE_Compressed (accuracy <= 9 / 8 / 9), 3 Repeat: the table of the last
//             block of this frame that had sequences (none: CORRUPT).  Then ONE backward bitstream: the three initial states
//             (LL, OF, ML); per sequence the extra bits of offset, match length, literal length, then -- except after the last --
//             the state updates of LL, ML, OF.  It must end exactly at its first bit.  Offset code N: value (1 << N) + N bits;
//             value > 3: offset = value - 3, else a repeat offset (1, 2, 3, +1 when the literal length is 0; 4 means
//             Repeated_Offset1 - 1).  The three repeat offsets start at 1, 4, 8 and persist across the blocks of a frame.
//             An offset of 0, beyond the window or before the start of the frame's output: CORRUPT.  Literals left over after
//             the last sequence are copied; literals that run out early: CORRUPT.
//
// Two steps, the LZ4 pair's roles (ops.unpack_events_aedat4):
//   aedat4_zstd_kernel<false>  MEASURE, one wavefront per packet at a time: walks frames and block headers without storing.  A
//                              frame that states its Frame_Content_Size counts that; another one is walked: Raw and RLE sizes from
//                              the block header, Compressed ones from the literals header plus the sum of the match lengths.
//   aedat4_zstd_kernel<true>   DECODE: the same walk, complete: the tree and the FSE tables of a block are built in LDS (one lane,
//                              then a barrier), up to four lanes decode the Huffman streams into the workgroup's literal slot in
//                              the workspace (128 KiB: a block's literals do not fit in LDS beside the tables).  Every lane decodes
//                              every sequence, redundantly and in step (the same bits, the same branch: no lane waits for
//                              another's result), and every copy is executed by all 64 lanes.  Match history is the staging
//                              buffer itself: before a match's loads the wave waits for its own stores (own_stores_done of aedat4_payload.h).
//                              The content checksum is verified when asked; the decoded size must equal what MEASURE found and
//                              the Frame_Content_Size.
// A launch has at most kZstdGrid workgroups, each walking packets blockIdx.x, + gridDim.x, ...: the literal slots are per workgroup.
// The kernels DETECT a damaged stream and never interpret one: every read is checked against the payload, every store against
// the packet's slot.  Integer work on fixed positions: two runs are bitwise equal.
#include "aedat4_payload.h"
#include "events_packets.h"
#include "xxh_wave.h"

namespace scpose {

namespace {

constexpr int kMaxDecoded = kAedat4MaxDecoded;
constexpr int kBlockMax = 1 << 17;                   // Block_Maximum_Size, and the bytes of a literal slot
constexpr int kZstdGrid = 512;                       // workgroups (and literal slots) of one launch
constexpr int kHufLog = 11, kLLLog = 9, kOFLog = 8, kMLLog = 9, kWeightLog = 6;
constexpr int kLLSyms = 36, kOFSyms = 32, kMLSyms = 53;

__constant__ const int8_t kLLNorm[kLLSyms] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                              2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
__constant__ const int8_t kOFNorm[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
__constant__ const int8_t kMLNorm[kMLSyms] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                              1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
__constant__ const uint32_t kLLBase[kLLSyms] = {0,  1,  2,  3,  4,  5,  6,  7,  8,   9,   10,  11,   12,   13,   14,   15,    16,    18,
                                                20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
__constant__ const uint8_t kLLBits[kLLSyms] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                               1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
__constant__ const uint32_t kMLBase[kMLSyms] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16,  17,  18,  19,   20,
                                                21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,  35,  37,  39,   41,
                                                43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
__constant__ const uint8_t kMLBits[kMLSyms] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                               0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

struct FseCell {
  uint16_t base;
  uint8_t sym, nb;
};

struct ZLds {
  uint16_t huf[1 << kHufLog];                        // symbol | code length << 8
  FseCell ll[1 << kLLLog], of[1 << kOFLog], ml[1 << kMLLog], wt[1 << kWeightLog];
  int16_t norm[256];
  uint16_t next[256];
  uint8_t weight[256];
  int ret, log;                                      // what lane 0 hands to the wave
};

__device__ __forceinline__ int highbit(uint32_t v) { return 31 - __clz((int)v); }

// Lane 0 runs f (a serial table build in LDS, which leaves the table's log in s.log); every lane gets its result and, unless
// that is negative, the log.  Called by all lanes of the workgroup.
template <class F>
__device__ __forceinline__ int lane0(ZLds& s, int* log, F f) {
  if (threadIdx.x == 0) s.ret = f();
  __syncthreads();
  const int r = s.ret;
  if (r >= 0) *log = s.log;
  __syncthreads();
  return r;
}

// A backward bitstream over p[0, n): bit k is bit (k & 7) of byte k >> 3; `left` bits are unread, the next one read is bit
// left - 1.  Bits below bit 0 read as zeros and make `left` negative: the caller checks; once `left` is negative every read is 0.
// Private to a lane, or the same in every lane.
struct Bits {
  const uint8_t* p;
  long long n, left, cbit;
  unsigned long long cache;                          // bits [cbit, cbit + 64)

  __device__ __forceinline__ bool init(const uint8_t* bytes, long long count) {
    p = bytes;
    n = count;
    left = 0;
    cbit = LLONG_MAX;
    cache = 0;
    if (n < 1 || p[n - 1] == 0) return false;
    left = 8 * (n - 1) + highbit(p[n - 1]);
    return true;
  }
  __device__ __forceinline__ void load() {
    const long long cb = ((left - 1) >> 3) - 7;     // the cache's first byte; its last holds bit left - 1 (left > 0 here)
    cbit = 8 * cb;
    if (cb >= 0) cache = (unsigned long long)ld64(p + cb);
    else {
      cache = 0;
      for (int k = 0; k < 8; ++k)
        if (cb + k >= 0 && cb + k < n) cache |= (unsigned long long)p[cb + k] << (8 * k);
    }
  }
  __device__ __forceinline__ uint32_t peek(int nb) {                         // nb <= 32
    if (nb == 0 || left <= 0) return 0;               // nothing is left: zeros, whatever the cache holds
    const long long lo = left - nb;
    if (lo < cbit) load();                           // then cbit <= left - 57 <= lo (nb <= 32), and lo - cbit <= 63
    return (uint32_t)((cache >> (lo - cbit)) & ((1ull << nb) - 1));
  }
  __device__ __forceinline__ uint32_t read(int nb) {
    const uint32_t v = peek(nb);
    left -= nb;
    return v;
  }
};

// An FSE table description at p[0, n) -> s.norm[0, *nsym), *log; returns the bytes it takes, -1: damaged.  Lane 0.
__device__ int fse_read_norm(ZLds& s, const uint8_t* p, long long n, int max_log, int max_syms, int* log, int* nsym) {
  long long bit = 0;
  auto take = [&](int nb) -> uint32_t {              // forward, little-endian; past the end: zeros (the final check catches it)
    uint32_t v = 0;
    for (int k = 0; k < 3; ++k) {
      const long long b = (bit >> 3) + k;
      if (b < n) v |= (uint32_t)p[b] << (8 * k);
    }
    v = (v >> (bit & 7)) & ((1u << nb) - 1);
    bit += nb;
    return v;
  };
  const int al = (int)take(4) + 5;
  if (al > max_log) return -1;
  int remaining = 1 << al, sym = 0;
  while (remaining > 0 && sym < max_syms) {
    const int bits = highbit((uint32_t)remaining + 1) + 1;
    uint32_t val = take(bits);
    const uint32_t lower = (1u << (bits - 1)) - 1, thresh = (1u << bits) - 1 - ((uint32_t)remaining + 1);
    if ((val & lower) < thresh) {
      bit -= 1;
      val &= lower;
    } else if (val > lower) val -= thresh;
    const int proba = (int)val - 1;
    remaining -= proba < 0 ? 1 : proba;
    s.norm[sym++] = (int16_t)proba;
    if (proba == 0) {
      for (;;) {
        const int rep = (int)take(2);
        for (int i = 0; i < rep && sym < max_syms; ++i) s.norm[sym++] = 0;
        if (rep != 3 || sym >= max_syms || bit > 8 * n) break;
      }
    }
    if (bit > 8 * n) return -1;
  }
  if (remaining != 0 || bit > 8 * n) return -1;
  *log = al;
  *nsym = sym;
  return (int)((bit + 7) >> 3);
}

// s.norm[0, nsym) -> the decode table t of 1 << log cells; false: the probabilities do not fill the table.  Lane 0.
__device__ bool fse_build(ZLds& s, FseCell* t, int log, int nsym) {
  const int size = 1 << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
  int high = size - 1, total = 0;
  for (int i = 0; i < nsym; ++i) {
    const int c = s.norm[i];
    total += c < 0 ? 1 : c;
    if (c == -1) {
      if (high < 0) return false;
      t[high--].sym = (uint8_t)i;
      s.next[i] = 1;
    } else s.next[i] = (uint16_t)c;
  }
  if (total != size) return false;
  int pos = 0;
  for (int i = 0; i < nsym; ++i)
    for (int k = 0; k < s.norm[i]; ++k) {
      t[pos].sym = (uint8_t)i;
      do pos = (pos + step) & mask;
      while (pos > high);
    }
  if (pos != 0) return false;
  for (int u = 0; u < size; ++u) {
    const uint32_t x = s.next[t[u].sym]++;
    const int nb = log - highbit(x);
    t[u].nb = (uint8_t)nb;
    t[u].base = (uint16_t)((x << nb) - size);
  }
  return true;
}

// The table of one symbol type for this block, by its mode.  All lanes.  -> bytes taken from p[0, n), -1: CORRUPT; *log updated
// (Repeat leaves table and *log as they are).  *is_predef: the table holds the predefined distribution already, from an earlier
// block of this frame, and is not built again.
__device__ int seq_table(ZLds& s, int mode, FseCell* t, int max_log, int max_syms, const int8_t* predef, int predef_syms,
                         int predef_log, const uint8_t* p, long long n, bool have_previous, int* log, bool* is_predef) {
  if (mode == 3) return have_previous ? 0 : -1;
  if (mode == 0 && *is_predef) return 0;
  *is_predef = mode == 0;
  return lane0(s, log, [&]() -> int {
    if (mode == 0) {
      for (int i = 0; i < predef_syms; ++i) s.norm[i] = predef[i];
      s.log = predef_log;
      return fse_build(s, t, predef_log, predef_syms) ? 0 : -1;
    }
    if (mode == 1) {
      if (n < 1 || p[0] >= max_syms) return -1;
      t[0] = FseCell{0, p[0], 0};
      s.log = 0;
      return 1;
    }
    int al = 0, nsym = 0;
    const int used = fse_read_norm(s, p, n, max_log, max_syms, &al, &nsym);
    if (used < 0 || !fse_build(s, t, al, nsym)) return -1;
    s.log = al;
    return used;
  });
}

// A Huffman tree description at p[0, n) -> s.huf, s.log = maxbits; returns the bytes it takes, -1: damaged.  Lane 0.
__device__ int huf_table(ZLds& s, const uint8_t* p, long long n) {
  if (n < 1) return -1;
  const int h = p[0];
  int nsym = 0, used;
  if (h >= 128) {
    nsym = h - 127;
    used = 1 + (nsym + 1) / 2;
    if (used > n) return -1;
    for (int i = 0; i < nsym; ++i) s.weight[i] = (i & 1) ? (p[1 + i / 2] & 15) : (p[1 + i / 2] >> 4);
  } else {
    used = 1 + h;
    if (h == 0 || used > n) return -1;
    int al = 0, tsyms = 0;
    const int head = fse_read_norm(s, p + 1, h, kWeightLog, 256, &al, &tsyms);
    if (head < 0 || !fse_build(s, s.wt, al, tsyms)) return -1;
    Bits b;
    if (!b.init(p + 1 + head, h - head)) return -1;
    uint32_t st1 = b.read(al), st2 = b.read(al);
    if (b.left < 0) return -1;
    for (;;) {
      if (nsym >= 254) return -1;
      s.weight[nsym++] = s.wt[st1].sym;
      if (s.wt[st1].nb > b.left) {
        s.weight[nsym++] = s.wt[st2].sym;
        break;
      }
      st1 = s.wt[st1].base + b.read(s.wt[st1].nb);
      if (nsym >= 254) return -1;
      s.weight[nsym++] = s.wt[st2].sym;
      if (s.wt[st2].nb > b.left) {
        s.weight[nsym++] = s.wt[st1].sym;
        break;
      }
      st2 = s.wt[st2].base + b.read(s.wt[st2].nb);
    }
  }
  uint32_t sum = 0;
  for (int i = 0; i < nsym; ++i) {
    const int w = s.weight[i];
    if (w > kHufLog) return -1;
    if (w) sum += 1u << (w - 1);
  }
  if (sum == 0) return -1;
  const int maxbits = highbit(sum) + 1;
  if (maxbits > kHufLog) return -1;
  const uint32_t gap = (1u << maxbits) - sum;
  if (gap & (gap - 1)) return -1;
  s.weight[nsym++] = (uint8_t)(highbit(gap) + 1);
  uint32_t start[kHufLog + 2] = {};
  for (int i = 0; i < nsym; ++i) start[s.weight[i] + 1] += s.weight[i] ? 1u << (s.weight[i] - 1) : 0;
  start[1] = 0;
  for (int w = 2; w <= maxbits; ++w) start[w] += start[w - 1];             // start[w]: the first cell of weight w
  for (int i = 0; i < nsym; ++i) {
    const int w = s.weight[i];
    if (!w) continue;
    const uint32_t cells = 1u << (w - 1);
    for (uint32_t u = 0; u < cells; ++u) s.huf[start[w] + u] = (uint16_t)(i | ((maxbits + 1 - w) << 8));
    start[w] += cells;
  }
  s.log = maxbits;
  return used;
}

// What a frame carries from block to block
struct FrameState {
  long long start;                                   // of the frame's output
  unsigned long long window;
  uint32_t rep[3];
  int ll_log, of_log, ml_log, huf_log;
  bool have_huf, have_seq;
  bool predef[3];                                    // the LL / OF / ML table in LDS is the predefined one
};

constexpr int kBad = SCPOSE_AEDAT4_CORRUPT;

// One Compressed block at b[0, bs) -> dst[out ...]; returns the new `out`, -1: CORRUPT.  limit: what `out` may reach.  All lanes.
template <bool STORE>
__device__ long long compressed_block(ZLds& s, FrameState& f, const uint8_t* b, long long bs, uint8_t* dst, long long out,
                                      long long limit, uint8_t* lits) {
  if (bs < 1) return -1;
  const int ltype = b[0] & 3, fmt = (b[0] >> 2) & 3;
  long long regen, comp = 0, lp;                     // lp: where the literals' content starts
  int streams = 1;
  if (ltype < 2) {
    const int hb = fmt == 1 ? 2 : fmt == 3 ? 3 : 1;
    if (bs < hb) return -1;
    regen = fmt == 1 ? (b[0] >> 4) | (b[1] << 4) : fmt == 3 ? (b[0] >> 4) | (b[1] << 4) | (b[2] << 12) : b[0] >> 3;
    lp = hb;
    comp = ltype == 0 ? regen : 1;
  } else {
    const int hb = fmt < 2 ? 3 : fmt + 2, nb = fmt < 2 ? 10 : fmt == 2 ? 14 : 18;
    if (bs < hb) return -1;
    unsigned long long v = 0;
    for (int k = 0; k < hb; ++k) v |= (unsigned long long)b[k] << (8 * k);
    regen = (long long)((v >> 4) & ((1u << nb) - 1));
    comp = (long long)((v >> (4 + nb)) & ((1u << nb) - 1));
    streams = fmt == 0 ? 1 : 4;
    lp = hb;
  }
  if (regen > kBlockMax || lp + comp > bs) return -1;
  const uint8_t* lit = b + lp;                       // Raw: the literals themselves; RLE: lit[0], regen times
  if (ltype >= 2) {
    long long sp = 0;                                // inside the compressed literals
    if (ltype == 2) {
      if (STORE) {
        const int used = lane0(s, &f.huf_log, [&]() -> int { return huf_table(s, lit, comp); });
        if (used < 0) return -1;
        sp = used;
      }
      f.have_huf = true;
    } else if (!f.have_huf) return -1;
    if (STORE) {
      // up to four lanes, a stream each; the others wait at the vote
      long long sizes[4] = {comp - sp, 0, 0, 0}, first[4] = {sp, 0, 0, 0}, count[4] = {regen, 0, 0, 0};
      if (streams == 4) {
        if (comp - sp < 6) return -1;
        const long long each = (regen + 3) / 4;
        first[0] = sp + 6;
        long long total = 0;
        for (int k = 0; k < 3; ++k) {
          sizes[k] = ld16(lit + sp + 2 * k);
          first[k + 1] = first[k] + sizes[k];
          count[k] = each;
          total += sizes[k];
        }
        sizes[3] = comp - sp - 6 - total;
        count[3] = regen - 3 * each;
        if (sizes[3] < 1 || count[3] < 0) return -1;
      }
      bool bad = false;
      if ((int)threadIdx.x < streams) {
        const int k = threadIdx.x;
        Bits bits;
        bad = !bits.init(lit + first[k], sizes[k]);
        if (!bad) {
          uint8_t* to = lits + (streams == 4 ? k * ((regen + 3) / 4) : 0);
          const int log = f.huf_log;
          for (long long i = 0; i < count[k] && bits.left >= 0; ++i) {
            const uint32_t e = s.huf[bits.peek(log)];
            to[i] = (uint8_t)e;
            bits.left -= e >> 8;
          }
          bad = bits.left != 0;
        }
      }
      own_stores_done();
      if (__any(bad)) return -1;
      lit = lits;
    }
  }
  const bool lit_rle = ltype == 1;

  // the sequences
  long long sp = lp + comp;
  if (sp >= bs) return -1;
  long long nseq = b[sp++];
  if (nseq >= 128) {
    if (nseq == 255) {
      if (sp + 2 > bs) return -1;
      nseq = ld16(b + sp) + 0x7F00;
      sp += 2;
    } else {
      if (sp + 1 > bs) return -1;
      nseq = ((nseq - 128) << 8) + b[sp++];
    }
  }
  const long long out0 = out;
  long long used = 0;                                // literals consumed
  auto literals = [&](long long count) {
    if (STORE)
      for (long long i = threadIdx.x; i < count; i += kWave) dst[out + i] = lit_rle ? lit[0] : lit[used + i];
    used += count;
    out += count;
  };
  if (nseq == 0) {
    if (sp != bs || out + regen > limit) return -1;
    literals(regen);
    return out;
  }
  if (sp >= bs) return -1;
  const int modes = b[sp++];
  if (modes & 3) return -1;
  int r = seq_table(s, modes >> 6, s.ll, kLLLog, kLLSyms, kLLNorm, kLLSyms, 6, b + sp, bs - sp, f.have_seq, &f.ll_log, &f.predef[0]);
  if (r < 0) return -1;
  sp += r;
  r = seq_table(s, (modes >> 4) & 3, s.of, kOFLog, kOFSyms, kOFNorm, 29, 5, b + sp, bs - sp, f.have_seq, &f.of_log, &f.predef[1]);
  if (r < 0) return -1;
  sp += r;
  r = seq_table(s, (modes >> 2) & 3, s.ml, kMLLog, kMLSyms, kMLNorm, kMLSyms, 6, b + sp, bs - sp, f.have_seq, &f.ml_log, &f.predef[2]);
  if (r < 0) return -1;
  sp += r;
  Bits bits;
  if (!bits.init(b + sp, bs - sp)) return -1;
  uint32_t stl = bits.read(f.ll_log), sto = bits.read(f.of_log), stm = bits.read(f.ml_log);
  for (long long i = 0; i < nseq; ++i) {
    const FseCell cl = s.ll[stl], co = s.of[sto], cm = s.ml[stm];
    const uint32_t ofv = (1u << co.sym) + bits.read(co.sym);
    const long long ml = kMLBase[cm.sym] + bits.read(kMLBits[cm.sym]);
    const long long ll = kLLBase[cl.sym] + bits.read(kLLBits[cl.sym]);
    if (i + 1 < nseq) {
      stl = cl.base + bits.read(cl.nb);
      stm = cm.base + bits.read(cm.nb);
      sto = co.base + bits.read(co.nb);
    }
    if (bits.left < 0) return -1;
    uint32_t offset;
    if (ofv > 3) {
      offset = ofv - 3;
      f.rep[2] = f.rep[1];
      f.rep[1] = f.rep[0];
      f.rep[0] = offset;
    } else {
      const int idx = (int)ofv + (ll == 0);          // 1 .. 4
      if (idx == 1) offset = f.rep[0];
      else {
        offset = idx == 4 ? f.rep[0] - 1 : f.rep[idx - 1];
        if (idx != 2) f.rep[2] = f.rep[1];
        f.rep[1] = f.rep[0];
        f.rep[0] = offset;
      }
    }
    if (used + ll > regen || out + ll + ml > limit) return -1;
    literals(ll);
    if (offset == 0 || offset > f.window || (long long)offset > out - f.start) return -1;
    if (STORE) {
      own_stores_done();
      const uint8_t* from = dst + (out - offset);
      for (uint32_t k = threadIdx.x; k < (uint32_t)ml; k += kWave) dst[out + k] = from[k < offset ? k : k % offset];
    }
    out += ml;
  }
  if (bits.left != 0) return -1;
  f.have_seq = true;
  if (out + (regen - used) > limit) return -1;
  literals(regen - used);
  if (out - out0 > kBlockMax) return -1;
  return out;
}

// One payload p[0, len) -> dst[0, cap); *size <- the decoded bytes; returns the status.  All lanes, the same answer in each.
template <bool STORE>
__device__ int zstd_payload(ZLds& s, const uint8_t* p, long long len, uint8_t* dst, long long cap, int verify, uint8_t* lits,
                            long long* size) {
  long long pos = 0, out = 0;
  int st = 0;
  bool any = false;
  while (pos < len) {
    if (pos + 4 > len) return st | kBad;
    const uint32_t magic = ld32(p + pos);
    if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {      // skippable
      if (pos + 8 > len) return st | kBad;
      const long long skip = ld32(p + pos + 4);
      if (pos + 8 + skip > len) return st | kBad;
      pos += 8 + skip;
      continue;
    }
    if (magic != 0xFD2FB528u || pos + 5 > len) return st | kBad;
    any = true;
    const int fhd = p[pos + 4];
    pos += 5;
    const int fcs_flag = fhd >> 6, did_bytes = (fhd & 3) == 3 ? 4 : (fhd & 3);
    const bool single = (fhd & 0x20) != 0, checksum = (fhd & 4) != 0;
    const int fcs_bytes = fcs_flag == 0 ? (single ? 1 : 0) : 1 << fcs_flag;
    if ((fhd & 8) || pos + (single ? 0 : 1) + did_bytes + fcs_bytes > len) return st | kBad;
    FrameState f{out, 0, {1, 4, 8}, 0, 0, 0, 0, false, false, {false, false, false}};
    if (!single) {
      const int wd = p[pos++];
      const unsigned long long base = 1ull << (10 + (wd >> 3));
      f.window = base + (base >> 3) * (wd & 7);
    }
    for (int k = 0; k < did_bytes; ++k)
      if (p[pos++] != 0) return st | kBad;           // a dictionary
    unsigned long long fcs = 0;
    for (int k = 0; k < fcs_bytes; ++k) fcs |= (unsigned long long)p[pos++] << (8 * k);
    if (fcs_bytes == 2) fcs += 256;
    if (single) f.window = fcs;
    const long long block_max = f.window < (unsigned long long)kBlockMax ? (long long)f.window : kBlockMax;
    const bool by_fcs = !STORE && fcs_bytes != 0;    // MEASURE takes the frame's word for its size
    if (by_fcs) {
      if (fcs > (unsigned long long)(cap - out)) return st | kBad;
      out += (long long)fcs;
    }
    for (;;) {                                       // the blocks
      if (pos + 3 > len) return st | kBad;
      const uint32_t bh = p[pos] | (p[pos + 1] << 8) | (p[pos + 2] << 16);
      pos += 3;
      const int type = (bh >> 1) & 3;
      const long long bs = bh >> 3, in_bytes = type == 1 ? 1 : bs;
      if (type == 3 || bs > block_max || pos + in_bytes > len) return st | kBad;
      if (!by_fcs) {
        const long long limit = out + block_max < cap ? out + block_max : cap;
        if (type < 2) {
          if (out + bs > limit) return st | kBad;
          if (STORE)
            for (long long i = threadIdx.x; i < bs; i += kWave) dst[out + i] = p[pos + (type == 0 ? i : 0)];
          out += bs;
        } else {
          out = compressed_block<STORE>(s, f, p + pos, bs, dst, out, limit, lits);
          if (out < 0) return st | kBad;
        }
      }
      pos += in_bytes;
      if (bh & 1) break;
    }
    if (checksum) {
      if (pos + 4 > len) return st | kBad;
      if (STORE && verify) {
        own_stores_done();
        if ((uint32_t)xxh64_wave(dst + f.start, out - f.start) != ld32(p + pos)) st |= SCPOSE_AEDAT4_CHECKSUM;
      }
      pos += 4;
    }
    if (!by_fcs && fcs_bytes != 0 && fcs != (unsigned long long)(out - f.start)) return st | kBad;
  }
  if (!any) return st | kBad;
  *size = out;
  return st;
}

// The workgroup walks packets blockIdx.x, + gridDim.x, ...; lits + blockIdx.x * kBlockMax is its literal slot.  Slots as
// aedat4_lz4_kernel of events_aedat4_read.hip.
template <bool STORE>
__global__ __launch_bounds__(kWave) void aedat4_zstd_kernel(const uint8_t* __restrict__ file, const int64_t* __restrict__ packets,
                                                            int64_t n, int32_t* size, const int64_t* __restrict__ off,
                                                            uint8_t* staging, int64_t staging_bytes, int verify, int32_t* status,
                                                            uint8_t* lits) {
  __shared__ ZLds s;
  for (int64_t pk = blockIdx.x; pk < n; pk += gridDim.x) {
    long long cap = kMaxDecoded, got = 0;
    uint8_t* dst = nullptr;
    if (STORE) {
      if (status[pk] != 0) continue;                 // measured as damaged: nothing to decode
      cap = size[pk];
      if (off[pk] < 0 || off[pk] + cap > staging_bytes) {                  // the caller's buffer is not the one measure sized
        if (threadIdx.x == 0) status[pk] |= SCPOSE_AEDAT4_CORRUPT;
        continue;
      }
      dst = staging + off[pk];
    }
    int st = zstd_payload<STORE>(s, file + packets[2 * pk], packets[2 * pk + 1], dst, cap, verify,
                                 lits + (size_t)blockIdx.x * kBlockMax, &got);
    if (STORE && !(st & kBad) && got != cap) st |= kBad;                   // decode and measure disagree
    if (threadIdx.x == 0) {
      if (STORE) status[pk] |= st;
      else {
        status[pk] = st;
        size[pk] = st ? 0 : (int32_t)got;
      }
    }
    __syncthreads();
  }
}

inline int64_t grid_of(int64_t n) { return n < kZstdGrid ? n : kZstdGrid; }

}  // namespace

// the reader's workspace (events_aedat4_read.hip), then one literal slot per workgroup
size_t events_aedat4_zstd_workspace_bytes(int64_t n_packets) {
  return align256(events_aedat4_workspace_bytes(n_packets)) + (size_t)(n_packets > 0 ? grid_of(n_packets) : 1) * kBlockMax;
}

int32_t events_aedat4_zstd_measure_launch(const uint8_t* file, const int64_t* packets, int64_t n, int64_t* total_status, uint8_t* wsp,
                                          hipStream_t stream) {
  const Aedat4Slots sl = events_aedat4_slots(n, wsp);
  if (n > 0)
    hipLaunchKernelGGL(aedat4_zstd_kernel<false>, dim3((unsigned)grid_of(n)), dim3(kWave), 0, stream, file, packets, n, sl.size, sl.off,
                       (uint8_t*)nullptr, (int64_t)0, 0, sl.status, (uint8_t*)nullptr);
  return events_aedat4_sizes_launch(n, total_status, wsp, stream);
}

int32_t events_aedat4_zstd_decode_launch(const uint8_t* file, const int64_t* packets, int64_t n, uint8_t* staging,
                                         int64_t staging_bytes, int verify, uint8_t* wsp, hipStream_t stream) {
  const Aedat4Slots sl = events_aedat4_slots(n, wsp);
  if (n > 0)
    hipLaunchKernelGGL(aedat4_zstd_kernel<true>, dim3((unsigned)grid_of(n)), dim3(kWave), 0, stream, file, packets, n, sl.size, sl.off,
                       staging, staging_bytes, verify, sl.status, wsp + align256(events_aedat4_workspace_bytes(n)));
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
