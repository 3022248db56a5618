// PNG files -> frames or network crops on the device.  The host (png_read.py) walks the chunks, joins the IDAT
// payloads of an image into one zlib stream and hands over a descriptor per image: stream offset and length, sizes, colour type,
// palette.  Bit depth 8, not interlaced, colour types 0, 2, 3, 4, 6.  tests/png_decode_restated.py says the same in Python.
//
//   png_inflate_kernel    one wavefront per image.  Every lane walks the same bit stream (the control flow is wave-uniform), so a
//                         symbol costs what it costs one lane; what the wave shares is the rest: the input window and the last
//                         32 KiB of output live in LDS, the first-level tables of a block are filled 64 entries at a time, a match
//                         is copied by all lanes, the Adler-32 of a match is one wave reduction, and the output leaves LDS in
//                         coalesced words.  Writes the filtered scan lines, h x (1 + w channels) bytes, into the image's plane.
//                         It DETECTS every abnormal stream (SCPOSE_PNG_CORRUPT, _CHECKSUM) and never interprets one: the host
//                         decoder says what a damaged file means.  Bytes past the plane are decoded and summed, not stored.
//   png_unfilter_kernel   one wavefront per image, bands of 64 rows in order.  Inside a band lane k owns row r0 + k and the lanes
//                         run skewed: at step s lane k reconstructs pixel s - k, whose left neighbour is its own last result and
//                         whose up and up-left neighbours are the last two results of lane k - 1 (a cross-lane move).  All five
//                         filter types take this one path.  In place.  A filter byte above 4 sets SCPOSE_PNG_FILTER.  An image
//                         that inflate left CORRUPT is not looked at: its plane is incomplete.
//   png_output_kernel     one thread per pixel: gray replicated, palette looked up, alpha dropped -> (n, h, w, 3) RGB or BGR.
//   png_crop_kernel       the decoders' shared crop tail (crop_tail.h), each tap fetched from the unfiltered plane through the same
//                         expansion.  Only the rows down to the window's last are unfiltered.
#include "common.h"
#include "crop_tail.h"

namespace scpose {
namespace {

constexpr int kWave = 64;
constexpr int kDesc = SCPOSE_PNG_DESC_BYTES, kDescHead = 64;
constexpr int kWin = 32768;              // deflate's window: the output ring in LDS
constexpr int kFlush = 4096;             // the ring is written out when this much of it is new
constexpr int kInWords = 1024;           // input window in LDS, 32-bit words
constexpr int kLitBits = 10, kDistBits = 8;

struct Desc {
  long long off, len;
  int32_t h, w, color_type, channels;
};
__device__ __forceinline__ Desc load_desc(const uint8_t* __restrict__ desc, int img) {
  const uint8_t* d = desc + (size_t)img * kDesc;
  const long long* q = reinterpret_cast<const long long*>(d);
  const int32_t* v = reinterpret_cast<const int32_t*>(d + 16);
  return {q[0], q[1], v[0], v[1], v[2], v[3]};
}

__host__ __device__ inline size_t plane_stride(int h, int w, int channels) {
  return (((size_t)h * (1 + (size_t)w * channels)) + 15) & ~(size_t)15;
}

__constant__ uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// A canonical Huffman code in LDS: codes per length, the symbols sorted by (length, symbol), and a first-level table on the next
// `bits` bits of the stream (code length << 9 | symbol; 0: a longer code, or no code at all).
struct Code {
  uint16_t count[16];
  uint16_t offs[16];        // scratch of the sort
  uint16_t symbol[288];
};

// The bit reader: wave-uniform.  The stream's words come through an LDS window; words past the stream read as 0 and `used() > total`
// says the input is exhausted.
struct Bits {
  const uint8_t* __restrict__ src;   // the stream (4-byte aligned)
  long long len;                     // bytes
  uint32_t* win;                     // LDS, kInWords
  long long word;                    // index of the next word to take
  long long base;                    // first word of the window
  unsigned long long buf;
  int cnt;

  __device__ __forceinline__ void fill_window() {
    base = word;
    __syncthreads();
    for (int i = threadIdx.x; i < kInWords; i += kWave) {
      const long long b = (base + i) * 4;
      uint32_t v = 0;
      if (b + 4 <= len) v = *reinterpret_cast<const uint32_t*>(src + b);
      else
        for (int k = 0; k < 4; ++k)
          if (b + k < len) v |= (uint32_t)src[b + k] << (8 * k);
      win[i] = v;
    }
    __syncthreads();
  }
  __device__ __forceinline__ void seek(long long byte) {
    word = byte >> 2;
    fill_window();
    buf = win[0];
    word += 1;
    cnt = 32 - 8 * (int)(byte & 3);
    buf >>= 8 * (int)(byte & 3);
  }
  __device__ __forceinline__ void need32() {      // at least 32 bits in buf
    if (cnt < 32) {
      if (word - base >= kInWords) fill_window();
      buf |= (unsigned long long)win[word - base] << cnt;
      word += 1;
      cnt += 32;
    }
  }
  __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)buf & ((1u << n) - 1u); }
  __device__ __forceinline__ void drop(int n) { buf >>= n; cnt -= n; }
  __device__ __forceinline__ uint32_t take(int n) {   // n <= 16, after need32()
    const uint32_t v = peek(n);
    drop(n);
    return v;
  }
  __device__ __forceinline__ long long used_bits() const { return word * 32 - cnt; }
  __device__ __forceinline__ bool exhausted() const { return used_bits() > len * 8; }
};

// counts the lengths, checks the set, sorts the symbols (lane 0) -- then every lane fills its share of the first-level table.
// allow_single: an incomplete set passes when its longest code has one bit (zlib: one distance code, or none).  -> false: corrupt
__device__ bool build_code(const uint8_t* lens, int n, bool allow_single, Code& c, uint16_t* lut, int lut_bits) {
  __shared__ int ok;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int l = 0; l < 16; ++l) c.count[l] = 0;
    for (int s = 0; s < n; ++s) c.count[lens[s]] += 1;
    c.count[0] = 0;
    int left = 1, longest = 0;
    bool good = true;
    for (int l = 1; l < 16; ++l) {
      left = (left << 1) - c.count[l];
      if (left < 0) { good = false; break; }
      if (c.count[l]) longest = l;
    }
    if (good && left > 0 && !(allow_single && longest <= 1)) good = false;
    if (good) {
      c.offs[1] = 0;
      for (int l = 1; l < 15; ++l) c.offs[l + 1] = c.offs[l] + c.count[l];
      for (int s = 0; s < n; ++s)
        if (lens[s]) c.symbol[c.offs[lens[s]]++] = (uint16_t)s;
    }
    ok = good;
  }
  __syncthreads();
  if (!ok) return false;
  for (int i = threadIdx.x; i < (1 << lut_bits); i += kWave) {      // the stream's next bits, first bit lowest
    int code = 0, first = 0, index = 0;
    uint16_t e = 0;
    for (int l = 1; l <= lut_bits; ++l) {
      code |= (i >> (l - 1)) & 1;
      const int cnt = c.count[l];
      if (code - cnt < first) { e = (uint16_t)((l << 9) | c.symbol[index + (code - first)]); break; }
      index += cnt;
      first = (first + cnt) << 1;
      code <<= 1;
    }
    lut[i] = e;
  }
  __syncthreads();
  return true;
}

// the next symbol of code c: -1 when the bits are no code.  After need32(); consumes at most 15 bits.
__device__ __forceinline__ int next_symbol(Bits& b, const Code& c, const uint16_t* lut, int lut_bits) {
  const uint16_t e = lut[b.peek(lut_bits)];
  if (e) {
    b.drop(e >> 9);
    return e & 511;
  }
  int code = 0, first = 0, index = 0;
  uint32_t bits = b.peek(15);
  for (int l = 1; l < 16; ++l) {
    code |= bits & 1;
    bits >>= 1;
    const int cnt = c.count[l];
    if (code - cnt < first) {
      b.drop(l);
      return c.symbol[index + (code - first)];
    }
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  return -1;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
  return v;
}

// The output side: the ring, the Adler-32 and the plane.
struct Out {
  uint8_t* ring;                     // LDS, kWin
  uint8_t* __restrict__ plane;       // the image's plane (16-byte aligned)
  unsigned long long need;           // bytes of the plane
  unsigned long long pos;            // bytes produced
  unsigned long long flushed;        // bytes of them written to the plane or dropped; a multiple of 4
  uint32_t a, b;                     // Adler-32, both below 65521

  // ring -> plane for [flushed, upto): whole words by all lanes, the plane's last bytes one by one
  __device__ __forceinline__ void flush(unsigned long long upto) {
    __syncthreads();
    const uint32_t* ring32 = reinterpret_cast<const uint32_t*>(ring);
    for (unsigned long long p = flushed + 4ull * threadIdx.x; p < upto; p += 4ull * kWave) {
      if (p >= need) break;
      const uint32_t v = ring32[(p & (kWin - 1)) >> 2];
      if (p + 4 <= need && p + 4 <= upto) *reinterpret_cast<uint32_t*>(plane + p) = v;
      else
        for (int k = 0; k < 4; ++k)
          if (p + k < need && p + k < upto) plane[p + k] = (uint8_t)(v >> (8 * k));
    }
    flushed = upto;
    __syncthreads();
  }
  __device__ __forceinline__ void maybe_flush() {
    if (pos - flushed >= kFlush) flush(pos & ~3ull);
  }
  __device__ __forceinline__ void literal(uint32_t v) {
    if (threadIdx.x == 0) ring[pos & (kWin - 1)] = (uint8_t)v;
    a += v; if (a >= 65521u) a -= 65521u;
    b += a; if (b >= 65521u) b -= 65521u;
    pos += 1;
  }
  // `n` bytes (n <= 65535) whose i-th is byte(i): stored by all lanes, summed by one reduction per 256 bytes
  template <typename F>
  __device__ __forceinline__ void run(int n, F byte) {
    for (int i0 = 0; i0 < n; i0 += 256) {
      const int m = n - i0 < 256 ? n - i0 : 256;
      uint32_t s1 = 0, s2 = 0;
      for (int i = threadIdx.x; i < m; i += kWave) {
        const uint32_t v = byte(i0 + i);
        ring[(pos + i) & (kWin - 1)] = (uint8_t)v;
        s1 += v;
        s2 += (uint32_t)(m - i) * v;
      }
      s1 = wave_sum(s1);
      s2 = wave_sum(s2);
      b = (b + (uint32_t)m * a + s2) % 65521u;       // m a < 2^24, s2 < 2^24: no overflow
      a = (a + s1) % 65521u;
      pos += m;
      maybe_flush();
    }
  }
};

struct InflateLds {
  uint32_t in[kInWords];
  uint8_t ring[kWin];
  Code lit, dist, cl;
  uint16_t lit_lut[1 << kLitBits];
  uint16_t dist_lut[1 << kDistBits];
  uint16_t cl_lut[1 << 7];
  uint8_t lens[352];                 // [0, 19) the code-length code's lengths, [24, 24 + HLIT + HDIST) the block's; or the fixed 320
};

__global__ __launch_bounds__(kWave) void png_inflate_kernel(const uint8_t* __restrict__ desc, const uint8_t* __restrict__ data,
                                                            uint8_t* __restrict__ planes, size_t stride, int32_t* __restrict__ status) {
  __shared__ InflateLds s;
  const int img = blockIdx.x;
  const Desc d = load_desc(desc, img);
  Out o{s.ring, planes + (size_t)img * stride, (unsigned long long)d.h * (1ull + (unsigned long long)d.w * d.channels), 0, 0, 1, 0};
  Bits in{data + d.off, d.len, s.in, 0, 0, 0, 0};
  int st = 0;
  int fixed_built = 0;                   // which tables the LDS holds: 1 = the fixed ones
  if (d.len < 2) st = SCPOSE_PNG_CORRUPT;
  else in.seek(2);
  while (!st) {
    in.need32();
    const uint32_t final = in.take(1), kind = in.take(2);
    if (in.exhausted() || kind == 3) { st = SCPOSE_PNG_CORRUPT; break; }
    if (kind == 0) {
      in.drop(in.cnt & 7);
      in.need32();
      const uint32_t ln = in.take(16);
      in.need32();
      const uint32_t nln = in.take(16);
      const long long at = in.used_bits() >> 3;
      if (in.exhausted() || ln != (~nln & 0xFFFFu) || at + (long long)ln > d.len) { st = SCPOSE_PNG_CORRUPT; break; }
      const uint8_t* __restrict__ p = in.src + at;
      o.run((int)ln, [&](int i) { return (uint32_t)p[i]; });
      in.seek(at + ln);
    } else {
      if (kind == 1) {
        if (fixed_built != 1) {
          __syncthreads();
          for (int i = threadIdx.x; i < 320; i += kWave) s.lens[i] = i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : (i < 288 ? 8 : 5)));
          build_code(s.lens, 288, false, s.lit, s.lit_lut, kLitBits);
          build_code(s.lens + 288, 32, false, s.dist, s.dist_lut, kDistBits);
          fixed_built = 1;
        }
      } else {
        fixed_built = 0;
        in.need32();
        const int hlit = (int)in.take(5) + 257, hdist = (int)in.take(5) + 1, hclen = (int)in.take(4) + 4;
        if (hlit > 286 || hdist > 30) { st = SCPOSE_PNG_CORRUPT; break; }
        __syncthreads();
        if (threadIdx.x < 19) s.lens[threadIdx.x] = 0;
        __syncthreads();
        for (int i = 0; i < hclen; ++i) {
          in.need32();
          const uint32_t v = in.take(3);
          if (threadIdx.x == 0) s.lens[kClOrder[i]] = (uint8_t)v;
        }
        if (in.exhausted() || !build_code(s.lens, 19, false, s.cl, s.cl_lut, 7)) { st = SCPOSE_PNG_CORRUPT; break; }
        int idx = 0, prev = 0;
        const int total = hlit + hdist;
        while (idx < total) {
          in.need32();
          const int sym = next_symbol(in, s.cl, s.cl_lut, 7);
          if (sym < 0) { st = SCPOSE_PNG_CORRUPT; break; }
          int rep = 1, v = sym;
          if (sym == 16) {
            if (idx == 0) { st = SCPOSE_PNG_CORRUPT; break; }
            v = prev; rep = 3 + (int)in.take(2);
          } else if (sym == 17) { v = 0; rep = 3 + (int)in.take(3); }
          else if (sym == 18) { v = 0; rep = 11 + (int)in.take(7); }
          if (in.exhausted() || idx + rep > total) { st = SCPOSE_PNG_CORRUPT; break; }
          // lane 0 alone wrote the code-length lengths above; these go where the code-length code does not read
          if (threadIdx.x == 0)
            for (int k = 0; k < rep; ++k) s.lens[24 + idx + k] = (uint8_t)v;
          idx += rep;
          prev = v;
        }
        if (st) break;
        __syncthreads();
        if (s.lens[24 + 256] == 0) { st = SCPOSE_PNG_CORRUPT; break; }
        if (!build_code(s.lens + 24, hlit, true, s.lit, s.lit_lut, kLitBits) ||
            !build_code(s.lens + 24 + hlit, hdist, true, s.dist, s.dist_lut, kDistBits)) { st = SCPOSE_PNG_CORRUPT; break; }
      }
      for (;;) {                           // the symbols of the block
        in.need32();
        const int sym = next_symbol(in, s.lit, s.lit_lut, kLitBits);
        if (sym < 0 || sym > 285 || in.exhausted()) { st = SCPOSE_PNG_CORRUPT; break; }
        if (sym < 256) {
          o.literal((uint32_t)sym);
          o.maybe_flush();
          continue;
        }
        if (sym == 256) break;
        in.need32();
        const int ln = kLenBase[sym - 257] + (int)in.take(kLenExtra[sym - 257]);
        in.need32();
        const int ds = next_symbol(in, s.dist, s.dist_lut, kDistBits);
        if (ds < 0 || ds > 29) { st = SCPOSE_PNG_CORRUPT; break; }
        in.need32();
        const uint32_t dist = kDistBase[ds] + in.take(kDistExtra[ds]);
        if (in.exhausted() || dist > o.pos || dist > (uint32_t)kWin) { st = SCPOSE_PNG_CORRUPT; break; }
        // every source byte lies before the match: where the distance is shorter than the length the pattern repeats.
        // The ring is exactly deflate's window, so at a distance within 258 bytes of 32 768 the slot byte i is stored to is the slot
        // byte j = i - (32768 - distance) <= i is loaded from.  The copy is right because no load comes after the store that
        // overwrites its slot: Out::run loads byte(i) before it stores byte i in program order, a wave's LDS operations complete
        // in the order they are issued, the 64 lanes of one iteration load in ONE instruction that precedes their one store
        // instruction, and a later iteration only stores to slots whose j lies in an earlier or the same iteration (the loads and
        // stores may alias, so the compiler keeps their order).  tests: the hand_far_matches case (distances 32768 and 32758).
        __syncthreads();
        const uint32_t from = (uint32_t)(o.pos - dist);
        const uint8_t* ring = s.ring;
        o.run(ln, [&](int i) { return (uint32_t)ring[(from + ((uint32_t)i < dist ? (uint32_t)i : (uint32_t)i % dist)) & (kWin - 1)]; });
      }
      if (st) break;
    }
    if (final) {
      in.drop(in.cnt & 7);
      const long long at = in.used_bits() >> 3;
      if (at + 4 <= d.len) {               // a stream cut inside its trailer is not checked: zlib never reports what it has not read
        in.need32();
        const uint32_t t = (uint32_t)in.buf;
        const uint32_t want = (t >> 24) | ((t >> 8) & 0xFF00u) | ((t << 8) & 0xFF0000u) | (t << 24);
        if (want != ((o.b << 16) | o.a)) st |= SCPOSE_PNG_CHECKSUM;
      }
      if (o.pos < o.need) st |= SCPOSE_PNG_CORRUPT;
      break;
    }
  }
  o.flush(o.pos);
  if (threadIdx.x == 0) status[img] = st;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// rows: how many rows of image blockIdx.x to reconstruct (all h, or down to the crop window's last row: rows_of[img])
__global__ __launch_bounds__(kWave) void png_unfilter_kernel(uint8_t* __restrict__ planes, size_t stride, int h, int w, int bpp,
                                                             const int32_t* __restrict__ rows_of, int32_t* __restrict__ status) {
  const int img = blockIdx.x, lane = threadIdx.x;
  uint8_t* plane = planes + (size_t)img * stride;
  const size_t line = 1 + (size_t)w * bpp;
  // an image whose stream is corrupt has no complete plane: what lies behind the bytes inflate produced is whatever the workspace
  // held, so neither its filter bytes are judged nor its rows reconstructed -- the status stays what inflate found
  if (status[img] & SCPOSE_PNG_CORRUPT) return;
  int bad = 0;
  for (int r = lane; r < h; r += kWave) bad |= plane[(size_t)r * line] > 4;
  if (__any(bad) && lane == 0) status[img] |= SCPOSE_PNG_FILTER;
  const int rows = rows_of ? (rows_of[img] < h ? rows_of[img] : h) : h;
  for (int r0 = 0; r0 < rows; r0 += kWave) {
    const int r = r0 + lane;
    const bool live = r < rows;
    uint8_t* row = plane + (size_t)(live ? r : r0) * line + 1;
    const uint8_t* above = r0 ? plane + (size_t)(r0 - 1) * line + 1 : nullptr;      // lane 0's up row: the band before, already done
    int f = live ? plane[(size_t)r * line] : 0;
    if (f > 4) f = 0;
    uint32_t last = 0, last2 = 0;            // this lane's pixels x - 1 and x - 2, bytes packed
    for (int s = 0; s < w + kWave - 1; ++s) {
      uint32_t up = __shfl_up(last, 1, kWave), ul = __shfl_up(last2, 1, kWave);
      const int x = s - lane;
      if (lane == 0) {
        up = 0; ul = 0;
        if (above && x < w) {
          for (int k = 0; k < bpp; ++k) {
            up |= (uint32_t)above[(size_t)x * bpp + k] << (8 * k);
            if (x > 0) ul |= (uint32_t)above[(size_t)(x - 1) * bpp + k] << (8 * k);
          }
        }
      }
      if (live && x >= 0 && x < w) {
        uint32_t cur = 0;
        for (int k = 0; k < bpp; ++k) {
          const int a = (last >> (8 * k)) & 255, b = (up >> (8 * k)) & 255, c = (ul >> (8 * k)) & 255;
          const int pred = f == 0 ? 0 : (f == 1 ? a : (f == 2 ? b : (f == 3 ? (a + b) >> 1 : paeth(a, b, c))));
          const int v = (row[(size_t)x * bpp + k] + pred) & 255;
          row[(size_t)x * bpp + k] = (uint8_t)v;
          cur |= (uint32_t)v << (8 * k);
        }
        last2 = last;
        last = cur;
      }
    }
    __threadfence();                         // the band's last row is the next band's up row, read by another lane
    __syncthreads();
  }
}

// pixel (x, y) of the frame from the unfiltered plane: gray replicated, palette looked up, alpha dropped
__device__ __forceinline__ Rgb png_pixel(const uint8_t* __restrict__ plane, size_t line, int bpp, int color_type,
                                         const uint8_t* __restrict__ palette, int x, int y) {
  const uint8_t* p = plane + (size_t)y * line + 1 + (size_t)x * bpp;
  if (color_type == 3) {
    const uint8_t* e = palette + 3 * (int)p[0];
    return {e[0], e[1], e[2]};
  }
  if (bpp < 3) return {p[0], p[0], p[0]};
  return {p[0], p[1], p[2]};
}

__global__ __launch_bounds__(256) void png_output_kernel(const uint8_t* __restrict__ desc, const uint8_t* __restrict__ planes, size_t stride,
                                                         int h, int w, int bpp, int bgr, uint8_t* __restrict__ out) {
  const int img = blockIdx.y;
  const int64_t total = (int64_t)h * w;
  const int color_type = load_desc(desc, img).color_type;
  const uint8_t* palette = desc + (size_t)img * kDesc + kDescHead;
  const uint8_t* plane = planes + (size_t)img * stride;
  uint8_t* o = out + (size_t)img * total * 3;
  for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < total; pix += (int64_t)gridDim.x * 256) {
    const Rgb v = png_pixel(plane, 1 + (size_t)w * bpp, bpp, color_type, palette, (int)(pix % w), (int)(pix / w));
    o[pix * 3] = (uint8_t)(bgr ? v.b : v.r);
    o[pix * 3 + 1] = (uint8_t)v.g;
    o[pix * 3 + 2] = (uint8_t)(bgr ? v.r : v.b);
  }
}

__global__ void png_rows_kernel(RoiChunk rois, int img0, int count, int32_t* __restrict__ rows_of) {
  if ((int)threadIdx.x < count) rows_of[img0 + threadIdx.x] = rois.v[threadIdx.x][1] + rois.v[threadIdx.x][3];
}

// The crop tail (crop_tail.h) of frame img0 + blockIdx.y: the window bounds the rows png_unfilter_kernel has reconstructed.
__global__ __launch_bounds__(kCropThreads) void png_crop_kernel(const uint8_t* __restrict__ desc, const uint8_t* __restrict__ planes, size_t stride,
                                                                int h, int w, int bpp, int bgr, const double* __restrict__ minv, RoiChunk rois,
                                                                int img0, int oh, int ow, uint8_t* __restrict__ out) {
  const int img = img0 + (int)blockIdx.y;
  const int color_type = load_desc(desc, img).color_type;
  const uint8_t* palette = desc + (size_t)img * kDesc + kDescHead;
  const uint8_t* plane = planes + (size_t)img * stride;
  const auto px = [&](int32_t x, int32_t y) { return png_pixel(plane, 1 + (size_t)w * bpp, bpp, color_type, palette, x, y); };
  crop_tail(px, h, w, false, bgr, minv + (size_t)img * 6, rois.v[blockIdx.y], oh, ow, out + (size_t)img * ((int64_t)oh * ow) * 3);
}

// the workspace: the descriptors as uploaded, the rows to unfilter per image, the planes
struct Plan {
  uint8_t* desc;
  int32_t* rows;
  uint8_t* planes;
  size_t stride, bytes;
};
Plan make_plan(int n, int h, int w, int channels, uint8_t* ws) {
  Plan p{};
  size_t o = 0;
  p.desc = ws + o; o += (size_t)n * kDesc;
  p.rows = reinterpret_cast<int32_t*>(ws + o); o += (((size_t)n * 4) + 255) & ~(size_t)255;
  o = (o + 255) & ~(size_t)255;
  p.planes = ws + o;
  p.stride = plane_stride(h, w, channels);
  p.bytes = o + (size_t)n * p.stride;
  return p;
}

int32_t launch_inflate(const Plan& p, const uint8_t* desc_host, const uint8_t* data, int n, int32_t* status, hipStream_t stream) {
  SCP_CHECK_HIP(hipMemcpyAsync(p.desc, desc_host, (size_t)n * kDesc, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)n), dim3(kWave), 0, stream, p.desc, data, p.planes, p.stride, status);
  return SCPOSE_OK;
}

}  // namespace

size_t png_decode_workspace_bytes(int n, int h, int w, int channels) { return make_plan(n, h, w, channels, nullptr).bytes; }

int32_t png_decode_launch(const uint8_t* desc_host, const uint8_t* data, int n, int h, int w, int channels, int bgr, uint8_t* out,
                          int32_t* status, uint8_t* ws, hipStream_t stream) {
  const Plan p = make_plan(n, h, w, channels, ws);
  if (int32_t rc = launch_inflate(p, desc_host, data, n, status, stream)) return rc;
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(kWave), 0, stream, p.planes, p.stride, h, w, channels, nullptr, status);
  const int64_t groups = ((int64_t)h * w + 255) / 256;
  hipLaunchKernelGGL(png_output_kernel, dim3((unsigned)(groups < 4096 ? groups : 4096), (unsigned)n), dim3(256), 0, stream, p.desc, p.planes,
                     p.stride, h, w, channels, bgr, out);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t png_decode_crop_launch(const uint8_t* desc_host, const uint8_t* data, int n, int h, int w, int channels, int bgr, const double* minv,
                               const int32_t* roi_host, int out_h, int out_w, uint8_t* crops, int32_t* status, uint8_t* ws,
                               hipStream_t stream) {
  const Plan p = make_plan(n, h, w, channels, ws);
  if (int32_t rc = launch_inflate(p, desc_host, data, n, status, stream)) return rc;
  for_each_roi_chunk(roi_host, n, [&](const RoiChunk& rois, int img0, int count) {
    hipLaunchKernelGGL(png_rows_kernel, dim3(1), dim3(kRoiChunk), 0, stream, rois, img0, count, p.rows);
  });
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(kWave), 0, stream, p.planes, p.stride, h, w, channels, p.rows, status);
  for_each_roi_chunk(roi_host, n, [&](const RoiChunk& rois, int img0, int count) {
    hipLaunchKernelGGL(png_crop_kernel, crop_tail_grid(out_h, out_w, count), dim3(kCropThreads), 0, stream, p.desc, p.planes, p.stride, h, w,
                       channels, bgr, minv, rois, img0, out_h, out_w, crops);
  });
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
