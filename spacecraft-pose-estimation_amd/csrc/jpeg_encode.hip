// (N, H, W, 3) uint8 RGB frames on the device -> baseline JPEG byte streams, byte for byte what libjpeg's baseline encoder writes
// with the standard Huffman tables (PIL's save with its defaults): jccolor.c's rgb_ycc_convert, the edge expansion of jcsample.c /
// jcprepct.c, h2v2_downsample, jfdctint.c's forward DCT, jcdctmgr.c's quantiser, jccoefct.c's dummy blocks, jchuff.c's coder.
// The opposite direction of jpeg_decode.hip.  The host (jpeg_write.py) supplies the bytes in front of the scan (SOI .. SOS) and
// the Huffman tables as one code | length << 16 word per symbol; the quantisation tables follow from `quality` (jcparam.c).
//
//   jpeg_enc_dct_kernel     one thread per block in scan order: colour conversion, edge replication, 4:2:0 downsampling, forward DCT
//       in registers, quantiser; 64 int16 in zig-zag order.  Edges: columns are replicated to the block grid of the component
//       BEFORE downsampling, rows to an even count before and the downsampled rows to the block grid after; a Y block of a
//       4:2:0 MCU that lies wholly outside the block grid is a "dummy": zero but for the DC value of the block before it.
//   jpeg_enc_bits_kernel    one thread per block: the bits its code words take (DC difference against the block of the same
//       component before it in the scan).
//   jpeg_enc_scan_*         per image, scan_device.h's three passes: exclusive scan of the bit counts, the image's total.
//   jpeg_enc_zero_kernel    zeroes the words the image's bits will occupy.
//   jpeg_enc_emit_kernel    one thread per block: the same walk, code words written at the block's bit offset, MSB first in
//       32-bit words.  A word shared with a neighbouring block is joined with atomicOr (order-independent: two runs are bitwise
//       equal), a word the block owns alone is stored.  The last block adds the fill of ones up to the byte.
//   jpeg_enc_count_kernel / jpeg_enc_sizes_kernel / jpeg_enc_offsets_kernel   0xFF bytes per tile of 4096 raw bytes, their
//       scan per image, the size of every stream, the int64 offsets of the packed streams and the capacity check.
//   jpeg_enc_write_kernel   header, the raw bytes with a 00 after every FF, EOI.
//
// Capacity.  A coefficient takes at most 16 bits of code and 11 bits of value (a ZRL run belongs to the coefficient that ends
// it: 3 x 11 + 16 + 10 bits spread over at least 48 coefficients; EOB, 4 bits, stands for at least one), so a block takes at most
// 64 x 27 = 1728 bits = 216 bytes and an image blocks x 216 bytes before stuffing, the fill included (the bound is whole bytes).
// Stuffing at most doubles it: header + 432 x blocks + 2 (EOI) bytes per image always suffice.  The streams are packed; an
// image whose end lies past the caller's capacity gets SCPOSE_JPEG_ENC_CAPACITY and not one of its bytes is written.
// No floating point; integer atomics only.
#include "jpeg_common.h"
#include "scan_device.h"

#include <utility>

namespace scpose {

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kScanThreads, "the scan bodies of scan_device.h run in the workgroups of this file");
constexpr int kBlockBits = 64 * 27;                  // see "Capacity"
constexpr int kBlockWords = kBlockBits / 32;
constexpr int kTileBytes = kThreads * 16;            // raw bytes per workgroup of the stuffing passes
constexpr int kTileWords = kTileBytes / 4;

struct EncGeo {
  int32_t n, h, w, mode, bpm, ycount, hs, mcus_x, mcus_y, n_blocks, ybc, ybr, scan_tiles, raw_tiles, header_bytes;
  int64_t raw_words;     // per image, a multiple of kTileWords
};

EncGeo make_geo(int n, int h, int w, int mode, int header_bytes) {
  const JpegFrame f = jpeg_frame(h, w, mode);
  EncGeo g{};
  g.n = n; g.h = h; g.w = w; g.mode = mode; g.header_bytes = header_bytes;
  g.hs = f.hs; g.ycount = f.ycount; g.bpm = f.bpm; g.mcus_x = f.mcus_x; g.mcus_y = f.mcus_y; g.n_blocks = f.n_blocks;
  g.ybc = (w + 7) / 8; g.ybr = (h + 7) / 8;
  g.scan_tiles = (g.n_blocks + kScanTile - 1) / kScanTile;
  const int64_t words = (int64_t)g.n_blocks * kBlockWords + 1;
  g.raw_tiles = (int32_t)((words + kTileWords - 1) / kTileWords);
  g.raw_words = (int64_t)g.raw_tiles * kTileWords;
  return g;
}

// T.81 annex K.1 in natural order; jcparam.c scales them: jpeg_quality_scaling, jpeg_add_quant_table with force_baseline
__constant__ uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// the K-th coefficient in zig-zag order: its place is a constant expression
template <int K>
__device__ __forceinline__ int32_t zig_of(const int32_t (&ws)[8][8]) {
  constexpr int i = kZigzag[K];
  return ws[i >> 3][i & 7];
}

// packed[i] = coefficients 2 i and 2 i + 1 of the zig-zag order as two int16; a dummy block keeps its DC value alone
template <int... I>
__device__ __forceinline__ void pack_zigzag(const int32_t (&ws)[8][8], bool dummy, uint32_t (&packed)[32], std::integer_sequence<int, I...>) {
  ((packed[I] = ((uint32_t)((dummy && I != 0) ? 0 : zig_of<2 * I>(ws)) & 0xffffu) | ((uint32_t)(dummy ? 0 : zig_of<2 * I + 1>(ws)) << 16)), ...);
}

// jfdctint.c's jpeg_fdct_islow (the constants: jpeg_common.h)
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(const int32_t (&d)[8], int32_t (&out)[8]) {
  constexpr int N = FIRST ? 13 - 2 : 13 + 2;
  constexpr int32_t half = 1 << (N - 1);
  int32_t tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  int32_t tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  out[0] = FIRST ? (tmp10 + tmp11) * 4 : (tmp10 + tmp11 + 2) >> 2;
  out[4] = FIRST ? (tmp10 - tmp11) * 4 : (tmp10 - tmp11 + 2) >> 2;
  int32_t z1 = (tmp12 + tmp13) * F0541;
  out[2] = (z1 + tmp13 * F0765 + half) >> N;
  out[6] = (z1 - tmp12 * F1847 + half) >> N;
  z1 = tmp4 + tmp7;
  int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int32_t z5 = (z3 + z4) * F1175;
  tmp4 *= F0298; tmp5 *= F2053; tmp6 *= F3072; tmp7 *= F1501;
  z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
  z3 += z5; z4 += z5;
  out[7] = (tmp4 + z1 + z3 + half) >> N;
  out[5] = (tmp5 + z2 + z4 + half) >> N;
  out[3] = (tmp6 + z2 + z3 + half) >> N;
  out[1] = (tmp7 + z1 + z4 + half) >> N;
}

// jccolor.c, SCALEBITS 16: the weights of one component
struct Ycc {
  int32_t r, g, b, add;
};
__device__ __forceinline__ Ycc ycc_of(int comp) {
  if (comp == 0) return {19595, 38470, 7471, 32768};
  if (comp == 1) return {-11059, -21709, 32768, (128 << 16) + 32767};
  return {32768, -27439, -5329, (128 << 16) + 32767};
}
// the component's sample of pixel (x, y), both inside the frame
__device__ __forceinline__ int32_t ycc_sample(const uint8_t* __restrict__ frame, int32_t w, int32_t x, int32_t y, const Ycc& k) {
  const uint8_t* p = frame + ((size_t)y * w + x) * 3;
  return (k.r * (int32_t)p[0] + k.g * (int32_t)p[1] + k.b * (int32_t)p[2] + k.add) >> 16;
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_dct_kernel(const uint8_t* __restrict__ frames, EncGeo geo, int quality,
                                                                int16_t* __restrict__ coef) {
  __shared__ int32_t q[2][64];                         // the divisors: 8 x the quantisation table (the DCT's output is scaled by 8)
  if (threadIdx.x < 128) {
    const int32_t scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int32_t v = ((int32_t)kBaseQuant[threadIdx.x >> 6][threadIdx.x & 63] * scale + 50) / 100;
    q[threadIdx.x >> 6][threadIdx.x & 63] = 8 * (v < 1 ? 1 : (v > 255 ? 255 : v));
  }
  __syncthreads();
  const int img = blockIdx.y;
  const int32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= geo.n_blocks) return;
  const int32_t mcu = b / geo.bpm, blk = b - mcu * geo.bpm;
  const int comp = mcu_comp_index(blk, geo.ycount);
  const int32_t mx = mcu % geo.mcus_x, my = mcu / geo.mcus_x;
  int32_t bx = mx, by = my;                            // block coordinates in the component's plane
  bool dummy = false;
  if (comp == 0 && geo.hs == 2) {
    bx = 2 * mx + (blk & 1); by = 2 * my + (blk >> 1);
    if (by >= geo.ybr) {                               // a dummy row: the DC value of block 1, itself a dummy when the column is
      dummy = true;
      by = 2 * my; bx = 2 * mx + 1 < geo.ybc ? 2 * mx + 1 : 2 * mx;
    } else if (bx >= geo.ybc) {
      dummy = true;
      bx -= 1;
    }
  }
  const uint8_t* frame = frames + (size_t)img * geo.h * geo.w * 3;
  const bool sub = comp != 0 && geo.hs == 2;
  const Ycc kc = ycc_of(comp);
  const int32_t crows = (geo.h + 1) >> 1;              // downsampled rows that hold data
  int32_t ws[8][8];                                    // [row][column]
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int32_t d[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int32_t px = bx * 8 + c, py = by * 8 + r;
      int32_t v;
      if (!sub) {
        v = ycc_sample(frame, geo.w, px < geo.w ? px : geo.w - 1, py < geo.h ? py : geo.h - 1, kc);
      } else {
        const int32_t cy = py < crows ? py : crows - 1;
        const int32_t xa = 2 * px < geo.w ? 2 * px : geo.w - 1, xb = 2 * px + 1 < geo.w ? 2 * px + 1 : geo.w - 1;
        const int32_t ya = 2 * cy, yb = 2 * cy + 1 < geo.h ? 2 * cy + 1 : geo.h - 1;
        v = (ycc_sample(frame, geo.w, xa, ya, kc) + ycc_sample(frame, geo.w, xb, ya, kc) + ycc_sample(frame, geo.w, xa, yb, kc) +
             ycc_sample(frame, geo.w, xb, yb, kc) + 1 + (px & 1)) >> 2;
      }
      d[c] = v - 128;
    }
    fdct_1d<true>(d, ws[r]);
  }
  const int32_t* qc = q[comp != 0];
  uint32_t packed[32];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int32_t d[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = ws[r][c];
    fdct_1d<false>(d, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) {                      // jcdctmgr.c: round half away from zero
      const int32_t div = qc[r * 8 + c], v = o[r];
      const int32_t a = ((v < 0 ? -v : v) + (div >> 1)) / div;
      ws[r][c] = v < 0 ? -a : a;
    }
  }
  pack_zigzag(ws, dummy, packed, std::make_integer_sequence<int, 32>{});
  uint4* dst = reinterpret_cast<uint4*>(coef + ((size_t)img * geo.n_blocks + b) * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) dst[i] = make_uint4(packed[4 * i], packed[4 * i + 1], packed[4 * i + 2], packed[4 * i + 3]);
}

// MSB-first bit writer into 32-bit words; see the head of the file
struct BitSink {
  uint32_t* words;       // the image's raw words
  int64_t cap, word;     // words of the region, next word to write
  uint64_t acc;
  int32_t n;             // bits held in acc (the low n), < 32 between two puts
  bool first;
  __device__ __forceinline__ void init(uint32_t* w, int64_t cap_words, int64_t bit) {
    words = w; cap = cap_words; word = bit >> 5; acc = 0; n = (int32_t)(bit & 31); first = true;
  }
  __device__ __forceinline__ void put(uint32_t v, int len) {      // len <= 31, v < 2^len
    acc = (acc << len) | v;
    n += len;
    if (n >= 32) {
      n -= 32;
      const uint32_t out = (uint32_t)(acc >> n);
      if (word < cap) {
        if (first) atomicOr(words + word, out); else words[word] = out;
      }
      first = false;
      ++word;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0 && word < cap) atomicOr(words + word, (uint32_t)(acc << (32 - n)));
  }
};

__device__ __forceinline__ int32_t bit_size(int32_t v) { return 32 - __clz(v < 0 ? -v : v); }

// The code words of block b; returns their bits.  huff: [DC lum, AC lum, DC chroma, AC chroma][256] in LDS
template <bool EMIT>
__device__ __forceinline__ int32_t code_block(const EncGeo& geo, const int16_t* __restrict__ coef_img, int32_t b, const uint32_t* huff,
                                              BitSink& sink) {
  const int32_t mcu = b / geo.bpm, blk = b - mcu * geo.bpm;
  const McuComp mc = mcu_comp_of_block(blk, geo.ycount);
  const bool luma = mc.comp == 0;
  const uint32_t* dc = huff + (luma ? 0 : 512);
  const uint32_t* ac = dc + 256;
  const uint4* src = reinterpret_cast<const uint4*>(coef_img + (size_t)b * 64);
  uint32_t u[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 v = src[i];
    u[4 * i] = v.x; u[4 * i + 1] = v.y; u[4 * i + 2] = v.z; u[4 * i + 3] = v.w;
  }
  int32_t pred = 0;                                    // the DC value of the component's block before this one in the scan
  if (blk > mc.first) pred = coef_img[(size_t)(b - 1) * 64];
  else if (mcu > 0) pred = coef_img[(size_t)(b - geo.bpm + mc.count - 1) * 64];   // the component's last block of the MCU before
  int32_t bits = 0;
  {
    const int32_t diff = (int32_t)(int16_t)(u[0] & 0xffffu) - pred;
    const int32_t s = bit_size(diff);
    const uint32_t e = dc[s & 255];
    const int len = (int)((e >> 16) & 31u);
    bits += len + s;
    if (EMIT) {
      sink.put(e & ((1u << len) - 1u), len);
      if (s) sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
    }
  }
  int32_t run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int32_t v = (int32_t)(int16_t)((k & 1) ? u[k >> 1] >> 16 : u[k >> 1] & 0xffffu);
    if (v == 0) {
      ++run;
    } else {
      while (run > 15) {                               // ZRL
        const uint32_t e = ac[0xF0];
        const int len = (int)((e >> 16) & 31u);
        bits += len;
        if (EMIT) sink.put(e & ((1u << len) - 1u), len);
        run -= 16;
      }
      const int32_t s = bit_size(v);
      const uint32_t e = ac[((run << 4) | s) & 255];
      const int len = (int)((e >> 16) & 31u);
      bits += len + s;
      if (EMIT) {
        sink.put(e & ((1u << len) - 1u), len);
        sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u), s);
      }
      run = 0;
    }
  }
  if (run > 0) {                                       // EOB
    const uint32_t e = ac[0];
    const int len = (int)((e >> 16) & 31u);
    bits += len;
    if (EMIT) sink.put(e & ((1u << len) - 1u), len);
  }
  return bits;
}

__device__ __forceinline__ void load_huff(const uint32_t* __restrict__ huff, uint32_t* lds) {
  for (int i = threadIdx.x; i < 1024; i += kThreads) lds[i] = huff[i];
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_bits_kernel(EncGeo geo, const int16_t* __restrict__ coef,
                                                                 const uint32_t* __restrict__ huff, int32_t* __restrict__ bits) {
  __shared__ uint32_t tab[1024];
  load_huff(huff, tab);
  const int img = blockIdx.y;
  const int32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= geo.n_blocks) return;
  BitSink none;
  bits[(size_t)img * geo.n_blocks + b] = code_block<false>(geo, coef + (size_t)img * geo.n_blocks * 64, b, tab, none);
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_scan_reduce_kernel(EncGeo geo, const int32_t* __restrict__ bits, int32_t* __restrict__ aggr) {
  __shared__ int32_t lds[kThreads];
  scan_tile_reduce<0, false>(bits + (size_t)blockIdx.y * geo.n_blocks, geo.n_blocks, aggr + (size_t)blockIdx.y * geo.scan_tiles, lds);
}

// one workgroup per image
__global__ __launch_bounds__(kThreads) void jpeg_enc_scan_aggr_kernel(EncGeo geo, int32_t* __restrict__ aggr, int32_t* __restrict__ total_bits) {
  __shared__ int32_t lds[kThreads];
  const int32_t total = scan_aggregates<0>(aggr + (size_t)blockIdx.x * geo.scan_tiles, geo.scan_tiles, lds);
  if (threadIdx.x == 0) total_bits[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_scan_apply_kernel(EncGeo geo, int32_t* bits, const int32_t* __restrict__ aggr) {
  __shared__ int32_t lds[kThreads];
  int32_t* p = bits + (size_t)blockIdx.y * geo.n_blocks;
  scan_tile_apply<0, false, true>(p, p, geo.n_blocks, aggr + (size_t)blockIdx.y * geo.scan_tiles, lds);
}

// raw bytes of image img: the bits and the fill; 0 when they do not fit the region (tables other than a Huffman code's)
__device__ __forceinline__ int64_t raw_bytes_of(const EncGeo& geo, const int32_t* __restrict__ total_bits, int img) {
  const int64_t t = total_bits[img];
  return t >= 0 && t <= (int64_t)geo.n_blocks * kBlockBits ? (t + 7) >> 3 : 0;
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_zero_kernel(EncGeo geo, const int32_t* __restrict__ total_bits, uint32_t* __restrict__ raw) {
  const int img = blockIdx.y;
  const int64_t need = ((raw_bytes_of(geo, total_bits, img) + 3) >> 2) + 1;            // words, one past the last for the emit's tail
  const int64_t w0 = (int64_t)blockIdx.x * kTileWords + (int64_t)threadIdx.x * 4;
  if (w0 < need && w0 + 4 <= geo.raw_words) *reinterpret_cast<uint4*>(raw + (size_t)img * geo.raw_words + w0) = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_emit_kernel(EncGeo geo, const int16_t* __restrict__ coef, const uint32_t* __restrict__ huff,
                                                                 const int32_t* __restrict__ offsets, const int32_t* __restrict__ total_bits,
                                                                 uint32_t* raw) {
  __shared__ uint32_t tab[1024];
  load_huff(huff, tab);
  const int img = blockIdx.y;
  const int32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= geo.n_blocks || raw_bytes_of(geo, total_bits, img) == 0) return;
  BitSink sink;
  sink.init(raw + (size_t)img * geo.raw_words, ((raw_bytes_of(geo, total_bits, img) + 3) >> 2) + 1, offsets[(size_t)img * geo.n_blocks + b]);
  code_block<true>(geo, coef + (size_t)img * geo.n_blocks * 64, b, tab, sink);
  if (b == geo.n_blocks - 1) {
    const int fill = (int)(-total_bits[img] & 7);
    if (fill) sink.put((1u << fill) - 1u, fill);
  }
  sink.finish();
}

__device__ __forceinline__ uint32_t raw_byte(const uint4& v, int i) {
  const uint32_t w = i < 4 ? v.x : (i < 8 ? v.y : (i < 12 ? v.z : v.w));
  return (w >> (24 - 8 * (i & 3))) & 255u;
}

// 0xFF bytes among the 16 raw bytes of this thread (the bytes past the end of the stream are not counted)
__device__ __forceinline__ int32_t ff_of(const uint4& v, int64_t byte0, int64_t n_raw) {
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) c += (byte0 + i < n_raw && raw_byte(v, i) == 255u) ? 1 : 0;
  return c;
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_count_kernel(EncGeo geo, const int32_t* __restrict__ total_bits,
                                                                  const uint32_t* __restrict__ raw, int32_t* __restrict__ ff_count) {
  __shared__ int32_t lds[kThreads];
  const int img = blockIdx.y;
  const int64_t n_raw = raw_bytes_of(geo, total_bits, img);
  if ((int64_t)blockIdx.x * kTileBytes >= n_raw) return;                                // the whole workgroup
  const int64_t byte0 = (int64_t)blockIdx.x * kTileBytes + (int64_t)threadIdx.x * 16;
  int32_t c = 0;
  if (byte0 < n_raw) c = ff_of(*reinterpret_cast<const uint4*>(raw + (size_t)img * geo.raw_words + (byte0 >> 2)), byte0, n_raw);
  const int32_t tot = block_inclusive_scan<0>(c, lds);
  if (threadIdx.x == kThreads - 1) ff_count[(size_t)img * geo.raw_tiles + blockIdx.x] = tot;
}

// one workgroup per image: tile_off[t] = 0xFF bytes before tile t, sizes[img] = bytes of the whole stream
__global__ __launch_bounds__(kThreads) void jpeg_enc_sizes_kernel(EncGeo geo, const int32_t* __restrict__ total_bits,
                                                                  const int32_t* __restrict__ ff_count, int64_t* __restrict__ tile_off,
                                                                  int64_t* __restrict__ sizes, int32_t* __restrict__ status) {
  __shared__ int32_t lds[kThreads];
  const int img = blockIdx.x;
  const int64_t n_raw = raw_bytes_of(geo, total_bits, img);
  const int64_t tiles = (n_raw + kTileBytes - 1) / kTileBytes;
  const int64_t ff = scan_tile_counts(ff_count + (size_t)img * geo.raw_tiles, tiles, tile_off + (size_t)img * geo.raw_tiles, lds);
  if (threadIdx.x == 0) {
    sizes[img] = geo.header_bytes + n_raw + ff + 2;
    status[img] = n_raw == 0 ? SCPOSE_JPEG_ENC_TABLES : 0;
  }
}

// one thread: the streams are packed in image order; n <= 65535 additions
__global__ void jpeg_enc_offsets_kernel(EncGeo geo, const int64_t* __restrict__ sizes, int64_t capacity, int64_t* __restrict__ offsets,
                                        int32_t* __restrict__ status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t at = 0;
  offsets[0] = 0;
  for (int i = 0; i < geo.n; ++i) {
    at += sizes[i];
    offsets[i + 1] = at;
    if (at > capacity) status[i] |= SCPOSE_JPEG_ENC_CAPACITY;
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_enc_write_kernel(EncGeo geo, const int32_t* __restrict__ total_bits,
                                                                  const uint32_t* __restrict__ raw, const int64_t* __restrict__ tile_off,
                                                                  const int64_t* __restrict__ offsets, const int32_t* __restrict__ status,
                                                                  const uint8_t* __restrict__ header, uint8_t* __restrict__ out) {
  __shared__ int32_t lds[kThreads];
  const int img = blockIdx.y;
  const int64_t n_raw = raw_bytes_of(geo, total_bits, img);
  if ((int64_t)blockIdx.x * kTileBytes >= n_raw || status[img] != 0) return;            // the whole workgroup
  uint8_t* dst = out + offsets[img];
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < geo.header_bytes; i += kThreads) dst[i] = header[i];
  const int64_t byte0 = (int64_t)blockIdx.x * kTileBytes + (int64_t)threadIdx.x * 16;
  uint4 v = make_uint4(0, 0, 0, 0);
  int32_t c = 0;
  if (byte0 < n_raw) {
    v = *reinterpret_cast<const uint4*>(raw + (size_t)img * geo.raw_words + (byte0 >> 2));
    c = ff_of(v, byte0, n_raw);
  }
  const int32_t inc = block_inclusive_scan<0>(c, lds);
  if (byte0 >= n_raw) return;
  uint8_t* p = dst + geo.header_bytes + byte0 + tile_off[(size_t)img * geo.raw_tiles + blockIdx.x] + (inc - c);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (byte0 + i < n_raw) {
      const uint32_t x = raw_byte(v, i);
      *p++ = (uint8_t)x;
      if (x == 255u) *p++ = 0;
    }
  }
  if (byte0 + 16 >= n_raw) { p[0] = 0xFF; p[1] = 0xD9; }                                // EOI behind the last raw byte
}

struct EncPlan {
  int16_t* coef;
  int32_t *bits, *aggr, *total_bits, *ff_count;
  int64_t *tile_off, *sizes;
  uint32_t* raw;
  size_t bytes;
};

EncPlan make_plan(const EncGeo& g, uint8_t* ws) {
  EncPlan p{};
  Carve c{ws};
  const size_t blocks = (size_t)g.n * g.n_blocks;
  p.coef = c.take<int16_t>(blocks * 64);
  p.bits = c.take<int32_t>(blocks);
  p.aggr = c.take<int32_t>((size_t)g.n * g.scan_tiles);
  p.total_bits = c.take<int32_t>((size_t)g.n);
  p.ff_count = c.take<int32_t>((size_t)g.n * g.raw_tiles);
  p.tile_off = c.take<int64_t>((size_t)g.n * g.raw_tiles);
  p.sizes = c.take<int64_t>((size_t)g.n);
  p.raw = c.take<uint32_t>((size_t)g.n * g.raw_words);
  p.bytes = c.bytes();
  return p;
}

// ---- overlay: the outline of ImageDraw.rectangle(width=2) and the discs of ImageDraw.ellipse over an 11 x 11 box
// the rows of the disc, bit c = column c
__constant__ uint16_t kDisc[11] = {248, 508, 1022, 2047, 2047, 2047, 2047, 2047, 1022, 508, 248};

// thread t of a frame: 4 rows x W (the rows y0, y0 + 1, y1 - 1, y1), then 4 columns x H
__global__ __launch_bounds__(kThreads) void overlay_rect_kernel(uint8_t* frames, int32_t h, int32_t w, const int32_t* __restrict__ bboxes) {
  const int img = blockIdx.y;
  const int32_t t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= 4 * (w + h)) return;
  const int32_t* bb = bboxes + 4 * (size_t)img;
  const int64_t x0 = bb[0], y0 = bb[1], x1 = x0 + bb[2], y1 = y0 + bb[3];
  int64_t x, y;
  if (t < 4 * w) {
    const int s = t / w;
    x = t - s * w;
    y = s == 0 ? y0 : (s == 1 ? y0 + 1 : (s == 2 ? y1 - 1 : y1));
  } else {
    const int32_t u = t - 4 * w;
    const int s = u / h;
    y = u - s * h;
    x = s == 0 ? x0 : (s == 1 ? x0 + 1 : (s == 2 ? x1 - 1 : x1));
  }
  if (x < x0 || x > x1 || y < y0 || y > y1 || x < 0 || x >= w || y < 0 || y >= h) return;
  uint8_t* p = frames + (((size_t)img * h + (size_t)y) * w + (size_t)x) * 3;
  p[0] = 0; p[1] = 255; p[2] = 0;
}

__global__ __launch_bounds__(kThreads) void overlay_disc_kernel(uint8_t* frames, int32_t h, int32_t w, const double* __restrict__ points, int32_t j) {
  const int img = blockIdx.y;
  const int32_t t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= j * 121) return;
  const int32_t pt = t / 121, m = t - pt * 121, r = m / 11, c = m - r * 11;
  if (!((kDisc[r] >> c) & 1)) return;
  const double px = points[((size_t)img * j + pt) * 2], py = points[((size_t)img * j + pt) * 2 + 1];
  if (!(fabs(px) <= 1.7e308) || !(fabs(py) <= 1.7e308)) return;                        // NaN and the infinities
  if (fabs(px) >= 1e9 || fabs(py) >= 1e9) return;                                       // far outside every frame
  const int64_t x = (int64_t)(int32_t)px - 5 + c, y = (int64_t)(int32_t)py - 5 + r;     // the conversion truncates toward zero
  if (x < 0 || x >= w || y < 0 || y >= h) return;
  uint8_t* p = frames + (((size_t)img * h + (size_t)y) * w + (size_t)x) * 3;
  p[0] = 0; p[1] = 0; p[2] = 255;
}

}  // namespace

size_t jpeg_encode_workspace_bytes(int n, int h, int w, int mode) { return make_plan(make_geo(n, h, w, mode, 0), nullptr).bytes; }

int64_t jpeg_encode_capacity_bytes(int n, int h, int w, int mode, int header_bytes) {
  return (int64_t)n * (header_bytes + 2 * (int64_t)(kBlockBits / 8) * jpeg_blocks(h, w, mode) + 2);
}

int32_t jpeg_encode_launch(const uint8_t* frames, int n, int h, int w, int mode, int quality, const uint32_t* huff, const uint8_t* header,
                           int header_bytes, uint8_t* out, int64_t capacity, int64_t* offsets, int32_t* status, uint8_t* ws,
                           hipStream_t stream) {
  const EncGeo g = make_geo(n, h, w, mode, header_bytes);
  const EncPlan p = make_plan(g, ws);
  const dim3 tg(kThreads), blocks_grid((unsigned)((g.n_blocks + kThreads - 1) / kThreads), (unsigned)n);
  const dim3 scan_grid((unsigned)g.scan_tiles, (unsigned)n), raw_grid((unsigned)g.raw_tiles, (unsigned)n);
  hipLaunchKernelGGL(jpeg_enc_dct_kernel, blocks_grid, tg, 0, stream, frames, g, quality, p.coef);
  hipLaunchKernelGGL(jpeg_enc_bits_kernel, blocks_grid, tg, 0, stream, g, p.coef, huff, p.bits);
  hipLaunchKernelGGL(jpeg_enc_scan_reduce_kernel, scan_grid, tg, 0, stream, g, p.bits, p.aggr);
  hipLaunchKernelGGL(jpeg_enc_scan_aggr_kernel, dim3((unsigned)n), tg, 0, stream, g, p.aggr, p.total_bits);
  hipLaunchKernelGGL(jpeg_enc_scan_apply_kernel, scan_grid, tg, 0, stream, g, p.bits, p.aggr);
  hipLaunchKernelGGL(jpeg_enc_zero_kernel, raw_grid, tg, 0, stream, g, p.total_bits, p.raw);
  hipLaunchKernelGGL(jpeg_enc_emit_kernel, blocks_grid, tg, 0, stream, g, p.coef, huff, p.bits, p.total_bits, p.raw);
  hipLaunchKernelGGL(jpeg_enc_count_kernel, raw_grid, tg, 0, stream, g, p.total_bits, p.raw, p.ff_count);
  hipLaunchKernelGGL(jpeg_enc_sizes_kernel, dim3((unsigned)n), tg, 0, stream, g, p.total_bits, p.ff_count, p.tile_off, p.sizes, status);
  hipLaunchKernelGGL(jpeg_enc_offsets_kernel, dim3(1), dim3(64), 0, stream, g, p.sizes, capacity, offsets, status);
  hipLaunchKernelGGL(jpeg_enc_write_kernel, raw_grid, tg, 0, stream, g, p.total_bits, p.raw, p.tile_off, offsets, status, header, out);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t overlay_draw_launch(uint8_t* frames, int n, int h, int w, const int32_t* bboxes, const double* points, int j, hipStream_t stream) {
  hipLaunchKernelGGL(overlay_rect_kernel, dim3((unsigned)((4 * (w + h) + kThreads - 1) / kThreads), (unsigned)n), dim3(kThreads), 0, stream,
                     frames, h, w, bboxes);
  if (j > 0)
    hipLaunchKernelGGL(overlay_disc_kernel, dim3((unsigned)((j * 121 + kThreads - 1) / kThreads), (unsigned)n), dim3(kThreads), 0, stream,
                       frames, h, w, points, j);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
