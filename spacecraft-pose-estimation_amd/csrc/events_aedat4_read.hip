// The event packets of an AEDAT-4.0 recording -> (t, x, y, p) on the device: the reader of the files a
// DVXplorer / DV writes, next to the AEDAT-2.0 reader (events_aedat2_read.hip).  tests/events_aedat4_restated.py says the same in
// Python.  The host (event_read.parse_aedat4) reads the header and walks the packet headers; it hands over the whole file and one
// descriptor per EVENT packet, (payload offset, payload size) as two int64.
//
// The format (all integers little-endian):
//   file     the 14 bytes "#!AER-DAT4.0\r\n"; a uint32 length L and L bytes of IOHeader flatbuffer (identifier "IOHE" at bytes 4..8;
//            field 0 compression int32: 0 NONE, 1 LZ4, 2 LZ4_HIGH, 3 ZSTD, 4 ZSTD_HIGH; field 1 dataTablePosition int64, default -1;
//            field 2 infoNode, the XML that names the streams); then packets up to dataTablePosition (or the end of the file):
//            int32 streamID, int32 size, `size` payload bytes.  What lies at dataTablePosition (an FTAB table) is not read.
//   payload  the packet's flatbuffer, raw under NONE, else ONE complete LZ4 frame.  An event packet has the identifier "EVTS", at
//            bytes 8..12 when the buffer is size-prefixed (uint32 size, uint32 root offset, "EVTS": what writers emit) or at bytes
//            4..8 when it is not.  Root table field 0 is a vector of 16-byte structs: int64 t (microseconds) at 0, int16 x at 8,
//            int16 y at 10, uint8 on at 12, 3 pad bytes.  Walked the flatbuffer way: int32 soffset back to the vtable, uint16
//            field slot, uint32 uoffset to the vector, uint32 count, every step checked against the payload.
//   LZ4      frame: magic 04 22 4D 18, FLG (bits 7..6 version = 01, bit 5 block independence, 4 block checksum, 3 content size
//            present, 2 content checksum, 0 dictionary id), BD (bits 6..4 block maximum: 4 -> 64 KiB, 5 -> 256 KiB, 6 -> 1 MiB,
//            7 -> 4 MiB), an 8-byte content size if flagged, HC = (xxh32(FLG .. before HC) >> 8) & 0xFF.  Blocks: a uint32 size
//            word (bit 31: stored; 0: the end mark), the data, a uint32 xxh32 of the data as stored if block checksums are on.
//            After the end mark a uint32 xxh32 of the whole output if flagged.  Linked blocks (bit 5 clear) may match into the
//            output of earlier blocks; the window is 64 KiB (offsets are 16 bits).
//            block: sequences of token (high nibble literal length, low nibble match length - 4; a nibble of 15 is extended by
//            bytes, summed until a byte below 255), the literals, a 2-byte offset (0 is invalid), the match length extension.  The
//            last sequence of a block ends after its literals.  A match may overlap its own output (offset < length).
//
// Six steps, two small read-backs between them (ops.unpack_events_aedat4):
//   aedat4_lz4_kernel<false>  MEASURE, one wavefront per packet: walks the frame and its sequences without copying -> the decoded
//                             size and a status per packet.
//   aedat4_sizes_kernel       one workgroup, scan_device.h: staging offsets (sizes rounded up to 16), total and status.
//   aedat4_lz4_kernel<true>   DECODE, one wavefront per packet: the same wave-uniform walk; literals and matches are copied by all
//                             lanes, an overlapping match reads source byte start + (i mod offset).  The output goes straight to
//                             the packet's piece of the staging buffer in global memory and a match reads it back from there:
//                             before a match's loads the wave waits for its own stores (own_stores_done of aedat4_payload.h).  Block and content
//                             checksums are verified when asked.  Under NONE none of these three run: the staging buffer is the file.
//   aedat4_count_kernel       one thread per packet: the flatbuffer walk down to the vector's count.
//   aedat4_counts_kernel      one workgroup, packet_counts of events_packets.h: event offsets, n_events, status, the first time stamp.
//   aedat4_unpack_kernel      one workgroup per packet: 16-byte struct loads, lane after lane, to the four columns in file order.
// The counts step, the gate and the tally of the unpack step, the time before a packet and the shared part of the workspace plan are
// the ones the AEDAT-3.1 reader uses too: events_packets.h states them once.
// The kernels DETECT a damaged stream and never interpret one: every read is checked against the payload, every match against the
// output produced so far, every store against the measured size.  Integer work on fixed positions: two runs are bitwise equal.
#include "aedat4_payload.h"
#include "events_packets.h"
#include "xxh_wave.h"

namespace scpose {

namespace {

constexpr int kInWin = 4096;                         // input window in LDS, bytes
constexpr int kMaxDecoded = kAedat4MaxDecoded;      // decoded bytes of one packet: 256 of them, each rounded up to 16, sum within int32
static_assert(256ll * ((kMaxDecoded + 15) & ~15) <= INT_MAX, "scan_tile_counts sums 256 padded sizes in an int32");
constexpr int kMaxCount = kAedat4MaxCount;          // events of one packet, for the same reason

// The input side: wave-uniform byte reads of the payload through an LDS window.  The CALLER checks a position against the payload;
// the window zero-fills what lies past it.
struct In {
  const uint8_t* src;
  long long len;
  uint8_t* win;                      // LDS, kInWin
  long long base;                    // payload position of win[0]; -kInWin before the first fill

  __device__ __forceinline__ void fill(long long pos) {
    base = pos;
    __syncthreads();
    for (int i = 4 * threadIdx.x; i < kInWin; i += 4 * kWave) {
      const long long b = base + i;
      uint32_t v = 0;
      if (b + 4 <= len) v = ld32(src + b);
      else
        for (int k = 0; k < 4; ++k)
          if (b + k < len) v |= (uint32_t)src[b + k] << (8 * k);
      *reinterpret_cast<uint32_t*>(win + i) = v;
    }
    __syncthreads();
  }
  __device__ __forceinline__ uint32_t byte(long long pos) {
    if (pos < base || pos >= base + kInWin) fill(pos);
    return win[pos - base];
  }
  __device__ __forceinline__ uint32_t u32(long long pos) {
    return byte(pos) | (byte(pos + 1) << 8) | (byte(pos + 2) << 16) | (byte(pos + 3) << 24);
  }
};

// a length nibble of 15 extended by bytes; -> false: the block ends inside the extension
__device__ __forceinline__ bool extend(In& in, long long& ip, long long iend, long long& len) {
  for (;;) {
    if (ip >= iend) return false;
    const uint32_t b = in.byte(ip++);
    len += b;
    if (b != 255) return true;
  }
}

struct Lz4Lds {
  uint8_t win[kInWin];
  uint32_t sw[256];
};

// One wavefront per packet.  STORE false: measure -> size[pk] (0 unless the status is 0), status[pk].  STORE true: decode into
// staging + off[pk], at most size[pk] bytes, and nothing at all unless that piece lies inside the staging_bytes of the buffer;
// status[pk] |= what it finds.
template <bool STORE>
__global__ __launch_bounds__(kWave) void aedat4_lz4_kernel(const uint8_t* __restrict__ file, const int64_t* __restrict__ packets,
                                                           int32_t* size, const int64_t* __restrict__ off, uint8_t* staging,
                                                           int64_t staging_bytes, int verify, int32_t* status) {
  __shared__ Lz4Lds s;
  const int pk = blockIdx.x;
  In in{file + packets[2 * pk], packets[2 * pk + 1], s.win, -(long long)kInWin};
  const long long len = in.len;
  int st = 0;
  long long cap = kMaxDecoded;
  uint8_t* dst = nullptr;
  if (STORE) {
    if (status[pk] != 0) return;                     // measured as damaged: nothing to decode
    cap = size[pk];
    if (off[pk] < 0 || off[pk] + cap > staging_bytes) {                    // the caller's buffer is not the one measure sized
      if (threadIdx.x == 0) status[pk] |= SCPOSE_AEDAT4_CORRUPT;
      return;
    }
    dst = staging + off[pk];
  }
  long long out = 0, pos = 0;
  unsigned long long content = 0;                    // the frame's content size, when FLG bit 3 says it is there
  int flg = 0;
  do {
    if (len < 7 || in.u32(0) != 0x184D2204u) { st = SCPOSE_AEDAT4_CORRUPT; break; }
    flg = (int)in.byte(4);
    const int bd = (int)in.byte(5);
    const int bmax_code = (bd >> 4) & 7;
    if ((flg >> 6) != 1 || (flg & 3) != 0 || (bd & 0x8F) != 0 || bmax_code < 4) { st = SCPOSE_AEDAT4_CORRUPT; break; }
    const long long bmax = 1ll << (8 + 2 * bmax_code);
    const bool linked = !(flg & 0x20), bsum = (flg & 0x10) != 0;
    const long long hc_at = 6 + ((flg & 8) ? 8 : 0);
    if (len < hc_at + 1) { st = SCPOSE_AEDAT4_CORRUPT; break; }
    if (flg & 8) content = (unsigned long long)in.u32(6) | ((unsigned long long)in.u32(10) << 32);
    if (((xxh32_wave(in.src + 4, hc_at - 4, s.sw) >> 8) & 0xFFu) != in.byte(hc_at)) { st = SCPOSE_AEDAT4_CORRUPT; break; }
    pos = hc_at + 1;
    for (;;) {                                       // the blocks
      if (pos + 4 > len) { st = SCPOSE_AEDAT4_CORRUPT; break; }
      const uint32_t word = in.u32(pos);
      pos += 4;
      if (word == 0) break;
      const long long bs = word & 0x7FFFFFFFu;
      if (bs > bmax || pos + bs + (bsum ? 4 : 0) > len) { st = SCPOSE_AEDAT4_CORRUPT; break; }
      if (STORE && bsum && verify && xxh32_wave(in.src + pos, bs, s.sw) != in.u32(pos + bs)) st |= SCPOSE_AEDAT4_CHECKSUM;
      const long long first = linked ? 0 : out;      // the earliest output a match of this block may read
      const long long limit = out + bmax < cap ? out + bmax : cap;
      if (word >> 31) {                              // stored
        if (out + bs > limit) { st |= SCPOSE_AEDAT4_CORRUPT; break; }
        if (STORE)
          for (long long i = threadIdx.x; i < bs; i += kWave) dst[out + i] = in.src[pos + i];
        out += bs;
      } else {
        long long ip = pos;
        const long long iend = pos + bs;
        for (;;) {                                   // the sequences
          if (ip >= iend) { st |= SCPOSE_AEDAT4_CORRUPT; break; }
          const uint32_t token = in.byte(ip++);
          long long lit = token >> 4;
          if (lit == 15 && !extend(in, ip, iend, lit)) { st |= SCPOSE_AEDAT4_CORRUPT; break; }
          if (ip + lit > iend || out + lit > limit) { st |= SCPOSE_AEDAT4_CORRUPT; break; }
          if (STORE)
            for (long long i = threadIdx.x; i < lit; i += kWave) dst[out + i] = in.src[ip + i];
          ip += lit;
          out += lit;
          if (ip == iend) break;                     // the last sequence ends after its literals
          if (ip + 2 > iend) { st |= SCPOSE_AEDAT4_CORRUPT; break; }
          const long long offset = in.byte(ip) | (in.byte(ip + 1) << 8);
          ip += 2;
          long long ml = token & 15;
          if (ml == 15 && !extend(in, ip, iend, ml)) { st |= SCPOSE_AEDAT4_CORRUPT; break; }
          ml += 4;
          if (offset == 0 || offset > out - first || out + ml > limit) { st |= SCPOSE_AEDAT4_CORRUPT; break; }
          if (STORE) {
            own_stores_done();
            const uint8_t* from = dst + (out - offset);
            const uint32_t period = (uint32_t)offset;
            for (uint32_t i = threadIdx.x; i < (uint32_t)ml; i += kWave) dst[out + i] = from[i < period ? i : i % period];
          }
          out += ml;
        }
        if (st & SCPOSE_AEDAT4_CORRUPT) break;
      }
      pos += bs + (bsum ? 4 : 0);
    }
    if (st & SCPOSE_AEDAT4_CORRUPT) break;
    if (flg & 4) {                                   // content checksum
      if (pos + 4 > len) { st |= SCPOSE_AEDAT4_CORRUPT; break; }
      if (STORE && verify) {
        own_stores_done();
        if (xxh32_wave(dst, out, s.sw) != in.u32(pos)) st |= SCPOSE_AEDAT4_CHECKSUM;
      }
    }
    if ((flg & 8) && content != (unsigned long long)out) st |= SCPOSE_AEDAT4_CORRUPT;
    if (STORE && out != cap) st |= SCPOSE_AEDAT4_CORRUPT;                  // decode and measure disagree
  } while (false);
  if (threadIdx.x == 0) {
    if (STORE) status[pk] |= st;
    else {
      status[pk] = st;
      size[pk] = st ? 0 : (int32_t)out;
    }
  }
}

// one workgroup: size[i] rounded up to 16 (in place), their exclusive scan -> off, total_status <- [staging bytes, status]
__global__ __launch_bounds__(kThreads) void aedat4_sizes_kernel(int32_t* size, int32_t* padded, const int32_t* status, int64_t n,
                                                                int64_t* off, int64_t* total_status) {
  __shared__ int32_t sc[kThreads];
  int st = 0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    padded[i] = (size[i] + 15) & ~15;
    st |= status[i];
  }
  __syncthreads();
  const int64_t total = scan_tile_counts(padded, n, off, sc);
  st = block_or(st, sc);
  if (threadIdx.x == 0) {
    total_status[0] = total;
    total_status[1] = st;
  }
}

// one thread per packet.  The payload of packet i: (packets[2 i], packets[2 i + 1]) of `src` when size is null (NONE: src is the
// file), else (off[i], size[i]) (src is the staging buffer).  -> count[i], data[i] (position of the first struct in src), first_t,
// last_t; status[i] |= FLATBUFFER.  A packet whose status is already set counts no events.
__global__ __launch_bounds__(kThreads) void aedat4_count_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ packets,
                                                                const int64_t* __restrict__ off, const int32_t* __restrict__ size,
                                                                int64_t n, int32_t* count, int64_t* data, int64_t* first_t,
                                                                int64_t* last_t, int32_t* status, int fresh_status) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int st0 = fresh_status ? 0 : status[i];
  int64_t at = size ? off[i] : packets[2 * i];
  int64_t len = size ? size[i] : packets[2 * i + 1];
  int32_t cnt = 0;
  int64_t where = 0;
  bool ok = st0 == 0;
  if (ok) {
    const uint8_t* b = src + at;
    ok = false;
    do {
      int64_t skip;
      if (len >= 12 && ld32(b + 8) == 0x53545645u) skip = 4;             // "EVTS", size-prefixed
      else if (len >= 8 && ld32(b + 4) == 0x53545645u) skip = 0;
      else break;
      b += skip;
      at += skip;
      len -= skip;
      const int64_t root = ld32(b);
      if (root < 4 || root + 4 > len) break;
      const int64_t vt = root - (int64_t)(int32_t)ld32(b + root);
      if (vt < 0 || vt + 4 > len) break;
      const int64_t vsize = ld16(b + vt);
      if (vsize < 4 || vt + vsize > len) break;
      const int64_t slot = vsize >= 6 ? ld16(b + vt + 4) : 0;
      if (slot == 0) { ok = true; break; }           // the field is absent: no events
      const int64_t fpos = root + slot;
      if (fpos + 4 > len) break;
      const int64_t vec = fpos + (int64_t)ld32(b + fpos);
      if (vec + 4 > len) break;
      const int64_t c = ld32(b + vec);
      if (c > kMaxCount || vec + 4 + 16 * c > len) break;
      cnt = (int32_t)c;
      where = at + vec + 4;
      ok = true;
    } while (false);
  }
  count[i] = cnt;
  data[i] = where;
  first_t[i] = cnt ? ld64(src + where) : 0;
  last_t[i] = cnt ? ld64(src + where + 16 * (int64_t)(cnt - 1)) : 0;
  status[i] = st0 | ((ok || st0) ? 0 : SCPOSE_AEDAT4_FLATBUFFER);
}

// one workgroup: packet_counts of events_packets.h; t0 is the first event's time whatever the status
__global__ __launch_bounds__(kThreads) void aedat4_counts_kernel(const int32_t* count, const int32_t* status, const int64_t* first_t,
                                                                 int64_t n, int64_t* ev_off, int32_t* prev, int32_t* scratch,
                                                                 int64_t* count_status) {
  __shared__ int32_t sc[kThreads];
  packet_counts(count, status, first_t, n, ev_off, prev, scratch, count_status, true, sc);
}

// one workgroup per packet; nothing is written unless the status word is 0 and the columns hold n_events rows
__global__ __launch_bounds__(kThreads) void aedat4_unpack_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ count,
                                                                 const int64_t* __restrict__ data, const int64_t* __restrict__ ev_off,
                                                                 const int64_t* __restrict__ last_t, const int32_t* __restrict__ prev,
                                                                 int32_t h, int32_t w, int rebase,
                                                                 int64_t* __restrict__ t_out, int32_t* __restrict__ x_out,
                                                                 int32_t* __restrict__ y_out, int8_t* __restrict__ p_out,
                                                                 int64_t capacity, int64_t* count_status) {
  __shared__ int32_t s_red[2];
  if (!unpack_gate(count_status, capacity, SCPOSE_AEDAT4_RANGE, SCPOSE_AEDAT4_CAPACITY)) return;
  const int pk = blockIdx.x;
  const int32_t cnt = count[pk];
  if (cnt == 0) return;
  const uint8_t* ev = src + data[pk];
  const int64_t row0 = ev_off[pk], sub = rebase ? count_status[2] : 0;
  int32_t nback = 0, nout = 0;
  for (int32_t j = threadIdx.x; j < cnt; j += kThreads) {
    const uint4 v = ld_as<uint4>(ev + 16 * (int64_t)j);
    const int64_t t = (int64_t)(((unsigned long long)v.y << 32) | v.x);
    TimeBefore tb{true, 0};                          // the event before this one: the struct before it, or another packet's last
    if (j > 0) tb.t = ld64(ev + 16 * (int64_t)(j - 1));
    else tb = time_before_packet(prev, last_t, pk);
    nback += tb.have && t < tb.t;
    const int32_t x = (int16_t)(v.z & 0xFFFFu), y = (int16_t)(v.z >> 16);
    nout += x < 0 || x >= w || y < 0 || y >= h;
    t_out[row0 + j] = t - sub;
    x_out[row0 + j] = x;
    y_out[row0 + j] = y;
    p_out[row0 + j] = (int8_t)((v.w & 0xFFu) != 0);
  }
  unpack_tally(nback, nout, s_red, count_status, SCPOSE_AEDAT4_RANGE);
}

// the shared arrays and the LZ4 side's; `scratch` is `padded`, which is free once the staging offsets are scanned
struct Plan : PacketPlan {
  int32_t *size, *padded;
  int64_t *off, *data;
  size_t bytes;
};

Plan plan(int64_t n, uint8_t* wsp) {
  const size_t cnt = packet_plan_count(n);
  Carve c{wsp};
  Plan p{packet_plan(c, cnt, false), nullptr, nullptr, nullptr, nullptr, 0};
  p.size = c.take<int32_t>(cnt);
  p.scratch = p.padded = c.take<int32_t>(cnt);
  p.off = c.take<int64_t>(cnt);
  p.data = c.take<int64_t>(cnt);
  p.bytes = c.bytes();
  return p;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

size_t events_aedat4_workspace_bytes(int64_t n_packets) { return plan(n_packets, nullptr).bytes; }

// what a measure / decode pair of another compression (events_aedat4_zstd.hip) shares with this one
Aedat4Slots events_aedat4_slots(int64_t n, uint8_t* wsp) {
  const Plan pl = plan(n, wsp);
  return {pl.size, pl.off, pl.status};
}

int32_t events_aedat4_sizes_launch(int64_t n, int64_t* total_status, uint8_t* wsp, hipStream_t stream) {
  const Plan pl = plan(n, wsp);
  hipLaunchKernelGGL(aedat4_sizes_kernel, dim3(1), dim3(kThreads), 0, stream, pl.size, pl.padded, pl.status, n, pl.off, total_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t events_aedat4_measure_launch(const uint8_t* file, const int64_t* packets, int64_t n, int64_t* total_status, uint8_t* wsp,
                                     hipStream_t stream) {
  const Plan pl = plan(n, wsp);
  if (n > 0)
    hipLaunchKernelGGL(aedat4_lz4_kernel<false>, dim3((unsigned)n), dim3(kWave), 0, stream, file, packets, pl.size, pl.off,
                       (uint8_t*)nullptr, (int64_t)0, 0, pl.status);
  return events_aedat4_sizes_launch(n, total_status, wsp, stream);
}

int32_t events_aedat4_decode_launch(const uint8_t* file, const int64_t* packets, int64_t n, uint8_t* staging, int64_t staging_bytes,
                                    int verify, uint8_t* wsp, hipStream_t stream) {
  const Plan pl = plan(n, wsp);
  if (n > 0)
    hipLaunchKernelGGL(aedat4_lz4_kernel<true>, dim3((unsigned)n), dim3(kWave), 0, stream, file, packets, pl.size, pl.off, staging,
                       staging_bytes, verify, pl.status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t events_aedat4_count_launch(const uint8_t* src, const int64_t* packets, int64_t n, int staged,
                                   int64_t* count_status, uint8_t* wsp, hipStream_t stream) {
  const Plan pl = plan(n, wsp);
  if (n > 0)
    hipLaunchKernelGGL(aedat4_count_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, stream, src, packets, pl.off,
                       staged ? pl.size : (const int32_t*)nullptr, n, pl.count, pl.data, pl.first_t, pl.last_t, pl.status, !staged);
  hipLaunchKernelGGL(aedat4_counts_kernel, dim3(1), dim3(kThreads), 0, stream, pl.count, pl.status, pl.first_t, n, pl.ev_off,
                     pl.prev, pl.scratch, count_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t events_aedat4_unpack_launch(const uint8_t* src, int64_t n, int h, int w, int rebase, int64_t* t, int32_t* x, int32_t* y,
                                    int8_t* p, int64_t capacity, int64_t* count_status, uint8_t* wsp, hipStream_t stream) {
  const Plan pl = plan(n, wsp);
  if (n > 0)
    hipLaunchKernelGGL(aedat4_unpack_kernel, dim3((unsigned)n), dim3(kThreads), 0, stream, src, pl.count, pl.data, pl.ev_off, pl.last_t,
                       pl.prev, h, w, rebase, t, x, y, p, capacity, count_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
