// The polarity packets of an AEDAT-3.1 recording -> (t, x, y, p) on the device: the reader of the files
// cAER and DV before 1.0 write for DAVIS240, DAVIS346 and DVS128 cameras, between the AEDAT-2.0 reader (events_aedat2_read.hip)
// and the AEDAT-4.0 one (events_aedat4_read.hip).  tests/events_aedat3_restated.py says the same in Python.  The host
// (event_read.parse_aedat3) reads the text header and walks the packet headers; it hands over the whole file and one descriptor
// per POLARITY packet of the chosen source, (payload offset, eventNumber, eventTSOverflow) as three int64.
//
// The format (all integers little-endian), restated from its published description:
//   file     text lines that each start with '#' and end with "\r\n": "#!AER-DAT3.1", "#Format: RAW", one or more
//            "#Source <id>: <name>", optionally "#Start-Time: ..." and other '#' lines, last "#!END-HEADER".  Then packets up to the
//            end of the file.
//   packet   a 28-byte header, then eventCapacity * eventSize payload bytes.  Header: int16 eventType at 0 (0 special, 1 polarity,
//            2 frame, 3 IMU6, 4 IMU9, ...), int16 eventSource at 2, int32 eventSize at 4, int32 eventTSOffset at 8, int32
//            eventTSOverflow at 12, int32 eventCapacity at 16, int32 eventNumber at 20, int32 eventValid at 24.  The first
//            eventNumber events of the payload are the packet's events; what follows them up to the capacity is never read.
//   polarity eventType 1, eventSize 8, eventTSOffset 4: uint32 data at 0 (bit 0 valid, bit 1 polarity, bits 2..16 y, bits 17..31
//            x), int32 ts at 4 in microseconds; t = (int64(eventTSOverflow) << 31) | ts.  The origin is the upper-left pixel, as in
//            4.0: nothing is flipped.  Events whose valid bit is clear are dropped.  A negative ts, on a valid or an invalid event,
//            is corrupt.
//
// Three steps, one small read-back after the second (ops.unpack_events_aedat3):
//   aedat3_count_kernel    one workgroup per packet: 8-byte event loads, the valid bits counted per wavefront by ballot and
//                          population count and summed per workgroup -> count, the t of the packet's first and last valid event,
//                          status (a negative ts, a count that differs from the header's eventValid, which sits 4 bytes before
//                          the payload).
//   aedat3_counts_kernel   one workgroup, packet_counts of events_packets.h: event offsets, n_events, status, the first time stamp,
//                          the previous packet that holds a valid event.
//   aedat3_unpack_kernel   one workgroup per packet, 256 events at a time: a lane's row is the packet's offset, plus the valid
//                          events of the earlier 64-event groups, plus the population count of the ballot below the lane.
// The counts step, the gate and the tally of the unpack step, the time before a packet and the workspace plan are the ones the
// AEDAT-4.0 reader uses too: events_packets.h states them once.
// The kernels DETECT a damaged packet and never interpret one: every read is checked against eventNumber * 8 bytes, every store
// against the rows the count step gave the packet.  Integer work on fixed positions: two runs are bitwise equal.
#include "events_packets.h"

namespace scpose {

namespace {

constexpr int kWaves = kThreads / kWave;
constexpr int kMaxCount = (1 << 23) - 1;             // events of one packet: scan_tile_counts sums 256 counts in an int32
static_assert(256ll * kMaxCount <= INT_MAX, "scan_tile_counts sums 256 counts in an int32");

// event j of a payload; the payload starts wherever the header's text and the packets before it end, so no alignment is assumed
__device__ __forceinline__ uint2 ld_event(const uint8_t* ev, int32_t j) { return ld_as<uint2>(ev + 8 * (int64_t)j); }

__device__ __forceinline__ int64_t event_t(int64_t overflow, uint32_t ts) { return (overflow << 31) | (int64_t)ts; }

// one workgroup per packet -> count[pk], first_t[pk], last_t[pk] (of the valid events; 0 without one), status[pk]
__global__ __launch_bounds__(kThreads) void aedat3_count_kernel(const uint8_t* __restrict__ file, const int64_t* __restrict__ packets,
                                                                int32_t* count, int64_t* first_t, int64_t* last_t, int32_t* status) {
  __shared__ int32_t s_count, s_first, s_last, s_status;
  const int pk = blockIdx.x;
  const int64_t at = packets[3 * pk], num64 = packets[3 * pk + 1], overflow = packets[3 * pk + 2];
  if (at < 4 || num64 < 0 || num64 > kMaxCount || overflow < 0 || overflow > INT_MAX) {   // wave-uniform: nothing of it is read
    if (threadIdx.x == 0) {
      count[pk] = 0;
      first_t[pk] = last_t[pk] = 0;
      status[pk] = SCPOSE_AEDAT3_CORRUPT;
    }
    return;
  }
  const int32_t num = (int32_t)num64;
  const uint8_t* ev = file + at;
  if (threadIdx.x == 0) {
    s_count = 0;
    s_first = INT_MAX;
    s_last = -1;
    s_status = 0;
  }
  __syncthreads();
  int32_t wave_count = 0, first_j = INT_MAX, last_j = -1;
  uint32_t first_ts = 0, last_ts = 0;
  int st = 0;
  for (int32_t j0 = 0; j0 < num; j0 += kThreads) {   // j0 is uniform: every lane of a wavefront reaches the ballot
    const int32_t j = j0 + threadIdx.x;
    bool valid = false;
    if (j < num) {
      const uint2 v = ld_event(ev, j);
      valid = (v.x & 1u) != 0;
      if ((int32_t)v.y < 0) st = SCPOSE_AEDAT3_CORRUPT;
      if (valid) {
        if (first_j == INT_MAX) {
          first_j = j;
          first_ts = v.y;
        }
        last_j = j;
        last_ts = v.y;
      }
    }
    wave_count += __popcll(__ballot(valid));
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && wave_count) atomicAdd(&s_count, wave_count);
  if (first_j != INT_MAX) atomicMin(&s_first, first_j);
  if (last_j >= 0) atomicMax(&s_last, last_j);
  if (st) atomicOr(&s_status, st);
  __syncthreads();
  if (first_j != INT_MAX && first_j == s_first) first_t[pk] = event_t(overflow, first_ts);
  if (last_j >= 0 && last_j == s_last) last_t[pk] = event_t(overflow, last_ts);
  if (threadIdx.x == 0) {
    const int32_t stated = ld_as<int32_t>(ev - 4);   // the header's eventValid
    const int32_t s = s_status | (stated != s_count ? SCPOSE_AEDAT3_VALID_MISMATCH : 0);
    count[pk] = s ? 0 : s_count;
    status[pk] = s;
    if (s_first == INT_MAX) first_t[pk] = last_t[pk] = 0;
  }
}

// one workgroup: packet_counts of events_packets.h; t0 is 0 when the status is set
__global__ __launch_bounds__(kThreads) void aedat3_counts_kernel(const int32_t* count, const int32_t* status, const int64_t* first_t,
                                                                 int64_t n, int64_t* ev_off, int32_t* prev, int32_t* scratch,
                                                                 int64_t* count_status) {
  __shared__ int32_t sc[kThreads];
  packet_counts(count, status, first_t, n, ev_off, prev, scratch, count_status, false, sc);
}

// one workgroup per packet; nothing is written unless the status word is 0 and the columns hold n_events rows
__global__ __launch_bounds__(kThreads) void aedat3_unpack_kernel(const uint8_t* __restrict__ file, const int64_t* __restrict__ packets,
                                                                 const int32_t* __restrict__ count, const int64_t* __restrict__ ev_off,
                                                                 const int64_t* __restrict__ last_t, const int32_t* __restrict__ prev,
                                                                 int32_t h, int32_t w, int rebase,
                                                                 int64_t* __restrict__ t_out, int32_t* __restrict__ x_out,
                                                                 int32_t* __restrict__ y_out, int8_t* __restrict__ p_out,
                                                                 int64_t capacity, int64_t* count_status) {
  __shared__ int32_t s_cnt[2][kWaves];
  __shared__ int64_t s_last[2][kWaves];
  __shared__ int32_t s_red[2];
  if (!unpack_gate(count_status, capacity, SCPOSE_AEDAT3_RANGE, SCPOSE_AEDAT3_CAPACITY)) return;
  const int pk = blockIdx.x;
  const int32_t rows = count[pk];                    // the status is 0: eventNumber is within 0 .. kMaxCount
  if (rows == 0) return;
  const int32_t num = (int32_t)packets[3 * pk + 1];
  const int64_t overflow = packets[3 * pk + 2];
  const uint8_t* ev = file + packets[3 * pk];
  const int64_t row0 = ev_off[pk], sub = rebase ? count_status[2] : 0;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const unsigned long long below_me = (1ull << lane) - 1;
  const TimeBefore tb = time_before_packet(prev, last_t, pk);
  bool have_before = tb.have;                        // uniform, as `before` and `run` are
  int64_t before = tb.t;
  int32_t run = 0;                                   // valid events of the chunks done
  int32_t nback = 0, nout = 0;
  for (int32_t j0 = 0, buf = 0; j0 < num; j0 += kThreads, buf ^= 1) {
    const int32_t j = j0 + threadIdx.x;
    uint2 v = make_uint2(0u, 0u);
    if (j < num) v = ld_event(ev, j);
    const bool valid = j < num && (v.x & 1u) != 0;
    const int64_t t = event_t(overflow, v.y);
    const unsigned long long ballot = __ballot(valid);
    const unsigned long long lower = ballot & below_me;
    // the valid lane before this one and the wavefront's last valid lane: every lane takes part in both exchanges
    const int64_t t_lower = __shfl(t, lower ? 63 - __clzll(lower) : lane, kWave);
    const int64_t t_top = __shfl(t, ballot ? 63 - __clzll(ballot) : lane, kWave);
    if (lane == 0) {
      s_cnt[buf][wave] = __popcll(ballot);
      s_last[buf][wave] = t_top;
    }
    __syncthreads();                                 // one barrier per chunk: the next chunk writes the other half
    int32_t wave_row = run;
    bool have = have_before;
    int64_t t_before = before;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int32_t c = s_cnt[buf][k];
      const int64_t tl = s_last[buf][k];
      if (k < wave) {
        wave_row += c;
        if (c) { have = true; t_before = tl; }
      }
      run += c;
      if (c) { have_before = true; before = tl; }
    }
    if (valid) {
      if (lower) { have = true; t_before = t_lower; }
      const int32_t r = wave_row + __popcll(lower);
      const int32_t x = (int32_t)(v.x >> 17), y = (int32_t)((v.x >> 2) & 0x7FFFu);
      nback += have && t < t_before;
      nout += x >= w || y >= h;
      if (r < rows) {                                // the rows the count step gave this packet
        t_out[row0 + r] = t - sub;
        x_out[row0 + r] = x;
        y_out[row0 + r] = y;
        p_out[row0 + r] = (int8_t)((v.x >> 1) & 1u);
      }
    }
  }
  unpack_tally(nback, nout, s_red, count_status, SCPOSE_AEDAT3_RANGE);
}

struct Plan : PacketPlan {
  size_t bytes;
};

Plan plan(int64_t n, uint8_t* wsp) {
  Carve c{wsp};
  Plan p{packet_plan(c, packet_plan_count(n), true), 0};
  p.bytes = c.bytes();
  return p;
}

}  // namespace

size_t events_aedat3_workspace_bytes(int64_t n_packets) { return plan(n_packets, nullptr).bytes; }

int32_t events_aedat3_count_launch(const uint8_t* file, const int64_t* packets, int64_t n, int64_t* count_status, uint8_t* wsp,
                                   hipStream_t stream) {
  const Plan pl = plan(n, wsp);
  if (n > 0)
    hipLaunchKernelGGL(aedat3_count_kernel, dim3((unsigned)n), dim3(kThreads), 0, stream, file, packets, pl.count, pl.first_t, pl.last_t,
                       pl.status);
  hipLaunchKernelGGL(aedat3_counts_kernel, dim3(1), dim3(kThreads), 0, stream, pl.count, pl.status, pl.first_t, n, pl.ev_off, pl.prev,
                     pl.scratch, count_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t events_aedat3_unpack_launch(const uint8_t* file, const int64_t* packets, int64_t n, int h, int w, int rebase, int64_t* t,
                                    int32_t* x, int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status, uint8_t* wsp,
                                    hipStream_t stream) {
  const Plan pl = plan(n, wsp);
  if (n > 0)
    hipLaunchKernelGGL(aedat3_unpack_kernel, dim3((unsigned)n), dim3(kThreads), 0, stream, file, packets, pl.count, pl.ev_off, pl.last_t,
                       pl.prev, h, w, rebase, t, x, y, p, capacity, count_status);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
