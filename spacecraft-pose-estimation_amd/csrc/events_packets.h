// What the two packet readers share (events_aedat3_read.hip, events_aedat4_read.hip; DESIGN.md section 5a, "Packet readers"):
// the host hands over one descriptor per packet, a per-packet count step fills count / status / first_t / last_t, ONE workgroup
// scans them (packet_counts), a read-back sizes the columns, and one workgroup per packet unpacks its events behind
// unpack_gate and closes with unpack_tally.  How one packet is decoded is the format's own and stays in its file.
//
// Device functions and one plan struct only, under the contract of scan_device.h: every body below that takes `lds` or `s_red`
// is called by ALL threads of a workgroup of exactly kThreads = kScanThreads threads, `lds` pointing at kScanThreads int32
// words of LDS that the caller does not use across the call.  The __global__ wrappers and their launches stay in the client files.
#pragma once
#include "common.h"
#include "scan_device.h"

namespace scpose {

constexpr int kWave = 64;
constexpr int kThreads = kScanThreads;

// The per-packet arrays both readers carve from one workspace, max(n, 1) elements each (never an empty workspace).  Carve aligns
// every region to 256 bytes, so a reader's total does not depend on the order in which it carves its own arrays around these.
struct PacketPlan {
  int32_t *count, *status, *prev, *scratch;
  int64_t *ev_off, *first_t, *last_t;
};
inline size_t packet_plan_count(int64_t n) { return (size_t)(n > 0 ? n : 1); }
// own_scratch false: the caller points `scratch` at an int32 array of its own that is free during packet_counts
inline PacketPlan packet_plan(Carve& c, size_t cnt, bool own_scratch) {
  PacketPlan p{};
  p.count = c.take<int32_t>(cnt);
  p.status = c.take<int32_t>(cnt);
  p.prev = c.take<int32_t>(cnt);
  if (own_scratch) p.scratch = c.take<int32_t>(cnt);
  p.ev_off = c.take<int64_t>(cnt);
  p.first_t = c.take<int64_t>(cnt);
  p.last_t = c.take<int64_t>(cnt);
  return p;
}

// ONE workgroup: ev_off <- the exclusive scan of count, count_status <- [n_events, status, t0, 0, 0, 0] with n_events = 0 unless
// the OR of the packets' status words is 0; prev[i] <- minus the index of the last packet before i that holds an event (INT_MAX:
// none), an exclusive min-scan; `scratch` serves the min-scan whose total is the first packet that holds one, whose first_t is t0.
// t0_despite_status: what t0 is when the status is set -- that first_t all the same (AEDAT-4.0), or 0 (AEDAT-3.1).
__device__ __forceinline__ void packet_counts(const int32_t* count, const int32_t* status, const int64_t* first_t, int64_t n,
                                              int64_t* ev_off, int32_t* prev, int32_t* scratch, int64_t* count_status,
                                              bool t0_despite_status, int32_t* lds) {
  int st = 0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    st |= status[i];
    prev[i] = count[i] ? -(int32_t)i : INT_MAX;
    scratch[i] = count[i] ? (int32_t)i : INT_MAX;
  }
  __syncthreads();
  const int64_t total = scan_tile_counts(count, n, ev_off, lds);
  scan_aggregates<1>(prev, n, lds);
  const int32_t first = scan_aggregates<1>(scratch, n, lds);
  st = block_or(st, lds);
  if (threadIdx.x == 0) {
    count_status[0] = st ? 0 : total;
    count_status[1] = st;
    count_status[2] = ((t0_despite_status || !st) && first != INT_MAX) ? first_t[first] : 0;
    count_status[3] = 0;
    count_status[4] = 0;
    count_status[5] = 0;
  }
}

// Whether an unpack workgroup may proceed, the same answer for all its threads: not when a status bit other than the format's
// RANGE bit is set (RANGE is what the tallies of other workgroups of the same launch set), and not when the columns are shorter
// than the events counted, which sets the format's CAPACITY bit.
__device__ __forceinline__ bool unpack_gate(int64_t* count_status, int64_t capacity, int range_bit, int capacity_bit) {
  if ((count_status[1] & ~(int64_t)range_bit) != 0) return false;
  if (count_status[0] > capacity) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      atomicOr(reinterpret_cast<unsigned long long*>(count_status) + 1, (unsigned long long)capacity_bit);
    return false;
  }
  return true;
}

// The time of the last event before packet pk's first, that of the previous packet that holds any; have false: there is none
struct TimeBefore {
  bool have;
  int64_t t;
};
__device__ __forceinline__ TimeBefore time_before_packet(const int32_t* __restrict__ prev, const int64_t* __restrict__ last_t, int pk) {
  const int32_t q = prev[pk];
  return {q != INT_MAX, q != INT_MAX ? last_t[-(int64_t)q] : 0};
}

// The end of an unpack workgroup: the threads' backward steps and out-of-sensor events, summed in the LDS pair s_red, join
// count_status[3] and [4]; an out-of-sensor event sets the format's RANGE bit.  The first barrier below orders the zeroing of
// s_red before the threads' atomics, whatever the caller's loop did (one chunk, one event, none for this thread): the caller
// neither zeroes s_red nor owes a barrier.
__device__ __forceinline__ void unpack_tally(int32_t nback, int32_t nout, int32_t* s_red, int64_t* count_status, int range_bit) {
  if (threadIdx.x == 0) s_red[0] = s_red[1] = 0;
  __syncthreads();
  if (nback) atomicAdd(&s_red[0], nback);
  if (nout) atomicAdd(&s_red[1], nout);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* cs = reinterpret_cast<unsigned long long*>(count_status);
    if (s_red[0]) atomicAdd(cs + 3, (unsigned long long)s_red[0]);
    if (s_red[1]) {
      atomicAdd(cs + 4, (unsigned long long)s_red[1]);
      atomicOr(cs + 1, (unsigned long long)range_bit);
    }
  }
}

}  // namespace scpose
