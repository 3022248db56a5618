// Parallel-prefix primitives and workgroup reductions of the event kernels (events_exposure / events_csv / events_write /
// dvs_emulator / the AEDAT readers and writers; events_packets.h builds the packet readers' shared steps on them): device
// functions only, the __global__ wrappers and their launches stay in the client files.
//
// Contract: every body below is called by ALL threads of a workgroup of exactly kScanThreads threads (it contains barriers),
// with `lds` pointing at kScanThreads int32 words of LDS that the caller does not use across the call.
// Everything is int32 / int64 arithmetic in an association order that is a function of the tile size alone: two runs are
// bitwise equal ("Scan primitives").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

namespace scpose {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 16;
constexpr int kScanTile = kScanThreads * kScanItems;   // 4096 elements per workgroup of the device-wide scan

// OP 0: sum, 1: min
template <int OP>
__device__ __forceinline__ int32_t sc_op(int32_t a, int32_t b) { return OP == 0 ? a + b : (a < b ? a : b); }
template <int OP>
__device__ __forceinline__ int32_t sc_id() { return OP == 0 ? 0 : INT_MAX; }

// ---- block scan: Hillis-Steele in LDS; thread kScanThreads - 1 gets the workgroup's total
template <int OP>
__device__ int32_t block_inclusive_scan(int32_t v, int32_t* lds) {
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const int32_t a = tid >= off ? lds[tid - off] : sc_id<OP>();
    __syncthreads();
    lds[tid] = sc_op<OP>(lds[tid], a);
    __syncthreads();
  }
  const int32_t r = lds[tid];
  __syncthreads();
  return r;
}

// ---- block OR: every thread gets the OR of the workgroup's v; lds[0] alone is used
__device__ __forceinline__ int block_or(int v, int32_t* lds) {
  __syncthreads();
  if (threadIdx.x == 0) lds[0] = 0;
  __syncthreads();
  if (v) atomicOr(&lds[0], v);
  __syncthreads();
  const int r = lds[0];
  __syncthreads();
  return r;
}

// ---- device-wide int32 scan of len elements in three passes over ceil(len / kScanTile) tiles; element j of the scanned
// sequence is in[REV ? len - 1 - j : j].  Workgroup b of the first and the third pass owns tile b.
// pass 1, one workgroup per tile: aggr[b] = op over tile b
template <int OP, bool REV>
__device__ __forceinline__ void scan_tile_reduce(const int32_t* __restrict__ in, int64_t len, int32_t* __restrict__ aggr,
                                                 int32_t* lds) {
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  int32_t acc = sc_id<OP>();
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t j = base + k * kScanThreads + threadIdx.x;
    if (j < len) acc = sc_op<OP>(acc, in[REV ? len - 1 - j : j]);
  }
  const int32_t tot = block_inclusive_scan<OP>(acc, lds);
  if (threadIdx.x == kScanThreads - 1) aggr[blockIdx.x] = tot;
}

// pass 2, ONE workgroup: aggr[b] <- op(aggr[0 .. b - 1]) (identity for b = 0), kScanThreads aggregates per step with a
// carry; returns op over all nb aggregates to every thread
template <int OP>
__device__ __forceinline__ int32_t scan_aggregates(int32_t* __restrict__ aggr, int64_t nb, int32_t* lds) {
  int32_t carry = sc_id<OP>();
  for (int64_t b0 = 0; b0 < nb; b0 += kScanThreads) {
    const int64_t b = b0 + threadIdx.x;
    const int32_t v = b < nb ? aggr[b] : sc_id<OP>();
    const int32_t inc = block_inclusive_scan<OP>(v, lds);
    lds[threadIdx.x] = inc;
    __syncthreads();
    const int32_t before = threadIdx.x == 0 ? carry : sc_op<OP>(carry, lds[threadIdx.x - 1]);
    const int32_t total = lds[kScanThreads - 1];
    __syncthreads();
    if (b < nb) aggr[b] = before;
    carry = sc_op<OP>(carry, total);
  }
  return carry;
}

// pass 3, one workgroup per tile: out[j] = op over the sequence up to j (inclusive; EXCL: up to j - 1); out may alias in
template <int OP, bool REV, bool EXCL>
__device__ __forceinline__ void scan_tile_apply(const int32_t* in, int32_t* out, int64_t len, const int32_t* __restrict__ aggr,
                                                int32_t* lds) {
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int32_t v[kScanItems];
  int32_t acc = sc_id<OP>();
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t j = base + k;
    v[k] = j < len ? in[REV ? len - 1 - j : j] : sc_id<OP>();
    acc = sc_op<OP>(acc, v[k]);
  }
  const int32_t inc = block_inclusive_scan<OP>(acc, lds);
  lds[threadIdx.x] = inc;
  __syncthreads();
  int32_t run = sc_op<OP>(aggr[blockIdx.x], threadIdx.x == 0 ? sc_id<OP>() : lds[threadIdx.x - 1]);   // everything before this thread
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t j = base + k;
    const int32_t after = sc_op<OP>(run, v[k]);
    if (j < len) out[REV ? len - 1 - j : j] = EXCL ? run : after;
    run = after;
  }
}

// ---- tile-count scan, ONE workgroup: tile_off[b] = sum of counts[0 .. b - 1] as int64, kScanThreads counts per step with an
// int64 carry; returns the total to every thread.  The sum of kScanThreads consecutive counts must fit int32.
__device__ __forceinline__ int64_t scan_tile_counts(const int32_t* __restrict__ counts, int64_t nb, int64_t* __restrict__ tile_off,
                                                    int32_t* lds) {
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += kScanThreads) {
    const int64_t b = b0 + threadIdx.x;
    const int32_t v = b < nb ? counts[b] : 0;
    const int32_t inc = block_inclusive_scan<0>(v, lds);
    lds[threadIdx.x] = inc;
    __syncthreads();
    const int32_t chunk = lds[kScanThreads - 1];
    __syncthreads();
    if (b < nb) tile_off[b] = carry + inc - v;
    carry += chunk;
  }
  return carry;
}

}  // namespace scpose
