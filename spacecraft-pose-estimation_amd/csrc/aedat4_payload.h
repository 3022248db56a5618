// What the payload decoders of the AEDAT-4.0 reader share (events_aedat4_read.hip: LZ4 frames, events_aedat4_zstd.hip: Zstandard
// frames; DESIGN.md section 5a.7, "Payload decoders").  Both decode into the staging buffer in global memory and read their match
// history back from it.
//
// Device functions only.  Contract: called by ALL 64 lanes of a workgroup of exactly one wavefront.
#pragma once
#include "common.h"

namespace scpose {

// A match (and a checksum of the output, and a copy out of the ZSTD literal slot) reads what this wave stored earlier, through
// other lanes: the loads must not overtake the stores.  One wavefront's vector memory operations reach the cache in the order
// they are issued; the wait below makes the stores complete first all the same, and the fences keep the compiler from moving the
// loads above them.
__device__ __forceinline__ void own_stores_done() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace scpose
