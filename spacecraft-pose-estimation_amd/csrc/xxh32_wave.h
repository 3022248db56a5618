// xxh32 by one wavefront, shared by the AEDAT-4.0 reader (events_aedat4_read.hip: the LZ4 frames' header, block and content
// checksums) and writer (events_aedat4_write.hip: the header and content checksums it emits).  Device functions only.
//
// Contract: xxh32_wave is called by ALL threads of a workgroup of exactly 64 threads (it contains barriers), with `sw` pointing
// at 256 words of LDS that the caller does not use across the call.
#pragma once
#include "common.h"   // ld32

namespace scpose {

constexpr uint32_t kXxhP1 = 2654435761u, kXxhP2 = 2246822519u, kXxhP3 = 3266489917u, kXxhP4 = 668265263u, kXxhP5 = 374761393u;

__device__ __forceinline__ uint32_t rotl(uint32_t v, int r) { return (v << r) | (v >> (32 - r)); }

// xxh32 (seed 0) of n bytes at p, by one wavefront: lane l carries accumulator l & 3 over the 16-byte stripes, 64 stripes at a time
// through `sw` (256 words of LDS); every lane returns the digest.
__device__ inline uint32_t xxh32_wave(const uint8_t* p, long long n, uint32_t* sw) {
  constexpr int kWave = 64;
  const int lane = threadIdx.x, a = lane & 3;
  uint32_t acc = a == 0 ? kXxhP1 + kXxhP2 : (a == 1 ? kXxhP2 : (a == 2 ? 0u : 0u - kXxhP1));
  const long long full = n >> 4;
  for (long long s0 = 0; s0 < full; s0 += kWave) {
    const int m = full - s0 < kWave ? (int)(full - s0) : kWave;
    __syncthreads();
    for (int k = 0; k < 4; ++k) {
      const int wi = lane + kWave * k;
      if (wi < 4 * m) sw[wi] = ld32(p + (s0 << 4) + 4 * wi);
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) acc = rotl(acc + sw[4 * j + a] * kXxhP2, 13) * kXxhP1;
  }
  uint32_t h = kXxhP5;
  if (n >= 16)
    h = rotl((uint32_t)__shfl((int)acc, 0, kWave), 1) + rotl((uint32_t)__shfl((int)acc, 1, kWave), 7) +
        rotl((uint32_t)__shfl((int)acc, 2, kWave), 12) + rotl((uint32_t)__shfl((int)acc, 3, kWave), 18);
  h += (uint32_t)n;
  const uint8_t* q = p + (full << 4);
  int r = (int)(n & 15);
  for (; r >= 4; r -= 4, q += 4) h = rotl(h + ld32(q) * kXxhP3, 17) * kXxhP4;
  for (; r > 0; --r, ++q) h = rotl(h + (uint32_t)*q * kXxhP5, 11) * kXxhP1;
  h ^= h >> 15;
  h *= kXxhP2;
  h ^= h >> 13;
  h *= kXxhP3;
  h ^= h >> 16;
  return h;
}

}  // namespace scpose
