// xxh32 and XXH64 by one wavefront: the checksums of the AEDAT-4.0 payloads.  xxh32: the LZ4 frames' header, block and content
// checksums the reader verifies (events_aedat4_read.hip) and the header and content checksums the writer emits
// (events_aedat4_write.hip).  XXH64: the content checksum of a Zstandard frame, its low 32 bits (events_aedat4_zstd.hip).
// Device functions only.
//
// Contract: both are called by ALL threads of a workgroup of exactly 64 threads.  xxh32_wave contains barriers, and `sw` points
// at 256 words of LDS that the caller does not use across the call; xxh64_wave has neither.
#pragma once
#include "common.h"   // ld32

namespace scpose {

constexpr uint32_t kXxhP1 = 2654435761u, kXxhP2 = 2246822519u, kXxhP3 = 3266489917u, kXxhP4 = 668265263u, kXxhP5 = 374761393u;

__device__ __forceinline__ uint32_t rotl(uint32_t v, int r) { return (v << r) | (v >> (32 - r)); }
__device__ __forceinline__ unsigned long long rotl(unsigned long long v, int r) { return (v << r) | (v >> (64 - r)); }

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

// XXH64 (seed 0) of p[0, n), the same value in every lane; lanes 0..3 carry the four accumulators.  All lanes.
__device__ inline unsigned long long xxh64_wave(const uint8_t* p, long long n) {
  constexpr unsigned long long P1 = 11400714785074694791ull, P2 = 14029467366897019727ull, P3 = 1609587929392839161ull,
                               P4 = 9650029242287828579ull, P5 = 2870177450012600261ull;
  auto round = [&](unsigned long long acc, unsigned long long in) { return rotl(acc + in * P2, 31) * P1; };
  unsigned long long h;
  long long at = 0;
  if (n >= 32) {
    const int k = threadIdx.x & 3;
    unsigned long long v = k == 0 ? P1 + P2 : k == 1 ? P2 : k == 2 ? 0 : 0 - P1;
    const long long stripes = n / 32;
    if (threadIdx.x < 4)
      for (long long i = 0; i < stripes; ++i) v = round(v, (unsigned long long)ld64(p + 32 * i + 8 * k));
    const unsigned long long v1 = __shfl(v, 0), v2 = __shfl(v, 1), v3 = __shfl(v, 2), v4 = __shfl(v, 3);
    h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
    h = (h ^ round(0, v1)) * P1 + P4;
    h = (h ^ round(0, v2)) * P1 + P4;
    h = (h ^ round(0, v3)) * P1 + P4;
    h = (h ^ round(0, v4)) * P1 + P4;
    at = 32 * stripes;
  } else h = P5;
  h += (unsigned long long)n;
  for (; at + 8 <= n; at += 8) h = rotl(h ^ round(0, (unsigned long long)ld64(p + at)), 27) * P1 + P4;
  if (at + 4 <= n) {
    h = rotl(h ^ ((unsigned long long)ld32(p + at) * P1), 23) * P2 + P3;
    at += 4;
  }
  for (; at < n; ++at) h = rotl(h ^ (p[at] * P5), 11) * P1;
  h ^= h >> 33;
  h *= P2;
  h ^= h >> 29;
  h *= P3;
  h ^= h >> 32;
  return h;
}

}  // namespace scpose
