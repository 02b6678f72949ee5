// The keyed bijection sigma_p of [0, n) that every permutation null of the library shuffles with (enrichment.hip: cell-type labels; autocorr.hip:
// whole marker rows): a six-round balanced Feistel network over 4^h >= n with cycle walking, the round function a splitmix64 of
// (key, round, right half) -- counter-based, so any (permutation, cell) is computed on its own and a numpy loop reproduces it
// (include/ribca_hip.h states it under ribca_nhood_perm_counts; tests/enrichment_numpy.py restates it).
//     K = s(s(s(seed) ^ image) ^ p):   perm_image_key gives s(s(seed) ^ image) on the host, perm_key folds p in on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ribca {

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// h = max(1, (bit_length(n - 1) + 1) / 2): the width of one half of the network, 4^h >= n
inline int perm_half_bits(int n) {
  int bits = 0;      // bit_length(n - 1)
  while (bits < 32 && ((uint64_t)(n - 1) >> bits) != 0) ++bits;
  const int h = (bits + 1) / 2;
  return h > 1 ? h : 1;
}

inline uint64_t perm_image_key(uint64_t seed, int32_t image) { return splitmix64(splitmix64(seed) ^ (uint64_t)image); }

__device__ __forceinline__ uint64_t perm_key(uint64_t image_key, uint64_t p) { return splitmix64(image_key ^ p); }

// sigma(i) under the key: the pass repeated until the value is back inside [0, n).  The walk follows the cycle of i in a bijection of [0, 4^h), so
// it ends after at most 4^h - n + 1 passes; the loop is capped at 4^h all the same and reports n (no cell) if the cap is ever reached.
__device__ __forceinline__ uint32_t feistel_walk(uint64_t key, uint32_t i, uint32_t n, int h) {
  const uint64_t mask = (1ull << h) - 1;
  const uint64_t domain = 1ull << (2 * h);
  uint64_t v = i;
  for (uint64_t pass = 0; pass < domain; ++pass) {
    uint64_t L = v >> h, R = v & mask;
#pragma unroll
    for (uint64_t r = 0; r < 6; ++r) {
      const uint64_t f = splitmix64(key ^ ((r << 32) | R)) >> (64 - h);
      const uint64_t t = L ^ f;
      L = R;
      R = t;
    }
    v = (L << h) | R;
    if (v < n) return (uint32_t)v;
  }
  return n;
}

}  // namespace ribca
