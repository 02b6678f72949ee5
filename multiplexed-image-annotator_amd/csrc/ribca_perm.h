// The permutation nulls of the library, all of them on ONE keyed bijection sigma_p of [0, n): a six-round balanced Feistel network over 4^h >= n
// with cycle walking, the round function a splitmix64 of (key, round, right half) -- counter-based, so any (permutation, cell) is computed on its
// own and a numpy loop reproduces it (include/ribca_hip.h states it under ribca_nhood_perm_counts; tests/enrichment_numpy.py restates it).
//     K = s(s(s(seed) ^ image) ^ p):   PermKeys gives h and s(s(seed) ^ image) on the host, perm_sigma folds p in on the device.
// Users: enrichment.hip and contact.hip (cell-type labels as byte rows: launch_perm_labels), autocorr.hip and local_autocorr.hip (whole marker
// rows, the latter with the inverse: launch_perm_rows), nearest.hip (its own scatter of coordinates through perm_sigma).  The two shuffle kernels
// live in perm.hip; the batch rule, the range refusal and the keys every one of the five entry points shares are below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <limits>

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

// what a launch needs of (n, seed, image): the half width and s(s(seed) ^ image)
struct PermKeys {
  int h;
  uint64_t image_key;
  PermKeys(int n, uint64_t seed, int32_t image) : h(perm_half_bits(n)), image_key(splitmix64(splitmix64(seed) ^ (uint64_t)image)) {}
};

// B = min(P, most, max(1, cap_bytes / bytes_per_perm)): the permutations whose shuffled copies a workspace holds at once (one when a single copy is
// larger than the cap; no cap by default)
inline int perm_batch(int P, int most, long long bytes_per_perm = 1, long long cap_bytes = std::numeric_limits<long long>::max()) {
  return (int)std::min<long long>(std::min(P, most), std::max(1ll, cap_bytes / bytes_per_perm));
}

// the refusal of (image, p0, P) every permutation entry point shares: 0 when they are in range, else the message is recorded under the entry
// point's name `who` and the status returned (perm.hip)
int perm_range_check(const char* who, int32_t image, int64_t p0, int32_t P);

constexpr uint8_t kPermSkip = 255;      // a byte of launch_perm_labels that is no label: never indexes a T x T histogram (T <= 64)
constexpr int kCellChunk = 256;         // cells of one workgroup of launch_perm_rows, and of one chunk of the kernels that read its rows

inline int chunks_of_cells(int n) { return (n + kCellChunk - 1) / kCellChunk; }

// L, the doubles from one copied row to the next: the power of two >= C up to 16, a multiple of 16 above, so that a row of up to 16 channels lies in
// one 128-byte line and no tile of 16 channels straddles one (the padding is never written and never read)
inline int row_ld(int C) {
  if (C > 16) return (C + 15) / 16 * 16;
  int ld = 1;
  while (ld < C) ld *= 2;
  return ld;
}

// labels[j][i] = (uint8) cell_type[sigma_{p0 + j}(i)] for j < batch, kPermSkip where that is outside [0, T) (or the walk reported no cell)
void launch_perm_labels(const int32_t* cell_type, int n, int T, int h, uint64_t image_key, uint64_t p0, int batch, uint8_t* labels, hipStream_t s);
// zp[j][i][0 .. C) = z[sigma_{p0 + j}(i)][:] in rows of ld doubles (+0.0 if the walk ever reported no cell) for j < batch; inv != nullptr:
// also inv[j][sigma_{p0 + j}(i)] = i -- sigma is a bijection of [0, n), so every word of inv has exactly one writer
void launch_perm_rows(const double* z, int n, int C, int ld, int h, uint64_t image_key, uint64_t p0, int batch, double* zp, int32_t* inv,
                      hipStream_t s);

// sigma_p(i) of the image whose key is image_key, K = s(image_key ^ p): the pass repeated until the value is back inside [0, n).  The walk follows
// the cycle of i in a bijection of [0, 4^h), so it ends after at most 4^h - n + 1 passes; the loop is capped at 4^h all the same and reports n (no
// cell) if the cap is ever reached.  Every kernel that shuffles calls this and nothing else.
__device__ __forceinline__ uint32_t perm_sigma(uint64_t image_key, uint64_t p, uint32_t i, uint32_t n, int h) {
  const uint64_t key = splitmix64(image_key ^ p);
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
