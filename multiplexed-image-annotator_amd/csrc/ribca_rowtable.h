// The per-row open-addressing table of the mask kernels that count pixels per (row, key) pair: contact.hip (cell, neighbouring cell) and
// overlap.hip (cell, object of a second mask).  A workspace holds (n, S) keys and (n, S) 64-bit sums; kernels insert with global_insert, and
// contact_rows_kernel writes every row out sorted by key.  Slot positions depend on the arrival order, ranks and integer sums do not.
#pragma once
#include <limits.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "ribca_scratch.h"

namespace ribca {
namespace {

constexpr int CT_N_MAX = 1 << 21;
constexpr int CT_S_MIN = 8, CT_S_MAX = 1024;
constexpr int CT_ROWS = 4;                   // rows of one contact_rows workgroup: one wave each

static_assert(CT_ROWS * CT_S_MAX * 4 <= 16 * 1024, "LDS of contact_rows");

__global__ __launch_bounds__(256) void contact_init_kernel(int32_t* __restrict__ keys, unsigned long long* __restrict__ sums, size_t slots,
                                                           int32_t* __restrict__ flag, int n, int32_t* __restrict__ over) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < slots; e += stride) {
    keys[e] = -1;
    sums[e] = 0ull;
  }
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)n; e += stride) flag[e] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    over[0] = 0;
    over[1] = INT_MAX;
  }
}

// sums[i][slot of j] += count; at most S probes, then the overflow of row i is recorded
__device__ __forceinline__ void global_insert(int32_t* __restrict__ keys, unsigned long long* __restrict__ sums, int32_t* __restrict__ flag,
                                              int32_t* __restrict__ over, int S, int log_s, int i, int j, unsigned int count) {
  int32_t* __restrict__ row = keys + (size_t)i * S;
  int slot = (int)(((uint32_t)j * 0x9E3779B1u) >> (32 - log_s));
  for (int probe = 0; probe < S; ++probe) {
    const int32_t old = atomicCAS(&row[slot], -1, j);
    if (old == -1 || old == j) {
      atomicAdd(&sums[(size_t)i * S + slot], (unsigned long long)count);
      return;
    }
    slot = (slot + 1) & (S - 1);
  }
  if (atomicExch(&flag[i], 1) == 0) atomicAdd(&over[0], 1);
  atomicMin(&over[1], i);
}

// nbr[i], pairs[i] = the entries of row i in ascending key order, -1 / 0 behind them; degree[i] = their number: one wave per row
__global__ __launch_bounds__(64 * CT_ROWS) void contact_rows_kernel(const int32_t* __restrict__ keys, const unsigned long long* __restrict__ sums, int n,
                                                                    int S, int32_t* __restrict__ nbr, unsigned long long* __restrict__ pairs,
                                                                    int32_t* __restrict__ degree, int32_t* __restrict__ over) {
  __shared__ int row[CT_ROWS][CT_S_MAX];
  __shared__ int filled[CT_ROWS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * CT_ROWS + w;
  const bool live = i < n;
  if (lane == 0) filled[w] = 0;
  if (live)
    for (int e = lane; e < S; e += 64) row[w][e] = keys[(size_t)i * S + e];
  __syncthreads();
  if (live) {
    int mine = 0;
    for (int e = lane; e < S; e += 64) mine += row[w][e] >= 0 ? 1 : 0;
    if (mine) atomicAdd(&filled[w], mine);
  }
  __syncthreads();
  if (live) {
    const int deg = filled[w];
    for (int e = lane; e < S; e += 64) {
      const int key = row[w][e];
      if (key >= 0) {
        int rank = 0;
        for (int o = 0; o < S; ++o) {
          const int other = row[w][o];
          rank += other >= 0 && other < key ? 1 : 0;
        }
        nbr[(size_t)i * S + rank] = key;      // distinct keys: distinct ranks below deg
        pairs[(size_t)i * S + rank] = sums[(size_t)i * S + e];
      }
      if (e >= deg) {
        nbr[(size_t)i * S + e] = -1;
        pairs[(size_t)i * S + e] = 0ull;
      }
    }
    if (lane == 0) degree[i] = deg;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && over[0] == 0) over[1] = -1;      // nobody else touches over in this launch
}

int log2_of_slots(int S) {      // 3 .. 10 for a power of two in 8 .. 1024, -1 otherwise
  for (int b = 3; b <= 10; ++b)
    if (S == 1 << b) return b;
  return -1;
}

bool table_sizes_ok(int H, int W, int n, int S) {
  return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) && n >= 1 && n <= CT_N_MAX && S >= CT_S_MIN && S <= CT_S_MAX && log2_of_slots(S) > 0;
}

struct ContactWs {
  int32_t* keys;                  // (n, S): the key of a slot, -1 = free
  unsigned long long* sums;       // (n, S): its pixel count
  int32_t* flag;                  // (n): the row did not fit
};

ContactWs carve_contact(Carver& cv, int n, int S) {
  ContactWs w;
  w.keys = cv.take<int32_t>((size_t)n * S);
  w.sums = cv.take<unsigned long long>((size_t)n * S);
  w.flag = cv.take<int32_t>((size_t)n);
  return w;
}

}  // namespace
}  // namespace ribca
