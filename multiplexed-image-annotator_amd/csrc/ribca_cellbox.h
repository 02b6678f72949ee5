// What the per-cell kernels over (ids, bbox) share (intensities.hip, localization.hip): the clipped box of a cell, whose pixels in row-major order
// are the elements of the stated sums, and the ballot scan that ranks a 256-thread workgroup's flagged pixels without atomics.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ribca {

// the box of a cell, clipped; pixel e of it in row-major order is (r0 + e / bw, c0 + e % bw); total = 0: no pixel (ids[i] <= 0 or an empty box)
struct Box {
  int r0, c0, bw;
  unsigned total;
};

__device__ __forceinline__ Box clipped_box(const int32_t* __restrict__ b, int32_t id, int H, int W) {
  const int rmin = max(b[0], 0), rmax = min(b[1], H - 1), cmin = max(b[2], 0), cmax = min(b[3], W - 1);
  Box box;
  box.r0 = rmin, box.c0 = cmin, box.bw = cmax - cmin + 1;
  box.total = id > 0 && rmin <= rmax && cmin <= cmax ? (unsigned)(rmax - rmin + 1) * (unsigned)box.bw : 0u;      // <= H W < 2^31
  return box;
}

// rank of this thread's flagged pixel among the flagged pixels of a chunk of 256 (one per thread of a four-wave workgroup), and their number m;
// one barrier, wave_tot (in LDS) alternates by parity
__device__ __forceinline__ int chunk_rank(int (&wave_tot)[2][4], bool flag, int parity, int& m) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  if (lane == 0) wave_tot[parity][wave] = __popcll(b);
  __syncthreads();
  const int t0 = wave_tot[parity][0], t1 = wave_tot[parity][1], t2 = wave_tot[parity][2], t3 = wave_tot[parity][3];
  m = t0 + t1 + t2 + t3;
  const int before = wave == 0 ? 0 : wave == 1 ? t0 : wave == 2 ? t0 + t1 : t0 + t1 + t2;
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

}  // namespace ribca
