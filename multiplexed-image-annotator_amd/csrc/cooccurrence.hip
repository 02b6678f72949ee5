// Co-occurrence by distance (Annotator.cooccurrence_by_distance; in the spirit of squidpy's co_occurrence and of cross-type Ripley counts): for
// every ORDERED pair of cells i != j of one image, counts[b][type_i][type_j] += 1 for the one band b with r2[b - 1] < d2 <= r2[b] (band 0:
// d2 <= r2[0]; beyond r2[B - 1]: not counted).  Brute force in fp64, the squared distance exactly as knn.hip forms it (d = dx*dx; d += dy*dy, no
// contraction), so a numpy loop reproduces every comparison, ties at a band edge included.
//   one thread per query cell, 256 per workgroup; the candidates of the workgroup's slice (blockIdx.y: every gridDim.y-th tile of CO_TILE cells)
//   streamed through LDS together with their labels; a pair inside r2[B - 1] finds its band by a five-step branch-free binary search over the 32
//   thresholds held in LDS (padded with +inf) and is counted with one integer atomic -- into a [B][T][T] LDS histogram while that fits 64 KiB
//   (three sizes of it, so that the common B T^2 keeps more workgroups on a CU), flushed with one 64-bit global atomic per non-zero entry; above
//   that, up to T = 254, straight into the global tensor, as the counting of knn.hip does above 32 types.  Integer atomics only: the result does
//   not depend on the order or on the launch geometry.
// n = 1e5 cells -> 1e10 distance evaluations, 391 query workgroups: the candidate split (up to CO_SPLIT) fills the chip.  No workspace.
#include <math.h>

#include <algorithm>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_status.h"

namespace ribca {
namespace {

constexpr int CO_BANDS = 32;
constexpr int CO_T_MAX = 254;            // the most the uint8 index image of colorize holds, as in knn.hip
constexpr int CO_N_MAX = 1 << 21;        // 4.4e12 pairs, seconds on one card; the work is quadratic and a larger call is refused
constexpr int CO_TILE = 512;             // candidates of one LDS tile
constexpr int CO_SPLIT = 8;              // at most this many candidate slices (gridDim.y)
constexpr int CO_WGS = 3072;             // workgroups the split aims at: a few rounds of the 256 CUs
constexpr int CO_HIST_SMALL = 4096, CO_HIST_MID = 8192, CO_HIST_MAX = 16384;      // 32-bit counters of the three LDS forms

static_assert(CO_HIST_MAX * 4 <= 64 * 1024, "the LDS histogram");
static_assert(CO_BANDS == 32, "the band search takes five steps over 31 thresholds");
static_assert(256ll * CO_N_MAX < (1ll << 32), "a 32-bit LDS count cannot wrap within one workgroup: 256 query cells times at most n candidates");

struct Edges { double r2[CO_BANDS]; };      // by value: B thresholds, +inf behind them

int fail(const char* msg) { return api_fail(msg); }

// kWords: 32-bit counters of the LDS histogram (B T T <= kWords); 0: every count is an atomic on the global tensor
template <int kWords>
__global__ __launch_bounds__(256) void radial_pair_counts_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                 const int32_t* __restrict__ type, int n, int T, int B, Edges edges,
                                                                 unsigned long long* __restrict__ counts) {
  __shared__ double sx[CO_TILE], sy[CO_TILE], sthr[CO_BANDS];
  __shared__ int st[CO_TILE];
  __shared__ unsigned int hist[kWords ? kWords : 1];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * 256 + tid;
  const int words = B * T * T;
  if (kWords)
    for (int e = tid; e < words; e += 256) hist[e] = 0;
  if (tid < CO_BANDS) sthr[tid] = edges.r2[tid];
  const double rmax = edges.r2[B - 1];
  const double qx = q < n ? x[q] : 0.0, qy = q < n ? y[q] : 0.0;
  const int tq = q < n ? type[q] : -1;
  const bool valid = (unsigned)tq < (unsigned)T;
  const int row = valid ? tq * T : 0;
  const int TT = T * T;
  for (int base = blockIdx.y * CO_TILE; base < n; base += gridDim.y * CO_TILE) {      // uniform over the workgroup
    __syncthreads();
    for (int i = tid; i < CO_TILE; i += 256) {
      const int j = base + i;
      sx[i] = j < n ? x[j] : 0.0;
      sy[i] = j < n ? y[j] : 0.0;
      st[i] = j < n ? type[j] : -1;
    }
    __syncthreads();
    const int lim = n - base < CO_TILE ? n - base : CO_TILE;
    if (!valid) continue;
    for (int i = 0; i < lim; ++i) {
      const double dx = sx[i] - qx, dy = sy[i] - qy;
      const double d = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
      if (d <= rmax && base + i != q) {
        const int tc = st[i];
        if ((unsigned)tc < (unsigned)T) {
          int b = 0;      // the thresholds below d: all of them lie in sthr[0 .. 30], since d <= r2[B - 1]
#pragma unroll
          for (int step = 16; step >= 1; step >>= 1)
            if (d > sthr[b + step - 1]) b += step;
          const int e = b * TT + row + tc;
          if (kWords) atomicAdd(&hist[e], 1u);
          else atomicAdd(&counts[e], 1ull);
        }
      }
    }
  }
  if (!kWords) return;
  __syncthreads();
  for (int e = tid; e < words; e += 256)
    if (hist[e]) atomicAdd(&counts[e], (unsigned long long)hist[e]);
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_radial_pair_counts_ws_bytes(int32_t n, int32_t T, int32_t B) {
  (void)n; (void)T; (void)B;
  return 0;      // the histogram lives in LDS
}

int ribca_radial_pair_counts(const double* x, const double* y, const int32_t* cell_type, int32_t n, int32_t T, const double* r2_host, int32_t B,
                             uint64_t* counts, void* ws, int64_t ws_bytes, void* stream) {
  (void)ws;
  if (!x || !y || !cell_type || !r2_host || !counts) return fail("ribca_radial_pair_counts: NULL buffer");
  if (n < 1 || n > CO_N_MAX) return fail("ribca_radial_pair_counts: needs 1 <= n <= 2^21");
  if (T < 1 || T > CO_T_MAX) return fail("ribca_radial_pair_counts: needs 1 <= T <= 254");
  if (B < 1 || B > CO_BANDS) return fail("ribca_radial_pair_counts: needs 1 <= B <= 32");
  Edges edges;
  for (int b = 0; b < CO_BANDS; ++b) edges.r2[b] = INFINITY;
  for (int b = 0; b < B; ++b) {
    const double r = r2_host[b];
    if (!isfinite(r) || r < 0.0 || (b > 0 && !(r > r2_host[b - 1])))
      return fail("ribca_radial_pair_counts: the squared radii must be finite, non-negative and strictly increasing");
    edges.r2[b] = r;
  }
  if (ws_bytes < ribca_radial_pair_counts_ws_bytes(n, T, B)) return fail("ribca_radial_pair_counts: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int gx = (n + 255) / 256;
  const int tiles = (n + CO_TILE - 1) / CO_TILE;
  const int gy = std::min(tiles, std::min(CO_SPLIT, std::max(1, CO_WGS / gx)));
  const dim3 grid((unsigned)gx, (unsigned)gy);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  const long long words = (long long)B * T * T;
  if (words <= CO_HIST_SMALL)
    hipLaunchKernelGGL(radial_pair_counts_kernel<CO_HIST_SMALL>, grid, dim3(256), 0, s, x, y, cell_type, n, T, B, edges, out);
  else if (words <= CO_HIST_MID)
    hipLaunchKernelGGL(radial_pair_counts_kernel<CO_HIST_MID>, grid, dim3(256), 0, s, x, y, cell_type, n, T, B, edges, out);
  else if (words <= CO_HIST_MAX)
    hipLaunchKernelGGL(radial_pair_counts_kernel<CO_HIST_MAX>, grid, dim3(256), 0, s, x, y, cell_type, n, T, B, edges, out);
  else
    hipLaunchKernelGGL(radial_pair_counts_kernel<0>, grid, dim3(256), 0, s, x, y, cell_type, n, T, B, edges, out);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
