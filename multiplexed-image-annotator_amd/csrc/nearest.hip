// Nearest cell of every type (Annotator.nearest_type_distances; scimap's spatial_distance, spatstat's Gcross): for every cell i and every cell
// type b the squared distance to the nearest OTHER cell of type b and that cell's index (ribca_nearest_by_type), and, under the label permutations
// of ribca_perm.h, how many cells of type a have their nearest b-cell in each radius band (ribca_nearest_perm_counts).  Brute force in fp64, the
// squared distance as the header states it for ribca_radial_pair_counts (dx*dx and dy*dy rounded on their own, then added: contraction is off
// for this file), so a numpy loop reproduces every comparison.  include/ribca_hip.h states the contract; tests/nearest_numpy.py restates it.
//   The cells are sorted ONCE per call by (type, index) -- a stable counting sort in three small kernels (type_hist, type_scan, type_place): slot
//   = rank[i], order = rank^-1, seg[b] .. seg[b + 1] = the slots of type b, labels outside [0, T) in a last segment of their own that is never a
//   target.  The coordinates are held in slot order as (x, y) pairs.
//   nearest_scan  grid (chunks of 256 query slots, types): the workgroup streams ONE segment through LDS tiles of NR_TILE candidates, one 16-byte
//                 broadcast read per candidate, and every thread keeps one (min, slot) pair in registers -- no table of T running minima, which a
//                 label-indexed register array would send to scratch.  The segment is scanned in ascending slot = ascending cell index with a
//                 strict <, which is the lowest-index rule; the cell itself is excluded by its slot, and only in the tiles that overlap the
//                 workgroup's own slots.
//   perm_scatter  the null needs no sort per permutation: thread i computes s = sigma_p(i) and writes (x[i], y[i]) to slot rank[s] of the
//                 permutation's copy.  sigma_p is a bijection, so every slot has one writer, and segment b then holds exactly the positions that
//                 carry label b under p; the segment offsets never change.
//   perm_counts   grid (chunks, types, permutations of the batch): the same scan on the permutation's copy, the query's label being the segment
//                 its slot lies in.  No (n, T) table: the minimum finds its band by the branch-free search of cooccurrence.hip and is counted
//                 into an LDS histogram [B][T] -- the target type is the workgroup's, so B T <= 2048 counters always fit -- flushed with one
//                 64-bit integer atomic per non-zero entry.  Integer atomics only.
// Permutations are batched through the workspace by the rule of ribca_perm.h.  Measured forms: DESIGN.md section 18.
#include <math.h>

#include <algorithm>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_perm.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

#pragma clang fp contract(off)      // the rounding intrinsics are plain operators here and would be fused

namespace ribca {
namespace {

constexpr int NR_BANDS = 32;
constexpr int NR_T_MAX = 254;               // the most the uint8 index image of colorize holds, as in cooccurrence.hip
constexpr int NR_T_PERM = 64;               // the permutation counts: a (P, B, T, T) tensor
constexpr int NR_N_MAX = 1 << 21;           // the cap of ribca_radial_pair_counts: the work is quadratic
constexpr int NR_TILE = 512;                // candidates of one LDS tile
constexpr int NR_SORT = 1024;               // cells of one workgroup of the counting sort
constexpr int NR_BINS = 256;                // row length of the per-chunk histograms: T + 1 <= 255 bins
constexpr int NR_BATCH = 32;                // permutations whose coordinates the workspace holds at most
constexpr long long NR_COPY_BYTES = 64ll << 20;      // ... and the bytes of them it holds at most (one permutation when a single one is larger)

static_assert(NR_T_MAX + 1 < NR_BINS, "one bin per type and one for the labels outside the range");
static_assert(NR_BANDS == 32, "the band search takes five steps over 31 thresholds");
static_assert(NR_BANDS * NR_T_PERM * 4 <= 16 * 1024, "the LDS histogram of perm_counts");
static_assert(NR_TILE % 256 == 0 && NR_SORT % 256 == 0, "whole rounds of a 256-thread workgroup");

struct Edges { double r2[NR_BANDS]; };      // by value: B thresholds, +inf behind them

int fail(const char* msg) { return api_fail(msg); }

__device__ __forceinline__ int bin_of(int32_t type, int T) { return (unsigned)type < (unsigned)T ? type : T; }

// hist[chunk][bin] = the cells of the chunk in each bin; the whole row of NR_BINS words is written
__global__ __launch_bounds__(256) void type_hist_kernel(const int32_t* __restrict__ type, int n, int T, int32_t* __restrict__ hist) {
  __shared__ int h[NR_BINS];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const int first = blockIdx.x * NR_SORT;
  for (int e = tid; e < NR_SORT; e += 256)
    if (first + e < n) atomicAdd(&h[bin_of(type[first + e], T)], 1);
  __syncthreads();
  hist[(size_t)blockIdx.x * NR_BINS + tid] = h[tid];
}

// one workgroup: hist[chunk][bin] becomes the cells of the bin in the chunks before it, seg[0 .. T + 1] the exclusive scan of the bin totals
__global__ __launch_bounds__(NR_BINS) void type_scan_kernel(int32_t* __restrict__ hist, int chunks, int T, int32_t* __restrict__ seg) {
  __shared__ int total[NR_BINS];
  const int tid = threadIdx.x;
  int run = 0;
  for (int c = 0; c < chunks; ++c) {
    const int v = hist[(size_t)c * NR_BINS + tid];
    hist[(size_t)c * NR_BINS + tid] = run;
    run += v;
  }
  total[tid] = run;
  __syncthreads();
  if (tid == 0) {
    int at = 0;
    for (int b = 0; b <= T; ++b) {
      seg[b] = at;
      at += total[b];
    }
    seg[T + 1] = at;      // = n
  }
}

// slot of cell i = seg[bin] + the cells of the bin in earlier chunks + those before i in its own chunk: rank, order, the slot's bin and the
// coordinates in slot order (sxy may be NULL: the permutation entry point scatters its own)
__global__ __launch_bounds__(256) void type_place_kernel(const double* __restrict__ x, const double* __restrict__ y, const int32_t* __restrict__ type,
                                                         int n, int T, const int32_t* __restrict__ hist, const int32_t* __restrict__ seg,
                                                         int32_t* __restrict__ rank, int32_t* __restrict__ order, int32_t* __restrict__ slot_bin,
                                                         double2* __restrict__ sxy) {
  __shared__ int sb[NR_SORT];
  const int tid = threadIdx.x;
  const int first = blockIdx.x * NR_SORT;
  for (int e = tid; e < NR_SORT; e += 256) sb[e] = first + e < n ? bin_of(type[first + e], T) : -1;
  __syncthreads();
  for (int e = tid; e < NR_SORT; e += 256) {
    const int i = first + e;
    if (i >= n) break;
    const int bin = sb[e];
    int before = 0;
    for (int k = 0; k < e; ++k) before += sb[k] == bin ? 1 : 0;
    const int slot = seg[bin] + hist[(size_t)blockIdx.x * NR_BINS + bin] + before;
    rank[i] = slot;
    order[slot] = i;
    slot_bin[slot] = bin;
    if (sxy) sxy[slot] = make_double2(x[i], y[i]);
  }
}

// the minimum of d2 over the slots [lo, hi) of pts for the query (qx, qy) at slot q, and the first slot that attains it: every thread of the
// workgroup calls it with the same lo, hi (barriers inside)
__device__ __forceinline__ void scan_segment(const double2* __restrict__ pts, int lo, int hi, int q0, int q, double qx, double qy, double2* tile,
                                             double& best, int& at) {
  const int tid = threadIdx.x;
  for (int base = lo; base < hi; base += NR_TILE) {      // uniform over the workgroup
    __syncthreads();
    for (int i = tid; i < NR_TILE; i += 256) tile[i] = base + i < hi ? pts[base + i] : make_double2(0.0, 0.0);
    __syncthreads();
    const int lim = hi - base < NR_TILE ? hi - base : NR_TILE;
    if (base < q0 + 256 && base + lim > q0) {      // the tile holds slots of this workgroup's own queries
#pragma unroll 4
      for (int i = 0; i < lim; ++i) {
        const double2 c = tile[i];
        const double dx = c.x - qx, dy = c.y - qy;
        const double d = dx * dx + dy * dy;      // three roundings: contraction is off
        if (d < best && base + i != q) {
          best = d;
          at = base + i;
        }
      }
    } else {
#pragma unroll 4
      for (int i = 0; i < lim; ++i) {
        const double2 c = tile[i];
        const double dx = c.x - qx, dy = c.y - qy;
        const double d = dx * dx + dy * dy;      // three roundings: contraction is off
        if (d < best) {
          best = d;
          at = base + i;
        }
      }
    }
  }
}

// near2[i][b], arg[i][b] for the cell i at every slot of the chunk and b = blockIdx.y
__global__ __launch_bounds__(256) void nearest_scan_kernel(const double2* __restrict__ sxy, const int32_t* __restrict__ seg,
                                                           const int32_t* __restrict__ order, int n, int T, double* __restrict__ near2,
                                                           int32_t* __restrict__ arg) {
  __shared__ double2 tile[NR_TILE];
  const int q0 = blockIdx.x * 256, q = q0 + threadIdx.x;
  const int b = blockIdx.y;
  const bool live = q < n;
  const double2 own = live ? sxy[q] : make_double2(0.0, 0.0);
  double best = INFINITY;
  int at = -1;
  scan_segment(sxy, seg[b], seg[b + 1], q0, q, own.x, own.y, tile, best, at);
  if (!live) return;
  const size_t o = (size_t)order[q] * T + b;
  near2[o] = best;
  arg[o] = at >= 0 ? order[at] : -1;
}

// pxy[j][rank[sigma_{p0 + j}(i)]] = (x[i], y[i]): grid (chunks of 256 cells, batch)
__global__ __launch_bounds__(256) void nearest_perm_scatter_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                                   const int32_t* __restrict__ rank, int n, int h, uint64_t image_key, uint64_t p0,
                                                                   double2* __restrict__ pxy) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = perm_sigma(image_key, p0 + blockIdx.y, (uint32_t)i, (uint32_t)n, h);
  if (s < (uint32_t)n) pxy[(size_t)blockIdx.y * n + rank[s]] = make_double2(x[i], y[i]);
}

// counts[j][band][a][b] += the query slots of the chunk whose segment is a < T and whose nearest slot of segment b = blockIdx.y lies in the band:
// grid (chunks, types, batch)
__global__ __launch_bounds__(256) void nearest_perm_counts_kernel(const double2* __restrict__ pxy, const int32_t* __restrict__ seg,
                                                                  const int32_t* __restrict__ slot_bin, int n, int T, int B, Edges edges,
                                                                  unsigned long long* __restrict__ counts) {
  __shared__ double2 tile[NR_TILE];
  __shared__ double sthr[NR_BANDS];
  __shared__ unsigned int hist[NR_BANDS * NR_T_PERM];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int lo = seg[b], hi = seg[b + 1];
  if (lo == hi) return;      // uniform: nobody carries b
  const double2* __restrict__ pts = pxy + (size_t)blockIdx.z * n;
  const int words = B * T;
  for (int e = tid; e < words; e += 256) hist[e] = 0;
  if (tid < NR_BANDS) sthr[tid] = edges.r2[tid];
  const int q0 = blockIdx.x * 256, q = q0 + tid;
  const bool live = q < n;
  const double2 own = live ? pts[q] : make_double2(0.0, 0.0);
  const int a = live ? slot_bin[q] : T;
  double best = INFINITY;
  int at = -1;
  scan_segment(pts, lo, hi, q0, q, own.x, own.y, tile, best, at);      // its first barrier orders the zeroes and the thresholds
  if (a < T && best <= edges.r2[B - 1]) {
    int band = 0;      // the thresholds below the minimum: all of them lie in sthr[0 .. 30]
#pragma unroll
    for (int step = 16; step >= 1; step >>= 1)
      if (best > sthr[band + step - 1]) band += step;
    atomicAdd(&hist[band * T + a], 1u);
  }
  __syncthreads();
  unsigned long long* __restrict__ out = counts + (size_t)blockIdx.z * B * T * T;
  for (int e = tid; e < words; e += 256)
    if (hist[e]) atomicAdd(&out[(size_t)e * T + b], (unsigned long long)hist[e]);      // e = band T + a
}

int sort_chunks(int n) { return (n + NR_SORT - 1) / NR_SORT; }

// B = min(P, 32, max(1, 64 MiB / (16 n)))
int batch_of(int n, int P) { return perm_batch(P, NR_BATCH, 16ll * n, NR_COPY_BYTES); }

struct NearestWs {
  int32_t* hist;         // (chunks, NR_BINS): the counting sort
  int32_t* seg;          // (T + 2)
  int32_t* rank;         // (n): the slot of a cell
  int32_t* order;        // (n): the cell of a slot
  int32_t* slot_bin;     // (n): the segment of a slot
  double2* xy;           // (copies, n): the coordinates in slot order
};

NearestWs carve_nearest(Carver& cv, int n, int T, int copies) {
  NearestWs w;
  w.hist = cv.take<int32_t>((size_t)sort_chunks(n) * NR_BINS);
  w.seg = cv.take<int32_t>((size_t)T + 2);
  w.rank = cv.take<int32_t>((size_t)n);
  w.order = cv.take<int32_t>((size_t)n);
  w.slot_bin = cv.take<int32_t>((size_t)n);
  w.xy = cv.take<double2>((size_t)copies * n);
  return w;
}

void launch_sort(const double* x, const double* y, const int32_t* type, int n, int T, const NearestWs& w, bool with_xy, hipStream_t s) {
  const int chunks = sort_chunks(n);
  hipLaunchKernelGGL(type_hist_kernel, dim3((unsigned)chunks), dim3(256), 0, s, type, n, T, w.hist);
  hipLaunchKernelGGL(type_scan_kernel, dim3(1), dim3(NR_BINS), 0, s, w.hist, chunks, T, w.seg);
  hipLaunchKernelGGL(type_place_kernel, dim3((unsigned)chunks), dim3(256), 0, s, x, y, type, n, T, w.hist, w.seg, w.rank, w.order, w.slot_bin,
                     with_xy ? w.xy : (double2*)nullptr);
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_nearest_by_type_ws_bytes(int32_t n, int32_t T) {
  if (n < 1 || n > NR_N_MAX || T < 1 || T > NR_T_MAX) return 0;
  Carver cv(nullptr);
  carve_nearest(cv, n, T, 1);
  return (int64_t)cv.off;
}

int ribca_nearest_by_type(const double* x, const double* y, const int32_t* cell_type, int32_t n, int32_t T, double* near2, int32_t* arg, void* ws,
                          int64_t ws_bytes, void* stream) {
  if (!x || !y || !cell_type || !near2 || !arg || !ws) return fail("ribca_nearest_by_type: NULL buffer");
  if (n < 1 || n > NR_N_MAX) return fail("ribca_nearest_by_type: needs 1 <= n <= 2^21");
  if (T < 1 || T > NR_T_MAX) return fail("ribca_nearest_by_type: needs 1 <= T <= 254");
  if (ws_bytes < ribca_nearest_by_type_ws_bytes(n, T)) return fail("ribca_nearest_by_type: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Carver cv(ws);
  const NearestWs w = carve_nearest(cv, n, T, 1);
  launch_sort(x, y, cell_type, n, T, w, true, s);
  hipLaunchKernelGGL(nearest_scan_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)T), dim3(256), 0, s, w.xy, w.seg, w.order, n, T, near2, arg);
  RIBCA_FINISH();
  return 0;
}

int64_t ribca_nearest_perm_counts_ws_bytes(int32_t n, int32_t T, int32_t P) {
  if (n < 1 || n > NR_N_MAX || T < 1 || T > NR_T_PERM || P < 1) return 0;
  Carver cv(nullptr);
  carve_nearest(cv, n, T, batch_of(n, P));
  return (int64_t)cv.off;
}

int ribca_nearest_perm_counts(const double* x, const double* y, const int32_t* cell_type, int32_t n, int32_t T, const double* r2_host, int32_t B,
                              uint64_t seed, int32_t image, int64_t p0, int32_t P, uint64_t* counts, void* ws, int64_t ws_bytes, void* stream) {
  if (!x || !y || !cell_type || !r2_host || !counts || !ws) return fail("ribca_nearest_perm_counts: NULL buffer");
  if (n < 1 || n > NR_N_MAX) return fail("ribca_nearest_perm_counts: needs 1 <= n <= 2^21");
  if (T < 1 || T > NR_T_PERM) return fail("ribca_nearest_perm_counts: needs 1 <= T <= 64");
  if (B < 1 || B > NR_BANDS) return fail("ribca_nearest_perm_counts: needs 1 <= B <= 32");
  Edges edges;
  for (int b = 0; b < NR_BANDS; ++b) edges.r2[b] = INFINITY;
  for (int b = 0; b < B; ++b) {
    const double r = r2_host[b];
    if (!isfinite(r) || r < 0.0 || (b > 0 && !(r > r2_host[b - 1])))
      return fail("ribca_nearest_perm_counts: the squared radii must be finite, non-negative and strictly increasing");
    edges.r2[b] = r;
  }
  if (perm_range_check("ribca_nearest_perm_counts", image, p0, P)) return 1;
  if (ws_bytes < ribca_nearest_perm_counts_ws_bytes(n, T, P)) return fail("ribca_nearest_perm_counts: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int batch_max = batch_of(n, P);
  Carver cv(ws);
  const NearestWs w = carve_nearest(cv, n, T, batch_max);
  launch_sort(x, y, cell_type, n, T, w, false, s);
  const int chunks = (n + 255) / 256;
  const PermKeys k(n, seed, image);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  for (int64_t j0 = 0; j0 < P; j0 += batch_max) {      // the batches follow one another on the stream: the copies are reused
    const int batch = (int)std::min<int64_t>(batch_max, P - j0);
    hipLaunchKernelGGL(nearest_perm_scatter_kernel, dim3((unsigned)chunks, (unsigned)batch), dim3(256), 0, s, x, y, w.rank, n, k.h, k.image_key,
                       (uint64_t)(p0 + j0), w.xy);
    hipLaunchKernelGGL(nearest_perm_counts_kernel, dim3((unsigned)chunks, (unsigned)T, (unsigned)batch), dim3(256), 0, s, w.xy, w.seg, w.slot_bin, n,
                       T, B, edges, out + (size_t)j0 * B * T * T);
  }
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
