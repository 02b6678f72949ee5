// Tissue regions (reference spatial_methods.tissue_region_partition, spatial_methods.py:133-198, which hands the (n, 8 T) composition table to
// scikit-learn's PCA(0.99) and KMeans on the host, unseeded): the parts of both that touch all n rows.  DESIGN.md section 11 states the
// arithmetic; tests/regions_numpy.py reproduces it bit for bit with numpy loops.
//
// PCA.  The table is never formed: its entries are count / size with small integer counts (the int16 output of ribca_knn_compositions,
// 0 .. 255), so the column sums and the Gram matrix G = C^T C of the COUNTS are exact integers.
//   region_colsum   one thread per column, a chunk of 1024 rows per workgroup, int64 atomics; also flags a count outside 0 .. 255.
//   region_gram     one 64 x 64 tile of G per workgroup and chunk of 1024 rows, 4 x 4 outputs per thread, int16 operands through LDS, int32
//                   accumulators (<= 1024 * 255^2 < 2^26 per chunk), int64 atomics into G.  Only tiles on or above the diagonal are computed;
//                   each is written to both places.  Integer sums do not depend on their order: any geometry gives the same G.
//                   Integer VALU, not the i8 matrix cores: counts reach 200, which a signed i8 operand does not hold (two planes per operand
//                   would be needed), and at the pipeline's F = 8 T <= 144 the whole product is 2 GFLOP -- launch-bound either way.
//   region_project  Y[i, j] = sum over f ascending of (C[i, f] / size[f] - mean[f]) * V[j, f], fp64, every operation rounded on its own.
//
// k-means (fp64, scikit-learn's KMeans defaults restated).  d2(i, c) = sum over f ascending of (y[i, f] - c[f])^2, no contraction.
//   kmeans_trials   k-means++: d2 of up to 8 candidate rows against all rows, min with the running minimum, and the potential of every
//                   candidate summed in a fixed order (rows of a 1024-chunk ascending, then the chunks ascending).
//   kmeans_assign   label = least (d2, j); counts the labels that changed with an integer atomic.
//   kmeans_update   THE summation order of the centre sums: rows in chunks of 1024; per chunk and (cluster, dimension) the rows added in
//                   ascending order (one thread owns a dimension, all clusters of it in LDS); then the chunks added in ascending order; one
//                   division by the count.  No float atomics: the sums do not depend on the launch geometry.
//   kmeans_finalize centres = sums / counts, and per centre the squared shift summed over the dimensions in ascending order.  The host reads
//                   (changed, counts, shifts) -- 4 + 12 k bytes -- once per iteration and decides to stop.  No kernel waits for another.
//   kmeans_relocate scikit-learn's rule for an empty cluster, applied to the sums before the division (rare; the host picks the rows).
#include <cmath>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

// every sum and product rounds on its own: the projections and distances are the ones a plain numpy restatement computes
#pragma clang fp contract(off)

namespace ribca {
namespace {

constexpr int RG_TILE = 64;           // Gram tile edge
constexpr int RG_SUB = 64;            // rows staged in LDS at a time
constexpr int RG_FMAX = 2032;         // 8 neighbourhood sizes x 254 cell types
constexpr int RG_COUNT_MAX = 255;     // largest neighbourhood size ribca_knn_compositions takes
constexpr int KM_KMAX = 256;
constexpr int KM_CT = 8;              // centres per register tile
constexpr int KM_DT = 256;            // dimensions per LDS tile
constexpr int KM_THREADS = 128;
constexpr int KM_ACC_DOUBLES = 4096;  // 32 KiB of per-chunk centre sums in LDS

int fail(const char* msg) { return api_fail(msg); }

// ------------------------------------------------------------------------------------------------------------------------------ PCA
__global__ __launch_bounds__(256) void region_colsum_kernel(const int16_t* __restrict__ counts, int n, int F, long long* __restrict__ colsum,
                                                            unsigned* __restrict__ flag) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int r0 = blockIdx.y * kSumChunk;
  const int r1 = r0 + kSumChunk < n ? r0 + kSumChunk : n;
  int s = 0;
  bool bad = false;
  for (int r = r0; r < r1; ++r) {
    const int v = counts[(size_t)r * F + f];
    bad |= (unsigned)v > (unsigned)RG_COUNT_MAX;
    s += v & 0xFF;      // bounded whatever the input holds; an out-of-range count fails the call
  }
  atomicAdd(reinterpret_cast<unsigned long long*>(&colsum[f]), (unsigned long long)s);
  if (bad) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void region_gram_kernel(const int16_t* __restrict__ counts, int n, int F, int tiles,
                                                          long long* __restrict__ gram) {
  __shared__ __attribute__((aligned(8))) int16_t sa[RG_SUB][RG_TILE];
  __shared__ __attribute__((aligned(8))) int16_t sb[RG_SUB][RG_TILE];
  // blockIdx.x enumerates the tile pairs ta <= tb, row by row
  int ta = 0, rest = blockIdx.x;
  while (rest >= tiles - ta) { rest -= tiles - ta; ++ta; }
  const int tb = ta + rest;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int r0 = blockIdx.y * kSumChunk;
  const int r1 = r0 + kSumChunk < n ? r0 + kSumChunk : n;
  int acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0;
  for (int base = r0; base < r1; base += RG_SUB) {
    __syncthreads();
    for (int i = tid; i < RG_SUB * RG_TILE; i += 256) {
      const int r = i >> 6, c = i & 63;
      const int row = base + r, ca = ta * RG_TILE + c, cb = tb * RG_TILE + c;
      sa[r][c] = (row < r1 && ca < F) ? (int16_t)(counts[(size_t)row * F + ca] & 0xFF) : (int16_t)0;
      sb[r][c] = (row < r1 && cb < F) ? (int16_t)(counts[(size_t)row * F + cb] & 0xFF) : (int16_t)0;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < RG_SUB; ++r) {
      const short4 a = *reinterpret_cast<const short4*>(&sa[r][ty * 4]);
      const short4 b = *reinterpret_cast<const short4*>(&sb[r][tx * 4]);
      const int av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += av[u] * bv[v];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int a = ta * RG_TILE + ty * 4 + u, b = tb * RG_TILE + tx * 4 + v;
      if (a < F && b < F && acc[u][v] != 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&gram[(size_t)a * F + b]), (unsigned long long)acc[u][v]);
        if (ta != tb) atomicAdd(reinterpret_cast<unsigned long long*>(&gram[(size_t)b * F + a]), (unsigned long long)acc[u][v]);
      }
    }
}

// 32 rows x 64 components per workgroup: thread (row, lane) owns components lane, lane + 8, ... of its row; x = C / size - mean of 64
// columns at a time in LDS beside the matching piece of V.  The accumulators see the columns in ascending order.
constexpr int PJ_ROWS = 32;
constexpr int PJ_COMPS = 64;
constexpr int PJ_FT = 64;

__global__ __launch_bounds__(256) void region_project_kernel(const int16_t* __restrict__ counts, int n, int F, const double* __restrict__ size_col,
                                                             const double* __restrict__ mean, const double* __restrict__ comps, int d,
                                                             double* __restrict__ y) {
  __shared__ double xs[PJ_ROWS][PJ_FT + 1];
  __shared__ double vs[PJ_COMPS][PJ_FT + 1];
  const int tid = threadIdx.x, row = tid >> 3, lane = tid & 7;
  const int i0 = blockIdx.x * PJ_ROWS, j0 = blockIdx.y * PJ_COMPS;
  double acc[PJ_COMPS / 8];
#pragma unroll
  for (int u = 0; u < PJ_COMPS / 8; ++u) acc[u] = 0.0;
  for (int f0 = 0; f0 < F; f0 += PJ_FT) {
    __syncthreads();
    for (int i = tid; i < PJ_ROWS * PJ_FT; i += 256) {
      const int r = i / PJ_FT, c = i % PJ_FT;
      const int gi = i0 + r, f = f0 + c;
      xs[r][c] = (gi < n && f < F) ? (double)counts[(size_t)gi * F + f] / size_col[f] - mean[f] : 0.0;
    }
    for (int i = tid; i < PJ_COMPS * PJ_FT; i += 256) {
      const int j = i / PJ_FT, c = i % PJ_FT;
      const int gj = j0 + j, f = f0 + c;
      vs[j][c] = (gj < d && f < F) ? comps[(size_t)gj * F + f] : 0.0;
    }
    __syncthreads();
    const int lim = F - f0 < PJ_FT ? F - f0 : PJ_FT;
    for (int c = 0; c < lim; ++c) {
      const double x = xs[row][c];
#pragma unroll
      for (int u = 0; u < PJ_COMPS / 8; ++u) acc[u] = acc[u] + x * vs[lane + 8 * u][c];
    }
  }
  const int gi = i0 + row;
  if (gi < n) {
#pragma unroll
    for (int u = 0; u < PJ_COMPS / 8; ++u) {
      const int gj = j0 + lane + 8 * u;
      if (gj < d) y[(size_t)gi * d + gj] = acc[u];
    }
  }
}

// -------------------------------------------------------------------------------------------------------------------------- k-means
// d2 of row q against KM_CT centre rows (row c of the tile = src[rows[c]], rows[c] < 0 = unused): one thread per row, the centres through
// an LDS tile every lane reads at the same address (a broadcast), KM_DT dimensions at a time, partial sums kept across the tiles.
__device__ __forceinline__ void km_dist_tile(const double* __restrict__ y, int n, int d, int q, const double* __restrict__ src, const int (&rows)[KM_CT],
                                             double* cs /* [KM_CT][KM_DT] */, double (&s)[KM_CT]) {
#pragma unroll
  for (int c = 0; c < KM_CT; ++c) s[c] = 0.0;
  for (int f0 = 0; f0 < d; f0 += KM_DT) {
    const int lim = d - f0 < KM_DT ? d - f0 : KM_DT;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < KM_CT; ++c)
      for (int f = threadIdx.x; f < lim; f += KM_THREADS) cs[c * KM_DT + f] = rows[c] >= 0 ? src[(size_t)rows[c] * d + f0 + f] : 0.0;
    __syncthreads();
    if (q < n) {
      const double* yr = y + (size_t)q * d + f0;
      for (int f = 0; f < lim; ++f) {
        const double v = yr[f];
#pragma unroll
        for (int c = 0; c < KM_CT; ++c) {
          const double e = v - cs[c * KM_DT + f];
          s[c] = s[c] + e * e;
        }
      }
    }
  }
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_trials_kernel(const double* __restrict__ y, int n, int d, const int32_t* __restrict__ cand, int L,
                                                                   const double* __restrict__ closest, double* __restrict__ cand_d2) {
  __shared__ double cs[KM_CT * KM_DT];
  const int q = blockIdx.x * KM_THREADS + threadIdx.x;
  int rows[KM_CT];
#pragma unroll
  for (int c = 0; c < KM_CT; ++c) {
    const int r = c < L ? cand[c] : -1;
    rows[c] = (r >= 0 && r < n) ? r : -1;
  }
  double s[KM_CT];
  km_dist_tile(y, n, d, q, y, rows, cs, s);
  if (q >= n) return;
  const double cl = closest ? closest[q] : INFINITY;
#pragma unroll
  for (int c = 0; c < KM_CT; ++c)
    if (c < L) cand_d2[(size_t)c * n + q] = s[c] < cl ? s[c] : cl;      // numpy.minimum on finite values
}

// part[ch * L + t] = rows of chunk ch of candidate t added in ascending order
__global__ __launch_bounds__(64) void kmeans_pot_chunk_kernel(const double* __restrict__ cand_d2, int n, int L, int chunks, double* __restrict__ part) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= L * chunks) return;
  const int t = i / chunks, ch = i % chunks;
  const int r0 = ch * kSumChunk;
  const int r1 = r0 + kSumChunk < n ? r0 + kSumChunk : n;
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s = s + cand_d2[(size_t)t * n + r];
  part[ch * L + t] = s;
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const double* __restrict__ y, int n, int d, const double* __restrict__ centres, int k,
                                                                   int32_t* __restrict__ labels, double* __restrict__ mind2,
                                                                   unsigned* __restrict__ changed) {
  __shared__ double cs[KM_CT * KM_DT];
  const int q = blockIdx.x * KM_THREADS + threadIdx.x;
  double best = INFINITY;
  int bj = 0;      // a row without a comparable distance (NaN) stays in cluster 0: the label is always a valid index
  for (int c0 = 0; c0 < k; c0 += KM_CT) {
    int rows[KM_CT];
#pragma unroll
    for (int c = 0; c < KM_CT; ++c) rows[c] = c0 + c < k ? c0 + c : -1;
    double s[KM_CT];
    km_dist_tile(y, n, d, q, centres, rows, cs, s);
#pragma unroll
    for (int c = 0; c < KM_CT; ++c)
      if (c0 + c < k && s[c] < best) {      // ascending j, strict <: the least (d2, j)
        best = s[c];
        bj = c0 + c;
      }
  }
  if (q >= n) return;
  if (labels[q] != bj) atomicAdd(changed, 1u);
  labels[q] = bj;
  if (mind2) mind2[q] = best;
}

// one workgroup = one chunk of 1024 rows x DT dimensions (DT = blockDim.x, k * DT <= KM_ACC_DOUBLES); thread t owns dimension f of every cluster
__global__ __launch_bounds__(256) void kmeans_partial_kernel(const double* __restrict__ y, int n, int d, const int32_t* __restrict__ labels, int k,
                                                             double* __restrict__ psum /* [chunks][k][d] */, int32_t* __restrict__ pcnt /* [chunks][k] */) {
  __shared__ double acc[KM_ACC_DOUBLES];
  __shared__ int cnt[KM_KMAX];
  const int DT = blockDim.x, t = threadIdx.x;
  const int f = blockIdx.y * DT + t;
  const int ch = blockIdx.x;
  const int r0 = ch * kSumChunk;
  const int r1 = r0 + kSumChunk < n ? r0 + kSumChunk : n;
  for (int c = 0; c < k; ++c) acc[c * DT + t] = 0.0;
  const bool counter = blockIdx.y == 0 && t == 0;
  if (counter)
    for (int c = 0; c < k; ++c) cnt[c] = 0;
  if (f < d) {
    for (int r = r0; r < r1; ++r) {
      const int c = labels[r];
      if ((unsigned)c >= (unsigned)k) continue;
      acc[c * DT + t] = acc[c * DT + t] + y[(size_t)r * d + f];
      if (counter) cnt[c] += 1;
    }
    for (int c = 0; c < k; ++c) psum[((size_t)ch * k + c) * d + f] = acc[c * DT + t];
  }
  if (counter)
    for (int c = 0; c < k; ++c) pcnt[(size_t)ch * k + c] = cnt[c];
}

// one workgroup per centre.  stat: [0] labels changed, [1 .. k] counts, [1 + k .. 1 + 2 k) squared shift of every centre (all as fp64)
__global__ __launch_bounds__(256) void kmeans_finalize_kernel(const double* __restrict__ sums, const int32_t* __restrict__ counts, int k, int d,
                                                              const double* __restrict__ old, double* __restrict__ out, const unsigned* __restrict__ changed,
                                                              double* __restrict__ stat) {
  __shared__ double sq[256];
  const int c = blockIdx.x, t = threadIdx.x;
  const int cnt = counts[c];
  double shift = 0.0;
  for (int f0 = 0; f0 < d; f0 += 256) {
    const int f = f0 + t;
    __syncthreads();
    if (f < d) {
      const double o = old[(size_t)c * d + f];
      const double v = cnt > 0 ? sums[(size_t)c * d + f] / (double)cnt : o;
      out[(size_t)c * d + f] = v;
      const double e = v - o;
      sq[t] = e * e;
    }
    __syncthreads();
    if (t == 0) {
      const int lim = d - f0 < 256 ? d - f0 : 256;
      for (int i = 0; i < lim; ++i) shift = shift + sq[i];
    }
  }
  if (t == 0) {
    stat[1 + c] = (double)cnt;
    stat[1 + k + c] = shift;
    if (c == 0) stat[0] = changed ? (double)changed[0] : 0.0;
  }
}

// scikit-learn's _relocate_empty_clusters_dense on the sums: for m = 0 .. n_empty - 1 in order, row far[m] leaves the sum of its cluster and
// becomes the whole sum of empty cluster empty[m].  One workgroup; a thread owns a dimension, so the order of the m is kept.
__global__ __launch_bounds__(256) void kmeans_relocate_kernel(const double* __restrict__ y, int n, int d, int k, const int32_t* __restrict__ labels,
                                                              const int32_t* __restrict__ far, const int32_t* __restrict__ empty, int m_count,
                                                              double* __restrict__ sums, int32_t* __restrict__ counts) {
  for (int m = 0; m < m_count; ++m) {
    const int row = far[m], dst = empty[m];
    if (row < 0 || row >= n || dst < 0 || dst >= k) continue;
    const int src = labels[row];
    if (src < 0 || src >= k) continue;
    for (int f = threadIdx.x; f < d; f += 256) {
      const double v = y[(size_t)row * d + f];
      sums[(size_t)src * d + f] = sums[(size_t)src * d + f] - v;
      sums[(size_t)dst * d + f] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      counts[dst] = 1;
      counts[src] -= 1;
    }
    __syncthreads();
  }
}

int km_partial_threads(int k) {
  int dt = 256;
  while (dt > 16 && k * dt > KM_ACC_DOUBLES) dt >>= 1;
  return dt;
}

const char* km_range(int n, int d, int k) {
  if (n < 1) return "needs n >= 1";
  if (d < 1 || d > RG_FMAX) return "needs 1 <= d <= 2032";
  if (k < 1 || k > KM_KMAX) return "needs 1 <= k <= 256";
  if (k > n) return "needs k <= n";
  return nullptr;
}

int km_fail(const char* name, const char* why) {
  char buf[160];
  snprintf(buf, sizeof(buf), "%s: %s", name, why);
  return api_fail(buf);
}

// the workspace of ribca_kmeans_update: the per-chunk centre sums and counts of kmeans_partial_kernel
struct KmUpdateWs {
  double* psum;       // [chunks][k][d]
  int32_t* pcnt;      // [chunks][k]
};

KmUpdateWs carve_kmeans_update(Carver& c, int n, int d, int k) {
  const size_t chunks = chunks_of(n);
  KmUpdateWs w;
  w.psum = c.take<double>(chunks * k * d);
  w.pcnt = c.take<int32_t>(chunks * k);
  return w;
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_region_gram_ws_bytes(int32_t n, int32_t F) { return (n < 1 || F < 1 || F > RG_FMAX) ? 0 : 256; }      // the range flag

int ribca_region_gram(const int16_t* counts, int32_t n, int32_t F, int64_t* colsum, int64_t* gram, void* ws, int64_t ws_bytes, void* stream) {
  if (!counts || !colsum || !gram || !ws) return fail("ribca_region_gram: NULL buffer");
  if (n < 1) return fail("ribca_region_gram: needs n >= 1");
  if (F < 1 || F > RG_FMAX) return fail("ribca_region_gram: needs 1 <= F <= 2032");
  if (ws_bytes < ribca_region_gram_ws_bytes(n, F)) return fail("ribca_region_gram: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned* flag = static_cast<unsigned*>(ws);
  HIP_TRY(hipMemsetAsync(flag, 0, 256, s));
  HIP_TRY(hipMemsetAsync(colsum, 0, sizeof(int64_t) * (size_t)F, s));
  HIP_TRY(hipMemsetAsync(gram, 0, sizeof(int64_t) * (size_t)F * F, s));
  const int chunks = chunks_of(n), tiles = (F + RG_TILE - 1) / RG_TILE;
  hipLaunchKernelGGL(region_colsum_kernel, dim3((F + 255) / 256, chunks), dim3(256), 0, s, counts, n, F, reinterpret_cast<long long*>(colsum), flag);
  hipLaunchKernelGGL(region_gram_kernel, dim3(tiles * (tiles + 1) / 2, chunks), dim3(256), 0, s, counts, n, F, tiles,
                     reinterpret_cast<long long*>(gram));
  RIBCA_FINISH();
  unsigned host = 0;
  HIP_TRY(hipMemcpyAsync(&host, flag, sizeof(host), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (host) return fail("ribca_region_gram: a count lies outside 0 .. 255");
  return 0;
}

int ribca_region_project(const int16_t* counts, int32_t n, int32_t F, const double* size_col, const double* mean, const double* comps, int32_t d,
                         double* y, void* stream) {
  if (!counts || !size_col || !mean || !comps || !y) return fail("ribca_region_project: NULL buffer");
  if (n < 1) return fail("ribca_region_project: needs n >= 1");
  if (F < 1 || F > RG_FMAX) return fail("ribca_region_project: needs 1 <= F <= 2032");
  if (d < 1 || d > F) return fail("ribca_region_project: needs 1 <= d <= F");
  hipLaunchKernelGGL(region_project_kernel, dim3((n + PJ_ROWS - 1) / PJ_ROWS, (d + PJ_COMPS - 1) / PJ_COMPS), dim3(256), 0, (hipStream_t)stream, counts,
                     n, F, size_col, mean, comps, d, y);
  RIBCA_FINISH();
  return 0;
}

int64_t ribca_kmeans_trials_ws_bytes(int32_t n, int32_t n_cand) {      // one fp64 partial potential per (chunk, candidate)
  if (n < 1 || n_cand < 1 || n_cand > KM_CT) return 0;
  return (int64_t)sizeof(double) * n_cand * chunks_of(n);
}

int ribca_kmeans_trials(const double* y, int32_t n, int32_t d, const int32_t* cand, int32_t n_cand, const double* closest, double* cand_d2,
                        double* pot, void* ws, int64_t ws_bytes, void* stream) {
  if (!y || !cand || !cand_d2 || !pot || !ws) return fail("ribca_kmeans_trials: NULL buffer");
  if (const char* why = km_range(n, d, 1)) return km_fail("ribca_kmeans_trials", why);
  if (n_cand < 1 || n_cand > KM_CT) return fail("ribca_kmeans_trials: needs 1 <= n_cand <= 8");
  if (ws_bytes < ribca_kmeans_trials_ws_bytes(n, n_cand)) return fail("ribca_kmeans_trials: workspace too small");
  const int chunks = chunks_of(n);
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(kmeans_trials_kernel, dim3((n + KM_THREADS - 1) / KM_THREADS), dim3(KM_THREADS), 0, s, y, n, d, cand, n_cand, closest, cand_d2);
  hipLaunchKernelGGL(kmeans_pot_chunk_kernel, dim3((n_cand * chunks + 63) / 64), dim3(64), 0, s, cand_d2, n, n_cand, chunks, part);
  launch_chunk_total(part, chunks, n_cand, pot, s);
  RIBCA_FINISH();
  return 0;
}

int ribca_kmeans_assign(const double* y, int32_t n, int32_t d, const double* centres, int32_t k, int32_t* labels, double* mind2, uint32_t* changed,
                        void* stream) {
  if (!y || !centres || !labels || !changed) return fail("ribca_kmeans_assign: NULL buffer");
  if (const char* why = km_range(n, d, k)) return km_fail("ribca_kmeans_assign", why);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(changed, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3((n + KM_THREADS - 1) / KM_THREADS), dim3(KM_THREADS), 0, s, y, n, d, centres, k, labels, mind2, changed);
  RIBCA_FINISH();
  return 0;
}

int64_t ribca_kmeans_update_ws_bytes(int32_t n, int32_t d, int32_t k) {
  if (km_range(n, d, k)) return 0;
  Carver c(nullptr);
  carve_kmeans_update(c, n, d, k);
  return (int64_t)c.off;
}

int ribca_kmeans_finalize(const double* sums, const int32_t* counts, int32_t k, int32_t d, const double* centres_old, double* centres_new,
                          const uint32_t* changed, double* stat, void* stream) {
  if (!sums || !counts || !centres_old || !centres_new || !stat) return fail("ribca_kmeans_finalize: NULL buffer");
  if (const char* why = km_range(k, d, k)) return km_fail("ribca_kmeans_finalize", why);
  hipLaunchKernelGGL(kmeans_finalize_kernel, dim3(k), dim3(256), 0, (hipStream_t)stream, sums, counts, k, d, centres_old, centres_new, changed, stat);
  RIBCA_FINISH();
  return 0;
}

int ribca_kmeans_update(const double* y, int32_t n, int32_t d, const int32_t* labels, int32_t k, const double* centres_old, double* centres_new,
                        double* sums, int32_t* counts, const uint32_t* changed, double* stat, void* ws, int64_t ws_bytes, void* stream) {
  if (!y || !labels || !centres_old || !centres_new || !sums || !counts || !stat || !ws) return fail("ribca_kmeans_update: NULL buffer");
  if (const char* why = km_range(n, d, k)) return km_fail("ribca_kmeans_update", why);
  if (ws_bytes < ribca_kmeans_update_ws_bytes(n, d, k)) return fail("ribca_kmeans_update: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int chunks = chunks_of(n);
  Carver c(ws);
  const KmUpdateWs w = carve_kmeans_update(c, n, d, k);
  const int dt = km_partial_threads(k);
  hipLaunchKernelGGL(kmeans_partial_kernel, dim3(chunks, (d + dt - 1) / dt), dim3(dt), 0, s, y, n, d, labels, k, w.psum, w.pcnt);
  launch_chunk_total(w.psum, chunks, k * d, sums, s, w.pcnt, k, counts);
  RIBCA_FINISH();
  return ribca_kmeans_finalize(sums, counts, k, d, centres_old, centres_new, changed, stat, stream);
}

int ribca_kmeans_relocate(const double* y, int32_t n, int32_t d, int32_t k, const int32_t* labels, const int32_t* far_rows, const int32_t* empty_ids,
                          int32_t n_empty, double* sums, int32_t* counts, void* stream) {
  if (!y || !labels || !far_rows || !empty_ids || !sums || !counts) return fail("ribca_kmeans_relocate: NULL buffer");
  if (const char* why = km_range(n, d, k)) return km_fail("ribca_kmeans_relocate", why);
  if (n_empty < 1 || n_empty >= k) return fail("ribca_kmeans_relocate: needs 1 <= n_empty < k");
  hipLaunchKernelGGL(kmeans_relocate_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, y, n, d, k, labels, far_rows, empty_ids, n_empty, sums, counts);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
