// The numeric core of the "extra cell types" step (reference Annotator._find_extra_cell_types, model.py:642-675): umap-learn 0.5's
// fit_transform restated for the GPU -- exact k-NN in marker space, the fuzzy membership weights of every neighbour, and the layout SGD
// (optimize_layout_euclidean with move_other).  The graph union and the spectral start stay on the host (manifold.py); HDBSCAN's O(n^2) part is hdbscan.hip.
//
// knn_dense: one thread per query row, candidate rows streamed through LDS tiles that every lane reads at the same address (a broadcast:
//   no bank conflicts), the KM best (distance, index) pairs kept sorted in registers as in knn.hip.  Distances are fp32 sums of squared
//   differences in dimension order, no fma contraction, no |x|^2 + |y|^2 - 2 x.y expansion.  dim <= 64: the query row lives in registers
//   (padded with zeros to DP: (0 - 0)^2 adds an exact +0); 64 < dim <= 256: in LDS, one row per lane at an odd stride (conflict-free).
// fuzzy_weights: umap's smooth_knn_dist + compute_membership_strengths, one thread per row; the global-mean floor of rows without a
//   positive distance is applied afterwards by one workgroup that also computes that mean (fixed order: deterministic).
// optimize: a Jacobi epoch -- every vertex sums the forces of its out-edges (attraction + negative samples) and the move_other terms of
//   its in-edges in a fixed order into registers, then a second kernel moves the vertices and advances the sampling state.  No atomics;
//   the negative samples come from a counter-based hash of (seed, epoch, edge, sample).  Same input, same bits.
#include <cmath>

#include "ribca_common.h"
#include "ribca_kernels.h"
#include "ribca_scratch.h"

// every sum and product below rounds on its own (HIP contracts a * b + c into an fma by default): the distances and forces are the ones
// a plain numpy restatement computes
#pragma clang fp contract(off)

namespace ribca {

// ----------------------------------------------------------------------------------------------------------------- exact k-NN
constexpr int KD_THREADS = 256;      // register form
constexpr int KD_LDS_THREADS = 64;   // LDS form (dim > 64): 64 query rows of <= 257 floats
constexpr int KD_LDS_TILE = 16;      // candidate rows per LDS tile of the LDS form

__device__ __forceinline__ bool kd_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

template <int KM>
__device__ __forceinline__ void kd_insert(float (&bd)[KM], int (&bi)[KM], float d, int j) {
  if (!kd_less(d, j, bd[KM - 1], bi[KM - 1])) return;
  bd[KM - 1] = d;
  bi[KM - 1] = j;
#pragma unroll
  for (int p = KM - 1; p >= 1; --p) {
    if (kd_less(bd[p], bi[p], bd[p - 1], bi[p - 1])) {
      const float td = bd[p]; bd[p] = bd[p - 1]; bd[p - 1] = td;
      const int ti = bi[p]; bi[p] = bi[p - 1]; bi[p - 1] = ti;
    }
  }
}

template <int KM>
__device__ __forceinline__ void kd_store(const float (&bd)[KM], const int (&bi)[KM], int q, int k, int32_t* idx, float* dist) {
#pragma unroll
  for (int p = 0; p < KM; ++p)
    if (p < k) {
      idx[(size_t)q * k + p] = bi[p];
      dist[(size_t)q * k + p] = sqrtf(bd[p]);
    }
}

// DP: padded dimension (16, 32, 64); tile rows sized so the tile is 16 KiB
template <int DP, int KM>
__global__ __launch_bounds__(KD_THREADS) void knn_dense_reg_kernel(const float* __restrict__ x, int n, int dim, int k,
                                                                   int32_t* __restrict__ idx, float* __restrict__ dist) {
  constexpr int TILE = 4096 / DP;
  __shared__ float4 tile[TILE * DP / 4];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * KD_THREADS + tid;
  float qv[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) qv[d] = (q < n && d < dim) ? x[(size_t)q * dim + d] : 0.f;
  float bd[KM];
  int bi[KM];
#pragma unroll
  for (int p = 0; p < KM; ++p) { bd[p] = INFINITY; bi[p] = 0x7FFFFFFF; }
  float* tf = reinterpret_cast<float*>(tile);
  for (int base = 0; base < n; base += TILE) {
    __syncthreads();
    for (int i = tid; i < TILE * DP; i += KD_THREADS) {
      const int r = i / DP, d = i % DP;
      const int j = base + r;
      tf[i] = (j < n && d < dim) ? x[(size_t)j * dim + d] : 0.f;
    }
    __syncthreads();
    const int lim = n - base < TILE ? n - base : TILE;
    if (q < n) {
      for (int i = 0; i < lim; ++i) {
        float s = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < DP / 4; ++d4) {
          const float4 c = tile[i * (DP / 4) + d4];      // same address in every lane: broadcast
          const float e0 = c.x - qv[4 * d4], e1 = c.y - qv[4 * d4 + 1], e2 = c.z - qv[4 * d4 + 2], e3 = c.w - qv[4 * d4 + 3];
          s = s + e0 * e0;
          s = s + e1 * e1;
          s = s + e2 * e2;
          s = s + e3 * e3;
        }
        kd_insert<KM>(bd, bi, s, base + i);
      }
    }
  }
  if (q < n) kd_store<KM>(bd, bi, q, k, idx, dist);
}

template <int KM>
__global__ __launch_bounds__(KD_LDS_THREADS) void knn_dense_lds_kernel(const float* __restrict__ x, int n, int dim, int k,
                                                                       int32_t* __restrict__ idx, float* __restrict__ dist) {
  constexpr int DMAX = 256;
  __shared__ float sq[KD_LDS_THREADS * (DMAX + 1)];
  __shared__ float tile[KD_LDS_TILE * DMAX];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * KD_LDS_THREADS + tid;
  const int stride = dim | 1;      // odd: lane l reads bank (l * stride + d) mod 32, distinct over any 32 lanes
  const int q0 = blockIdx.x * KD_LDS_THREADS;
  for (int i = tid; i < KD_LDS_THREADS * dim; i += KD_LDS_THREADS) {
    const int r = i / dim, d = i % dim;
    sq[r * stride + d] = q0 + r < n ? x[(size_t)(q0 + r) * dim + d] : 0.f;
  }
  float bd[KM];
  int bi[KM];
#pragma unroll
  for (int p = 0; p < KM; ++p) { bd[p] = INFINITY; bi[p] = 0x7FFFFFFF; }
  const float* qrow = sq + tid * stride;
  for (int base = 0; base < n; base += KD_LDS_TILE) {
    __syncthreads();
    for (int i = tid; i < KD_LDS_TILE * dim; i += KD_LDS_THREADS) {
      const int j = base + i / dim;
      tile[i] = j < n ? x[(size_t)base * dim + i] : 0.f;
    }
    __syncthreads();
    const int lim = n - base < KD_LDS_TILE ? n - base : KD_LDS_TILE;
    if (q < n) {
      for (int i = 0; i < lim; ++i) {
        const float* c = tile + i * dim;      // broadcast
        float s = 0.f;
        for (int d = 0; d < dim; ++d) {
          const float e = c[d] - qrow[d];
          s = s + e * e;
        }
        kd_insert<KM>(bd, bi, s, base + i);
      }
    }
  }
  if (q < n) kd_store<KM>(bd, bi, q, k, idx, dist);
}

template <int KM>
static void launch_knn_dense_km(const float* x, int n, int dim, int k, int32_t* idx, float* dist, hipStream_t s) {
  const dim3 g((n + KD_THREADS - 1) / KD_THREADS), b(KD_THREADS);
  if (dim <= 16) hipLaunchKernelGGL((knn_dense_reg_kernel<16, KM>), g, b, 0, s, x, n, dim, k, idx, dist);
  else if (dim <= 32) hipLaunchKernelGGL((knn_dense_reg_kernel<32, KM>), g, b, 0, s, x, n, dim, k, idx, dist);
  else if (dim <= 64) hipLaunchKernelGGL((knn_dense_reg_kernel<64, KM>), g, b, 0, s, x, n, dim, k, idx, dist);
  else hipLaunchKernelGGL((knn_dense_lds_kernel<KM>), dim3((n + KD_LDS_THREADS - 1) / KD_LDS_THREADS), dim3(KD_LDS_THREADS), 0, s, x, n, dim, k,
                          idx, dist);
}

int launch_knn_dense(const float* x, int n, int dim, int k, int32_t* idx, float* dist, hipStream_t s) {
  if (n < 1 || k < 1 || k > n || k > 64 || dim < 1 || dim > 256) return 1;
  if (k <= 16) launch_knn_dense_km<16>(x, n, dim, k, idx, dist, s);
  else launch_knn_dense_km<64>(x, n, dim, k, idx, dist, s);
  return 0;
}

// ------------------------------------------------------------------------------------------------------- fuzzy membership weights
constexpr double SMOOTH_K_TOLERANCE = 1e-5;
constexpr double MIN_K_DIST_SCALE = 1e-3;

__device__ __forceinline__ void fuzzy_row_weights(const int32_t* idx, const float* dist, int row, int k, float sigma, float rho, float* w) {
  for (int j = 0; j < k; ++j) {
    const size_t e = (size_t)row * k + j;
    const float d = dist[e] - rho;
    float v;
    if (idx[e] == row) v = 0.f;
    else if (d <= 0.f || sigma == 0.f) v = 1.f;
    else v = expf(-(d / sigma));
    w[e] = v;
  }
}

__global__ __launch_bounds__(256) void fuzzy_weights_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist, int n, int k,
                                                            float* __restrict__ sigma, float* __restrict__ rho_out, float* __restrict__ w) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const float* di = dist + (size_t)row * k;
  // rho: the first positive distance (local_connectivity = 1, the row is sorted ascending)
  float rho = 0.f;
  for (int j = 0; j < k; ++j)
    if (di[j] > 0.f) { rho = di[j]; break; }
  const double target = log2((double)k);      // bandwidth 1
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int it = 0; it < 64; ++it) {
    double psum = 0.0;
    for (int j = 1; j < k; ++j) {
      const float d = di[j] - rho;
      psum += d > 0.f ? exp(-((double)d / mid)) : 1.0;
    }
    if (fabs(psum - target) < SMOOTH_K_TOLERANCE) break;
    if (psum > target) {
      hi = mid;
      mid = (lo + hi) / 2.0;
    } else {
      lo = mid;
      mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
    }
  }
  float sg = (float)mid;
  if (rho > 0.f) {      // floor at the row mean; rows without a positive distance get the global-mean floor in fuzzy_floor_kernel
    double m = 0.0;
    for (int j = 0; j < k; ++j) m += (double)di[j];
    m /= (double)k;
    if ((double)sg < MIN_K_DIST_SCALE * m) sg = (float)(MIN_K_DIST_SCALE * m);
  }
  sigma[row] = sg;
  rho_out[row] = rho;
  fuzzy_row_weights(idx, dist, row, k, sg, rho, w);
}

// one workgroup: the mean of all n * k distances (fp64, fixed summation order), then the floor of the rows whose rho is 0
__global__ __launch_bounds__(1024) void fuzzy_floor_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist, int n, int k,
                                                           float* __restrict__ sigma, const float* __restrict__ rho, float* __restrict__ w) {
  __shared__ double part[1024];
  const int tid = threadIdx.x;
  const size_t total = (size_t)n * k;
  double s = 0.0;
  for (size_t i = tid; i < total; i += 1024) s += (double)dist[i];
  part[tid] = s;
  for (int h = 512; h > 0; h >>= 1) {
    __syncthreads();
    if (tid < h) part[tid] += part[tid + h];
  }
  __syncthreads();
  const double floor_v = MIN_K_DIST_SCALE * (part[0] / (double)total);
  for (int row = tid; row < n; row += 1024) {
    if (rho[row] > 0.f || (double)sigma[row] >= floor_v) continue;
    const float sg = (float)floor_v;
    sigma[row] = sg;
    fuzzy_row_weights(idx, dist, row, k, sg, rho[row], w);
  }
}

int launch_umap_fuzzy_weights(const int32_t* idx, const float* dist, int n, int k, float* sigma, float* rho, float* w, hipStream_t s) {
  if (n < 1 || k < 2 || k > 64) return 1;
  hipLaunchKernelGGL(fuzzy_weights_kernel, dim3((n + 255) / 256), dim3(256), 0, s, idx, dist, n, k, sigma, rho, w);
  hipLaunchKernelGGL(fuzzy_floor_kernel, dim3(1), dim3(1024), 0, s, idx, dist, n, k, sigma, rho, w);
  return 0;
}

// ----------------------------------------------------------------------------------------------------------------- layout SGD
constexpr int UMAP_DMAX = 8;

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// negative sample p of edge e in epoch n: the top 32 bits of splitmix64(splitmix64(splitmix64(splitmix64(seed) ^ n) ^ e) ^ p) mod n_vertices
__device__ __forceinline__ int neg_sample(uint64_t epoch_key, int64_t e, int p, int nv) {
  const uint64_t h = splitmix64(splitmix64(epoch_key ^ (uint64_t)e) ^ (uint64_t)p);
  return (int)((uint32_t)(h >> 32) % (uint32_t)nv);
}

// -2ab d^(b-1) / (1 + a d^b) of the squared distance d, with d^b = exp(b log d) and d^(b-1) = d^b / d; 0 at d = 0
__device__ __noinline__ double attract_coeff(double dd, double a, double b) {
  if (!(dd > 0.0)) return 0.0;
  const double pb = exp(b * log(dd));
  return -2.0 * a * b * (pb / dd) / (a * pb + 1.0);
}

// 2 gamma b / ((0.001 + d) (1 + a d^b)) for d > 0
__device__ __noinline__ double repulse_coeff(double dd, double a, double b, double gamma) {
  return 2.0 * gamma * b / ((0.001 + dd) * (a * exp(b * log(dd)) + 1.0));
}

__device__ __forceinline__ double clip4(double v) { return v > 4.0 ? 4.0 : (v < -4.0 ? -4.0 : v); }

// squared distance: fp32 sum in dimension order, no contraction
__device__ __forceinline__ float rdist(const float (&a)[UMAP_DMAX], const float* __restrict__ other, int dim, float (&o)[UMAP_DMAX]) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < UMAP_DMAX; ++d)
    if (d < dim) {
      o[d] = other[d];
      const float e = a[d] - o[d];
      s = s + e * e;
    }
  return s;
}

struct UmapArgs {
  float* emb;
  int n, dim;
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* rev;
  const double* eps;      // epochs_per_sample per edge
  double a, b, gamma, neg_rate;
  uint64_t seed_key;
  double* next_sample;    // epoch_of_next_sample per edge
  double* next_neg;       // epoch_of_next_negative_sample per edge
  float* new_emb;         // (n, dim): the positions after the epoch
};

__global__ __launch_bounds__(256) void umap_forces_kernel(UmapArgs u, int epoch, double alpha) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= u.n) return;
  const int dim = u.dim;
  const double a = u.a, b = u.b;
  const double fe = (double)epoch;
  const uint64_t epoch_key = splitmix64(u.seed_key ^ (uint64_t)epoch);
  float cur[UMAP_DMAX], oth[UMAP_DMAX];
  double acc[UMAP_DMAX];
#pragma unroll
  for (int d = 0; d < UMAP_DMAX; ++d) {
    cur[d] = d < dim ? u.emb[(size_t)v * dim + d] : 0.f;
    oth[d] = 0.f;
    acc[d] = 0.0;
  }
  const int64_t e0 = u.indptr[v], e1 = u.indptr[v + 1];
  // 1. out-edges (v -> k) in CSR order, each followed by its negative samples
  for (int64_t e = e0; e < e1; ++e) {
    if (u.next_sample[e] > fe) continue;
    const int k = u.indices[e];
    const float d2 = rdist(cur, u.emb + (size_t)k * dim, dim, oth);
    const double g = attract_coeff((double)d2, a, b);
#pragma unroll
    for (int d = 0; d < UMAP_DMAX; ++d)
      if (d < dim) acc[d] += clip4(g * (double)(cur[d] - oth[d])) * alpha;
    const double epsn = u.eps[e] / u.neg_rate;
    const int n_neg = (int)((fe - u.next_neg[e]) / epsn);
    for (int p = 0; p < n_neg; ++p) {
      const int j = neg_sample(epoch_key, e, p, u.n);
      if (j == v) continue;
      const float s2 = rdist(cur, u.emb + (size_t)j * dim, dim, oth);
      if (!(s2 > 0.f)) continue;      // a coincident point: zero force
      const double dd = (double)s2;
      const double gr = repulse_coeff(dd, a, b, u.gamma);
#pragma unroll
      for (int d = 0; d < UMAP_DMAX; ++d)
        if (d < dim) acc[d] += clip4(gr * (double)(cur[d] - oth[d])) * alpha;
    }
  }
  // 2. move_other: the in-edges (k -> v), reached through rev, in the CSR order of v's row
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t r = u.rev[e];
    if (u.next_sample[r] > fe) continue;
    const int k = u.indices[e];
    const float d2 = rdist(cur, u.emb + (size_t)k * dim, dim, oth);
    const double g = attract_coeff((double)d2, a, b);
    // the head k moved by clip(g (x_k - x_v)) alpha, the tail v by its negative
#pragma unroll
    for (int d = 0; d < UMAP_DMAX; ++d)
      if (d < dim) acc[d] -= clip4(g * (double)(oth[d] - cur[d])) * alpha;
  }
#pragma unroll
  for (int d = 0; d < UMAP_DMAX; ++d)
    if (d < dim) u.new_emb[(size_t)v * dim + d] = (float)((double)cur[d] + acc[d]);
}

// moves the vertices and advances the sampling state of the edges of row v
__global__ __launch_bounds__(256) void umap_apply_kernel(UmapArgs u, int epoch) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= u.n) return;
  const double fe = (double)epoch;
  for (int d = 0; d < u.dim; ++d) u.emb[(size_t)v * u.dim + d] = u.new_emb[(size_t)v * u.dim + d];
  for (int64_t e = u.indptr[v]; e < u.indptr[v + 1]; ++e) {
    if (u.next_sample[e] > fe) continue;
    u.next_sample[e] += u.eps[e];
    const double epsn = u.eps[e] / u.neg_rate;
    const int n_neg = (int)((fe - u.next_neg[e]) / epsn);
    u.next_neg[e] += (double)n_neg * epsn;
  }
}

__global__ void umap_init_state_kernel(const double* __restrict__ eps, int64_t nnz, double neg_rate, double* __restrict__ next_sample,
                                       double* __restrict__ next_neg) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  next_sample[e] = eps[e];
  next_neg[e] = eps[e] / neg_rate;
}

// the workspace of launch_umap_optimize: the scratch members of UmapArgs
struct UmapWs {
  double *next_sample, *next_neg;
  float* new_emb;
};

UmapWs carve_umap_ws(Carver& c, int n, int dim, int64_t nnz) {
  UmapWs w;
  w.next_sample = c.take<double>(nnz);
  w.next_neg = c.take<double>(nnz);
  w.new_emb = c.take<float>((size_t)n * dim);
  return w;
}

int64_t umap_optimize_ws_bytes(int n, int dim, int64_t nnz) {
  if (n < 1 || dim < 1 || dim > UMAP_DMAX || nnz < 0) return 0;
  Carver c(nullptr);
  carve_umap_ws(c, n, dim, nnz);
  return (int64_t)c.off;
}

int launch_umap_optimize(float* emb, int n, int dim, const int64_t* indptr, const int32_t* indices, const int64_t* rev, const double* eps,
                         int64_t nnz, double a, double b, double gamma, double alpha0, double neg_rate, int n_epochs, uint64_t seed, void* ws,
                         hipStream_t s) {
  if (n < 1 || dim < 1 || dim > UMAP_DMAX || n_epochs < 0 || nnz < 0 || !(neg_rate > 0.0)) return 1;
  Carver c(ws);
  const UmapWs w = carve_umap_ws(c, n, dim, nnz);
  UmapArgs u;
  u.next_sample = w.next_sample; u.next_neg = w.next_neg; u.new_emb = w.new_emb;
  u.emb = emb; u.n = n; u.dim = dim; u.indptr = indptr; u.indices = indices; u.rev = rev; u.eps = eps;
  u.a = a; u.b = b; u.gamma = gamma; u.neg_rate = neg_rate;
  // host mirror of splitmix64 for the seed key
  uint64_t z = seed + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  u.seed_key = z ^ (z >> 31);
  if (nnz > 0)
    hipLaunchKernelGGL(umap_init_state_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, s, eps, nnz, neg_rate, u.next_sample, u.next_neg);
  const dim3 g((n + 255) / 256), bl(256);
  for (int ep = 0; ep < n_epochs; ++ep) {
    const double alpha = alpha0 * (1.0 - (double)ep / (double)n_epochs);
    hipLaunchKernelGGL(umap_forces_kernel, g, bl, 0, s, u, ep, alpha);
    hipLaunchKernelGGL(umap_apply_kernel, g, bl, 0, s, u, ep);
  }
  return 0;
}

}  // namespace ribca
