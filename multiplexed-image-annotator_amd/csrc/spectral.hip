// The spectral start of the UMAP embedding on the GPU (manifold.spectral_component_gpu; umap's spectral_layout, which hands the normalised
// Laplacian to ARPACK on the host): the three operations of a block eigensolver that touch all n rows.  DESIGN.md section 12 states the
// arithmetic; tests/spectral_numpy.py reproduces it bit for bit with numpy loops.  Everything is fp64, every product and sum rounds on its
// own (no fma contraction), no float atomics, no kernel waits for another.
//
//   spectral_spmm     Y = alpha (S X) + beta X + gamma Z with S = D^-1/2 A D^-1/2, A symmetric canonical CSR (the graph ribca_umap_optimize
//                     takes).  One thread per (row, column) of Y: (S X)[i, c] is ONE sequential sum over the entries e of row i in CSR order
//                     of ((dinv[i] * (double) w[e]) * dinv[j_e]) * X[j_e, c], started at 0.  The lanes of a row read the m columns of X[j_e, :]
//                     side by side (one coalesced piece per entry) and the entry itself from the same cache line; a row holds about 21
//                     entries, so no row needs more than its own thread per column.  An entry whose column lies outside [0, n) is skipped.
//   spectral_gram     G = U^T V.  THE summation order: rows in chunks of 1024; per chunk and output (a, b) the rows added in ascending order,
//                     started at 0 (one workgroup per chunk, an output per thread and 256-step, rows through LDS); then the chunks added in
//                     ascending order, started at 0.  The same order as the fixed-order sums of regions.hip.
//   spectral_combine  X[i, c] = (X[i, c] if add else 0) + sum over k ascending of U[i, k] * C[k, c]; C through LDS.
#include <cmath>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

#pragma clang fp contract(off)

namespace ribca {
namespace {

constexpr int SP_SUB = 16;          // rows staged in LDS at a time
constexpr int SP_PMAX = 48;         // widest block of the Gram / combine kernels
constexpr int SP_MMAX = 16;         // widest block of the SpMM
constexpr int SP_OUT = (SP_PMAX * SP_PMAX + 255) / 256;      // Gram outputs per thread

int fail(const char* msg) { return api_fail(msg); }

__global__ __launch_bounds__(256) void spectral_spmm_kernel(const long long* __restrict__ indptr, const int* __restrict__ indices,
                                                            const float* __restrict__ w, long long nnz, const double* __restrict__ dinv, int n, int m,
                                                            const double* __restrict__ x, double alpha, double beta, double gamma,
                                                            const double* z, double* y) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * m) return;
  const int i = (int)(t / m), c = (int)(t % m);
  long long e0 = indptr[i], e1 = indptr[i + 1];
  if (e0 < 0) e0 = 0;
  if (e1 > nnz) e1 = nnz;
  const double di = dinv[i];
  double acc = 0.0;
  for (long long e = e0; e < e1; ++e) {
    const int j = indices[e];
    if ((unsigned)j >= (unsigned)n) continue;
    const double coef = (di * (double)w[e]) * dinv[j];
    acc = acc + coef * x[(size_t)j * m + c];
  }
  double v = alpha * acc;
  if (beta != 0.0) v = v + beta * x[t];
  if (z) v = v + gamma * z[t];      // z may be y itself: this thread alone reads and writes element t
  y[t] = v;
}

__global__ __launch_bounds__(256) void spectral_gram_chunk_kernel(const double* __restrict__ u, const double* __restrict__ v, int n, int p, int q,
                                                                  double* __restrict__ part) {
  __shared__ double us[SP_SUB * SP_PMAX];
  __shared__ double vs[SP_SUB * SP_PMAX];
  const int tid = threadIdx.x, pq = p * q;
  const int r0 = blockIdx.x * kSumChunk;
  const int r1 = r0 + kSumChunk < n ? r0 + kSumChunk : n;
  int ia[SP_OUT], ib[SP_OUT];
  double acc[SP_OUT];
#pragma unroll
  for (int k = 0; k < SP_OUT; ++k) {
    const int o = tid + 256 * k < pq ? tid + 256 * k : pq - 1;      // an unused slot recomputes the last output and is not stored
    ia[k] = o / q;
    ib[k] = o % q;
    acc[k] = 0.0;
  }
  for (int base = r0; base < r1; base += SP_SUB) {
    const int lim = r1 - base < SP_SUB ? r1 - base : SP_SUB;
    __syncthreads();
    for (int i = tid; i < lim * p; i += 256) us[i] = u[(size_t)base * p + i];
    for (int i = tid; i < lim * q; i += 256) vs[i] = v[(size_t)base * q + i];
    __syncthreads();
    for (int r = 0; r < lim; ++r) {
#pragma unroll
      for (int k = 0; k < SP_OUT; ++k)
        if (256 * k < pq) acc[k] = acc[k] + us[r * p + ia[k]] * vs[r * q + ib[k]];
    }
  }
#pragma unroll
  for (int k = 0; k < SP_OUT; ++k)
    if (tid + 256 * k < pq) part[(size_t)blockIdx.x * pq + tid + 256 * k] = acc[k];
}

__global__ __launch_bounds__(256) void spectral_combine_kernel(const double* __restrict__ u, int n, int p, const double* __restrict__ cmat, int m, int add,
                                                               double* __restrict__ x) {
  __shared__ double cs[SP_PMAX * SP_PMAX];
  for (int i = threadIdx.x; i < p * m; i += 256) cs[i] = cmat[i];
  __syncthreads();
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * m) return;
  const long long i = t / m;
  const int c = (int)(t % m);
  double acc = add ? x[t] : 0.0;
  for (int k = 0; k < p; ++k) acc = acc + u[(size_t)i * p + k] * cs[k * m + c];
  x[t] = acc;
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int ribca_spectral_spmm(const int64_t* indptr, const int32_t* indices, const float* weights, int64_t nnz, const double* dinv, int32_t n, int32_t m,
                        const double* x, double alpha, double beta, double gamma, const double* z, double* y, void* stream) {
  if (!indptr || !dinv || !x || !y || (nnz > 0 && (!indices || !weights))) return fail("ribca_spectral_spmm: NULL buffer");
  if (n < 1) return fail("ribca_spectral_spmm: needs n >= 1");
  if (m < 1 || m > SP_MMAX) return fail("ribca_spectral_spmm: needs 1 <= m <= 16");
  if (nnz < 0) return fail("ribca_spectral_spmm: needs nnz >= 0");
  if (y == x) return fail("ribca_spectral_spmm: y must not be x (other rows read x)");
  const long long total = (long long)n * m;
  hipLaunchKernelGGL(spectral_spmm_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(indptr), indices, weights, (long long)nnz, dinv, n, m, x, alpha, beta, gamma, z, y);
  RIBCA_FINISH();
  return 0;
}

int64_t ribca_spectral_gram_ws_bytes(int32_t n, int32_t p, int32_t q) {
  if (n < 1 || p < 1 || p > SP_PMAX || q < 1 || q > SP_PMAX) return 0;
  return (int64_t)sizeof(double) * chunks_of(n) * p * q;
}

int ribca_spectral_gram(const double* u, const double* v, int32_t n, int32_t p, int32_t q, double* g, void* ws, int64_t ws_bytes, void* stream) {
  if (!u || !v || !g || !ws) return fail("ribca_spectral_gram: NULL buffer");
  if (n < 1) return fail("ribca_spectral_gram: needs n >= 1");
  if (p < 1 || p > SP_PMAX || q < 1 || q > SP_PMAX) return fail("ribca_spectral_gram: needs 1 <= p, q <= 48");
  if (ws_bytes < ribca_spectral_gram_ws_bytes(n, p, q)) return fail("ribca_spectral_gram: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int chunks = chunks_of(n), pq = p * q;
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(spectral_gram_chunk_kernel, dim3(chunks), dim3(256), 0, s, u, v, n, p, q, part);
  launch_chunk_total(part, chunks, pq, g, s);
  RIBCA_FINISH();
  return 0;
}

int ribca_spectral_combine(const double* u, int32_t n, int32_t p, const double* c, int32_t m, int32_t add, double* x, void* stream) {
  if (!u || !c || !x) return fail("ribca_spectral_combine: NULL buffer");
  if (n < 1) return fail("ribca_spectral_combine: needs n >= 1");
  if (p < 1 || p > SP_PMAX || m < 1 || m > SP_PMAX) return fail("ribca_spectral_combine: needs 1 <= p, m <= 48");
  if (x == u) return fail("ribca_spectral_combine: x must not be u");
  const long long total = (long long)n * m;
  hipLaunchKernelGGL(spectral_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u, n, p, c, m, add ? 1 : 0, x);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
