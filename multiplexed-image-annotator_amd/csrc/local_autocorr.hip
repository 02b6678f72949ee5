// Local indicators of spatial association (Annotator.local_autocorrelation; PySAL's esda.Moran_Local / G_Local): per cell and channel the
// neighbour sum ("lag") of the centred table over the fixed k-NN list, and how many of P conditional permutations -- the cell keeps its own row,
// the other n - 1 rows move around it with the keyed bijection sigma_p of ribca_perm.h -- give a lag at or above / at or below the observed one.
// One pair of counts serves local Moran's I and Getis-Ord Gi*: with z_i fixed the lag is their only random part.  include/ribca_hip.h states the
// arithmetic; tests/local_autocorr_numpy.py restates it.
//   local_lag    one thread per (cell, channel): the neighbours added in list order.
//   perm_rows    launch_perm_rows of ribca_perm.h with the INVERSE beside the rows, inv[b][sigma(i)] = i.  With it "sigma(j) == i" is
//                "j == inv[i]": the counting thread reads one coalesced word per permutation and no source index per neighbour.
//   perm_counts  one workgroup per (chunk of LA_CHUNK cells, tile of LA_COLS channels); the chunk's lists go through LDS once.  The thread (g, c)
//                owns channel c of LA_LEAF consecutive cells with z_i, lag_i and the two counters of each in registers; per permutation of the
//                batch and per cell it adds the neighbours in list order -- the cell's own value for j == i, zp[i] for j == inv[i], zp[j]
//                otherwise; the LA_COLS lanes of a cell read one 128-byte line of every neighbour's row -- and compares.  The counters are added
//                to ge / le once per batch: every (cell, channel) has one owner and the batches follow one another on the stream, so the
//                additions are plain loads and stores.
// Measured forms: DESIGN.md section 17.
#include <algorithm>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_perm.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

#pragma clang fp contract(off)

namespace ribca {
namespace {

constexpr int LA_N_MAX = 1 << 30;
constexpr int LA_C_MAX = 64;
constexpr int LA_M_MAX = 31;
constexpr int LA_CHUNK = kCellChunk;          // cells of one workgroup of perm_counts
constexpr int LA_COLS = 16;                   // channels of one workgroup of perm_counts: one 128-byte line of a copied row
constexpr int LA_LEAF = 4;                    // consecutive cells one thread owns
constexpr int LA_BATCH = 32;                  // permutations whose rows the workspace holds at most
constexpr long long LA_ROW_BYTES = 64ll << 20;      // ... and the bytes of rows it holds at most (one permutation when a single one is larger)
constexpr int LA_THREADS = LA_COLS * (LA_CHUNK / LA_LEAF);

static_assert(LA_THREADS <= 1024 && LA_THREADS % 64 == 0, "a workgroup of whole waves");
static_assert(LA_CHUNK * LA_M_MAX * 4 <= 64 * 1024, "static LDS of perm_counts_kernel: the lists of the chunk");

int fail(const char* msg) { return api_fail(msg); }

// lag[i][c] = (((+0.0 + z[j_0][c]) + z[j_1][c]) + ...) over the valid entries of the list of i: one thread per element of the (n, C) table
__global__ __launch_bounds__(256) void local_lag_kernel(const double* __restrict__ z, const int32_t* __restrict__ idx, int n, int C, int m,
                                                        double* __restrict__ lag) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * C) return;
  const int i = (int)(e / C), c = (int)(e % C);
  const int32_t* __restrict__ list = idx + (size_t)i * m;
  double s = 0.0;
  for (int q = 0; q < m; ++q) {
    const int32_t j = list[q];
    if ((unsigned)j < (unsigned)n) s = s + z[(size_t)j * C + c];
  }
  lag[e] = s;
}

// ge[i][c] += the permutations b of the batch with s_b[i][c] >= lag[i][c], le likewise with <=: grid (chunks, channel tiles)
__global__ __launch_bounds__(LA_THREADS) void local_perm_counts_kernel(const double* __restrict__ z, const double* __restrict__ lag,
                                                                       const int32_t* __restrict__ idx, const double* __restrict__ zp,
                                                                       const int32_t* __restrict__ inv, int n, int C, int ld, int m, int batch,
                                                                       uint32_t* __restrict__ ge, uint32_t* __restrict__ le) {
  __shared__ int32_t lists[LA_CHUNK * LA_M_MAX];      // read once, coalesced; the 16 lanes of a cell then share every entry
  const int tid = threadIdx.x;
  const int first = blockIdx.x * LA_CHUNK;
  {
    const int words = min(LA_CHUNK, n - first) * m;
    const int32_t* __restrict__ src = idx + (size_t)first * m;
    for (int e = tid; e < words; e += LA_THREADS) lists[e] = src[e];
  }
  __syncthreads();
  const int c = blockIdx.y * LA_COLS + tid % LA_COLS;
  const int i0 = first + (tid / LA_COLS) * LA_LEAF;
  if (c >= C || i0 >= n) return;      // no barrier below
  const int owned = min(LA_LEAF, n - i0);
  double zi[LA_LEAF], li[LA_LEAF];
  uint32_t nge[LA_LEAF], nle[LA_LEAF];
#pragma unroll
  for (int k = 0; k < LA_LEAF; ++k) {
    const bool live = k < owned;
    zi[k] = live ? z[(size_t)(i0 + k) * C + c] : 0.0;
    li[k] = live ? lag[(size_t)(i0 + k) * C + c] : 0.0;
    nge[k] = nle[k] = 0;
  }
  for (int b = 0; b < batch; ++b) {
    const double* __restrict__ rows = zp + (size_t)b * n * ld;
    const int32_t* __restrict__ back = inv + (size_t)b * n;
#pragma unroll
    for (int k = 0; k < LA_LEAF; ++k) {
      if (k < owned) {
        const int i = i0 + k;
        const int32_t from = back[i];
        const double moved = rows[(size_t)i * ld + c];      // z[sigma(i)]: what the cell that drew i's row gets instead
        const int32_t* list = lists + (i - first) * m;
        double s = 0.0;
#pragma unroll 2
        for (int q = 0; q < m; ++q) {
          const int32_t j = list[q];
          const bool ok = (unsigned)j < (unsigned)n;
          double v = ok ? rows[(size_t)j * ld + c] : 0.0;
          v = j == from ? moved : v;
          v = j == i ? zi[k] : v;
          s = ok ? s + v : s;
        }
        nge[k] += s >= li[k] ? 1u : 0u;
        nle[k] += s <= li[k] ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < LA_LEAF; ++k) {
    if (k < owned) {
      const size_t o = (size_t)(i0 + k) * C + c;
      ge[o] += nge[k];
      le[o] += nle[k];
    }
  }
}

bool sizes_ok(int n, int C) { return n >= 1 && n <= LA_N_MAX && C >= 1 && C <= LA_C_MAX; }

// B = min(P, 32, max(1, 64 MiB / (8 n L)))
int batch_of(int n, int C, int P) { return perm_batch(P, LA_BATCH, 8ll * n * row_ld(C), LA_ROW_BYTES); }

struct LocalWs {
  double* rows;      // (batch, n, L): the permuted rows
  int32_t* inv;      // (batch, n): the inverse of sigma
};

LocalWs carve_local(Carver& cv, int n, int C, int batch) {
  LocalWs w;
  w.rows = cv.take<double>((size_t)batch * n * row_ld(C));
  w.inv = cv.take<int32_t>((size_t)batch * n);
  return w;
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int ribca_local_lag(const double* z, const int32_t* idx, int32_t n, int32_t C, int32_t m, double* lag, void* stream) {
  if (!z || !idx || !lag) return fail("ribca_local_lag: NULL buffer");
  if (n < 1 || n > LA_N_MAX) return fail("ribca_local_lag: needs 1 <= n <= 2^30");
  if (C < 1 || C > LA_C_MAX) return fail("ribca_local_lag: needs 1 <= C <= 64");
  if (m < 1 || m > LA_M_MAX) return fail("ribca_local_lag: needs 1 <= m <= 31");
  const size_t blocks = ((size_t)n * C + 255) / 256;
  hipLaunchKernelGGL(local_lag_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, idx, n, C, m, lag);
  RIBCA_FINISH();
  return 0;
}

int64_t ribca_local_perm_counts_ws_bytes(int32_t n, int32_t C, int32_t P) {
  if (!sizes_ok(n, C) || P < 1) return 0;
  Carver cv(nullptr);
  carve_local(cv, n, C, batch_of(n, C, P));
  return (int64_t)cv.off;
}

int ribca_local_perm_counts(const double* z, const int32_t* idx, const double* lag, int32_t n, int32_t C, int32_t m, uint64_t seed, int32_t image,
                            int64_t p0, int32_t P, uint32_t* ge, uint32_t* le, void* ws, int64_t ws_bytes, void* stream) {
  if (!z || !idx || !lag || !ge || !le || !ws) return fail("ribca_local_perm_counts: NULL buffer");
  if (n < 1 || n > LA_N_MAX) return fail("ribca_local_perm_counts: needs 1 <= n <= 2^30");
  if (C < 1 || C > LA_C_MAX) return fail("ribca_local_perm_counts: needs 1 <= C <= 64");
  if (m < 1 || m > LA_M_MAX) return fail("ribca_local_perm_counts: needs 1 <= m <= 31");
  if (perm_range_check("ribca_local_perm_counts", image, p0, P)) return 1;
  if (ws_bytes < ribca_local_perm_counts_ws_bytes(n, C, P)) return fail("ribca_local_perm_counts: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int B = batch_of(n, C, P);
  Carver cv(ws);
  const LocalWs w = carve_local(cv, n, C, B);
  const int ld = row_ld(C), chunks = chunks_of_cells(n);
  const PermKeys k(n, seed, image);
  HIP_TRY(hipMemsetAsync(ge, 0, (size_t)n * C * sizeof(uint32_t), s));      // OVERWRITTEN: the batches add to zero
  HIP_TRY(hipMemsetAsync(le, 0, (size_t)n * C * sizeof(uint32_t), s));
  for (int64_t j0 = 0; j0 < P; j0 += B) {      // the batches follow one another on the stream: rows, inverse and the counts' owners are reused
    const int batch = (int)std::min<int64_t>(B, P - j0);
    launch_perm_rows(z, n, C, ld, k.h, k.image_key, (uint64_t)(p0 + j0), batch, w.rows, w.inv, s);
    hipLaunchKernelGGL(local_perm_counts_kernel, dim3((unsigned)chunks, (unsigned)((C + LA_COLS - 1) / LA_COLS)), dim3(LA_THREADS), 0, s, z, lag, idx,
                       w.rows, w.inv, n, C, ld, m, batch, ge, le);
  }
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
