// The permutation null of the neighbourhood co-occurrence counts (Annotator.neighborhood_enrichment; histoCAT / squidpy's nhood_enrichment): the
// k-NN graph of ribca_knn_neighbours stays fixed, the cell-type labels are shuffled within the image P times and the type pairs recounted.
// sigma_p and the byte rows of shuffled labels (launch_perm_labels; kPermSkip = a label outside [0, T): skipped here) are ribca_perm.h's.
//   perm_count       one workgroup per (slab of EN_SLAB cells, permutation): each thread reads its cell's byte, gathers the bytes of its m neighbours
//                    and counts the pairs into a T x T LDS histogram (<= 16 KiB) with integer atomics; then one 64-bit global atomic per non-zero
//                    entry.  Integer sums: the result is independent of the order and of the launch geometry.
#include <algorithm>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_perm.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

namespace ribca {
namespace {

constexpr int EN_M_MAX = 31;
constexpr int EN_T_MAX = 64;
constexpr int EN_N_MAX = 1 << 30;
constexpr int EN_BATCH = 128;        // permutations whose label rows the workspace holds at once (gridDim.y of both kernels)
constexpr int EN_SLAB = 4096;        // cells of one counting workgroup: 16 per thread, so a flush of T * T entries is paid once per 4096 * m counts

static_assert(EN_T_MAX * EN_T_MAX * 4 <= 16 * 1024, "the LDS histogram");
static_assert(kPermSkip >= EN_T_MAX, "a skipped byte never indexes the histogram");
static_assert((long long)EN_SLAB * EN_M_MAX < (1ll << 32), "a 32-bit LDS count cannot wrap within one slab");

int fail(const char* msg) { return api_fail(msg); }

// counts[j][a][b] += the pairs (label(i), label(idx[i][q])) of the slab's cells: grid (ceil(n / EN_SLAB), batch)
__global__ __launch_bounds__(256) void perm_count_kernel(const int32_t* __restrict__ idx, const uint8_t* __restrict__ labels, int n, int m, int T,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ unsigned int hist[EN_T_MAX * EN_T_MAX];
  const int tid = threadIdx.x;
  const int TT = T * T;
  for (int e = tid; e < TT; e += 256) hist[e] = 0;
  __syncthreads();
  const uint8_t* __restrict__ lab = labels + (size_t)blockIdx.y * n;
  const int first = blockIdx.x * EN_SLAB;
  const int last = min(n, first + EN_SLAB);
  for (int i = first + tid; i < last; i += 256) {
    const unsigned a = lab[i];
    if (a >= (unsigned)T) continue;
    const int32_t* __restrict__ row = idx + (size_t)i * m;
    for (int q = 0; q < m; ++q) {
      const int32_t j = row[q];
      if ((unsigned)j >= (unsigned)n) continue;
      const unsigned b = lab[j];
      if (b < (unsigned)T) atomicAdd(&hist[a * T + b], 1u);
    }
  }
  __syncthreads();
  unsigned long long* __restrict__ out = counts + (size_t)blockIdx.y * TT;
  for (int e = tid; e < TT; e += 256)
    if (hist[e]) atomicAdd(&out[e], (unsigned long long)hist[e]);
}

bool perm_sizes_ok(int n, int P) { return n >= 1 && n <= EN_N_MAX && P >= 1; }

uint8_t* carve_perm(Carver& cv, int n, int P) { return cv.take<uint8_t>((size_t)perm_batch(P, EN_BATCH) * (size_t)n); }

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_nhood_perm_counts_ws_bytes(int32_t n, int32_t P) {
  if (!perm_sizes_ok(n, P)) return 0;
  Carver cv(nullptr);
  carve_perm(cv, n, P);
  return (int64_t)cv.off;
}

int ribca_nhood_perm_counts(const int32_t* idx, const int32_t* cell_type, int32_t n, int32_t m, int32_t T, uint64_t seed, int32_t image, int64_t p0,
                            int32_t P, uint64_t* counts, void* ws, int64_t ws_bytes, void* stream) {
  if (!idx || !cell_type || !counts || !ws) return fail("ribca_nhood_perm_counts: NULL buffer");
  if (n < 1 || n > EN_N_MAX) return fail("ribca_nhood_perm_counts: needs 1 <= n <= 2^30");
  if (m < 1 || m > EN_M_MAX) return fail("ribca_nhood_perm_counts: needs 1 <= m <= 31");
  if (T < 1 || T > EN_T_MAX) return fail("ribca_nhood_perm_counts: needs 1 <= T <= 64");
  if (perm_range_check("ribca_nhood_perm_counts", image, p0, P)) return 1;
  if (ws_bytes < ribca_nhood_perm_counts_ws_bytes(n, P)) return fail("ribca_nhood_perm_counts: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Carver cv(ws);
  uint8_t* labels = carve_perm(cv, n, P);
  const PermKeys k(n, seed, image);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  for (int64_t j0 = 0; j0 < P; j0 += EN_BATCH) {      // the batches follow one another on the stream: the label rows are reused
    const int batch = (int)std::min<int64_t>(EN_BATCH, P - j0);
    launch_perm_labels(cell_type, n, T, k.h, k.image_key, (uint64_t)(p0 + j0), batch, labels, s);
    hipLaunchKernelGGL(perm_count_kernel, dim3((unsigned)((n + EN_SLAB - 1) / EN_SLAB), (unsigned)batch), dim3(256), 0, s, idx, labels, n, m, T,
                       out + (size_t)j0 * T * T);
  }
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
