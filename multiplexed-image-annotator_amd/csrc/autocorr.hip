// Spatial autocorrelation of the markers (Annotator.spatial_autocorrelation; squidpy's spatial_autocorr): the numerators of Moran's I and Geary's C
// of every channel over the fixed k-NN list of ribca_knn_neighbours, observed and under a permutation null in which whole rows of the (n, C) table
// move with the keyed bijection sigma_p of ribca_perm.h, whose launch_perm_rows copies them.  include/ribca_hip.h states the arithmetic;
// tests/autocorr_numpy.py restates it.  The rows of a batch are sized to stay inside the Infinity Cache for the gathers that follow (AC_ROW_BYTES).
//   chunk_stats  one workgroup per (chunk, permutation, tile of AC_COLS channels).  The neighbour lists of the chunk go through LDS once.  The
//                thread (g, c) owns channel c of the AC_LEAF consecutive cells [4 g, 4 g + 4) of the chunk: per cell it adds the neighbours in
//                list order (the AC_COLS lanes of a cell read one 128-byte line of every neighbour's row), and its (a, g) pairs meet in the first
//                two rounds of THE tree in registers; the last six rounds run over the 64 threads of a channel in LDS.  No atomics: every
//                partial has one owner.
//   chunk_total_kernel (ribca_scratch.h) adds the chunks in ascending order, one thread per (permutation, statistic, channel).
// Measured forms of chunk_stats: lists from global memory, rows of exactly C doubles, 16 or 8 cells per thread -- same bits,
// up to 1.75 times the time.  Gathering z[sigma(idx)] without the copied rows would save the workspace and make every neighbour read a random row
// of the whole table (m + 1 walks of sigma per cell as well); it was not built.
#include <algorithm>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_perm.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

#pragma clang fp contract(off)

namespace ribca {
namespace {

constexpr int AC_N_MAX = 1 << 30;
constexpr int AC_C_MAX = 64;
constexpr int AC_M_MAX = 31;
constexpr int AC_CHUNK = kCellChunk;          // cells of one chunk of THE tree: eight rounds of adjacent pairs
constexpr int AC_COLS = 16;                   // channels of one workgroup of chunk_stats
constexpr int AC_LEAF_ROUNDS = 2;             // rounds of the tree one thread does in registers ...
constexpr int AC_LEAF = 1 << AC_LEAF_ROUNDS;  // ... over this many consecutive cells
constexpr int AC_BATCH = 32;                  // permutations whose rows the workspace holds at most
constexpr long long AC_ROW_BYTES = 64ll << 20;      // ... and the bytes of rows it holds at most (one permutation when a single one is larger)

constexpr int AC_THREADS = AC_COLS * (AC_CHUNK / AC_LEAF);      // chunk_stats: one thread per (group of AC_LEAF cells, channel)

static_assert(AC_CHUNK == 256, "eight rounds of adjacent pairs");
static_assert(AC_THREADS <= 1024 && AC_THREADS % 64 == 0, "a workgroup of whole waves");
static_assert(AC_CHUNK * AC_M_MAX * 4 + 2 * AC_THREADS * 8 <= 64 * 1024, "static LDS of chunk_stats_kernel: the lists of the chunk and the two trees");

int fail(const char* msg) { return api_fail(msg); }

struct Pair { double a, g; };

// the (a_i, g_i) of cell i and channel c over rows of ld doubles; idx: the lists of the cells from i0 on; a cell past the end of the table is the
// +0.0 padding of its chunk
__device__ __forceinline__ Pair cell_terms(const double* __restrict__ rows, const int32_t* idx, int n, int ld, int m, int i, int i0, int c) {
  Pair r = {0.0, 0.0};
  if (i >= n) return r;
  const double zi = rows[(size_t)i * ld + c];
  const int32_t* list = idx + (size_t)(i - i0) * m;
  double s = 0.0, g = 0.0;
#pragma unroll 4
  for (int q = 0; q < m; ++q) {
    const int32_t j = list[q];
    const bool ok = (unsigned)j < (unsigned)n;
    const double v = ok ? rows[(size_t)j * ld + c] : 0.0;
    const double d = zi - v;
    s = ok ? s + v : s;
    g = ok ? g + d * d : g;
  }
  r.a = zi * s;
  r.g = g;
  return r;
}

// ROUNDS rounds of adjacent pairs over the 2^ROUNDS cells from i on
template <int ROUNDS>
__device__ __forceinline__ Pair leaf_tree(const double* __restrict__ rows, const int32_t* idx, int n, int ld, int m, int i, int i0, int c) {
  if constexpr (ROUNDS == 0) {
    return cell_terms(rows, idx, n, ld, m, i, i0, c);
  } else {
    const Pair lo = leaf_tree<ROUNDS - 1>(rows, idx, n, ld, m, i, i0, c);
    const Pair hi = leaf_tree<ROUNDS - 1>(rows, idx, n, ld, m, i + (1 << (ROUNDS - 1)), i0, c);
    Pair r;
    r.a = lo.a + hi.a;
    r.g = lo.g + hi.g;
    return r;
  }
}

// part[k][j][0][c] = the tree of a over chunk k under permutation j of the batch, part[k][j][1][c] that of g: grid (chunks, batch, channel tiles).
// row_stride = n ld doubles from one permutation's copied rows (ld = L doubles each) to the next; 0 and ld = C for the table itself (observed).
__global__ __launch_bounds__(AC_THREADS) void chunk_stats_kernel(const double* __restrict__ zp, size_t row_stride, int ld, const int32_t* __restrict__ idx,
                                                                 int n, int C, int m, double* __restrict__ part) {
  __shared__ double sa[AC_THREADS], sg[AC_THREADS];
  __shared__ int32_t lists[AC_CHUNK * AC_M_MAX];      // the neighbour lists of the chunk: read once, coalesced; the 16 lanes of a cell then share every entry
  const int tid = threadIdx.x;
  const int first = blockIdx.x * AC_CHUNK;
  {
    const int words = min(AC_CHUNK, n - first) * m;
    const int32_t* __restrict__ src = idx + (size_t)first * m;
    for (int e = tid; e < words; e += AC_THREADS) lists[e] = src[e];
  }
  __syncthreads();
  const int lc = tid % AC_COLS, grp = tid / AC_COLS;
  const int c = blockIdx.z * AC_COLS + lc;
  const double* __restrict__ rows = zp + (size_t)blockIdx.y * row_stride;
  Pair r = {0.0, 0.0};
  if (c < C) r = leaf_tree<AC_LEAF_ROUNDS>(rows, lists, n, ld, m, first + grp * AC_LEAF, first, c);
  sa[tid] = r.a;
  sg[tid] = r.g;
  __syncthreads();
  // the remaining rounds in place: the slot of group grp takes its right neighbour of the round; nobody writes a slot that is read in the same round
  for (int step = 1; step < AC_CHUNK / AC_LEAF; step <<= 1) {
    if (grp % (2 * step) == 0) {
      sa[tid] = sa[tid] + sa[tid + step * AC_COLS];
      sg[tid] = sg[tid] + sg[tid + step * AC_COLS];
    }
    __syncthreads();
  }
  if (grp == 0 && c < C) {
    double* __restrict__ out = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 2 * C;
    out[c] = sa[tid];
    out[C + c] = sg[tid];
  }
}

bool sizes_ok(int n, int C) { return n >= 1 && n <= AC_N_MAX && C >= 1 && C <= AC_C_MAX; }

// B = min(P, 32, max(1, 64 MiB / (8 n L)))
int batch_of(int n, int C, int P) { return perm_batch(P, AC_BATCH, 8ll * n * row_ld(C), AC_ROW_BYTES); }

struct AutocorrWs {
  double* rows;      // (batch, n, L): the permuted rows; none for the observed statistic
  double* part;      // (chunks, batch, 2, C)
};

AutocorrWs carve_autocorr(Carver& cv, int n, int C, int batch, bool rows) {
  AutocorrWs w;
  w.rows = rows ? cv.take<double>((size_t)batch * n * row_ld(C)) : nullptr;
  w.part = cv.take<double>((size_t)chunks_of_cells(n) * batch * 2 * C);
  return w;
}

void launch_stats(const double* rows, size_t row_stride, int ld, const int32_t* idx, int n, int C, int m, int batch, const AutocorrWs& w, double* out, hipStream_t s) {
  const int chunks = chunks_of_cells(n);
  hipLaunchKernelGGL(chunk_stats_kernel, dim3((unsigned)chunks, (unsigned)batch, (unsigned)((C + AC_COLS - 1) / AC_COLS)), dim3(AC_THREADS), 0, s, rows,
                     row_stride, ld, idx, n, C, m, w.part);
  launch_chunk_total(w.part, chunks, batch * 2 * C, out, s);
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_autocorr_observed_ws_bytes(int32_t n, int32_t C) {
  if (!sizes_ok(n, C)) return 0;
  Carver cv(nullptr);
  carve_autocorr(cv, n, C, 1, false);
  return (int64_t)cv.off;
}

int ribca_autocorr_observed(const double* z, const int32_t* idx, int32_t n, int32_t C, int32_t m, double* out, void* ws, int64_t ws_bytes, void* stream) {
  if (!z || !idx || !out || !ws) return fail("ribca_autocorr_observed: NULL buffer");
  if (n < 1 || n > AC_N_MAX) return fail("ribca_autocorr_observed: needs 1 <= n <= 2^30");
  if (C < 1 || C > AC_C_MAX) return fail("ribca_autocorr_observed: needs 1 <= C <= 64");
  if (m < 1 || m > AC_M_MAX) return fail("ribca_autocorr_observed: needs 1 <= m <= 31");
  if (ws_bytes < ribca_autocorr_observed_ws_bytes(n, C)) return fail("ribca_autocorr_observed: workspace too small");
  Carver cv(ws);
  const AutocorrWs w = carve_autocorr(cv, n, C, 1, false);
  launch_stats(z, 0, C, idx, n, C, m, 1, w, out, (hipStream_t)stream);
  RIBCA_FINISH();
  return 0;
}

int64_t ribca_autocorr_perm_ws_bytes(int32_t n, int32_t C, int32_t P) {
  if (!sizes_ok(n, C) || P < 1) return 0;
  Carver cv(nullptr);
  carve_autocorr(cv, n, C, batch_of(n, C, P), true);
  return (int64_t)cv.off;
}

int ribca_autocorr_perm(const double* z, const int32_t* idx, int32_t n, int32_t C, int32_t m, uint64_t seed, int32_t image, int64_t p0, int32_t P,
                        double* out, void* ws, int64_t ws_bytes, void* stream) {
  if (!z || !idx || !out || !ws) return fail("ribca_autocorr_perm: NULL buffer");
  if (n < 1 || n > AC_N_MAX) return fail("ribca_autocorr_perm: needs 1 <= n <= 2^30");
  if (C < 1 || C > AC_C_MAX) return fail("ribca_autocorr_perm: needs 1 <= C <= 64");
  if (m < 1 || m > AC_M_MAX) return fail("ribca_autocorr_perm: needs 1 <= m <= 31");
  if (perm_range_check("ribca_autocorr_perm", image, p0, P)) return 1;
  if (ws_bytes < ribca_autocorr_perm_ws_bytes(n, C, P)) return fail("ribca_autocorr_perm: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int B = batch_of(n, C, P);
  Carver cv(ws);
  const AutocorrWs w = carve_autocorr(cv, n, C, B, true);
  const int ld = row_ld(C);
  const PermKeys k(n, seed, image);
  for (int64_t j0 = 0; j0 < P; j0 += B) {      // the batches follow one another on the stream: rows and partials are reused
    const int batch = (int)std::min<int64_t>(B, P - j0);
    launch_perm_rows(z, n, C, ld, k.h, k.image_key, (uint64_t)(p0 + j0), batch, w.rows, nullptr, s);
    launch_stats(w.rows, (size_t)n * ld, ld, idx, n, C, m, batch, w, out + (size_t)j0 * 2 * C, s);
  }
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
