// The O(n^2) part of HDBSCAN* for the "extra cell types" step (reference Annotator._find_extra_cell_types, model.py:642-675, which calls
// HDBSCAN on the host): the core distances and the minimum spanning tree of the mutual-reachability graph of dense fp32 points.  The
// tree bookkeeping after the spanning tree (single linkage, condensing, stabilities, cluster selection) is cheap and stays on the host
// (manifold.py).  The arithmetic is fixed so that a numpy loop reproduces it bit for bit (tests/hdbscan_numpy.py):
//   d2(i, j)     fp32 sum of squared differences in dimension order, no fma contraction (the convention of knn_dense in umap.hip);
//   core2(i)     the min_samples-th smallest d2(i, .), the point itself counted;
//   mreach2(i,j) max(core2(i), core2(j), d2(i, j));
//   edge order   the total order (mreach2, min(i, j), max(i, j)): the minimum spanning tree under it is unique, so the result does not
//                depend on the launch geometry.  Every comparison is made on squared values; one sqrt when the weights are written.
//
// All three O(n^2) kernels have the shape of knn_dense: one thread per query row (the row in registers, zero-padded to DP: (0 - 0)^2 adds
// an exact +0), candidate rows streamed through a 16 KiB LDS tile that every lane reads at the same address (a broadcast: no bank
// conflicts).  dim <= 64.
//
// core_topk (min_samples <= 64): the KM smallest d2 of the row kept sorted in registers (values only: the k-th smallest VALUE does not
//   depend on how ties are ordered).
// core_bisect (min_samples > 64): no per-row list.  d2 >= +0, so its fp32 bit pattern orders like its value: 31 bisection steps on the bit
//   pattern, each one counting pass over all candidates, find the smallest pattern v with #{j : d2(i, j) <= v} >= min_samples.  The state
//   of a row is two registers.
// mreach_mst: Boruvka rounds.  Per round
//   1. boruvka_nearest: for every point i the least edge to a point of another component.  For a fixed i the order (min(i, j), max(i, j))
//      is the order of j, so an ascending scan with a strict `<` on mreach2 finds it.  The same kernel folds the edge into the
//      per-component minimum of the packed 64-bit key (mreach2 bits << 32 | min(i, j)) with an integer atomicMin (order-independent).
//   2. boruvka_second_key: 96 bits of key do not fit one atomic, so a second pass takes, among the points whose edge attains the
//      component's (mreach2, min(i, j)), the least max(i, j) -- again an integer atomicMin.
//   3. boruvka_pick: one thread per component label.  The picks form a forest whose every tree holds exactly one mutual pair (two
//      components that picked the same edge; the order is total, so there is no longer cycle).  Of that pair the lower label is the root
//      and keeps its label; every other component writes its edge and points to the component it picked.  A label that wrote an edge is
//      never a label again, so the edge goes to slot [label]: no counter decides a position, the output order is deterministic.
//   4. pointer jumping over the labels (double-buffered, ceil(log2(components)) steps), then every point takes its root's label.
//   The host reads the number of edges written in the round (4 bytes) and stops at one component: at most ceil(log2 n) rounds, one launch
//   sequence per round, no kernel ever waits for another workgroup.  No float atomics.  At the end the one unused slot (the surviving
//   label) is filled from slot n - 1, which gives n - 1 contiguous edges.
#include <cmath>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

// every sum and product rounds on its own: the distances are the ones a plain numpy restatement computes
#pragma clang fp contract(off)

namespace ribca {
namespace {

constexpr int HD_THREADS = 128;           // 100k rows -> 782 workgroups: three per CU
constexpr int HD_TILE_FLOATS = 4096;      // 16 KiB of candidate coordinates per tile
constexpr int HD_DMAX = 64;
constexpr int HD_KREG = 64;               // largest min_samples of the register form
constexpr unsigned HD_INF_BITS = 0x7F800000u;
constexpr unsigned long long HD_NO_KEY = ~0ull;
constexpr int HD_CTRL_WORDS = 64;         // ctrl[0]: non-finite flag; ctrl[1 + r]: edges written in round r

template <int DP>
__device__ __forceinline__ void hd_load_query(const float* __restrict__ x, int n, int dim, int q, float (&qv)[DP]) {
#pragma unroll
  for (int d = 0; d < DP; ++d) qv[d] = (q < n && d < dim) ? x[(size_t)q * dim + d] : 0.f;
}

// rows base .. base + 4096 / DP - 1 of x into the tile, zero beyond n and beyond dim
template <int DP>
__device__ __forceinline__ void hd_load_tile(const float* __restrict__ x, int n, int dim, int base, float* tf) {
  for (int i = threadIdx.x; i < HD_TILE_FLOATS; i += HD_THREADS) {
    const int r = i / DP, d = i % DP;
    const int j = base + r;
    tf[i] = (j < n && d < dim) ? x[(size_t)j * dim + d] : 0.f;
  }
}

template <int DP>
__device__ __forceinline__ float hd_dist2(const float4* tile, int i, const float (&qv)[DP]) {
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
  return s;
}

// ----------------------------------------------------------------------------------------------------------------- core distances
template <int DP, int KM>
__global__ __launch_bounds__(HD_THREADS) void core_topk_kernel(const float* __restrict__ x, int n, int dim, int k, float* __restrict__ core2,
                                                               unsigned* __restrict__ ctrl) {
  constexpr int TILE = HD_TILE_FLOATS / DP;
  __shared__ float4 tile[HD_TILE_FLOATS / 4];
  const int q = blockIdx.x * HD_THREADS + threadIdx.x;
  float qv[DP];
  hd_load_query<DP>(x, n, dim, q, qv);
  float bd[KM];
#pragma unroll
  for (int p = 0; p < KM; ++p) bd[p] = INFINITY;
  for (int base = 0; base < n; base += TILE) {
    __syncthreads();
    hd_load_tile<DP>(x, n, dim, base, reinterpret_cast<float*>(tile));
    __syncthreads();
    const int lim = n - base < TILE ? n - base : TILE;
    if (q < n) {
      for (int i = 0; i < lim; ++i) {
        const float s = hd_dist2<DP>(tile, i, qv);
        if (s < bd[KM - 1]) {      // a NaN never enters
          bd[KM - 1] = s;
#pragma unroll
          for (int p = KM - 1; p >= 1; --p) {
            const float lo = fminf(bd[p], bd[p - 1]), hi = fmaxf(bd[p], bd[p - 1]);
            bd[p - 1] = lo;
            bd[p] = hi;
          }
        }
      }
    }
  }
  if (q < n) {
    float c = INFINITY;
#pragma unroll
    for (int p = 0; p < KM; ++p)
      if (p == k - 1) c = bd[p];
    core2[q] = c;
    if (!(c < INFINITY)) atomicOr(&ctrl[0], 1u);
  }
}

template <int DP>
__global__ __launch_bounds__(HD_THREADS) void core_bisect_kernel(const float* __restrict__ x, int n, int dim, int k, float* __restrict__ core2,
                                                                 unsigned* __restrict__ ctrl) {
  constexpr int TILE = HD_TILE_FLOATS / DP;
  __shared__ float4 tile[HD_TILE_FLOATS / 4];
  const int q = blockIdx.x * HD_THREADS + threadIdx.x;
  float qv[DP];
  hd_load_query<DP>(x, n, dim, q, qv);
  // the answer lies in [lo, hi]; 2^31 > HD_INF_BITS + 1 patterns: 31 halvings reach lo == hi.  Every thread of the workgroup takes all 31
  // (they share the tile loads).  A row with fewer than k comparable distances (a NaN coordinate) ends above HD_INF_BITS: non-finite.
  unsigned lo = 0u, hi = HD_INF_BITS;
  for (int it = 0; it < 31; ++it) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    const float fm = __uint_as_float(mid);
    int cnt = 0;
    for (int base = 0; base < n; base += TILE) {
      __syncthreads();
      hd_load_tile<DP>(x, n, dim, base, reinterpret_cast<float*>(tile));
      __syncthreads();
      const int lim = n - base < TILE ? n - base : TILE;
      if (q < n)
        for (int i = 0; i < lim; ++i) cnt += hd_dist2<DP>(tile, i, qv) <= fm ? 1 : 0;
    }
    if (lo > hi) continue;      // fewer than k comparable distances: stays above HD_INF_BITS
    if (cnt >= k) hi = mid;
    else lo = mid + 1u;
  }
  if (q < n) {
    core2[q] = __uint_as_float(lo);
    if (lo >= HD_INF_BITS) atomicOr(&ctrl[0], 1u);
  }
}

template <int DP>
void launch_core(const float* x, int n, int dim, int k, float* core2, unsigned* ctrl, hipStream_t s) {
  const dim3 g((n + HD_THREADS - 1) / HD_THREADS), b(HD_THREADS);
  if (k <= 16) hipLaunchKernelGGL((core_topk_kernel<DP, 16>), g, b, 0, s, x, n, dim, k, core2, ctrl);
  else if (k <= HD_KREG) hipLaunchKernelGGL((core_topk_kernel<DP, HD_KREG>), g, b, 0, s, x, n, dim, k, core2, ctrl);
  else hipLaunchKernelGGL((core_bisect_kernel<DP>), g, b, 0, s, x, n, dim, k, core2, ctrl);
}

// ------------------------------------------------------------------------------------------------- mutual-reachability spanning tree
struct MstWs {
  unsigned* ctrl;               // HD_CTRL_WORDS
  int* comp;                    // component label of every point (a point index)
  unsigned* bw;                 // per point: mreach2 bits of its least outgoing edge
  int* bj;                      // per point: the other end, -1 = none
  unsigned long long* key1;     // per label: least (mreach2 bits << 32 | min(i, j))
  unsigned* key2;               // per label: least max(i, j) among the edges attaining key1
  int* pa;                      // per label: the label it merges into (pointer jumping, double-buffered)
  int* pb;
  int* eu;                      // per label: the edge it wrote
  int* ev;
  float* ew;
};

MstWs carve_mst_ws(Carver& c, int n) {
  MstWs w;
  w.ctrl = c.take<unsigned>(HD_CTRL_WORDS);
  w.key1 = c.take<unsigned long long>(n);
  w.comp = c.take<int>(n);
  w.bw = c.take<unsigned>(n);
  w.bj = c.take<int>(n);
  w.key2 = c.take<unsigned>(n);
  w.pa = c.take<int>(n);
  w.pb = c.take<int>(n);
  w.eu = c.take<int>(n);
  w.ev = c.take<int>(n);
  w.ew = c.take<float>(n);
  return w;
}

__global__ __launch_bounds__(256) void mst_init_kernel(const float* __restrict__ core2, int n, MstWs w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  w.comp[i] = i;
  w.key1[i] = HD_NO_KEY;
  w.key2[i] = 0xFFFFFFFFu;
  const float c = core2[i];
  if (!(c >= 0.f && c < INFINITY)) atomicOr(&w.ctrl[0], 1u);
}

template <int DP>
__global__ __launch_bounds__(HD_THREADS) void boruvka_nearest_kernel(const float* __restrict__ x, int n, int dim, const float* __restrict__ core2,
                                                                     MstWs w) {
  constexpr int TILE = HD_TILE_FLOATS / DP;
  __shared__ float4 tile[HD_TILE_FLOATS / 4];
  __shared__ float tcore[TILE];
  __shared__ int tcomp[TILE];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * HD_THREADS + tid;
  float qv[DP];
  hd_load_query<DP>(x, n, dim, q, qv);
  const float cq = q < n ? core2[q] : 0.f;
  const int mc = q < n ? w.comp[q] : -1;
  float best = INFINITY;
  int bj = -1;
  for (int base = 0; base < n; base += TILE) {
    __syncthreads();
    hd_load_tile<DP>(x, n, dim, base, reinterpret_cast<float*>(tile));
    for (int r = tid; r < TILE; r += HD_THREADS) {
      const int j = base + r;
      tcore[r] = j < n ? core2[j] : INFINITY;
      tcomp[r] = j < n ? w.comp[j] : -1;
    }
    __syncthreads();
    const int lim = n - base < TILE ? n - base : TILE;
    if (q < n) {
      for (int i = 0; i < lim; ++i) {
        float m = hd_dist2<DP>(tile, i, qv);      // a NaN stays a NaN and loses every comparison
        const float cj = tcore[i];
        if (cq > m) m = cq;
        if (cj > m) m = cj;
        if (m < best && tcomp[i] != mc) {         // ascending j, strict <: the least (mreach2, min(q, j), max(q, j))
          best = m;
          bj = base + i;
        }
      }
    }
  }
  if (q < n) {
    const unsigned bits = __float_as_uint(best);
    w.bw[q] = bits;
    w.bj[q] = bj;
    if (bj >= 0) {
      const unsigned u = (unsigned)(q < bj ? q : bj);
      atomicMin(&w.key1[mc], ((unsigned long long)bits << 32) | (unsigned long long)u);
    }
  }
}

__global__ __launch_bounds__(256) void boruvka_second_key_kernel(int n, MstWs w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int j = w.bj[i];
  if (j < 0) return;
  const int c = w.comp[i];
  const unsigned u = (unsigned)(i < j ? i : j), v = (unsigned)(i < j ? j : i);
  if ((((unsigned long long)w.bw[i] << 32) | (unsigned long long)u) == w.key1[c]) atomicMin(&w.key2[c], v);
}

__global__ __launch_bounds__(256) void boruvka_pick_kernel(int n, int round, MstWs w) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const unsigned long long k1 = w.key1[c];
  if (k1 == HD_NO_KEY) {      // not a live label, or a component without a finite outgoing edge
    w.pa[c] = c;
    return;
  }
  const int u = (int)(unsigned)(k1 & 0xFFFFFFFFull);
  const unsigned v = w.key2[c];
  if (u >= n || v >= (unsigned)n) {      // cannot happen (the point that set key1 also sets key2); never index with it if it did
    w.pa[c] = c;
    return;
  }
  const int cu = w.comp[u];
  const int other = cu == c ? w.comp[v] : cu;
  const bool mutual = w.key1[other] == k1 && w.key2[other] == v;
  if (mutual && c < other) {
    w.pa[c] = c;
    return;
  }
  w.pa[c] = other;
  w.eu[c] = u;
  w.ev[c] = (int)v;
  w.ew[c] = sqrtf(__uint_as_float((unsigned)(k1 >> 32)));
  atomicAdd(&w.ctrl[1 + round], 1u);
}

__global__ __launch_bounds__(256) void boruvka_jump_kernel(int n, const int* __restrict__ src, int* __restrict__ dst) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) dst[c] = src[src[c]];
}

// every point takes the label of its tree's root; the keys are reset for the next round
__global__ __launch_bounds__(256) void boruvka_relabel_kernel(int n, const int* __restrict__ root, MstWs w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  w.comp[i] = root[w.comp[i]];
  w.key1[i] = HD_NO_KEY;
  w.key2[i] = 0xFFFFFFFFu;
}

// slots 0 .. n - 1 without the surviving label -> n - 1 contiguous edges: the hole takes what slot n - 1 holds
__global__ __launch_bounds__(256) void mst_compact_kernel(int n, MstWs w, int32_t* __restrict__ eu, int32_t* __restrict__ ev, float* __restrict__ ew) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n - 1) return;
  const int src = s == w.comp[0] ? n - 1 : s;
  eu[s] = w.eu[src];
  ev[s] = w.ev[src];
  ew[s] = w.ew[src];
}

template <int DP>
void launch_nearest(const float* x, int n, int dim, const float* core2, const MstWs& w, hipStream_t s) {
  hipLaunchKernelGGL((boruvka_nearest_kernel<DP>), dim3((n + HD_THREADS - 1) / HD_THREADS), dim3(HD_THREADS), 0, s, x, n, dim, core2, w);
}

int fail(const char* msg) { return api_fail(msg); }

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_core_distance_ws_bytes(int32_t n, int32_t dim, int32_t min_samples) {      // the control words
  if (n < 2 || dim < 1 || dim > HD_DMAX || min_samples < 1 || min_samples > n) return 0;
  return HD_CTRL_WORDS * 4;
}

int ribca_core_distance(const float* x, int32_t n, int32_t dim, int32_t min_samples, float* core2, void* ws, int64_t ws_bytes, void* stream) {
  if (!x || !core2 || !ws) return fail("ribca_core_distance: NULL buffer");
  if (n < 2) return fail("ribca_core_distance: needs n >= 2");
  if (dim < 1 || dim > HD_DMAX) return fail("ribca_core_distance: needs 1 <= dim <= 64");
  if (min_samples < 1 || min_samples > n) return fail("ribca_core_distance: needs 1 <= min_samples <= n");
  if (ws_bytes < ribca_core_distance_ws_bytes(n, dim, min_samples)) return fail("ribca_core_distance: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned* ctrl = static_cast<unsigned*>(ws);
  HIP_TRY(hipMemsetAsync(ctrl, 0, HD_CTRL_WORDS * 4, s));
  if (dim <= 8) launch_core<8>(x, n, dim, min_samples, core2, ctrl, s);
  else if (dim <= 16) launch_core<16>(x, n, dim, min_samples, core2, ctrl, s);
  else if (dim <= 32) launch_core<32>(x, n, dim, min_samples, core2, ctrl, s);
  else launch_core<64>(x, n, dim, min_samples, core2, ctrl, s);
  RIBCA_FINISH();
  unsigned flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, ctrl, sizeof(flag), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (flag) return fail("ribca_core_distance: a core distance is not finite (NaN or infinite coordinates, or an overflowing distance)");
  return 0;
}

int64_t ribca_mreach_mst_ws_bytes(int32_t n) {
  if (n < 2) return 0;
  Carver c(nullptr);
  carve_mst_ws(c, n);
  return (int64_t)c.off;
}

int ribca_mreach_mst(const float* x, int32_t n, int32_t dim, const float* core2, int32_t* edges_u, int32_t* edges_v, float* edges_w, void* ws,
                     int64_t ws_bytes, void* stream) {
  if (!x || !core2 || !edges_u || !edges_v || !edges_w || !ws) return fail("ribca_mreach_mst: NULL buffer");
  if (n < 2) return fail("ribca_mreach_mst: needs n >= 2");
  if (dim < 1 || dim > HD_DMAX) return fail("ribca_mreach_mst: needs 1 <= dim <= 64");
  if (ws_bytes < ribca_mreach_mst_ws_bytes(n)) return fail("ribca_mreach_mst: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Carver c(ws);
  const MstWs w = carve_mst_ws(c, n);
  const dim3 g((n + 255) / 256), b(256);
  HIP_TRY(hipMemsetAsync(w.ctrl, 0, HD_CTRL_WORDS * 4, s));
  hipLaunchKernelGGL(mst_init_kernel, g, b, 0, s, core2, n, w);
  int max_rounds = 1;      // ceil(log2 n): every round at least halves the number of components
  while ((1ll << max_rounds) < (long long)n) ++max_rounds;
  int components = n;
  for (int round = 0; components > 1; ++round) {
    if (round >= max_rounds || 1 + round >= HD_CTRL_WORDS) return fail("ribca_mreach_mst: more than ceil(log2 n) rounds (internal error)");
    if (dim <= 8) launch_nearest<8>(x, n, dim, core2, w, s);
    else if (dim <= 16) launch_nearest<16>(x, n, dim, core2, w, s);
    else if (dim <= 32) launch_nearest<32>(x, n, dim, core2, w, s);
    else launch_nearest<64>(x, n, dim, core2, w, s);
    hipLaunchKernelGGL(boruvka_second_key_kernel, g, b, 0, s, n, w);
    hipLaunchKernelGGL(boruvka_pick_kernel, g, b, 0, s, n, round, w);
    // the longest chain of picks is shorter than the number of components: 2^steps >= components
    int* root = w.pa;
    int* spare = w.pb;
    for (long long reach = 1; reach < (long long)components; reach *= 2) {
      hipLaunchKernelGGL(boruvka_jump_kernel, g, b, 0, s, n, root, spare);
      int* t = root;
      root = spare;
      spare = t;
    }
    hipLaunchKernelGGL(boruvka_relabel_kernel, g, b, 0, s, n, root, w);
    RIBCA_FINISH();
    unsigned host[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(&host[0], w.ctrl, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&host[1], w.ctrl + 1 + round, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (host[0]) return fail("ribca_mreach_mst: a core distance is negative or not finite");
    if (host[1] == 0u || host[1] >= (unsigned)components)
      return fail("ribca_mreach_mst: no finite edge between the remaining components (NaN or overflowing distances)");
    components -= (int)host[1];
  }
  hipLaunchKernelGGL(mst_compact_kernel, g, b, 0, s, n, w, edges_u, edges_v, edges_w);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
