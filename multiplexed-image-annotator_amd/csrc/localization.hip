// Where a marker sits in the cell (Analyses.marker_localization; CellProfiler's MeasureObjectIntensityDistribution, "membrane vs interior" of the
// MIBI pipelines): the depth of every labelled pixel below the edge of its own cell, and per cell and channel the fp64 sum of the pixels of every
// depth shell in a FIXED order.  include/ribca_hip.h states both contracts, tests/localization_numpy.py restates them.
//   mask_depth<HALO, THREADS>   the inverse of expand.hip, on its tiling: one workgroup per LO_TILE x LO_TILE pixel tile, HALO the smallest of 2, 4,
//                       8, 16, 32 that holds D.  The tile and its halo go to LDS as max(label, 0), -1 outside the image: a pixel outside is never
//                       "a different pixel".  A tile without a labelled pixel writes zeros.  Otherwise the search over the disk runs in a separable
//                       form.  Phase 1: for every staged column and every row of the tile that holds a label, v = the smallest |dr| in 1 .. D at
//                       which the column carries another value inside the image (0: none).  Phase 2: a labelled pixel of label L walks its row
//                       outwards on either side; k columns away a pixel that is not L offers k^2 and ends the side, a pixel of L offers
//                       k^2 + v^2; the image edge ends a side, and so does k^2 >= the best so far.  Exact: along a run of L in the row, "differs
//                       from the pixel of this column" IS "differs from L", so the column minima are those of L, and the disk's minimum is the
//                       minimum over the columns of k^2 + the column's minimum; a column behind a pixel that is not L offers more than that
//                       pixel does.  Integers only, no atomics.
//   cell_shell_sums_small / cell_shell_sums   the three forms of intensities.hip, keyed by the shell of every pixel: one wave per box of at most
//                       LO_SMALL_BOX pixels, else one 256-thread workgroup per cell, resident (offsets and shells of at most LO_RESIDENT pixels
//                       in LDS) or streaming (the box walked again per channel, the compaction rank carried across chunks).  Element e of the cell
//                       in row-major order reaches partial e mod 256 whatever its shell; the thread that owns a partial keeps one accumulator per
//                       shell in registers (eight, selected by predicates: no indexed register array, nothing in scratch) and adds the element to
//                       the one of its shell only.  Pixel counts per shell and the deepest pixel: integer lane tallies, reduced by shuffles.
// No floating-point atomics, no loop that waits for another thread; every loop is bounded by the box, D or LO_RESIDENT.
#include <limits.h>
#include <stdint.h>

#include "../../include/ribca_hip.h"
#include "ribca_cellbox.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

#pragma clang fp contract(off)      // every addition of the shell sums rounds on its own, as the restatement does

namespace ribca {
namespace {

constexpr int LO_TILE = 32;                   // pixels of a workgroup's tile along either axis (ops.DEPTH_TILE)
constexpr int LO_D_MAX = 32;
constexpr int LO_BATCH = 6;                   // staged pixels a thread reads at once
constexpr int LO_RESERVED = 256;              // bytes of the workspace: the kernel keeps everything in LDS and does not touch it

constexpr int LO_THREADS = 256;               // threads of a workgroup = partials of the stated sum
constexpr int LO_RESIDENT = 4096;             // = IN_RESIDENT of intensities.hip (ops.INTENSITY_RESIDENT)
constexpr int LO_SMALL_BOX = 1024;            // = IN_SMALL_BOX (ops.INTENSITY_SMALL_BOX)
constexpr int LO_C_MAX = 64;
constexpr int LO_S_MAX = 8;
constexpr int LO_N_MAX = 1 << 21;
constexpr int LO_HW_MAX = 65535;

static_assert((LO_TILE + 2 * LO_D_MAX) * (LO_TILE + 2 * LO_D_MAX) * 4 + LO_TILE * (LO_TILE + 2 * LO_D_MAX) <= 64 * 1024, "LDS of mask_depth at D = 32");
static_assert(LO_D_MAX <= 255, "v of phase 1 is a byte");
static_assert(LO_THREADS == 256, "thread t holds partial t of the 256; the tree below is written for four waves");

int fail(const char* msg) { return api_fail(msg); }

// grid: the tiles in row-major order, tiles_x of them per row of tiles; THREADS threads per workgroup.  1 <= D <= HALO.
template <int HALO, int THREADS>
__global__ __launch_bounds__(THREADS) void mask_depth_kernel(const int32_t* __restrict__ mask, int H, int W, int D, int tiles_x, int32_t* __restrict__ depth2) {
  constexpr int SIDE = LO_TILE + 2 * HALO;      // the staged square
  __shared__ int lab[SIDE * SIDE];              // max(label, 0); -1 outside the image
  __shared__ uint8_t vd[LO_TILE * SIDE];        // phase 1, per (row of the tile, staged column) with a label: the smallest |dr| with another value, 0 without one
  const int tid = threadIdx.x;
  const int r0 = (int)(blockIdx.x / (unsigned)tiles_x) * LO_TILE, c0 = (int)(blockIdx.x % (unsigned)tiles_x) * LO_TILE;
  int has_label = 0;
  for (int e0 = tid; e0 < SIDE * SIDE; e0 += THREADS * LO_BATCH) {      // LO_BATCH global reads are issued before the first of them is used
    int32_t m[LO_BATCH];
    bool inside[LO_BATCH];
#pragma unroll
    for (int u = 0; u < LO_BATCH; ++u) {
      const int e = e0 + THREADS * u;
      const int r = r0 + e / SIDE - HALO, c = c0 + e % SIDE - HALO;
      inside[u] = e < SIDE * SIDE && r >= 0 && r < H && c >= 0 && c < W;
      m[u] = inside[u] ? mask[(size_t)r * W + c] : 0;
    }
#pragma unroll
    for (int u = 0; u < LO_BATCH; ++u) {
      const int e = e0 + THREADS * u;
      if (e >= SIDE * SIDE) continue;
      const int lr = e / SIDE - HALO, lc = e % SIDE - HALO;
      lab[e] = inside[u] ? (m[u] > 0 ? m[u] : 0) : -1;
      has_label |= (m[u] > 0 && lr >= 0 && lr < LO_TILE && lc >= 0 && lc < LO_TILE) ? 1 : 0;
    }
  }
  const int any_label = __syncthreads_or(has_label);      // a barrier: lab is complete behind it
  if (!any_label) {      // uniform over the workgroup: background only
    for (int e = tid; e < LO_TILE * LO_TILE; e += THREADS) {
      const int r = r0 + e / LO_TILE, c = c0 + e % LO_TILE;
      if (r < H && c < W) depth2[(size_t)r * W + c] = 0;
    }
    return;
  }
  for (int e = tid; e < LO_TILE * SIDE; e += THREADS) {
    const int base = (e / SIDE + HALO) * SIDE + e % SIDE;
    const int own = lab[base];
    int v = 0;
    if (own > 0) {      // phase 2 reads v under a label only
      for (int k = 1; k <= D; ++k) {      // rows base -+ k SIDE lie in the staged square: k <= D <= HALO
        const int a = lab[base - k * SIDE], b = lab[base + k * SIDE];
        if ((a >= 0 && a != own) || (b >= 0 && b != own)) {
          v = k;
          break;
        }
      }
    }
    vd[e] = (uint8_t)v;
  }
  __syncthreads();
  const int reach = D * D;
  for (int e = tid; e < LO_TILE * LO_TILE; e += THREADS) {
    const int row = e / LO_TILE, col = e % LO_TILE;
    const int r = r0 + row, c = c0 + col;
    if (r >= H || c >= W) continue;
    const size_t p = (size_t)r * W + c;
    const int at = (row + HALO) * SIDE + col + HALO, g = row * SIDE + col + HALO;      // columns -+ k lie in the staged row: k <= D <= HALO
    const int own = lab[at];
    if (own <= 0) {
      depth2[p] = 0;
      continue;
    }
    const int v0 = vd[g];
    int best = v0 ? v0 * v0 : reach + 1;
    for (int side = -1; side <= 1; side += 2) {
      // outwards: a column k away offers k^2 at the least, so from k^2 >= best on nothing improves -- the walk costs what the edge is away, not D
      for (int k = 1; k <= D && k * k < best; ++k) {
        const int x = lab[at + side * k];
        if (x < 0) break;      // the image ends here: nothing beyond it counts
        if (x != own) {
          best = k * k;
          break;
        }
        const int v = vd[g + side * k];
        if (v) best = min(best, k * k + v * v);
      }
    }
    depth2[p] = best <= reach ? best : -1;
  }
}

bool depth_sizes_ok(int H, int W, int D) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) && D >= 1 && D <= LO_D_MAX; }

bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

// ---- shell sums ----------------------------------------------------------------------------------------------------------------------------------
struct Edges {
  int32_t e2[LO_S_MAX - 1];      // the S - 1 squared edges, INT32_MAX behind them: no depth passes those
  int32_t S;
};

// a pixel deeper than the depth search went is in the last shell; any other in shell #{j : d > e2[j]}
__device__ __forceinline__ int shell_of(const Edges& ed, int d) {
  if (d == -1) return ed.S - 1;
  int s = 0;
#pragma unroll
  for (int j = 0; j < LO_S_MAX - 1; ++j) s += d > ed.e2[j] ? 1 : 0;
  return s;
}

__device__ __forceinline__ int wave_sum(int x) {      // lane 0 holds the total
  for (int s = 32; s >= 1; s >>= 1) x += __shfl_down(x, s);
  return x;
}
__device__ __forceinline__ int wave_max(int x) {
  for (int s = 32; s >= 1; s >>= 1) x = max(x, __shfl_down(x, s));
  return x;
}

// what a thread tallies over the pixels of the cell it looks at: pixels per shell, the largest depth2, whether one was -1
struct Tally {
  int cnt[LO_S_MAX];
  int deep, beyond;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < LO_S_MAX; ++k) cnt[k] = 0;
    deep = 0, beyond = 0;
  }
  __device__ __forceinline__ void add(int d, int s) {
#pragma unroll
    for (int k = 0; k < LO_S_MAX; ++k) cnt[k] += s == k ? 1 : 0;
    deep = max(deep, d), beyond |= d == -1 ? 1 : 0;
  }
  __device__ __forceinline__ void reduce_wave() {
#pragma unroll
    for (int k = 0; k < LO_S_MAX; ++k) cnt[k] = wave_sum(cnt[k]);
    deep = wave_max(deep), beyond = wave_max(beyond);
  }
};

// p[k] += v for the k that is s: eight predicated adds, so that p stays in registers
__device__ __forceinline__ void add_to_shell(double (&p)[LO_S_MAX], int s, double v) {
#pragma unroll
  for (int k = 0; k < LO_S_MAX; ++k) p[k] = s == k ? p[k] + v : p[k];
}

struct SmallShells {
  int32_t offs[LO_SMALL_BOX];
  uint8_t shell[LO_SMALL_BOX];
};

// one wave per cell; the barriers are those of a one-wave workgroup: they order its LDS writes before the reads of other lanes
__global__ __launch_bounds__(64) void cell_shell_sums_small_kernel(const float* __restrict__ image, int C, int H, int W, const int32_t* __restrict__ mask,
                                                                   const int32_t* __restrict__ depth2, const int32_t* __restrict__ ids,
                                                                   const int32_t* __restrict__ bbox, Edges ed, int32_t* __restrict__ count,
                                                                   int32_t* __restrict__ deepest, double* __restrict__ sums) {
  __shared__ SmallShells sh;
  const int lane = threadIdx.x;
  const size_t cell = blockIdx.x;
  const int32_t id = ids[cell];
  const int S = ed.S;
  const size_t HW = (size_t)H * W;
  const Box box = clipped_box(bbox + cell * 4, id, H, W);
  if (box.total > (unsigned)LO_SMALL_BOX) return;      // cell_shell_sums'
  unsigned a = 0;
  Tally tally;
  tally.clear();
  for (unsigned base = 0; base < box.total; base += 64) {
    const unsigned e = base + lane;
    bool in = false;
    int off = 0, s = 0;
    if (e < box.total) {
      off = (box.r0 + (int)(e / (unsigned)box.bw)) * W + box.c0 + (int)(e % (unsigned)box.bw);
      in = mask[off] == id;
    }
    if (in) {
      const int d = depth2[off];
      s = shell_of(ed, d);
      tally.add(d, s);
    }
    const unsigned long long b = __ballot(in);
    if (in) {
      const unsigned at = a + (unsigned)__popcll(b & ((1ull << lane) - 1ull));      // < box.total <= LO_SMALL_BOX
      sh.offs[at] = off;
      sh.shell[at] = (uint8_t)s;
    }
    a += (unsigned)__popcll(b);
  }
  tally.reduce_wave();
  if (lane == 0) {
    int32_t* __restrict__ out_count = count + cell * S;
#pragma unroll
    for (int k = 0; k < LO_S_MAX; ++k)
      if (k < S) out_count[k] = tally.cnt[k];
    deepest[cell] = tally.beyond ? -1 : tally.deep;
  }
  double* __restrict__ out_sums = sums + cell * C * S;
  if (a == 0) {
    for (int e = lane; e < C * S; e += 64) out_sums[e] = 0.0;
    return;
  }
  __syncthreads();      // offs and shell are written
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ plane = image + (size_t)c * HW;
    double p[4][LO_S_MAX];      // the partials lane + 64 u, one accumulator per shell
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < LO_S_MAX; ++k) p[u][k] = 0.0;
    for (unsigned base = 0; base < a; base += 256) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned j = base + 64 * u + lane;
        if (j < a) add_to_shell(p[u], sh.shell[j], (double)plane[sh.offs[j]]);
      }
    }
#pragma unroll
    for (int k = 0; k < LO_S_MAX; ++k) {
      double x = (p[0][k] + p[2][k]) + (p[1][k] + p[3][k]);      // s = 128, then s = 64
      for (int s = 32; s >= 1; s >>= 1) x += __shfl_down(x, s);
      if (lane == 0 && k < S) out_sums[c * S + k] = x;
    }
  }
}

struct Shells {
  int32_t offs[LO_RESIDENT];             // pixel offsets r W + c of the cell, row-major order
  uint8_t shell[LO_RESIDENT];            // and the shell of each
  double red[LO_S_MAX][LO_THREADS];
  float stage[LO_THREADS];               // streaming form: the chunk's values at (rank mod 256)
  uint8_t stage_shell[LO_THREADS];       //                 and their shells
  int wave_tot[2][4];
  int tally[4][LO_S_MAX + 2];            // per wave: the counts, the deepest, beyond
};
static_assert(sizeof(Shells) <= 64 * 1024, "LDS of cell_shell_sums");

// the stated tree over the 256 partials of every shell: s = 128, 64 through LDS, s = 32 .. 1 by shuffles, wave w takes the shells w and w + 4
__device__ __forceinline__ void tree_out(Shells& sh, const double (&p)[LO_S_MAX], int S, double* __restrict__ out) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int k = 0; k < LO_S_MAX; ++k)
    if (k < S) sh.red[k][t] = p[k];
  __syncthreads();
  for (int k = wave; k < S; k += 4) {
    double x = (sh.red[k][lane] + sh.red[k][lane + 128]) + (sh.red[k][lane + 64] + sh.red[k][lane + 192]);
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_down(x, s);      // lanes >= s hold values nobody reads
    if (lane == 0) out[k] = x;
  }
  __syncthreads();      // red is free for the next channel
}

__global__ __launch_bounds__(LO_THREADS) void cell_shell_sums_kernel(const float* __restrict__ image, int C, int H, int W, const int32_t* __restrict__ mask,
                                                                     const int32_t* __restrict__ depth2, const int32_t* __restrict__ ids,
                                                                     const int32_t* __restrict__ bbox, Edges ed, int32_t* __restrict__ count,
                                                                     int32_t* __restrict__ deepest, double* __restrict__ sums) {
  __shared__ Shells sh;
  const int t = threadIdx.x;
  const size_t cell = blockIdx.x;
  const int32_t id = ids[cell];
  const int S = ed.S;
  const size_t HW = (size_t)H * W;
  const Box box = clipped_box(bbox + cell * 4, id, H, W);
  if (box.total <= (unsigned)LO_SMALL_BOX) return;      // cell_shell_sums_small's

  // the area, the tallies, and the first LO_RESIDENT offsets and shells
  unsigned a = 0;
  int parity = 0;
  Tally tally;
  tally.clear();
  for (unsigned base = 0; base < box.total; base += LO_THREADS, parity ^= 1) {
    const unsigned e = base + t;
    bool in = false;
    int off = 0, s = 0;
    if (e < box.total) {
      off = (box.r0 + (int)(e / (unsigned)box.bw)) * W + box.c0 + (int)(e % (unsigned)box.bw);
      in = mask[off] == id;
    }
    if (in) {
      const int d = depth2[off];
      s = shell_of(ed, d);
      tally.add(d, s);
    }
    int m;
    const unsigned at = a + (unsigned)chunk_rank(sh.wave_tot, in, parity, m);
    if (in && at < (unsigned)LO_RESIDENT) sh.offs[at] = off, sh.shell[at] = (uint8_t)s;
    a += (unsigned)m;
  }
  tally.reduce_wave();
  if ((t & 63) == 0) {
    int* __restrict__ mine = sh.tally[t >> 6];
#pragma unroll
    for (int k = 0; k < LO_S_MAX; ++k) mine[k] = tally.cnt[k];
    mine[LO_S_MAX] = tally.deep, mine[LO_S_MAX + 1] = tally.beyond;
  }
  __syncthreads();      // offs, shell and tally are written
  if (t < S) count[cell * S + t] = sh.tally[0][t] + sh.tally[1][t] + sh.tally[2][t] + sh.tally[3][t];
  if (t == 0) {
    const int deep = max(max(sh.tally[0][LO_S_MAX], sh.tally[1][LO_S_MAX]), max(sh.tally[2][LO_S_MAX], sh.tally[3][LO_S_MAX]));
    const int beyond = sh.tally[0][LO_S_MAX + 1] | sh.tally[1][LO_S_MAX + 1] | sh.tally[2][LO_S_MAX + 1] | sh.tally[3][LO_S_MAX + 1];
    deepest[cell] = beyond ? -1 : deep;
  }
  double* __restrict__ out_sums = sums + cell * C * S;
  if (a == 0) {
    for (int e = t; e < C * S; e += LO_THREADS) out_sums[e] = 0.0;
    return;
  }

  if (a <= (unsigned)LO_RESIDENT) {
    for (int c = 0; c < C; ++c) {
      const float* __restrict__ plane = image + (size_t)c * HW;
      double p[LO_S_MAX];
#pragma unroll
      for (int k = 0; k < LO_S_MAX; ++k) p[k] = 0.0;
      for (unsigned j = t; j < a; j += LO_THREADS) add_to_shell(p, sh.shell[j], (double)plane[sh.offs[j]]);      // thread t IS partial t
      tree_out(sh, p, S, out_sums + c * S);
    }
    return;
  }

  // streaming form: element j of the cell goes to partial j mod 256 through sh.stage, its shell beside it
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ plane = image + (size_t)c * HW;
    double p[LO_S_MAX];
#pragma unroll
    for (int k = 0; k < LO_S_MAX; ++k) p[k] = 0.0;
    unsigned seen = 0;
    int par = 0;
    for (unsigned base = 0; base < box.total; base += LO_THREADS, par ^= 1) {
      const unsigned e = base + t;
      bool in = false;
      float v = 0.f;
      int s = 0;
      if (e < box.total) {
        const int off = (box.r0 + (int)(e / (unsigned)box.bw)) * W + box.c0 + (int)(e % (unsigned)box.bw);
        in = mask[off] == id;
        if (in) v = plane[off], s = shell_of(ed, depth2[off]);
      }
      int m;
      const unsigned at = seen + (unsigned)chunk_rank(sh.wave_tot, in, par, m);
      if (in) sh.stage[at & 255u] = v, sh.stage_shell[at & 255u] = (uint8_t)s;
      __syncthreads();
      if (((unsigned)t - seen & 255u) < (unsigned)m)      // slot t was written in this chunk: the ranks seen .. seen + m - 1, m <= 256
        add_to_shell(p, sh.stage_shell[t], (double)sh.stage[t]);
      seen += (unsigned)m;
      // the next write of stage comes behind the barrier of the next chunk_rank
    }
    tree_out(sh, p, S, out_sums + c * S);
  }
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_mask_depth_ws_bytes(int32_t H, int32_t W, int32_t D) {
  if (!depth_sizes_ok(H, W, D)) return 0;
  Carver cv(nullptr);
  cv.take<uint8_t>(LO_RESERVED);
  return (int64_t)cv.off;
}

int ribca_mask_depth(const int32_t* mask, int32_t H, int32_t W, int32_t D, int32_t* depth2, void* ws, int64_t ws_bytes, void* stream) {
  if (!mask || !depth2 || !ws) return fail("ribca_mask_depth: NULL buffer");
  if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return fail("ribca_mask_depth: needs 1 <= H, W and H W < 2^31");
  if (D < 1 || D > LO_D_MAX) return fail("ribca_mask_depth: needs 1 <= D <= 32");
  if (overlap(mask, depth2, (size_t)H * W * sizeof(int32_t))) return fail("ribca_mask_depth: mask and depth2 must not overlap");
  if (ws_bytes < ribca_mask_depth_ws_bytes(H, W, D)) return fail("ribca_mask_depth: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int tiles_x = (W + LO_TILE - 1) / LO_TILE, tiles_y = (H + LO_TILE - 1) / LO_TILE;      // tiles_x tiles_y < 2^31 / 1024 + H + W
  const dim3 grid((unsigned)((long long)tiles_x * tiles_y));
  // as for expand.hip: the wide halos hold few workgroups per CU in LDS, so each gets more threads to run the dependent LDS reads behind
  if (D <= 2) hipLaunchKernelGGL((mask_depth_kernel<2, 256>), grid, dim3(256), 0, s, mask, H, W, D, tiles_x, depth2);
  else if (D <= 4) hipLaunchKernelGGL((mask_depth_kernel<4, 256>), grid, dim3(256), 0, s, mask, H, W, D, tiles_x, depth2);
  else if (D <= 8) hipLaunchKernelGGL((mask_depth_kernel<8, 256>), grid, dim3(256), 0, s, mask, H, W, D, tiles_x, depth2);
  else if (D <= 16) hipLaunchKernelGGL((mask_depth_kernel<16, 512>), grid, dim3(512), 0, s, mask, H, W, D, tiles_x, depth2);
  else hipLaunchKernelGGL((mask_depth_kernel<32, 1024>), grid, dim3(1024), 0, s, mask, H, W, D, tiles_x, depth2);
  RIBCA_FINISH();
  return 0;
}

int ribca_cell_shell_sums(const float* image, int32_t C, int32_t H, int32_t W, const int32_t* mask, const int32_t* depth2, const int32_t* ids,
                          const int32_t* bbox, int32_t n, const int32_t* edges2, int32_t S, int32_t* count, int32_t* deepest, double* sums, void* stream) {
  if (n == 0) return 0;
  if (!image || !mask || !depth2 || !ids || !bbox || !edges2 || !count || !deepest || !sums) return fail("ribca_cell_shell_sums: NULL buffer");
  if (C < 1 || C > LO_C_MAX) return fail("ribca_cell_shell_sums: needs 1 <= C <= 64");
  if (H < 1 || W < 1 || H > LO_HW_MAX || W > LO_HW_MAX || (long long)H * W >= (1ll << 31))
    return fail("ribca_cell_shell_sums: needs 1 <= H, W <= 65535 and H W < 2^31");
  if (n < 1 || n > LO_N_MAX) return fail("ribca_cell_shell_sums: needs 1 <= n <= 2^21");
  if (S < 2 || S > LO_S_MAX) return fail("ribca_cell_shell_sums: needs 2 <= S <= 8");
  Edges ed;
  ed.S = S;
  for (int j = 0; j < LO_S_MAX - 1; ++j) {
    ed.e2[j] = j < S - 1 ? edges2[j] : INT32_MAX;      // edges2 is a HOST array
    if (j < S - 1 && (ed.e2[j] < 1 || (j > 0 && ed.e2[j] <= ed.e2[j - 1]))) return fail("ribca_cell_shell_sums: needs 1 <= edges2[0] < edges2[1] < ...");
  }
  hipLaunchKernelGGL(cell_shell_sums_small_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, image, C, H, W, mask, depth2, ids, bbox, ed, count,
                     deepest, sums);
  hipLaunchKernelGGL(cell_shell_sums_kernel, dim3((unsigned)n), dim3(LO_THREADS), 0, (hipStream_t)stream, image, C, H, W, mask, depth2, ids, bbox, ed, count,
                     deepest, sums);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
