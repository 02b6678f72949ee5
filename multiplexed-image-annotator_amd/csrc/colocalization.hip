// Per-cell marker colocalisation over the cell's own pixels (Annotator.marker_colocalization; CellProfiler's MeasureColocalization): for K
// selected channels the fp64 sums, the centred cross products of every channel pair and the sums of one channel over the pixels where another
// is above its gate, all in the FIXED order of intensities.hip (256 strided partials and a halving tree), and the pixel counts above both gates
// of every pair.  include/ribca_hip.h states the contract, tests/coloc_numpy.py restates it.
// One kernel, one 256-thread workgroup per cell.  It walks the clipped box in chunks of 256 pixels in row-major order and compacts the offsets
// of the cell's pixels into LDS with the ballot scan of ribca_cellbox.h, which also counts the area.
//   resident form    area <= CO_RESIDENT: beside the offsets, LDS holds one gate word per pixel (bit k: channel k above its gate).  The work is
//                    cut into TASKS that are handed out over the four waves and run without a barrier: a channel's sum; a CO_B x CO_B block of
//                    channel pairs of the cross products; a block of the gated sums.  A wave works its task in the wave form of
//                    cell_intensities_small: a lane holds the partials lane, lane + 64, lane + 128, lane + 192 of all 16 sums of the block in
//                    registers -- chosen by compile-time indices --, reloads the values through the offsets, and the 16 trees run by shuffles.
//                    The means of all K channels are finished, behind one barrier, before the first cross block.
//   streaming form   any larger label: the box is walked again per task with the compaction rank carried across chunks, so that element j
//                    still reaches partial j mod 256 through a 256-slot LDS stage; thread t IS partial t and the 16 trees of a block run
//                    through LDS, four per wave.
// The counts are integer adds in registers (a thread per pair) in both forms: no atomics at all.  Nothing is indexed by a label, a pixel or a
// runtime channel number outside LDS; no loop waits for another thread; every loop is bounded by the box, by K or by a constant.
// Measured form: DESIGN.md section 27.
#include <stdint.h>

#include "../../include/ribca_hip.h"
#include "ribca_cellbox.h"
#include "ribca_common.h"
#include "ribca_status.h"

#pragma clang fp contract(off)      // difference, product and sum round one operation at a time, as the restatement does

namespace ribca {
namespace {

constexpr int CO_THREADS = 256;               // threads of a workgroup = partials of the stated sum
constexpr int CO_RESIDENT = 4096;             // pixels of a cell whose offsets and gate words stay in LDS (ops.COLOC_RESIDENT)
constexpr int CO_B = 4;                       // channels on a side of a register block
constexpr int CO_BB = CO_B * CO_B;
constexpr int CO_K_MAX = 32;                  // a gate word is 32 bits
constexpr int CO_P_MAX = CO_K_MAX * (CO_K_MAX + 1) / 2;
constexpr int CO_PAIRS_PER_THREAD = (CO_P_MAX + CO_THREADS - 1) / CO_THREADS;
constexpr int CO_C_MAX = 64;
constexpr int CO_N_MAX = 1 << 21;
constexpr int CO_HW_MAX = 65535;

static_assert(CO_THREADS == 256, "thread t holds partial t of the 256; the trees below are written for four waves");
static_assert(CO_RESIDENT % CO_THREADS == 0, "the compaction keeps whole chunks");
static_assert(CO_K_MAX % CO_B == 0 && CO_BB % 4 == 0, "whole blocks; the streaming trees go four to a wave");

int fail(const char* msg) { return api_fail(msg); }

struct Selection {
  int32_t chan[CO_K_MAX];      // the K selected channels, 0 behind them
  float thr[CO_K_MAX];         // and their gates
  int32_t K;
};

struct Shared {
  union {
    struct {
      int32_t offs[CO_RESIDENT];       // pixel offsets r W + c of the cell, row-major order
      uint32_t gate[CO_RESIDENT];      // bit k: the value of channel k at that pixel is above thr[k]
    } res;
    double red[CO_BB][CO_THREADS];     // streaming form: the partials of a block's 16 sums
  };
  float stage[2 * CO_B][CO_THREADS];   // streaming form: the chunk's values at (rank mod 256), a block's channels
  uint32_t stage_gate[CO_THREADS];     //                 and their gate words
  double mean[CO_K_MAX];
  int32_t chan[CO_K_MAX];
  float thr[CO_K_MAX];
  int wave_tot[2][4];
};
static_assert(sizeof(Shared) <= 64 * 1024, "LDS of cell_coloc");

// index of the pair (k, l), k <= l, in the order (0,0), (0,1) .. (0,K-1), (1,1) ..
__device__ __forceinline__ int pair_index(int k, int l, int K) { return k * K - k * (k - 1) / 2 + (l - k); }

// the gate bits both[] pair p asks for; 0 for p >= P (no pixel has "all of no bits" counted: the caller skips it)
__device__ __forceinline__ uint32_t pair_bits(int p, int K) {
  int k = 0;
  for (int row = K; k < K && p >= row; --row) p -= row, ++k;      // at most K steps
  return k < K ? (1u << k) | (1u << (k + p)) : 0u;
}

// the stated tree over the 256 partials a wave holds four to a lane (lane, + 64, + 128, + 192): s = 128, s = 64, then the shuffles; lane 0
__device__ __forceinline__ double wave_tree(double p0, double p1, double p2, double p3) {
  double x = (p0 + p2) + (p1 + p3);
  for (int s = 32; s >= 1; s >>= 1) x += __shfl_down(x, s);      // lanes >= s hold values nobody reads
  return x;
}

// acc[i][j] += dr[i] * dc[j]: the 16 centred products of a block, every operation rounded on its own
__device__ __forceinline__ void cross_add(double (&acc)[CO_B][CO_B], const double (&dr)[CO_B], const double (&dc)[CO_B]) {
#pragma unroll
  for (int i = 0; i < CO_B; ++i)
#pragma unroll
    for (int j = 0; j < CO_B; ++j) acc[i][j] += dr[i] * dc[j];
}

// acc[i][j] += v[i] where gate j of the block (bit l0 + j of the word) is open; a closed gate skips the element
__device__ __forceinline__ void gated_add(double (&acc)[CO_B][CO_B], const double (&v)[CO_B], uint32_t word, int l0) {
#pragma unroll
  for (int i = 0; i < CO_B; ++i)
#pragma unroll
    for (int j = 0; j < CO_B; ++j) acc[i][j] = (word >> (l0 + j)) & 1u ? acc[i][j] + v[i] : acc[i][j];
}

__device__ __forceinline__ void clear(double (&acc)[CO_B][CO_B]) {
#pragma unroll
  for (int i = 0; i < CO_B; ++i)
#pragma unroll
    for (int j = 0; j < CO_B; ++j) acc[i][j] = 0.0;
}

// what a block writes: cross keeps the pairs k <= l of the block, gated every (k, l); x is valid in lane 0 (resident) / thread 0 of a wave
__device__ __forceinline__ void store_block(bool is_cross, int K, int k, int l, double x, double* __restrict__ out_cross, double* __restrict__ out_gated) {
  if (k >= K || l >= K) return;
  if (is_cross) {
    if (k <= l) out_cross[pair_index(k, l, K)] = x;
  } else {
    out_gated[k * K + l] = x;
  }
}

// task number -> (kind, row block, column block): first the nb (nb + 1) / 2 cross blocks bi <= bj, then the nb nb gated blocks
__device__ __forceinline__ void task_blocks(int task, int nb, bool& is_cross, int& bi, int& bj) {
  const int n_cross = nb * (nb + 1) / 2;
  is_cross = task < n_cross;
  if (is_cross) {
    bi = 0;
    for (int row = nb; task >= row; --row) task -= row, ++bi;      // at most nb steps
    bj = bi + task;
  } else {
    task -= n_cross;
    bi = task / nb, bj = task % nb;
  }
}

__global__ __launch_bounds__(CO_THREADS) void cell_coloc_kernel(const float* __restrict__ image, int H, int W, const int32_t* __restrict__ mask,
                                                                const int32_t* __restrict__ ids, const int32_t* __restrict__ bbox, Selection sel,
                                                                int32_t* __restrict__ area, int32_t* __restrict__ both, double* __restrict__ sums,
                                                                double* __restrict__ cross, double* __restrict__ gated) {
  __shared__ Shared sh;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);      // a task belongs to a wave: its loops are scalar
  const size_t cell = blockIdx.x;
  const int32_t id = ids[cell];
  const int K = sel.K, P = K * (K + 1) / 2, nb = (K + CO_B - 1) / CO_B;
  const int n_tasks = nb * (nb + 1) / 2 + nb * nb;
  const size_t HW = (size_t)H * W;
  const Box box = clipped_box(bbox + cell * 4, id, H, W);
  if (t < CO_K_MAX) sh.chan[t] = sel.chan[t], sh.thr[t] = sel.thr[t];

  // the area, and the first CO_RESIDENT offsets
  unsigned a = 0;
  int parity = 0;
  for (unsigned base = 0; base < box.total; base += CO_THREADS, parity ^= 1) {
    const unsigned e = base + t;
    bool in = false;
    int off = 0;
    if (e < box.total) {
      off = (box.r0 + (int)(e / (unsigned)box.bw)) * W + box.c0 + (int)(e % (unsigned)box.bw);
      in = mask[off] == id;
    }
    int m;
    const unsigned at = a + (unsigned)chunk_rank(sh.wave_tot, in, parity, m);
    if (in && at < (unsigned)CO_RESIDENT) sh.res.offs[at] = off;
    a += (unsigned)m;
  }
  int32_t* __restrict__ out_both = both + cell * P;
  double* __restrict__ out_sums = sums + cell * K;
  double* __restrict__ out_cross = cross + cell * P;
  double* __restrict__ out_gated = gated + cell * K * K;
  if (t == 0) area[cell] = (int32_t)a;
  if (a == 0) {
    for (int e = t; e < P; e += CO_THREADS) out_both[e] = 0, out_cross[e] = 0.0;
    for (int e = t; e < K; e += CO_THREADS) out_sums[e] = 0.0;
    for (int e = t; e < K * K; e += CO_THREADS) out_gated[e] = 0.0;
    return;
  }
  __syncthreads();      // offs, chan and thr are written
  const double count = (double)a;
  uint32_t want[CO_PAIRS_PER_THREAD];      // the pairs this thread counts: t, t + 256, ...
  int hits[CO_PAIRS_PER_THREAD];
#pragma unroll
  for (int q = 0; q < CO_PAIRS_PER_THREAD; ++q) want[q] = t + q * CO_THREADS < P ? pair_bits(t + q * CO_THREADS, K) : 0u, hits[q] = 0;

  if (a <= (unsigned)CO_RESIDENT) {
    // the gate words
    for (unsigned j = t; j < a; j += CO_THREADS) {
      const int off = sh.res.offs[j];
      uint32_t word = 0u;
      for (int k = 0; k < K; ++k) word |= image[(size_t)sh.chan[k] * HW + off] > sh.thr[k] ? 1u << k : 0u;
      sh.res.gate[j] = word;
    }
    // the sums and the means: a channel per wave
    for (int k = wave; k < K; k += 4) {
      const float* __restrict__ plane = image + (size_t)sh.chan[k] * HW;
      double p[4] = {0.0, 0.0, 0.0, 0.0};
      for (unsigned base = 0; base < a; base += CO_THREADS) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned j = base + 64 * u + lane;
          if (j < a) p[u] += (double)plane[sh.res.offs[j]];
        }
      }
      const double x = wave_tree(p[0], p[1], p[2], p[3]);
      if (lane == 0) out_sums[k] = x, sh.mean[k] = x / count;
    }
    __syncthreads();      // gate and mean are written
    // the counts: every thread reads the same word at a time
    for (unsigned j = 0; j < a; ++j) {
      const uint32_t word = sh.res.gate[j];
#pragma unroll
      for (int q = 0; q < CO_PAIRS_PER_THREAD; ++q) hits[q] += (word & want[q]) == want[q] ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < CO_PAIRS_PER_THREAD; ++q)
      if (want[q]) out_both[t + q * CO_THREADS] = hits[q];
    // the blocks
    for (int task = wave; task < n_tasks; task += 4) {
      bool is_cross;
      int bi, bj;
      task_blocks(task, nb, is_cross, bi, bj);
      const float* __restrict__ rows[CO_B];
      const float* __restrict__ cols[CO_B];
      double mr[CO_B], mc[CO_B];
#pragma unroll
      for (int i = 0; i < CO_B; ++i) {      // a block that reaches past K works its last channel again and stores nothing for it
        const int kr = min(bi * CO_B + i, K - 1), kc = min(bj * CO_B + i, K - 1);
        rows[i] = image + (size_t)sh.chan[kr] * HW, cols[i] = image + (size_t)sh.chan[kc] * HW;
        mr[i] = sh.mean[kr], mc[i] = sh.mean[kc];
      }
      double acc[4][CO_B][CO_B];      // [u]: the partials lane + 64 u
#pragma unroll
      for (int u = 0; u < 4; ++u) clear(acc[u]);
      for (unsigned base = 0; base < a; base += CO_THREADS) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned j = base + 64 * u + lane;
          if (j < a) {
            const int off = sh.res.offs[j];
            double dr[CO_B];
            if (is_cross) {
              double dc[CO_B];
#pragma unroll
              for (int i = 0; i < CO_B; ++i) dr[i] = (double)rows[i][off] - mr[i], dc[i] = (double)cols[i][off] - mc[i];
              cross_add(acc[u], dr, dc);
            } else {
#pragma unroll
              for (int i = 0; i < CO_B; ++i) dr[i] = (double)rows[i][off];
              gated_add(acc[u], dr, sh.res.gate[j], bj * CO_B);
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < CO_B; ++i)
#pragma unroll
        for (int j = 0; j < CO_B; ++j) {
          const double x = wave_tree(acc[0][i][j], acc[1][i][j], acc[2][i][j], acc[3][i][j]);
          if (lane == 0) store_block(is_cross, K, bi * CO_B + i, bj * CO_B + j, x, out_cross, out_gated);
        }
    }
    return;
  }

  // streaming form.  A walk hands thread t the element of rank = t (mod 256) of every chunk through the stage: the values of the channels
  // ks[0 .. nv) and, with `gates`, the gate word of all K channels.  `use` runs once per element a thread owns, `chunk(first, m)` once per
  // chunk behind the barrier that publishes the stage
  auto walk = [&](const int (&ks)[2 * CO_B], int nv, bool gates, auto use, auto chunk) {
    unsigned seen = 0;
    int par = 0;
    for (unsigned base = 0; base < box.total; base += CO_THREADS, par ^= 1) {
      const unsigned e = base + t;
      bool in = false;
      int off = 0;
      if (e < box.total) {
        off = (box.r0 + (int)(e / (unsigned)box.bw)) * W + box.c0 + (int)(e % (unsigned)box.bw);
        in = mask[off] == id;
      }
      int m;
      const unsigned at = seen + (unsigned)chunk_rank(sh.wave_tot, in, par, m);
      if (in) {
        const unsigned slot = at & 255u;
#pragma unroll
        for (int i = 0; i < 2 * CO_B; ++i)
          if (i < nv) sh.stage[i][slot] = image[(size_t)sh.chan[ks[i]] * HW + off];
        if (gates) {
          uint32_t word = 0u;
          for (int k = 0; k < K; ++k) word |= image[(size_t)sh.chan[k] * HW + off] > sh.thr[k] ? 1u << k : 0u;
          sh.stage_gate[slot] = word;
        }
      }
      __syncthreads();
      if (((unsigned)t - seen & 255u) < (unsigned)m) use();      // slot t was written in this chunk: the ranks seen .. seen + m - 1, m <= 256
      chunk(seen, (unsigned)m);
      seen += (unsigned)m;
      // the next write of the stage comes behind the barrier of the next chunk_rank
    }
  };
  // the stated trees over the 256 partials of a block's 16 sums: s = 128, 64 through LDS, s = 32 .. 1 by shuffles, four sums per wave;
  // `out(i, j, x)` runs in lane 0 of the wave that holds sum (i, j)
  auto trees = [&](const double (&acc)[CO_B][CO_B], auto out) {
#pragma unroll
    for (int i = 0; i < CO_B; ++i)
#pragma unroll
      for (int j = 0; j < CO_B; ++j) sh.red[i * CO_B + j][t] = acc[i][j];
    __syncthreads();
    for (int s = wave; s < CO_BB; s += 4) {
      const double x = wave_tree(sh.red[s][lane], sh.red[s][lane + 64], sh.red[s][lane + 128], sh.red[s][lane + 192]);
      if (lane == 0) out(s / CO_B, s % CO_B, x);
    }
    __syncthreads();      // red is free for the next block, and what `out` wrote to LDS is published
  };
  auto no_chunk = [](unsigned, unsigned) {};
  int ks[2 * CO_B];
  double acc[CO_B][CO_B];

  // the sums and the means, CO_B channels to a walk (row 0 of the block holds them), and in the first walk the counts
  for (int b = 0; b < nb; ++b) {
#pragma unroll
    for (int i = 0; i < 2 * CO_B; ++i) ks[i] = min(b * CO_B + (i % CO_B), K - 1);
    clear(acc);
    walk(ks, CO_B, b == 0,
         [&] {
#pragma unroll
           for (int j = 0; j < CO_B; ++j) acc[0][j] += (double)sh.stage[j][t];
         },
         [&](unsigned first, unsigned m) {
           if (b != 0) return;
           for (unsigned i = 0; i < m; ++i) {      // every thread reads the same word at a time
             const uint32_t word = sh.stage_gate[(first + i) & 255u];
#pragma unroll
             for (int q = 0; q < CO_PAIRS_PER_THREAD; ++q) hits[q] += (word & want[q]) == want[q] ? 1 : 0;
           }
         });
    trees(acc, [&](int i, int j, double x) {
      const int k = b * CO_B + j;
      if (i == 0 && k < K) out_sums[k] = x, sh.mean[k] = x / count;
    });
  }
#pragma unroll
  for (int q = 0; q < CO_PAIRS_PER_THREAD; ++q)
    if (want[q]) out_both[t + q * CO_THREADS] = hits[q];

  // the blocks, a walk each
  for (int task = 0; task < n_tasks; ++task) {
    bool is_cross;
    int bi, bj;
    task_blocks(task, nb, is_cross, bi, bj);
    double mr[CO_B], mc[CO_B];
#pragma unroll
    for (int i = 0; i < CO_B; ++i) {
      ks[i] = min(bi * CO_B + i, K - 1), ks[CO_B + i] = min(bj * CO_B + i, K - 1);
      mr[i] = sh.mean[ks[i]], mc[i] = sh.mean[ks[CO_B + i]];
    }
    clear(acc);
    if (is_cross) {
      walk(ks, 2 * CO_B, false,
           [&] {
             double dr[CO_B], dc[CO_B];
#pragma unroll
             for (int i = 0; i < CO_B; ++i) dr[i] = (double)sh.stage[i][t] - mr[i], dc[i] = (double)sh.stage[CO_B + i][t] - mc[i];
             cross_add(acc, dr, dc);
           },
           no_chunk);
    } else {
      walk(ks, CO_B, true,
           [&] {
             double v[CO_B];
#pragma unroll
             for (int i = 0; i < CO_B; ++i) v[i] = (double)sh.stage[i][t];
             gated_add(acc, v, sh.stage_gate[t], bj * CO_B);
           },
           no_chunk);
    }
    trees(acc, [&](int i, int j, double x) { store_block(is_cross, K, bi * CO_B + i, bj * CO_B + j, x, out_cross, out_gated); });
  }
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int ribca_cell_coloc(const float* image, int32_t C, int32_t H, int32_t W, const int32_t* mask, const int32_t* ids, const int32_t* bbox, int32_t n,
                     const int32_t* chan, const float* thr, int32_t K, int32_t* area, int32_t* both, double* sums, double* cross, double* gated,
                     void* stream) {
  if (n == 0) return 0;
  if (!image || !mask || !ids || !bbox || !chan || !thr || !area || !both || !sums || !cross || !gated) return fail("ribca_cell_coloc: NULL buffer");
  if (C < 1 || C > CO_C_MAX) return fail("ribca_cell_coloc: needs 1 <= C <= 64");
  if (H < 1 || W < 1 || H > CO_HW_MAX || W > CO_HW_MAX || (long long)H * W >= (1ll << 31))
    return fail("ribca_cell_coloc: needs 1 <= H, W <= 65535 and H W < 2^31");
  if (n < 1 || n > CO_N_MAX) return fail("ribca_cell_coloc: needs 1 <= n <= 2^21");
  if (K < 2 || K > CO_K_MAX) return fail("ribca_cell_coloc: needs 2 <= K <= 32");
  Selection sel;
  sel.K = K;
  for (int k = 0; k < CO_K_MAX; ++k) {
    sel.chan[k] = k < K ? chan[k] : 0, sel.thr[k] = k < K ? thr[k] : 0.f;      // chan and thr are HOST arrays
    if (k >= K) continue;
    if (sel.chan[k] < 0 || sel.chan[k] >= C) return fail("ribca_cell_coloc: needs 0 <= chan[k] < C");
    for (int j = 0; j < k; ++j)
      if (sel.chan[j] == sel.chan[k]) return fail("ribca_cell_coloc: chan holds a channel twice");
    if (!__builtin_isfinite(sel.thr[k])) return fail("ribca_cell_coloc: needs a finite thr[k]");
  }
  hipLaunchKernelGGL(cell_coloc_kernel, dim3((unsigned)n), dim3(CO_THREADS), 0, (hipStream_t)stream, image, H, W, mask, ids, bbox, sel, area, both,
                     sums, cross, gated);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
