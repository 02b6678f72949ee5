// Grows the labels of a segmentation mask by D pixels (ImageProcessor(expand_mask=D); scikit-image's expand_labels, steinbock / MCMICRO / QuPath
// "cell expansion" of a nuclear mask): every pixel without a label within Euclidean distance D of a labelled pixel takes the label of the
// nearest one, the SMALLEST label among those at exactly the smallest squared distance.  Integers only: include/ribca_hip.h states the contract,
// tests/expand_numpy.py restates it.
//   expand_tile<HALO, THREADS>   one workgroup per EX_TILE x EX_TILE pixel tile, HALO the smallest of 2, 4, 8, 16, 32 that holds D, 256 threads
//                       up to a halo of 8, 512 at 16 and 1024 at 32, where LDS leaves room for few workgroups per CU.  The tile and a halo
//                       of HALO pixels go to LDS as max(label, 0) (0 also outside the image), one global read per staged pixel.  A tile whose
//                       staged square holds no label, or whose own pixels hold no background, copies through.  Otherwise the search runs in
//                       its separable form.  Phase 1: for every staged column and every row of the tile the lexicographic minimum of
//                       (dr^2, label) over |dr| <= D -- the rows are tried outwards and the first distance with a label ends the loop, a
//                       larger dr^2 never wins within one column.  Phase 2: for every background pixel of the tile the lexicographic minimum
//                       of (dc^2 + g, label) over the columns |dc| <= D, tried outwards until dc^2 passes the best so far.  dc^2 is
//                       constant within a column, so the minimum over the disk is the minimum over the columns of the column minima:
//                       exact, ties included.  Lanes of a wave walk consecutive columns in both phases: the LDS reads are unit-stride.
// Tables in LDS, scalars in registers: nothing goes to scratch.  No atomics, and no loop waits for another thread.  Measured form: DESIGN.md
// section 22.
#include <limits.h>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

namespace ribca {
namespace {

constexpr int EX_TILE = 32;                   // pixels of a workgroup's tile along either axis
constexpr int EX_D_MAX = 32;
constexpr int EX_BATCH = 6;                   // staged pixels a thread reads at once
constexpr int EX_RESERVED = 256;              // bytes of the workspace: the kernel keeps everything in LDS and does not touch it

static_assert((EX_TILE + 2 * EX_D_MAX) * (EX_TILE + 2 * EX_D_MAX) * 4 + EX_TILE * (EX_TILE + 2 * EX_D_MAX) * 8 <= 64 * 1024, "LDS of expand_tile at D = 32");

int fail(const char* msg) { return api_fail(msg); }

// grid: the tiles in row-major order, tiles_x of them per row of tiles; THREADS threads per workgroup.  1 <= D <= HALO.
template <int HALO, int THREADS>
__global__ __launch_bounds__(THREADS) void expand_tile_kernel(const int32_t* __restrict__ mask, int H, int W, int D, int tiles_x, int32_t* __restrict__ out,
                                                          int32_t* __restrict__ dist2) {
  constexpr int SIDE = EX_TILE + 2 * HALO;      // the staged square
  __shared__ int lab[SIDE * SIDE];              // max(label, 0)
  __shared__ int gd[EX_TILE * SIDE];            // phase 1, per (row of the tile, staged column): the smallest dr^2 with a label, -1 without one
  __shared__ int gl[EX_TILE * SIDE];            //          and the smallest label at it
  const int tid = threadIdx.x;
  const int r0 = (int)(blockIdx.x / (unsigned)tiles_x) * EX_TILE, c0 = (int)(blockIdx.x % (unsigned)tiles_x) * EX_TILE;
  int has_label = 0, has_bg = 0;
  // EX_BATCH global reads are issued before the first of them is used: at D = 32 a thread stages 36 pixels and two workgroups share a CU
  for (int e0 = tid; e0 < SIDE * SIDE; e0 += THREADS * EX_BATCH) {
    int32_t m[EX_BATCH];
    bool inside[EX_BATCH];
#pragma unroll
    for (int u = 0; u < EX_BATCH; ++u) {
      const int e = e0 + THREADS * u;
      const int r = r0 + e / SIDE - HALO, c = c0 + e % SIDE - HALO;
      inside[u] = e < SIDE * SIDE && r >= 0 && r < H && c >= 0 && c < W;
      m[u] = inside[u] ? mask[(size_t)r * W + c] : 0;
    }
#pragma unroll
    for (int u = 0; u < EX_BATCH; ++u) {
      const int e = e0 + THREADS * u;
      if (e >= SIDE * SIDE) continue;
      const int lr = e / SIDE - HALO, lc = e % SIDE - HALO;
      const int v = m[u] > 0 ? m[u] : 0;
      has_bg |= (inside[u] && m[u] <= 0 && lr >= 0 && lr < EX_TILE && lc >= 0 && lc < EX_TILE) ? 1 : 0;
      lab[e] = v;
      has_label |= v > 0 ? 1 : 0;
    }
  }
  const int any_label = __syncthreads_or(has_label);      // both are barriers: lab is complete behind them
  const int any_bg = __syncthreads_or(has_bg);
  if (!any_label || !any_bg) {      // uniform over the workgroup: nothing to grow from, or nothing to grow into
    for (int e = tid; e < EX_TILE * EX_TILE; e += THREADS) {
      const int r = r0 + e / EX_TILE, c = c0 + e % EX_TILE;
      if (r >= H || c >= W) continue;
      const size_t p = (size_t)r * W + c;
      const int32_t m = mask[p];
      out[p] = m;
      if (dist2) dist2[p] = m > 0 ? 0 : -1;
    }
    return;
  }
  for (int e = tid; e < EX_TILE * SIDE; e += THREADS) {
    const int base = (e / SIDE + HALO) * SIDE + e % SIDE;
    int d = -1, l = lab[base];
    if (l > 0) {
      d = 0;
    } else {
      for (int k = 1; k <= D; ++k) {      // rows base -+ k SIDE lie in the staged square: k <= D <= HALO
        const int a = lab[base - k * SIDE], b = lab[base + k * SIDE];
        if (a > 0 || b > 0) {
          l = a > 0 && (b <= 0 || a < b) ? a : b;
          d = k * k;
          break;
        }
      }
    }
    gd[e] = d;
    gl[e] = l;
  }
  __syncthreads();
  const int reach = D * D;
  for (int e = tid; e < EX_TILE * EX_TILE; e += THREADS) {
    const int row = e / EX_TILE, col = e % EX_TILE;
    const int r = r0 + row, c = c0 + col;
    if (r >= H || c >= W) continue;
    const size_t p = (size_t)r * W + c;
    const int own = lab[(row + HALO) * SIDE + col + HALO];
    if (own > 0) {
      out[p] = own;
      if (dist2) dist2[p] = 0;
      continue;
    }
    int best = reach + 1, best_label = 0;
    const int g = row * SIDE + col + HALO;      // columns g -+ k lie in the row: k <= D <= HALO
    // outwards, both sides at once: a column k away offers k^2 at the least, so past k^2 > best nothing wins or ties -- the loop costs what the
    // nearest label is away, not D
    for (int k = 0; k <= D && k * k <= best; ++k) {
      for (int side = 0; side < 2; ++side) {
        const int at = side ? g + k : g - k;
        const int d = gd[at];
        if (d < 0) continue;
        const int d2 = d + k * k, l = gl[at];
        if (d2 < best || (d2 == best && l < best_label)) best = d2, best_label = l;      // d2 == reach + 1 never enters: every l > 0 = best_label
      }
    }
    const bool grown = best <= reach;
    out[p] = grown ? best_label : mask[p];      // zeros and negatives pass through
    if (dist2) dist2[p] = grown ? best : -1;
  }
}

bool sizes_ok(int H, int W, int D) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) && D >= 1 && D <= EX_D_MAX; }

bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_expand_labels_ws_bytes(int32_t H, int32_t W, int32_t D) {
  if (!sizes_ok(H, W, D)) return 0;
  Carver cv(nullptr);
  cv.take<uint8_t>(EX_RESERVED);
  return (int64_t)cv.off;
}

int ribca_expand_labels(const int32_t* mask, int32_t H, int32_t W, int32_t D, int32_t* out, int32_t* dist2, void* ws, int64_t ws_bytes, void* stream) {
  if (!mask || !out || !ws) return fail("ribca_expand_labels: NULL buffer");
  if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return fail("ribca_expand_labels: needs 1 <= H, W and H W < 2^31");
  if (D < 1 || D > EX_D_MAX) return fail("ribca_expand_labels: needs 1 <= D <= 32");
  const size_t bytes = (size_t)H * W * sizeof(int32_t);
  if (overlap(mask, out, bytes) || (dist2 && (overlap(mask, dist2, bytes) || overlap(out, dist2, bytes))))
    return fail("ribca_expand_labels: mask, out and dist2 must not overlap");
  if (ws_bytes < ribca_expand_labels_ws_bytes(H, W, D)) return fail("ribca_expand_labels: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int tiles_x = (W + EX_TILE - 1) / EX_TILE, tiles_y = (H + EX_TILE - 1) / EX_TILE;      // tiles_x tiles_y < 2^31 / 1024 + H + W
  const dim3 grid((unsigned)((long long)tiles_x * tiles_y));
  // the wide halos hold few workgroups per CU in LDS (four at 16, two at 32): more threads each, so that the dependent LDS reads of the two
  // phases have other waves to run behind
  if (D <= 2) hipLaunchKernelGGL((expand_tile_kernel<2, 256>), grid, dim3(256), 0, s, mask, H, W, D, tiles_x, out, dist2);
  else if (D <= 4) hipLaunchKernelGGL((expand_tile_kernel<4, 256>), grid, dim3(256), 0, s, mask, H, W, D, tiles_x, out, dist2);
  else if (D <= 8) hipLaunchKernelGGL((expand_tile_kernel<8, 256>), grid, dim3(256), 0, s, mask, H, W, D, tiles_x, out, dist2);
  else if (D <= 16) hipLaunchKernelGGL((expand_tile_kernel<16, 512>), grid, dim3(512), 0, s, mask, H, W, D, tiles_x, out, dist2);
  else hipLaunchKernelGGL((expand_tile_kernel<32, 1024>), grid, dim3(1024), 0, s, mask, H, W, D, tiles_x, out, dist2);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
