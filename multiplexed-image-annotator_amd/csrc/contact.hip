// The cell contact graph of a segmentation mask (Annotator.contact_analysis; histoCAT's neighbourhood analysis, steinbock's expansion graph): two
// cells are neighbours when pixels of theirs lie within a Euclidean reach of d pixels, and w(i, j) counts those ordered pixel pairs
// (ribca_contact_table), and the label-permutation null of the type pairs over ANY directed edge list (ribca_edge_perm_counts).  Integers only:
// include/ribca_hip.h states the contract, tests/contact_numpy.py restates it.
//   contact_init     the (n, S) hash table of the workspace (keys -1, sums 0), the overflow flags and over = (0, INT_MAX).
//   contact_stencil  one workgroup per CT_TILE x CT_TILE pixel tile: the tile and a d-wide halo go to LDS already mapped to cell indices (-1 = no
//                    cell, also outside the image), one global read of the mask per staged pixel.  Every foreground pixel walks the offsets of
//                    the disk in LDS ((dr, dc) loops with the integer disk test, no table) and keeps ONE run (neighbour, count) in scalars, so a
//                    stretch of offsets that meets the same cell is one event; no per-pixel array, nothing goes to scratch.  Events (i, j, count)
//                    are summed in an LDS hash table per workgroup (64-bit compare-and-swap on the key, 32-bit add on the count, CT_PROBES slots
//                    at most); an event that finds no slot goes straight to the global table.  The flush is one global insert per distinct pair.
//   global insert    open addressing in row i of the (n, S) table: a 32-bit compare-and-swap on the key, a 64-bit integer add on the sum, at most S
//                    probes, then the overflow is recorded (flag of the cell, count of flagged cells, lowest flagged cell).  A row holds S distinct
//                    keys whatever the arrival order, so it overflows exactly when its degree exceeds S.  No loop waits for another thread.
//   contact_rows     one wave per row: the keys to LDS, every entry finds its rank among the row's keys (they are distinct) and goes to that
//                    slot of the output; degree = the number of keys.  Slot positions depend on the arrival order, ranks and integer sums do not.
//   the null         the shuffled labels of a batch of permutations are the byte rows of ribca_perm.h (launch_perm_labels).
//   edge_count       one thread per directed edge of a slab, a [T][T] LDS histogram of at most 16 KiB, one 64-bit atomic per non-zero entry.
// The table itself -- contact_init, global_insert, contact_rows, its workspace layout -- is csrc/ribca_rowtable.h, shared with overlap.hip.
// Measured forms: DESIGN.md section 19.
#include <limits.h>

#include <algorithm>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_perm.h"
#include "ribca_rowtable.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

namespace ribca {
namespace {

constexpr int CT_TILE = 32;                  // pixels of a workgroup's tile along either axis
constexpr int CT_D_MAX = 8;                  // the reach: a halo of 8 pixels
constexpr int CT_SIDE = CT_TILE + 2 * CT_D_MAX;
constexpr int CT_HASH = 1024;                // entries of the workgroup's LDS table
constexpr int CT_HASH_BITS = 10;
constexpr int CT_PROBES = 8;                 // slots an event tries in LDS before it goes to the global table
constexpr unsigned long long CT_EMPTY = ~0ull;

constexpr int EP_T_MAX = 64;
constexpr int EP_N_MAX = 1 << 30;
constexpr int EP_BATCH = 128;                // permutations whose label rows the workspace holds at most
constexpr long long EP_ROW_BYTES = 64ll << 20;      // ... and the bytes of them (one row when a single one is larger)
constexpr int EP_SLAB = 4096;                // edges of one counting workgroup

static_assert(1 << CT_HASH_BITS == CT_HASH, "the LDS table is indexed by the top bits of a 32-bit hash");
static_assert(CT_TILE * CT_TILE % 256 == 0, "whole rounds of a 256-thread workgroup");
static_assert(CT_SIDE * CT_SIDE * 4 + CT_HASH * 12 <= 32 * 1024, "LDS of contact_stencil");
static_assert(EP_T_MAX * EP_T_MAX * 4 <= 16 * 1024, "the LDS histogram");
static_assert(kPermSkip >= EP_T_MAX, "a skipped byte never indexes the histogram");

int fail(const char* msg) { return api_fail(msg); }

// one event of the stencil: into the workgroup's table if one of CT_PROBES slots takes it, else into the global one
__device__ __forceinline__ void emit(unsigned long long* hkey, unsigned int* hcount, int32_t* __restrict__ keys,
                                     unsigned long long* __restrict__ sums, int32_t* __restrict__ flag, int32_t* __restrict__ over, int S, int log_s,
                                     int i, int j, unsigned int count) {
  const unsigned long long key = ((unsigned long long)(uint32_t)i << 32) | (uint32_t)j;
  uint32_t h = (uint32_t)i * 0x9E3779B1u ^ (uint32_t)j * 0x85EBCA77u;
  h ^= h >> 15;
  int slot = (int)((h * 0x2C1B3C6Du) >> (32 - CT_HASH_BITS));
  for (int probe = 0; probe < CT_PROBES; ++probe) {
    const unsigned long long old = atomicCAS(&hkey[slot], CT_EMPTY, key);
    if (old == CT_EMPTY || old == key) {
      atomicAdd(&hcount[slot], count);
      return;
    }
    slot = (slot + 1) & (CT_HASH - 1);
  }
  global_insert(keys, sums, flag, over, S, log_s, i, j, count);
}

// grid: the tiles in row-major order, tiles_x of them per row of tiles
__global__ __launch_bounds__(256) void contact_stencil_kernel(const int32_t* __restrict__ mask, int H, int W, const int32_t* __restrict__ label_to_cell,
                                                              int L, int n, int d, int tiles_x, int S, int log_s, int32_t* __restrict__ keys,
                                                              unsigned long long* __restrict__ sums, int32_t* __restrict__ flag,
                                                              int32_t* __restrict__ over) {
  __shared__ int cell[CT_SIDE * CT_SIDE];
  __shared__ unsigned long long hkey[CT_HASH];
  __shared__ unsigned int hcount[CT_HASH];
  const int tid = threadIdx.x;
  const int r0 = (int)(blockIdx.x / (unsigned)tiles_x) * CT_TILE, c0 = (int)(blockIdx.x % (unsigned)tiles_x) * CT_TILE;
  const int side = CT_TILE + 2 * d;
  for (int e = tid; e < CT_HASH; e += 256) {
    hkey[e] = CT_EMPTY;
    hcount[e] = 0u;
  }
  for (int e = tid; e < side * side; e += 256) {
    const int r = r0 - d + e / side, c = c0 - d + e % side;
    int v = -1;
    if (r >= 0 && r < H && c >= 0 && c < W) {
      const int32_t lab = mask[(size_t)r * W + c];
      if ((unsigned)lab < (unsigned)L) {
        const int32_t t = label_to_cell[lab];
        if ((unsigned)t < (unsigned)n) v = t;      // a table entry outside [0, n) is no cell: it never indexes a row
      }
    }
    cell[e] = v;
  }
  __syncthreads();
  const int d2 = d * d;
  for (int k = tid; k < CT_TILE * CT_TILE; k += 256) {
    const int pr = k / CT_TILE + d, pc = k % CT_TILE + d;      // in the staged square; pixels outside the image hold -1
    const int own = cell[pr * side + pc];
    if (own < 0) continue;
    int run = -1;
    unsigned int run_count = 0u;
    for (int dr = -d; dr <= d; ++dr) {
      for (int dc = -d; dc <= d; ++dc) {
        if (dr * dr + dc * dc > d2) continue;
        const int q = cell[(pr + dr) * side + pc + dc];
        if (q < 0 || q == own) continue;      // (0, 0) is the pixel itself
        if (q == run) {
          ++run_count;
        } else {
          if (run_count) emit(hkey, hcount, keys, sums, flag, over, S, log_s, own, run, run_count);
          run = q;
          run_count = 1u;
        }
      }
    }
    if (run_count) emit(hkey, hcount, keys, sums, flag, over, S, log_s, own, run, run_count);
  }
  __syncthreads();
  for (int e = tid; e < CT_HASH; e += 256) {
    const unsigned long long key = hkey[e];
    if (key != CT_EMPTY) global_insert(keys, sums, flag, over, S, log_s, (int)(key >> 32), (int)(uint32_t)key, hcount[e]);
  }
}

// counts[j][label(src[e])][label(dst[e])] += 1 over the slab's edges: grid (ceil(E / EP_SLAB), batch)
__global__ __launch_bounds__(256) void edge_count_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, long long E,
                                                         const uint8_t* __restrict__ labels, int n, int T, unsigned long long* __restrict__ counts) {
  __shared__ unsigned int hist[EP_T_MAX * EP_T_MAX];
  const int tid = threadIdx.x;
  const int TT = T * T;
  for (int e = tid; e < TT; e += 256) hist[e] = 0u;
  __syncthreads();
  const uint8_t* __restrict__ lab = labels + (size_t)blockIdx.y * n;
  const long long first = (long long)blockIdx.x * EP_SLAB;
  const long long last = first + EP_SLAB < E ? first + EP_SLAB : E;
  for (long long e = first + tid; e < last; e += 256) {
    const int32_t s = src[e], t = dst[e];
    if ((unsigned)s >= (unsigned)n || (unsigned)t >= (unsigned)n) continue;
    const unsigned a = lab[s], b = lab[t];
    if (a < (unsigned)T && b < (unsigned)T) atomicAdd(&hist[a * T + b], 1u);
  }
  __syncthreads();
  unsigned long long* __restrict__ out = counts + (size_t)blockIdx.y * TT;
  for (int e = tid; e < TT; e += 256)
    if (hist[e]) atomicAdd(&out[e], (unsigned long long)hist[e]);
}

bool edge_sizes_ok(int n, int P) { return n >= 1 && n <= EP_N_MAX && P >= 1; }

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_contact_table_ws_bytes(int32_t H, int32_t W, int32_t n, int32_t S) {
  if (!table_sizes_ok(H, W, n, S)) return 0;
  Carver cv(nullptr);
  carve_contact(cv, n, S);
  return (int64_t)cv.off;
}

int ribca_contact_table(const int32_t* mask, int32_t H, int32_t W, const int32_t* label_to_cell, int32_t L, int32_t n, int32_t d, int32_t S,
                        int32_t* nbr, uint64_t* pairs, int32_t* degree, int32_t* over, void* ws, int64_t ws_bytes, void* stream) {
  if (!mask || !label_to_cell || !nbr || !pairs || !degree || !over || !ws) return fail("ribca_contact_table: NULL buffer");
  if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return fail("ribca_contact_table: needs 1 <= H, W and H W < 2^31");
  if (L < 1) return fail("ribca_contact_table: needs 1 <= L");
  if (n < 1 || n > CT_N_MAX) return fail("ribca_contact_table: needs 1 <= n <= 2^21");
  if (d < 1 || d > CT_D_MAX) return fail("ribca_contact_table: needs 1 <= d <= 8");
  if (S < CT_S_MIN || S > CT_S_MAX || log2_of_slots(S) < 0) return fail("ribca_contact_table: S must be a power of two in 8 .. 1024");
  if (ws_bytes < ribca_contact_table_ws_bytes(H, W, n, S)) return fail("ribca_contact_table: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Carver cv(ws);
  const ContactWs w = carve_contact(cv, n, S);
  const size_t slots = (size_t)n * S;
  const int tiles_x = (W + CT_TILE - 1) / CT_TILE, tiles_y = (H + CT_TILE - 1) / CT_TILE;      // tiles_x tiles_y < 2^31 / 1024 + H + W
  hipLaunchKernelGGL(contact_init_kernel, dim3((unsigned)std::min<size_t>((slots + 255) / 256, 16384)), dim3(256), 0, s, w.keys, w.sums, slots, w.flag,
                     n, over);
  hipLaunchKernelGGL(contact_stencil_kernel, dim3((unsigned)((long long)tiles_x * tiles_y)), dim3(256), 0, s, mask, H, W, label_to_cell, L, n, d,
                     tiles_x, S, log2_of_slots(S), w.keys, w.sums, w.flag, over);
  hipLaunchKernelGGL(contact_rows_kernel, dim3((unsigned)((n + CT_ROWS - 1) / CT_ROWS)), dim3(64 * CT_ROWS), 0, s, w.keys, w.sums, n, S, nbr,
                     reinterpret_cast<unsigned long long*>(pairs), degree, over);
  RIBCA_FINISH();
  return 0;
}

int64_t ribca_edge_perm_counts_ws_bytes(int32_t n, int32_t P) {
  if (!edge_sizes_ok(n, P)) return 0;
  Carver cv(nullptr);
  cv.take<uint8_t>((size_t)perm_batch(P, EP_BATCH, n, EP_ROW_BYTES) * (size_t)n);
  return (int64_t)cv.off;
}

int ribca_edge_perm_counts(const int32_t* src, const int32_t* dst, int64_t E, const int32_t* cell_type, int32_t n, int32_t T, uint64_t seed,
                           int32_t image, int64_t p0, int32_t P, uint64_t* counts, void* ws, int64_t ws_bytes, void* stream) {
  if (!src || !dst || !cell_type || !counts || !ws) return fail("ribca_edge_perm_counts: NULL buffer");
  if (E < 1 || E >= (1ll << 31)) return fail("ribca_edge_perm_counts: needs 1 <= E < 2^31");
  if (n < 1 || n > EP_N_MAX) return fail("ribca_edge_perm_counts: needs 1 <= n <= 2^30");
  if (T < 1 || T > EP_T_MAX) return fail("ribca_edge_perm_counts: needs 1 <= T <= 64");
  if (perm_range_check("ribca_edge_perm_counts", image, p0, P)) return 1;
  if (ws_bytes < ribca_edge_perm_counts_ws_bytes(n, P)) return fail("ribca_edge_perm_counts: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int batch_max = perm_batch(P, EP_BATCH, n, EP_ROW_BYTES);
  Carver cv(ws);
  uint8_t* labels = cv.take<uint8_t>((size_t)batch_max * (size_t)n);
  const PermKeys k(n, seed, image);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  for (int64_t j0 = 0; j0 < P; j0 += batch_max) {      // the batches follow one another on the stream: the label rows are reused
    const int batch = (int)std::min<int64_t>(batch_max, P - j0);
    launch_perm_labels(cell_type, n, T, k.h, k.image_key, (uint64_t)(p0 + j0), batch, labels, s);
    hipLaunchKernelGGL(edge_count_kernel, dim3((unsigned)((E + EP_SLAB - 1) / EP_SLAB), (unsigned)batch), dim3(256), 0, s, src, dst, (long long)E,
                       labels, n, T, out + (size_t)j0 * T * T);
  }
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
