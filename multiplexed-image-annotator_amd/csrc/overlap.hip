// The sparse contingency table of two label images of one tile (Annotator.mask_matching, ops.overlap_pairs): the pixels every (cell of mask A,
// object of mask B) pair shares, the area of every cell and object, and the split of mask A into the part inside the objects its cells own and
// the rest (ribca_mask_compartments).  Integers only: include/ribca_hip.h states the contract, tests/overlap_numpy.py restates it.  The sibling of
// contact.hip without the stencil: the same workgroup hash, the same per-row table (csrc/ribca_rowtable.h).
//   overlap_init   area_a = 0, area_b = 0; the (n, S) table, its flags and over are initialised by contact_init.
//   overlap_tile   one workgroup per OV_TILE x OV_TILE pixel tile, one thread per run of OV_RUN consecutive pixels of a row: both masks are read
//                  once (one 16-byte load each where the rows allow it) and mapped through their tables on the way in (-1 = none).  The thread
//                  keeps ONE running (cell, object, count) in scalars, so a stretch of equal pairs is one event; no per-pixel array, nothing goes
//                  to scratch.  An event (i, j, c) goes to the workgroup's LDS hash (64-bit compare-and-swap on the key, 32-bit add on the count,
//                  OV_PROBES slots at most) as (i, j) when both exist, as (i, none) when i exists and as (none, j) when j exists; an event that
//                  finds no slot goes straight to the global table or counter.  The flush is one global insert per distinct pair and one global
//                  add per distinct cell and per distinct object of the tile.
//   contact_rows   sorts every row of the table by rank (ribca_rowtable.h).
//   compartments   elementwise, four pixels per thread with 16-byte loads and stores where all four images are 16-byte aligned.
// No loop waits for another thread; no floating-point operation anywhere.  Measured forms: DESIGN.md section 25.
#include <limits.h>

#include <algorithm>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_rowtable.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

namespace ribca {
namespace {

constexpr int OV_TILE = 32;                  // pixels of a workgroup's tile along either axis
constexpr int OV_RUN = 4;                    // consecutive pixels of a row per thread
constexpr int OV_HASH = 1024;                // entries of the workgroup's LDS table
constexpr int OV_HASH_BITS = 10;
constexpr int OV_PROBES = 8;                 // slots an event tries in LDS before it goes to global memory
constexpr unsigned long long OV_EMPTY = ~0ull;      // (none, none): never an event

static_assert(1 << OV_HASH_BITS == OV_HASH, "the LDS table is indexed by the top bits of a 32-bit hash");
static_assert(OV_TILE * OV_TILE == 256 * OV_RUN && OV_TILE % OV_RUN == 0, "one run per thread of a 256-thread workgroup");
static_assert(OV_HASH * 12 <= 16 * 1024, "LDS of overlap_tile");

int fail(const char* msg) { return api_fail(msg); }

__global__ __launch_bounds__(256) void overlap_init_kernel(int32_t* __restrict__ area_a, int n, int32_t* __restrict__ area_b, int m) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)n; e += stride) area_a[e] = 0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)m; e += stride) area_b[e] = 0;
}

// the rule of ribca_contact_table: the index table[label] when the label is inside the table and the index inside [0, count), else -1
__device__ __forceinline__ int owner_of(int32_t label, const int32_t* __restrict__ table, int L, int count) {
  if ((unsigned)label >= (unsigned)L) return -1;
  const int32_t t = table[label];
  return (unsigned)t < (unsigned)count ? t : -1;
}

// the destination of one (i, j, count) outside LDS: -1 = none, never both
__device__ __forceinline__ void to_global(int32_t* __restrict__ keys, unsigned long long* __restrict__ sums, int32_t* __restrict__ flag,
                                          int32_t* __restrict__ over, int S, int log_s, int32_t* __restrict__ area_a, int32_t* __restrict__ area_b,
                                          int i, int j, unsigned int count) {
  if (i >= 0 && j >= 0)
    global_insert(keys, sums, flag, over, S, log_s, i, j, count);
  else if (i >= 0)
    atomicAdd(&area_a[i], (int)count);
  else
    atomicAdd(&area_b[j], (int)count);
}

__device__ __forceinline__ void emit(unsigned long long* hkey, unsigned int* hcount, int32_t* __restrict__ keys,
                                     unsigned long long* __restrict__ sums, int32_t* __restrict__ flag, int32_t* __restrict__ over, int S, int log_s,
                                     int32_t* __restrict__ area_a, int32_t* __restrict__ area_b, int i, int j, unsigned int count) {
  const unsigned long long key = ((unsigned long long)(uint32_t)i << 32) | (uint32_t)j;
  uint32_t h = (uint32_t)i * 0x9E3779B1u ^ (uint32_t)j * 0x85EBCA77u;
  h ^= h >> 15;
  int slot = (int)((h * 0x2C1B3C6Du) >> (32 - OV_HASH_BITS));
  for (int probe = 0; probe < OV_PROBES; ++probe) {
    const unsigned long long old = atomicCAS(&hkey[slot], OV_EMPTY, key);
    if (old == OV_EMPTY || old == key) {
      atomicAdd(&hcount[slot], count);
      return;
    }
    slot = (slot + 1) & (OV_HASH - 1);
  }
  to_global(keys, sums, flag, over, S, log_s, area_a, area_b, i, j, count);
}

// one run of equal pairs: the pair, and either side on its own for the areas
__device__ __forceinline__ void event(unsigned long long* hkey, unsigned int* hcount, int32_t* __restrict__ keys,
                                      unsigned long long* __restrict__ sums, int32_t* __restrict__ flag, int32_t* __restrict__ over, int S, int log_s,
                                      int32_t* __restrict__ area_a, int32_t* __restrict__ area_b, int i, int j, unsigned int count) {
  if (i >= 0 && j >= 0) emit(hkey, hcount, keys, sums, flag, over, S, log_s, area_a, area_b, i, j, count);
  if (i >= 0) emit(hkey, hcount, keys, sums, flag, over, S, log_s, area_a, area_b, i, -1, count);
  if (j >= 0) emit(hkey, hcount, keys, sums, flag, over, S, log_s, area_a, area_b, -1, j, count);
}

// grid: the tiles in row-major order, tiles_x of them per row of tiles; vec: W % 4 == 0 and both masks 16-byte aligned
__global__ __launch_bounds__(256) void overlap_tile_kernel(const int32_t* __restrict__ mask_a, const int32_t* __restrict__ mask_b, int H, int W,
                                                           const int32_t* __restrict__ a_to_cell, int La, int n,
                                                           const int32_t* __restrict__ b_to_obj, int Lb, int m, int tiles_x, int vec, int S, int log_s,
                                                           int32_t* __restrict__ keys, unsigned long long* __restrict__ sums,
                                                           int32_t* __restrict__ flag, int32_t* __restrict__ over, int32_t* __restrict__ area_a,
                                                           int32_t* __restrict__ area_b) {
  __shared__ unsigned long long hkey[OV_HASH];
  __shared__ unsigned int hcount[OV_HASH];
  const int tid = threadIdx.x;
  for (int e = tid; e < OV_HASH; e += 256) {
    hkey[e] = OV_EMPTY;
    hcount[e] = 0u;
  }
  __syncthreads();
  const int r = (int)(blockIdx.x / (unsigned)tiles_x) * OV_TILE + tid / (OV_TILE / OV_RUN);
  const int c = (int)(blockIdx.x % (unsigned)tiles_x) * OV_TILE + tid % (OV_TILE / OV_RUN) * OV_RUN;
  if (r < H && c < W) {
    const size_t at = (size_t)r * W + c;
    int32_t la[OV_RUN], lb[OV_RUN];      // unrolled below: registers
    if (vec) {                            // c % 4 == 0 and W % 4 == 0: the four pixels are inside the row
      const int4 va = *reinterpret_cast<const int4*>(mask_a + at), vb = *reinterpret_cast<const int4*>(mask_b + at);
      la[0] = va.x, la[1] = va.y, la[2] = va.z, la[3] = va.w;
      lb[0] = vb.x, lb[1] = vb.y, lb[2] = vb.z, lb[3] = vb.w;
    } else {
#pragma unroll
      for (int k = 0; k < OV_RUN; ++k) {
        const bool in = c + k < W;
        la[k] = in ? mask_a[at + k] : -1;      // a negative label is no cell and no object
        lb[k] = in ? mask_b[at + k] : -1;
      }
    }
    int run_i = -1, run_j = -1;
    unsigned int run_count = 0u;
#pragma unroll
    for (int k = 0; k < OV_RUN; ++k) {
      const int i = owner_of(la[k], a_to_cell, La, n), j = owner_of(lb[k], b_to_obj, Lb, m);
      if (i == run_i && j == run_j) {
        ++run_count;      // a run of (none, none) counts too and is dropped below
      } else {
        if (run_count && (run_i >= 0 || run_j >= 0))
          event(hkey, hcount, keys, sums, flag, over, S, log_s, area_a, area_b, run_i, run_j, run_count);
        run_i = i, run_j = j, run_count = 1u;
      }
    }
    if (run_i >= 0 || run_j >= 0) event(hkey, hcount, keys, sums, flag, over, S, log_s, area_a, area_b, run_i, run_j, run_count);
  }
  __syncthreads();
  for (int e = tid; e < OV_HASH; e += 256) {
    const unsigned long long key = hkey[e];
    if (key != OV_EMPTY) to_global(keys, sums, flag, over, S, log_s, area_a, area_b, (int)(key >> 32), (int)(uint32_t)key, hcount[e]);
  }
}

// (inner, outer) of one pixel
__device__ __forceinline__ int2 split_pixel(int32_t la, int32_t lb, const int32_t* __restrict__ a_to_cell, int La, int n,
                                            const int32_t* __restrict__ b_to_obj, int Lb, int m, const int32_t* __restrict__ owner) {
  const int i = owner_of(la, a_to_cell, La, n);
  if (i < 0) return make_int2(0, 0);
  const int j = owner_of(lb, b_to_obj, Lb, m);
  return j >= 0 && owner[j] == i ? make_int2(la, 0) : make_int2(0, la);
}

// quads: whole groups of four pixels, one thread each (0 when a pointer is not 16-byte aligned); the pixels behind them one thread each
__global__ __launch_bounds__(256) void compartments_kernel(const int32_t* __restrict__ mask_a, const int32_t* __restrict__ mask_b, long long pixels,
                                                           long long quads, const int32_t* __restrict__ a_to_cell, int La, int n,
                                                           const int32_t* __restrict__ b_to_obj, int Lb, int m, const int32_t* __restrict__ owner,
                                                           int32_t* __restrict__ inner, int32_t* __restrict__ outer) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < quads) {
    const int4 va = reinterpret_cast<const int4*>(mask_a)[t], vb = reinterpret_cast<const int4*>(mask_b)[t];
    const int2 x = split_pixel(va.x, vb.x, a_to_cell, La, n, b_to_obj, Lb, m, owner);
    const int2 y = split_pixel(va.y, vb.y, a_to_cell, La, n, b_to_obj, Lb, m, owner);
    const int2 z = split_pixel(va.z, vb.z, a_to_cell, La, n, b_to_obj, Lb, m, owner);
    const int2 w = split_pixel(va.w, vb.w, a_to_cell, La, n, b_to_obj, Lb, m, owner);
    reinterpret_cast<int4*>(inner)[t] = make_int4(x.x, y.x, z.x, w.x);
    reinterpret_cast<int4*>(outer)[t] = make_int4(x.y, y.y, z.y, w.y);
  } else {
    const long long p = 4 * quads + (t - quads);
    if (p < pixels) {
      const int2 v = split_pixel(mask_a[p], mask_b[p], a_to_cell, La, n, b_to_obj, Lb, m, owner);
      inner[p] = v.x;
      outer[p] = v.y;
    }
  }
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

// no buffer from `first_out` on overlaps any other buffer of the list (the inputs before it may share memory)
bool outputs_apart(const void* const* bufs, const size_t* sizes, int count, int first_out) {
  for (int b = first_out; b < count; ++b)
    for (int a = 0; a < b; ++a)
      if (overlap(bufs[a], sizes[a], bufs[b], sizes[b])) return false;
  return true;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_mask_overlap_ws_bytes(int32_t H, int32_t W, int32_t n, int32_t S) {
  if (!table_sizes_ok(H, W, n, S)) return 0;
  Carver cv(nullptr);
  carve_contact(cv, n, S);
  return (int64_t)cv.off;
}

int ribca_mask_overlap(const int32_t* mask_a, const int32_t* mask_b, int32_t H, int32_t W, const int32_t* a_to_cell, int32_t La, int32_t n,
                       const int32_t* b_to_obj, int32_t Lb, int32_t m, int32_t S, int32_t* partner, uint64_t* inter, int32_t* degree,
                       int32_t* area_a, int32_t* area_b, int32_t* over, void* ws, int64_t ws_bytes, void* stream) {
  if (!mask_a || !mask_b || !a_to_cell || !b_to_obj || !partner || !inter || !degree || !area_a || !area_b || !over || !ws)
    return fail("ribca_mask_overlap: NULL buffer");
  if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return fail("ribca_mask_overlap: needs 1 <= H, W and H W < 2^31");
  if (La < 1 || Lb < 1) return fail("ribca_mask_overlap: needs 1 <= La, Lb");
  if (n < 1 || n > CT_N_MAX || m < 1 || m > CT_N_MAX) return fail("ribca_mask_overlap: needs 1 <= n, m <= 2^21");
  if (S < CT_S_MIN || S > CT_S_MAX || log2_of_slots(S) < 0) return fail("ribca_mask_overlap: S must be a power of two in 8 .. 1024");
  const int64_t need = ribca_mask_overlap_ws_bytes(H, W, n, S);
  if (ws_bytes < need) return fail("ribca_mask_overlap: workspace too small");
  const size_t px = (size_t)H * W * sizeof(int32_t), slots = (size_t)n * S;
  const void* bufs[11] = {mask_a, mask_b, a_to_cell, b_to_obj, partner, inter, degree, area_a, area_b, over, ws};
  const size_t sizes[11] = {px, px, (size_t)La * 4, (size_t)Lb * 4, slots * 4, slots * 8, (size_t)n * 4, (size_t)n * 4, (size_t)m * 4, 8, (size_t)need};
  if (!outputs_apart(bufs, sizes, 11, 4)) return fail("ribca_mask_overlap: the outputs and ws must not overlap each other or the inputs");
  hipStream_t s = (hipStream_t)stream;
  Carver cv(ws);
  const ContactWs w = carve_contact(cv, n, S);
  const int tiles_x = (W + OV_TILE - 1) / OV_TILE, tiles_y = (H + OV_TILE - 1) / OV_TILE;      // tiles_x tiles_y < 2^31 / 1024 + H + W
  const int vec = W % 4 == 0 && aligned16(mask_a) && aligned16(mask_b) ? 1 : 0;
  hipLaunchKernelGGL(contact_init_kernel, dim3((unsigned)std::min<size_t>((slots + 255) / 256, 16384)), dim3(256), 0, s, w.keys, w.sums, slots, w.flag,
                     n, over);
  hipLaunchKernelGGL(overlap_init_kernel, dim3((unsigned)std::min<size_t>(((size_t)std::max(n, m) + 255) / 256, 16384)), dim3(256), 0, s, area_a, n,
                     area_b, m);
  hipLaunchKernelGGL(overlap_tile_kernel, dim3((unsigned)((long long)tiles_x * tiles_y)), dim3(256), 0, s, mask_a, mask_b, H, W, a_to_cell, La, n,
                     b_to_obj, Lb, m, tiles_x, vec, S, log2_of_slots(S), w.keys, w.sums, w.flag, over, area_a, area_b);
  hipLaunchKernelGGL(contact_rows_kernel, dim3((unsigned)((n + CT_ROWS - 1) / CT_ROWS)), dim3(64 * CT_ROWS), 0, s, w.keys, w.sums, n, S, partner,
                     reinterpret_cast<unsigned long long*>(inter), degree, over);
  RIBCA_FINISH();
  return 0;
}

int ribca_mask_compartments(const int32_t* mask_a, const int32_t* mask_b, int32_t H, int32_t W, const int32_t* a_to_cell, int32_t La, int32_t n,
                            const int32_t* b_to_obj, int32_t Lb, int32_t m, const int32_t* owner, int32_t* inner, int32_t* outer, void* stream) {
  if (!mask_a || !mask_b || !a_to_cell || !b_to_obj || !owner || !inner || !outer) return fail("ribca_mask_compartments: NULL buffer");
  if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return fail("ribca_mask_compartments: needs 1 <= H, W and H W < 2^31");
  if (La < 1 || Lb < 1) return fail("ribca_mask_compartments: needs 1 <= La, Lb");
  if (n < 1 || n > CT_N_MAX || m < 1 || m > CT_N_MAX) return fail("ribca_mask_compartments: needs 1 <= n, m <= 2^21");
  const size_t px = (size_t)H * W * sizeof(int32_t);
  const void* bufs[7] = {mask_a, mask_b, a_to_cell, b_to_obj, owner, inner, outer};
  const size_t sizes[7] = {px, px, (size_t)La * 4, (size_t)Lb * 4, (size_t)m * 4, px, px};
  if (!outputs_apart(bufs, sizes, 7, 5)) return fail("ribca_mask_compartments: inner and outer must not overlap each other or the inputs");
  hipStream_t s = (hipStream_t)stream;
  const long long pixels = (long long)H * W;
  const long long quads = aligned16(mask_a) && aligned16(mask_b) && aligned16(inner) && aligned16(outer) ? pixels / 4 : 0;
  const long long threads = quads + (pixels - 4 * quads);
  hipLaunchKernelGGL(compartments_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, mask_a, mask_b, pixels, quads, a_to_cell, La, n,
                     b_to_obj, Lb, m, owner, inner, outer);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
