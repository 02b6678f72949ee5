// Cell outlines of a segmentation mask as closed rings of lattice vertices (Annotator.cell_outlines, ops.mask_rings): the boundary of every cell,
// traced exactly, exterior rings and hole rings apart.  Integers only: include/ribca_hip.h states the contract, tests/outlines_numpy.py restates it.
// Vertex (r, c) is the top-left corner of pixel (r, c), raster index r (W + 1) + c.  A boundary edge of cell i is a pixel side with i on its RIGHT
// and something else on its left; the successor of an edge is the left turn where i holds the pixel ahead on the left (a saddle when it does not
// hold the one ahead on the right: the two diagonal pixels are joined, the 8-connected foreground of components.hip), else straight on where it
// holds the pixel ahead on the right, else the right turn.
//   ol_init      rings = -1, total = 0, the candidate count = 0.
//   ol_tile      one workgroup per OL_TILE x OL_TILE pixel tile: the tile and one row and column of halo above and to the left go to LDS already
//                mapped to cell indices (-1 = no cell, also outside the image) and, the tile's own pixels, to the cell image of the workspace, so
//                that a walker's step is ONE dependent read and not mask then label_to_cell.  Vertex (r, c), r < H, c < W, is a CANDIDATE start of
//                an exterior ring of cell(SE) when NW, NE and SW are not that cell, and of a hole ring of cell(NE) when SW is that cell and SE is
//                not: the smallest vertex of every ring matches one of the two, most matches are not the smallest vertex of their ring.  The
//                candidates of a workgroup's tiles (the tiles are strided over at most OL_TILE_BLOCKS workgroups) are gathered in LDS and
//                appended to the workspace's list with one global atomic when the next tile might not fit, and at the end.
//   ol_walk      one thread per candidate, the launch strided over the list (its length is on the device only): the thread walks its ring from
//                the candidate edge (east for an exterior, south for a hole), ABORTS at the first vertex smaller than its own and CONFIRMS when
//                it is back on its first edge; then it takes a row of ``rings`` with one 64-bit atomic on ``total``.  A ring has one smallest
//                vertex and passes it once, so it is confirmed once.  About two steps per boundary edge on cell-like masks, 13 to 17 on a
//                serpentine or a comb.  Every walk is bounded by 2 (H + 1)(W + 1) steps, more than any ring has edges.
//   ol_vertices  one thread per ring row: checks that the row's start is a ring start of its cell (the two patterns), walks the ring again and
//                writes the vertices at which the direction changes into [first[k], first[k + 1]); a row that does not fit -- no ring of that
//                cell starts there, another vertex count, a range that is no range -- writes -1 into its own range and counts in ``bad``.  This
//                entry point has no workspace: a step reads mask, then label_to_cell.
// No loop waits for another thread; the launches are separate because each needs the whole of the one before.  The set of rows is a function of
// (mask, label_to_cell) alone; their order in ``rings`` is the arrival order.  Scalars in registers, lists in LDS: nothing goes to scratch.
#include <limits.h>

#include <algorithm>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

namespace ribca {
namespace {

constexpr int OL_TILE = 32;                   // pixels of a workgroup's tile along either axis
constexpr int OL_SIDE = OL_TILE + 1;          // ... and one row above, one column to the left
constexpr int OL_ROUNDS = (OL_SIDE * OL_SIDE + 255) / 256;      // staged pixels per thread of ol_tile
constexpr int OL_LIST = 2 * 2 * OL_TILE * OL_TILE;               // candidates a workgroup gathers in LDS: twice what one tile can have
constexpr int OL_TILE_BLOCKS = 2048;          // workgroups of ol_tile at most: the tiles are taken in strides
constexpr int OL_N_MAX = 1 << 21;
constexpr int OL_WALK_BLOCKS = 2048;          // workgroups of ol_walk at most: the list is walked in strides
constexpr int OL_COLS = 6;                    // cell, start, vertices, edges, area2, saddles

static_assert(OL_SIDE * OL_SIDE * 4 + OL_LIST * 4 <= 24 * 1024, "LDS of ol_tile");

int fail(const char* msg) { return api_fail(msg); }

// who owns pixel (r, c): the cell index, -1 for no cell and outside the image
struct ImageOwner {      // from the cell image ol_tile wrote
  const int32_t* __restrict__ cell;
  int H, W;
  __device__ __forceinline__ int operator()(int r, int c) const {
    return (unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W ? cell[(size_t)r * W + c] : -1;
  }
};

struct MaskOwner {       // the rule of ribca_contact_table
  const int32_t* __restrict__ mask;
  const int32_t* __restrict__ label_to_cell;
  int H, W, L, n;
  __device__ __forceinline__ int operator()(int r, int c) const {
    if ((unsigned)r >= (unsigned)H || (unsigned)c >= (unsigned)W) return -1;
    const int32_t lab = mask[(size_t)r * W + c];
    if ((unsigned)lab >= (unsigned)L) return -1;
    const int32_t t = label_to_cell[lab];
    return (unsigned)t < (unsigned)n ? t : -1;
  }
};

// directions: 0 east, 1 south, 2 west, 3 north.  One step of a ring of cell i: along d from vertex (r, c) to the next vertex, and d becomes the
// direction the ring leaves that vertex in.  Returns 1 when the vertex is passed as a saddle.
template <class Owner>
__device__ __forceinline__ int ring_step(const Owner& own, int i, int& r, int& c, int& d) {
  r += (d == 1) - (d == 3);
  c += (d == 0) - (d == 2);
  const int ahead_left = own(r - (d == 0 || d == 3), c - (d >= 2));
  const int ahead_right = own(r - (d >= 2), c - (d == 1 || d == 2));
  const bool left = ahead_left == i, straight = ahead_right == i;
  d = left ? (d + 3) & 3 : straight ? d : (d + 1) & 3;
  return left && !straight ? 1 : 0;
}

// twice the signed area under the unit edge that leaves (r, c) along d: x_k y_{k+1} - x_{k+1} y_k with x = c, y = r.  Summed over the unit edges
// of a ring it is the sum over its kept vertices: the vertices between them are collinear.
__device__ __forceinline__ long long edge_area2(int r, int c, int d) { return d == 0 ? -(long long)r : d == 1 ? (long long)c : d == 2 ? (long long)r : -(long long)c; }

__global__ __launch_bounds__(256) void ol_init_kernel(long long* __restrict__ rings, long long slots, unsigned long long* __restrict__ total,
                                                      unsigned long long* __restrict__ count) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < slots; e += stride) rings[e] = -1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *total = 0ull;
    if (count) *count = 0ull;
  }
}

// appends the workgroup's gathered candidates to the list of the workspace: ONE global atomic.  Every thread of the workgroup calls it.
__device__ __forceinline__ void flush_candidates(const uint32_t* list, unsigned int* fill, unsigned long long* base, uint32_t* __restrict__ cand,
                                                 unsigned long long* __restrict__ count) {
  __syncthreads();
  const int mine = (int)*fill;
  if (threadIdx.x == 0 && mine) *base = atomicAdd(count, (unsigned long long)mine);
  __syncthreads();
  for (int e = threadIdx.x; e < mine; e += 256) cand[*base + e] = list[e];      // base + mine <= 2 H W: every entry belongs to a pixel of the image
  __syncthreads();
  if (threadIdx.x == 0) *fill = 0u;
  __syncthreads();
}

// the tiles in row-major order, tiles_x of them per row of tiles, strided over the workgroups of the grid: a workgroup gathers the candidates of
// its tiles in LDS and appends them when the next tile might not fit, so that the counter of the list -- one address for the whole grid --
// takes about one atomic per workgroup and not one per tile
__global__ __launch_bounds__(256) void ol_tile_kernel(const int32_t* __restrict__ mask, int H, int W, const int32_t* __restrict__ label_to_cell, int L,
                                                      int n, int tiles_x, int tiles, int32_t* __restrict__ cell_image, uint32_t* __restrict__ cand,
                                                      unsigned long long* __restrict__ count) {
  __shared__ int cell[OL_SIDE * OL_SIDE];
  __shared__ uint32_t list[OL_LIST];
  __shared__ unsigned int fill;
  __shared__ unsigned long long base;
  const int tid = threadIdx.x;
  if (tid == 0) fill = 0u;
  __syncthreads();
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int r0 = tile / tiles_x * OL_TILE, c0 = tile % tiles_x * OL_TILE;
    if (fill > (unsigned)(OL_LIST - 2 * OL_TILE * OL_TILE)) flush_candidates(list, &fill, &base, cand, count);      // uniform: fill is read after a barrier
    // the staging is two dependent reads per pixel, mask then label_to_cell: all labels of a thread first, then all table entries
    int32_t lab[OL_ROUNDS];
#pragma unroll
    for (int k = 0; k < OL_ROUNDS; ++k) {
      const int e = tid + k * 256;
      const int r = r0 - 1 + e / OL_SIDE, c = c0 - 1 + e % OL_SIDE;
      lab[k] = e < OL_SIDE * OL_SIDE && (unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W ? mask[(size_t)r * W + c] : -1;
    }
    int32_t owner[OL_ROUNDS];
#pragma unroll
    for (int k = 0; k < OL_ROUNDS; ++k) owner[k] = (unsigned)lab[k] < (unsigned)L ? label_to_cell[lab[k]] : -1;
#pragma unroll
    for (int k = 0; k < OL_ROUNDS; ++k) {
      const int e = tid + k * 256;
      if (e >= OL_SIDE * OL_SIDE) continue;
      const int lr = e / OL_SIDE, lc = e % OL_SIDE;
      const int r = r0 - 1 + lr, c = c0 - 1 + lc;
      const int v = (unsigned)owner[k] < (unsigned)n ? owner[k] : -1;      // a table entry outside [0, n) is no cell
      cell[e] = v;
      if (lr > 0 && lc > 0 && r < H && c < W) cell_image[(size_t)r * W + c] = v;
    }
    __syncthreads();
    for (int k = tid; k < OL_TILE * OL_TILE; k += 256) {
      const int lr = k / OL_TILE, lc = k % OL_TILE;
      const int r = r0 + lr, c = c0 + lc;
      if (r >= H || c >= W) continue;
      const int nw = cell[lr * OL_SIDE + lc], ne = cell[lr * OL_SIDE + lc + 1];
      const int sw = cell[(lr + 1) * OL_SIDE + lc], se = cell[(lr + 1) * OL_SIDE + lc + 1];
      const uint32_t vertex = (uint32_t)(r * (W + 1) + c);
      if (se >= 0 && nw != se && ne != se && sw != se) list[atomicAdd(&fill, 1u)] = vertex * 2u;             // at most two per pixel of the tile
      if (ne >= 0 && ne == sw && se != ne) list[atomicAdd(&fill, 1u)] = vertex * 2u + 1u;
    }
    __syncthreads();      // the list and fill are whole, and nobody reads cell any more
  }
  flush_candidates(list, &fill, &base, cand, count);
}

__global__ __launch_bounds__(256) void ol_walk_kernel(const int32_t* __restrict__ cell_image, int H, int W, const uint32_t* __restrict__ cand,
                                                      const unsigned long long* __restrict__ count, long long cap, long long bound,
                                                      long long* __restrict__ rings, unsigned long long* __restrict__ total) {
  const ImageOwner own{cell_image, H, W};
  const unsigned long long m = *count, stride = (unsigned long long)gridDim.x * 256;
  for (unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q < m; q += stride) {
    const uint32_t code = cand[q];
    const int start = (int)(code >> 1), d0 = (int)(code & 1u);      // a hole ring leaves its start going south, an exterior going east
    const int rs = start / (W + 1), cs = start % (W + 1);
    const int i = d0 ? own(rs - 1, cs) : own(rs, cs);
    int r = rs, c = cs, d = d0;
    long long edges = 0, area2 = 0;
    int kept = 0, saddles = 0;
    bool closed = false;
    for (long long step = 0; step < bound; ++step) {      // a ring has fewer edges than bound: the walk closes or aborts before
      area2 += edge_area2(r, c, d);
      const int before = d;
      saddles += ring_step(own, i, r, c, d);
      ++edges;
      kept += d != before ? 1 : 0;
      const int v = r * (W + 1) + c;
      if (v < start) break;                               // another vertex of this ring is smaller: that one's walker confirms it
      if (v == start && d == d0) {
        closed = true;
        break;
      }
    }
    if (!closed) continue;
    const unsigned long long slot = atomicAdd(total, 1ull);
    if (slot < (unsigned long long)cap) {
      long long* __restrict__ row = rings + slot * OL_COLS;
      row[0] = i, row[1] = start, row[2] = kept, row[3] = edges, row[4] = area2, row[5] = saddles;
    }
  }
}

__global__ __launch_bounds__(256) void ol_vertices_kernel(const int32_t* __restrict__ mask, int H, int W, const int32_t* __restrict__ label_to_cell,
                                                          int L, int n, const long long* __restrict__ rings, int R, const long long* __restrict__ first,
                                                          long long bound, int32_t* __restrict__ vertices, int32_t* __restrict__ bad) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= R) return;
  const long long lo = first[k], hi = first[k + 1];
  if (lo < 0 || hi < lo || hi > first[R]) {      // no range of the buffer: nothing is written
    atomicAdd(bad, 1);
    return;
  }
  const long long want = hi - lo;
  const long long cell = rings[k * OL_COLS], start = rings[k * OL_COLS + 1];
  const MaskOwner own{mask, label_to_cell, H, W, L, n};
  bool ok = cell >= 0 && cell < n && start >= 0 && start < (long long)(H + 1) * (W + 1) && rings[k * OL_COLS + 2] == want && want >= 4;
  if (ok) {
    const int i = (int)cell;
    const int rs = (int)start / (W + 1), cs = (int)start % (W + 1);
    const int nw = own(rs - 1, cs - 1), ne = own(rs - 1, cs), sw = own(rs, cs - 1), se = own(rs, cs);
    int d0 = -1;
    if (se == i && nw != i && ne != i && sw != i) d0 = 0;
    else if (ne == i && sw == i && se != i) d0 = 1;
    ok = d0 >= 0;
    if (ok) {
      int r = rs, c = cs, d = d0;
      long long j = 1;
      bool closed = false;
      vertices[2 * lo] = rs, vertices[2 * lo + 1] = cs;
      for (long long step = 0; step < bound; ++step) {
        const int before = d;
        ring_step(own, i, r, c, d);
        const int v = r * (W + 1) + c;
        if (v < (int)start) break;                      // the start of a ring is its smallest vertex
        if (v == (int)start && d == d0) {
          closed = true;
          break;
        }
        if (d != before) {
          if (j >= want) break;                         // more vertices than the row says: stays inside its range
          vertices[2 * (lo + j)] = r, vertices[2 * (lo + j) + 1] = c;
          ++j;
        }
      }
      ok = closed && j == want;
    }
  }
  if (!ok) {
    for (long long j = lo; j < hi; ++j) vertices[2 * j] = -1, vertices[2 * j + 1] = -1;
    atomicAdd(bad, 1);
  }
}

bool sizes_ok(int H, int W) { return H >= 1 && W >= 1 && ((long long)H + 1) * ((long long)W + 1) < (1ll << 31); }

struct OutlineWs {
  unsigned long long* count;      // candidates in the list
  int32_t* cell_image;            // (H, W): the owner of every pixel
  uint32_t* cand;                 // 2 * vertex + (1 for a hole): two per pixel at most
};

OutlineWs carve_outlines(Carver& cv, int H, int W) {
  OutlineWs w;
  w.count = cv.take<unsigned long long>(1);
  w.cell_image = cv.take<int32_t>((size_t)H * W);
  w.cand = cv.take<uint32_t>(2 * (size_t)H * W);
  return w;
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_mask_rings_ws_bytes(int32_t H, int32_t W, int32_t n) {
  if (!sizes_ok(H, W) || n < 0 || n > OL_N_MAX) return 0;
  Carver cv(nullptr);
  carve_outlines(cv, H, W);
  return (int64_t)cv.off;
}

int ribca_mask_rings(const int32_t* mask, int32_t H, int32_t W, const int32_t* label_to_cell, int32_t L, int32_t n, int64_t cap, int64_t* rings,
                     int64_t* total, void* ws, int64_t ws_bytes, void* stream) {
  if (!mask || !label_to_cell || !rings || !total || !ws) return fail("ribca_mask_rings: NULL buffer");
  if (!sizes_ok(H, W)) return fail("ribca_mask_rings: needs 1 <= H, W and (H + 1)(W + 1) < 2^31");
  if (L < 1) return fail("ribca_mask_rings: needs 1 <= L");
  if (n < 0 || n > OL_N_MAX) return fail("ribca_mask_rings: needs 0 <= n <= 2^21");
  if (cap < 1 || cap > (1ll << 40)) return fail("ribca_mask_rings: needs 1 <= cap <= 2^40");
  const int64_t need = ribca_mask_rings_ws_bytes(H, W, n);
  if (ws_bytes < need) return fail("ribca_mask_rings: workspace too small");
  const size_t m_bytes = (size_t)H * W * sizeof(int32_t), t_bytes = (size_t)L * sizeof(int32_t), r_bytes = (size_t)cap * OL_COLS * sizeof(int64_t);
  const void* bufs[5] = {mask, label_to_cell, rings, total, ws};
  const size_t sizes[5] = {m_bytes, t_bytes, r_bytes, sizeof(int64_t), (size_t)need};
  for (int a = 0; a < 5; ++a)
    for (int b = a + 1; b < 5; ++b)
      if (overlap(bufs[a], sizes[a], bufs[b], sizes[b])) return fail("ribca_mask_rings: mask, label_to_cell, rings, total and ws must not overlap");
  hipStream_t s = (hipStream_t)stream;
  Carver cv(ws);
  const OutlineWs w = carve_outlines(cv, H, W);
  const long long slots = (long long)cap * OL_COLS;
  unsigned long long* tot = reinterpret_cast<unsigned long long*>(total);
  hipLaunchKernelGGL(ol_init_kernel, dim3((unsigned)std::min<long long>((slots + 255) / 256, 4096)), dim3(256), 0, s, reinterpret_cast<long long*>(rings),
                     slots, tot, w.count);
  if (n > 0) {
    const int tiles_x = (W + OL_TILE - 1) / OL_TILE, tiles_y = (H + OL_TILE - 1) / OL_TILE;      // tiles_x tiles_y < 2^31 / 1024 + H + W
    const int tiles = tiles_x * tiles_y;
    hipLaunchKernelGGL(ol_tile_kernel, dim3((unsigned)std::min(tiles, OL_TILE_BLOCKS)), dim3(256), 0, s, mask, H, W, label_to_cell, L, n, tiles_x, tiles,
                       w.cell_image, w.cand, w.count);
    const long long most = 2ll * H * W, bound = 2ll * (H + 1) * (W + 1);
    hipLaunchKernelGGL(ol_walk_kernel, dim3((unsigned)std::min<long long>((most + 255) / 256, OL_WALK_BLOCKS)), dim3(256), 0, s, w.cell_image, H, W,
                       w.cand, w.count, (long long)cap, bound, reinterpret_cast<long long*>(rings), tot);
  }
  RIBCA_FINISH();
  return 0;
}

int ribca_mask_ring_vertices(const int32_t* mask, int32_t H, int32_t W, const int32_t* label_to_cell, int32_t L, int32_t n, const int64_t* rings,
                             int32_t R, const int64_t* first, int32_t* vertices, int32_t* bad, void* stream) {
  if (!mask || !label_to_cell || !rings || !first || !vertices || !bad) return fail("ribca_mask_ring_vertices: NULL buffer");
  if (!sizes_ok(H, W)) return fail("ribca_mask_ring_vertices: needs 1 <= H, W and (H + 1)(W + 1) < 2^31");
  if (L < 1) return fail("ribca_mask_ring_vertices: needs 1 <= L");
  if (n < 0 || n > OL_N_MAX) return fail("ribca_mask_ring_vertices: needs 0 <= n <= 2^21");
  if (R < 0) return fail("ribca_mask_ring_vertices: needs 0 <= R");
  const size_t m_bytes = (size_t)H * W * sizeof(int32_t), t_bytes = (size_t)L * sizeof(int32_t), r_bytes = (size_t)R * OL_COLS * sizeof(int64_t);
  const void* bufs[6] = {mask, label_to_cell, rings, first, bad, vertices};
  const size_t sizes[6] = {m_bytes, t_bytes, r_bytes, ((size_t)R + 1) * sizeof(int64_t), sizeof(int32_t), 1};      // the size of vertices is on the device
  for (int a = 0; a < 6; ++a)
    for (int b = a + 1; b < 6; ++b)
      if (overlap(bufs[a], sizes[a], bufs[b], sizes[b]))
        return fail("ribca_mask_ring_vertices: mask, label_to_cell, rings, first, vertices and bad must not overlap");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  if (n > 0 && R > 0) {
    const long long bound = 2ll * (H + 1) * (W + 1);
    hipLaunchKernelGGL(ol_vertices_kernel, dim3((unsigned)(((long long)R + 255) / 256)), dim3(256), 0, s, mask, H, W, label_to_cell, L, n,
                       reinterpret_cast<const long long*>(rings), R, reinterpret_cast<const long long*>(first), bound, vertices, bad);
  }
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
