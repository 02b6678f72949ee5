// Per-cell morphology sums of a segmentation mask (Annotator.cell_morphology; steinbock's `measure regionprops`, MCMICRO's quantification table):
// for every cell its area, first and second raw moments, the 4-neighbour pixel edges that leave it (into another cell, into no cell, out of the
// image), the three perimeter classes of scikit-image's perimeter(neighbourhood=4), the bit-quad counts whose combination is the Euler number, the
// pixels inside a caller-given rectangle, and the bounding box.  Integers only: include/ribca_hip.h states the contract,
// tests/morphology_numpy.py restates it.
//   morph_init    sums = 0, bbox = (INT32_MAX, -1, INT32_MAX, -1).
//   morph_tile    one workgroup per MO_TILE x MO_TILE pixel tile: the tile and a 2-pixel halo go to LDS already mapped to cell indices (-1 = no
//                 cell, also outside the image), one global read of the mask per staged pixel; a second pass marks the border pixels of the tile
//                 and a 1-pixel ring (a pixel's perimeter class needs the border state of its eight neighbours).  A thread owns four consecutive
//                 pixels of one row and sums a stretch of them that lies in one cell in scalars (tile-local coordinates, 32 bits; sums of
//                 conditions, no conditional stores, or the compiler keeps the struct in memory), so a stretch is one event; the 2 x 2 windows are counted by the pixel in their lower right corner (the last row and column also take the
//                 windows that hang over the image), and only windows that are not uniform produce an event.  Events go to an LDS table keyed by
//                 cell (32-bit compare-and-swap on the key, MO_PROBES slots at most, 32-bit adds, min / max for the box); an event that finds no
//                 slot goes straight to the cell's global row.  The flush is once per distinct cell of the tile: the moments are moved from
//                 tile-local to image coordinates in 64 bits and added with 64-bit integer atomics, the box with 32-bit min / max.
// No per-pixel array, nothing indexed by a label: nothing goes to scratch.  No loop waits for another thread.  Measured form: DESIGN.md section 20.
#include <limits.h>

#include <algorithm>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

namespace ribca {
namespace {

constexpr int MO_TILE = 32;                   // pixels of a workgroup's tile along either axis
constexpr int MO_HALO = 2;
constexpr int MO_SIDE = MO_TILE + 2 * MO_HALO;      // the staged square
constexpr int MO_RING = MO_TILE + 2;                // the square whose border state is kept: the tile and one ring
constexpr int MO_SLOTS = 256;                 // entries of the workgroup's LDS table
constexpr int MO_SLOT_BITS = 8;
constexpr int MO_PROBES = 8;                  // slots an event tries in LDS before it goes to the global row
constexpr int MO_COLS = 16;
constexpr int MO_N_MAX = 1 << 21;
constexpr int MO_HW_MAX = 65535;
constexpr int MO_RESERVED = 256;              // bytes of the workspace: the kernels accumulate in the outputs and do not touch it

// columns of sums
constexpr int C_AREA = 0, C_R = 1, C_C = 2, C_RR = 3, C_CC = 4, C_RC = 5, C_E_CELL = 6, C_E_BG = 7, C_E_IMG = 8, C_PA = 9, C_PB = 10, C_PC = 11,
              C_Q1 = 12, C_Q3 = 13, C_QD = 14, C_RECT = 15;

static_assert(1 << MO_SLOT_BITS == MO_SLOTS, "the LDS table is indexed by the top bits of a 32-bit hash");
static_assert(MO_TILE * MO_TILE == 256 * 4, "four pixels of one row per thread");
static_assert(MO_SLOTS == 256, "the flush is one thread per slot");
static_assert(MO_SIDE * MO_SIDE * 4 + MO_RING * MO_RING + MO_SLOTS * (4 + MO_COLS * 4 + 16) <= 32 * 1024, "LDS of morph_tile");
static_assert(MO_TILE * MO_TILE * (MO_TILE - 1) * (MO_TILE - 1) < (1 << 30), "tile-local second moments in 32 bits");

int fail(const char* msg) { return api_fail(msg); }

__global__ __launch_bounds__(256) void morph_init_kernel(unsigned long long* __restrict__ sums, int32_t* __restrict__ bbox, int n) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)n * MO_COLS; e += stride) sums[e] = 0ull;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)n * 4; e += stride) bbox[e] = (e & 1) ? -1 : INT_MAX;
}

// what a stretch of pixels of one cell in one row of the tile adds up to, in tile-local coordinates
struct Stretch {
  int cell;                                  // -1: empty
  unsigned area, sr, sc, srr, scc, src;      // the raw moments over (dr, dc)
  unsigned e_cell, e_bg, e_img, pa, pb, pc, in_rect;
  int cmin, cmax;                            // dc of its first and last pixel; its row is the thread's
};

__device__ __forceinline__ void add64(unsigned long long* __restrict__ row, int col, unsigned long long v) {
  if (v) atomicAdd(&row[col], v);
}

// the moments of `area` pixels move from the tile's origin (r0, c0) to the image's; every term stays below 2^63 for H, W <= 65535, H W < 2^31
__device__ __forceinline__ void global_moments(unsigned long long* __restrict__ sums, int32_t* __restrict__ bbox, int cell, int r0, int c0,
                                               unsigned area, unsigned sr, unsigned sc, unsigned srr, unsigned scc, unsigned src, int rmin, int rmax,
                                               int cmin, int cmax) {
  unsigned long long* __restrict__ row = sums + (size_t)cell * MO_COLS;
  const unsigned long long a = area, R = (unsigned long long)r0, C = (unsigned long long)c0;
  atomicAdd(&row[C_AREA], a);
  add64(row, C_R, a * R + sr);
  add64(row, C_C, a * C + sc);
  add64(row, C_RR, a * R * R + 2ull * R * sr + srr);
  add64(row, C_CC, a * C * C + 2ull * C * sc + scc);
  add64(row, C_RC, a * R * C + R * sc + C * sr + src);
  int32_t* __restrict__ box = bbox + (size_t)cell * 4;
  atomicMin(&box[0], r0 + rmin);
  atomicMax(&box[1], r0 + rmax);
  atomicMin(&box[2], c0 + cmin);
  atomicMax(&box[3], c0 + cmax);
}

// one pixel edge that leaves the cell: out of the image, into another cell, or into no cell
__device__ __forceinline__ void leave(Stretch& s, bool outside, int other) {
  s.e_img += outside ? 1u : 0u;      // sums of conditions, not conditional stores: the stretch stays in registers
  s.e_cell += !outside && other >= 0 ? 1u : 0u;
  s.e_bg += !outside && other < 0 ? 1u : 0u;
}

// the slot of `cell` in the workgroup's table, -1 when MO_PROBES slots are taken by others
__device__ __forceinline__ int find_slot(int* hkey, int cell) {
  int slot = (int)(((uint32_t)cell * 0x9E3779B1u) >> (32 - MO_SLOT_BITS));
  for (int probe = 0; probe < MO_PROBES; ++probe) {
    const int old = atomicCAS(&hkey[slot], -1, cell);
    if (old == -1 || old == cell) return slot;
    slot = (slot + 1) & (MO_SLOTS - 1);
  }
  return -1;
}

__device__ __forceinline__ void lds_add(unsigned int* p, unsigned v) {
  if (v) atomicAdd(p, v);
}

__device__ __forceinline__ void emit_stretch(int* hkey, unsigned int (*hval)[MO_COLS], int (*hbox)[4], unsigned long long* __restrict__ sums,
                                             int32_t* __restrict__ bbox, int r0, int c0, int dr, const Stretch& s) {
  const int slot = find_slot(hkey, s.cell);
  if (slot >= 0) {
    unsigned int* v = hval[slot];
    atomicAdd(&v[C_AREA], s.area);
    lds_add(&v[C_R], s.sr);
    lds_add(&v[C_C], s.sc);
    lds_add(&v[C_RR], s.srr);
    lds_add(&v[C_CC], s.scc);
    lds_add(&v[C_RC], s.src);
    lds_add(&v[C_E_CELL], s.e_cell);
    lds_add(&v[C_E_BG], s.e_bg);
    lds_add(&v[C_E_IMG], s.e_img);
    lds_add(&v[C_PA], s.pa);
    lds_add(&v[C_PB], s.pb);
    lds_add(&v[C_PC], s.pc);
    lds_add(&v[C_RECT], s.in_rect);
    atomicMin(&hbox[slot][0], dr);
    atomicMax(&hbox[slot][1], dr);
    atomicMin(&hbox[slot][2], s.cmin);
    atomicMax(&hbox[slot][3], s.cmax);
    return;
  }
  global_moments(sums, bbox, s.cell, r0, c0, s.area, s.sr, s.sc, s.srr, s.scc, s.src, dr, dr, s.cmin, s.cmax);
  unsigned long long* __restrict__ row = sums + (size_t)s.cell * MO_COLS;
  add64(row, C_E_CELL, s.e_cell);
  add64(row, C_E_BG, s.e_bg);
  add64(row, C_E_IMG, s.e_img);
  add64(row, C_PA, s.pa);
  add64(row, C_PB, s.pb);
  add64(row, C_PC, s.pc);
  add64(row, C_RECT, s.in_rect);
}

// one cell holds k of a window's four pixels: q1 at k = 1, q3 at k = 3, qd at k = 2 on a diagonal
__device__ __forceinline__ void emit_quad(int* hkey, unsigned int (*hval)[MO_COLS], unsigned long long* __restrict__ sums, int cell, int k, bool diagonal) {
  int col;
  if (k == 1) col = C_Q1;
  else if (k == 3) col = C_Q3;
  else if (k == 2 && diagonal) col = C_QD;
  else return;
  const int slot = find_slot(hkey, cell);
  if (slot >= 0) atomicAdd(&hval[slot][col], 1u);
  else atomicAdd(&sums[(size_t)cell * MO_COLS + col], 1ull);
}

// the window  a b / c d : every distinct cell in it once, at its first pixel in reading order
__device__ __forceinline__ void quad(int* hkey, unsigned int (*hval)[MO_COLS], unsigned long long* __restrict__ sums, int a, int b, int c, int d) {
  if (a == b && b == c && c == d) return;
  if (a >= 0) emit_quad(hkey, hval, sums, a, 1 + (b == a) + (c == a) + (d == a), d == a);
  if (b >= 0 && b != a) emit_quad(hkey, hval, sums, b, 1 + (c == b) + (d == b), c == b);
  if (c >= 0 && c != a && c != b) emit_quad(hkey, hval, sums, c, 1 + (d == c), false);
  if (d >= 0 && d != a && d != b && d != c) emit_quad(hkey, hval, sums, d, 1, false);
}

// grid: the tiles in row-major order, tiles_x of them per row of tiles
__global__ __launch_bounds__(256) void morph_tile_kernel(const int32_t* __restrict__ mask, int H, int W, const int32_t* __restrict__ label_to_cell, int L,
                                                         int n, const int32_t* __restrict__ rect, int tiles_x, unsigned long long* __restrict__ sums,
                                                         int32_t* __restrict__ bbox) {
  __shared__ int cell[MO_SIDE * MO_SIDE];
  __shared__ uint8_t edge[MO_RING * MO_RING];      // 1: the pixel is a border pixel of its cell
  __shared__ int hkey[MO_SLOTS];
  __shared__ unsigned int hval[MO_SLOTS][MO_COLS];
  __shared__ int hbox[MO_SLOTS][4];
  const int tid = threadIdx.x;
  const int r0 = (int)(blockIdx.x / (unsigned)tiles_x) * MO_TILE, c0 = (int)(blockIdx.x % (unsigned)tiles_x) * MO_TILE;
  hkey[tid] = -1;
  for (int k = 0; k < MO_COLS; ++k) hval[tid][k] = 0u;
  hbox[tid][0] = INT_MAX, hbox[tid][1] = -1, hbox[tid][2] = INT_MAX, hbox[tid][3] = -1;
  for (int e = tid; e < MO_SIDE * MO_SIDE; e += 256) {
    const int r = r0 - MO_HALO + e / MO_SIDE, c = c0 - MO_HALO + e % MO_SIDE;
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
  for (int e = tid; e < MO_RING * MO_RING; e += 256) {
    const int p = (e / MO_RING + 1) * MO_SIDE + e % MO_RING + 1;      // in the staged square
    const int own = cell[p];
    edge[e] = own >= 0 && (cell[p - MO_SIDE] != own || cell[p + MO_SIDE] != own || cell[p - 1] != own || cell[p + 1] != own) ? 1 : 0;
  }
  __syncthreads();

  const int dr = tid >> 3, dc0 = (tid & 7) * 4;
  const int r = r0 + dr;
  Stretch s;
  s.cell = -1;
  int rr0 = 0, rr1 = 0, rc0 = 0, rc1 = 0;      // the rectangle of the stretch's cell
  if (r < H) {
    for (int k = 0; k < 4; ++k) {
      const int dc = dc0 + k, c = c0 + dc;
      if (c >= W) break;
      const int p = (dr + MO_HALO) * MO_SIDE + dc + MO_HALO;
      const int own = cell[p];
      const int up = cell[p - MO_SIDE], down = cell[p + MO_SIDE], left = cell[p - 1], right = cell[p + 1];
      quad(hkey, hval, sums, cell[p - MO_SIDE - 1], up, left, own);
      if (c == W - 1) quad(hkey, hval, sums, up, cell[p - MO_SIDE + 1], own, right);      // the windows that hang over the image: -1 out there
      if (r == H - 1) quad(hkey, hval, sums, left, own, cell[p + MO_SIDE - 1], down);
      if (c == W - 1 && r == H - 1) quad(hkey, hval, sums, own, right, down, cell[p + MO_SIDE + 1]);
      if (own != s.cell) {
        if (s.cell >= 0) emit_stretch(hkey, hval, hbox, sums, bbox, r0, c0, dr, s);
        s.cell = own;
        s.area = s.sr = s.sc = s.srr = s.scc = s.src = s.e_cell = s.e_bg = s.e_img = s.pa = s.pb = s.pc = s.in_rect = 0u;
        s.cmin = dc;
        if (own >= 0 && rect) {
          const int32_t* __restrict__ q = rect + (size_t)own * 4;
          rr0 = q[0], rr1 = q[1], rc0 = q[2], rc1 = q[3];
        }
      }
      if (own < 0) continue;
      s.area += 1u;
      s.sr += (unsigned)dr;
      s.sc += (unsigned)dc;
      s.srr += (unsigned)(dr * dr);
      s.scc += (unsigned)(dc * dc);
      s.src += (unsigned)(dr * dc);
      s.cmax = dc;
      if (rect && r >= rr0 && r < rr1 && c >= rc0 && c < rc1) s.in_rect += 1u;
      // the four pixel edges: a neighbour outside the image holds -1 in LDS as no cell does, the coordinates tell them apart
      if (up != own) leave(s, r == 0, up);
      if (down != own) leave(s, r == H - 1, down);
      if (left != own) leave(s, c == 0, left);
      if (right != own) leave(s, c == W - 1, right);
      const int b = (dr + 1) * MO_RING + dc + 1;      // in the ring square
      if (edge[b]) {
        const int na = (up == own && edge[b - MO_RING]) + (down == own && edge[b + MO_RING]) + (left == own && edge[b - 1]) + (right == own && edge[b + 1]);
        const int nb = (cell[p - MO_SIDE - 1] == own && edge[b - MO_RING - 1]) + (cell[p - MO_SIDE + 1] == own && edge[b - MO_RING + 1]) +
                       (cell[p + MO_SIDE - 1] == own && edge[b + MO_RING - 1]) + (cell[p + MO_SIDE + 1] == own && edge[b + MO_RING + 1]);
        const int v = 1 + 2 * na + 10 * nb;
        s.pa += v == 5 || v == 7 || v == 15 || v == 17 || v == 25 || v == 27 ? 1u : 0u;
        s.pb += v == 21 || v == 33 ? 1u : 0u;
        s.pc += v == 13 || v == 23 ? 1u : 0u;
      }
    }
    if (s.cell >= 0) emit_stretch(hkey, hval, hbox, sums, bbox, r0, c0, dr, s);
  }
  __syncthreads();
  const int key = hkey[tid];
  if (key >= 0) {
    const unsigned int* v = hval[tid];
    if (v[C_AREA]) global_moments(sums, bbox, key, r0, c0, v[C_AREA], v[C_R], v[C_C], v[C_RR], v[C_CC], v[C_RC], hbox[tid][0], hbox[tid][1], hbox[tid][2],
                                  hbox[tid][3]);
    unsigned long long* __restrict__ row = sums + (size_t)key * MO_COLS;
    for (int col = C_E_CELL; col < MO_COLS; ++col) add64(row, col, v[col]);
  }
}

bool sizes_ok(int H, int W, int n) {
  return H >= 1 && W >= 1 && H <= MO_HW_MAX && W <= MO_HW_MAX && (long long)H * W < (1ll << 31) && n >= 1 && n <= MO_N_MAX;
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_mask_morphology_ws_bytes(int32_t H, int32_t W, int32_t n) {
  if (!sizes_ok(H, W, n)) return 0;
  Carver cv(nullptr);
  cv.take<uint8_t>(MO_RESERVED);
  return (int64_t)cv.off;
}

int ribca_mask_morphology(const int32_t* mask, int32_t H, int32_t W, const int32_t* label_to_cell, int32_t L, int32_t n, const int32_t* rect,
                          uint64_t* sums, int32_t* bbox, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!mask || !label_to_cell || !sums || !bbox || !workspace) return fail("ribca_mask_morphology: NULL buffer");
  if (H < 1 || W < 1 || H > MO_HW_MAX || W > MO_HW_MAX || (long long)H * W >= (1ll << 31))
    return fail("ribca_mask_morphology: needs 1 <= H, W <= 65535 and H W < 2^31");
  if (L < 1) return fail("ribca_mask_morphology: needs 1 <= L");
  if (n < 1 || n > MO_N_MAX) return fail("ribca_mask_morphology: needs 1 <= n <= 2^21");
  if (workspace_bytes < ribca_mask_morphology_ws_bytes(H, W, n)) return fail("ribca_mask_morphology: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
  const int tiles_x = (W + MO_TILE - 1) / MO_TILE, tiles_y = (H + MO_TILE - 1) / MO_TILE;      // tiles_x tiles_y < 2^31 / 1024 + H + W
  hipLaunchKernelGGL(morph_init_kernel, dim3((unsigned)std::min<size_t>(((size_t)n * MO_COLS + 255) / 256, 16384)), dim3(256), 0, s, out, bbox, n);
  hipLaunchKernelGGL(morph_tile_kernel, dim3((unsigned)((long long)tiles_x * tiles_y)), dim3(256), 0, s, mask, H, W, label_to_cell, L, n, rect, tiles_x,
                     out, bbox);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
