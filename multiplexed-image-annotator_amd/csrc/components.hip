// Connected components of a segmentation mask (ImageProcessor(repair_mask=A), ops.repair_labels): every pixel gets the raster index of the first
// pixel of its component, every component its area, whether it touches the image border, and the smallest and largest label that borders it.
// A pixel v > 0 is of class v, every pixel <= 0 of the class "background"; foreground connects at 8-connectivity within its class, background at
// 4-connectivity, the pairing of the Euler number of morphology.py.  Integers only: include/ribca_hip.h states the contract,
// tests/components_numpy.py restates it.  A union-find whose representative is the smallest raster index, in launches of their own:
//   cc_tile      one workgroup per CC_TILE x CC_TILE pixel tile: classes to LDS, a parent array in LDS (parent <= own index, always), every pixel
//                united with its left and upper neighbours (foreground: the two upper diagonals too) by atomicMin, then every pixel writes the
//                GLOBAL raster index of its tile-local root as its parent.  Raster order inside a tile is raster order in the image.
//   cc_seam      one thread per pixel of a tile's first row or first column: unites it with its neighbours across the seam, the diagonal ones
//                for foreground.  Workgroups on different CUs read and write the parent array in this launch, so it is touched through agent-scope
//                atomics only (loads too: L1 is per CU and is not refreshed by other CUs' stores).
//   cc_flatten   root[p] = the end of p's parent chain, in place: a parent that another thread has already replaced by its root is still an
//                ancestor, so either value of a word leads to the same end.  Also writes every row of stats: 0, and INT32_MAX as lo of a root.
//   cc_stats     one workgroup per tile: the roots of the tile and the labels of the tile and a 1-pixel ring go to LDS; a thread sums a stretch
//                of four pixels of a row in scalars, stretches go to an LDS table keyed by root (twice as many slots as pixels: a probe sequence
//                ends on its own), and the flush is ONE global atomic per column and distinct root of the tile -- the exterior background of a
//                4096^2 image is one row of stats: 16 M adds to it would serialise, 16 k do not.
//   cc_finish    lo = 0 for the roots nothing borders (their hi stayed 0).
// The launches are separate because each needs the whole of the one before: the seam pass the tile-local roots of both sides, the flatten pass a
// parent array nobody unites in any more, the statistics the final roots, and a kernel boundary is the only device-wide barrier that makes no
// thread wait for another.  Every loop ends on its own: a find walks strictly decreasing indices, a union retries atomicMin with a strictly
// decreasing larger root.  Sums, min, max and or of integers: the result is a function of the mask alone.  Tables in LDS, scalars in registers:
// nothing goes to scratch.  Measured form: DESIGN.md section 23.
#include <limits.h>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

namespace ribca {
namespace {

constexpr int CC_TILE = 32;                   // pixels of a workgroup's tile along either axis
constexpr int CC_PIXELS = CC_TILE * CC_TILE;
constexpr int CC_SIDE = CC_TILE + 2;          // cc_stats: the tile and a 1-pixel ring
constexpr int CC_SLOTS = 2 * CC_PIXELS;       // cc_stats: entries of the LDS table, more than a tile has roots
constexpr int CC_SLOT_BITS = 11;
constexpr int CC_RESERVED = 256;              // bytes of the workspace: the kernels work in the outputs and do not touch it

static_assert(1 << CC_SLOT_BITS == CC_SLOTS, "the LDS table is indexed by the top bits of a 32-bit hash");
static_assert(CC_PIXELS == 256 * 4, "four pixels of one row per thread");
static_assert(CC_PIXELS * 4 + CC_SIDE * CC_SIDE * 4 + CC_SLOTS * 5 * 4 <= 64 * 1024, "LDS of cc_stats");

int fail(const char* msg) { return api_fail(msg); }

__device__ __forceinline__ int class_of(int32_t v) { return v > 0 ? v : 0; }

// ---- the union-find in LDS ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(volatile int* par, int x) {
  for (int p = par[x]; p != x; p = par[x]) x = p;      // p < x: strictly decreasing
  return x;
}

// after it a and b have one root once every union of the workgroup is through: the larger root is hung under the smaller one; where another
// thread hung it elsewhere first (old != a), what it pointed to is united with b in its place.  max(a, b) falls in every round.
__device__ __forceinline__ void lds_union(int* par, int a, int b) {
  for (;;) {
    a = lds_find(par, a);
    b = lds_find(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
}

// grid: the tiles in row-major order, tiles_x of them per row of tiles
__global__ __launch_bounds__(256) void cc_tile_kernel(const int32_t* __restrict__ mask, int H, int W, int tiles_x, int32_t* __restrict__ parent) {
  __shared__ int cls[CC_PIXELS];      // class, -1 outside the image
  __shared__ int par[CC_PIXELS];
  const int tid = threadIdx.x;
  const int r0 = (int)(blockIdx.x / (unsigned)tiles_x) * CC_TILE, c0 = (int)(blockIdx.x % (unsigned)tiles_x) * CC_TILE;
  for (int e = tid; e < CC_PIXELS; e += 256) {
    const int r = r0 + e / CC_TILE, c = c0 + e % CC_TILE;
    cls[e] = r < H && c < W ? class_of(mask[(size_t)r * W + c]) : -1;
    par[e] = e;
  }
  __syncthreads();
  int same = 1;
  for (int e = tid; e < CC_PIXELS; e += 256) same &= cls[e] < 0 || cls[e] == cls[0] ? 1 : 0;
  if (__syncthreads_and(same)) {      // uniform over the workgroup: one class in the whole tile (most of the background of a real image), one component
    for (int e = tid; e < CC_PIXELS; e += 256) {
      const int r = r0 + e / CC_TILE, c = c0 + e % CC_TILE;
      if (r < H && c < W) parent[(size_t)r * W + c] = r0 * W + c0;
    }
    return;
  }
  for (int e = tid; e < CC_PIXELS; e += 256) {
    const int v = cls[e];
    if (v < 0) continue;
    const int lr = e / CC_TILE, lc = e % CC_TILE;
    if (lc > 0 && cls[e - 1] == v) lds_union(par, e, e - 1);
    if (lr > 0) {
      if (cls[e - CC_TILE] == v) lds_union(par, e, e - CC_TILE);
      if (v > 0) {
        if (lc > 0 && cls[e - CC_TILE - 1] == v) lds_union(par, e, e - CC_TILE - 1);
        if (lc < CC_TILE - 1 && cls[e - CC_TILE + 1] == v) lds_union(par, e, e - CC_TILE + 1);
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < CC_PIXELS; e += 256) {
    const int r = r0 + e / CC_TILE, c = c0 + e % CC_TILE;
    if (r >= H || c >= W) continue;
    const int t = lds_find(par, e);
    parent[(size_t)r * W + c] = (r0 + t / CC_TILE) * W + c0 + t % CC_TILE;
  }
}

// ---- the union-find across workgroups: agent-scope atomics only ------------------------------------------------------------------------------------
__device__ __forceinline__ int agent_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int global_find(int32_t* parent, int x) {
  for (int p = agent_load(parent + x); p != x; p = agent_load(parent + x)) x = p;
  return x;
}

__device__ __forceinline__ void global_union(int32_t* parent, int a, int b) {
  for (;;) {
    a = global_find(parent, a);
    b = global_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

// thread t < n_h: pixel t % W of the horizontal seam t / W (row (t / W + 1) CC_TILE); the others: pixel (t - n_h) % H of the vertical seam
// (t - n_h) / H.  A seam pixel is united with the pixels of the tiles above / to the left that touch it.
__global__ __launch_bounds__(256) void cc_seam_kernel(const int32_t* __restrict__ mask, int H, int W, long long n_h, long long n_all, int32_t* parent) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_all) return;
  if (t < n_h) {
    const int r = ((int)(t / W) + 1) * CC_TILE, c = (int)(t % W);      // 1 <= r < H
    const int p = r * W + c;
    const int v = class_of(mask[p]);
    if (class_of(mask[p - W]) == v) global_union(parent, p, p - W);
    if (v > 0) {
      if (c > 0 && mask[p - W - 1] == v) global_union(parent, p, p - W - 1);
      if (c < W - 1 && mask[p - W + 1] == v) global_union(parent, p, p - W + 1);
    }
  } else {
    const long long u = t - n_h;
    const int c = ((int)(u / H) + 1) * CC_TILE, r = (int)(u % H);      // 1 <= c < W
    const int p = r * W + c;
    const int v = class_of(mask[p]);
    if (class_of(mask[p - 1]) == v) global_union(parent, p, p - 1);
    if (v > 0) {
      if (r > 0 && mask[p - W - 1] == v) global_union(parent, p, p - W - 1);
      if (r < H - 1 && mask[p + W - 1] == v) global_union(parent, p, p + W - 1);
    }
  }
}

// in place: other threads replace parents by roots meanwhile, and either value of a word is an ancestor of the pixel that holds it
__global__ __launch_bounds__(256) void cc_flatten_kernel(int32_t* root, int n, int32_t* __restrict__ stats) {
  const unsigned q0 = blockIdx.x * 256u + threadIdx.x;
  if (q0 >= (unsigned)n) return;
  const int p = (int)q0;
  int x = p;
  for (int q = root[x]; q != x; q = root[x]) x = q;
  if (x != p) root[p] = x;
  reinterpret_cast<int4*>(stats)[p] = make_int4(0, 0, x == p ? INT_MAX : 0, 0);
}

// ---- the statistics ----------------------------------------------------------------------------------------------------------------------------
struct Stretch {
  int root;      // -1: empty
  int area, border, lo, hi;
};

__device__ __forceinline__ void emit(int* hkey, int* harea, int* hborder, int* hlo, int* hhi, const Stretch& s) {
  int slot = (int)(((uint32_t)s.root * 0x9E3779B1u) >> (32 - CC_SLOT_BITS));
  for (int probe = 0; probe < CC_SLOTS; ++probe) {      // at most CC_PIXELS keys in CC_SLOTS slots: a free or own slot comes up
    const int old = atomicCAS(&hkey[slot], -1, s.root);
    if (old == -1 || old == s.root) break;
    slot = (slot + 1) & (CC_SLOTS - 1);
  }
  atomicAdd(&harea[slot], s.area);
  if (s.border) atomicOr(&hborder[slot], 1);
  if (s.hi > 0) {
    atomicMin(&hlo[slot], s.lo);
    atomicMax(&hhi[slot], s.hi);
  }
}

// grid: the tiles in row-major order.  stats rows were set by cc_flatten: lo = INT32_MAX at the roots
__global__ __launch_bounds__(256) void cc_stats_kernel(const int32_t* __restrict__ mask, const int32_t* __restrict__ root, int H, int W, int tiles_x,
                                                       int32_t* __restrict__ stats) {
  __shared__ int lab[CC_SIDE * CC_SIDE];      // max(label, 0), -1 outside the image
  __shared__ int rt[CC_PIXELS];
  __shared__ int hkey[CC_SLOTS];
  __shared__ int harea[CC_SLOTS];
  __shared__ int hborder[CC_SLOTS];
  __shared__ int hlo[CC_SLOTS];
  __shared__ int hhi[CC_SLOTS];
  const int tid = threadIdx.x;
  const int r0 = (int)(blockIdx.x / (unsigned)tiles_x) * CC_TILE, c0 = (int)(blockIdx.x % (unsigned)tiles_x) * CC_TILE;
  for (int e = tid; e < CC_SLOTS; e += 256) hkey[e] = -1, harea[e] = 0, hborder[e] = 0, hlo[e] = INT_MAX, hhi[e] = 0;
  for (int e = tid; e < CC_SIDE * CC_SIDE; e += 256) {
    const int r = r0 - 1 + e / CC_SIDE, c = c0 - 1 + e % CC_SIDE;
    lab[e] = r >= 0 && r < H && c >= 0 && c < W ? class_of(mask[(size_t)r * W + c]) : -1;
  }
  for (int e = tid; e < CC_PIXELS; e += 256) {
    const int r = r0 + e / CC_TILE, c = c0 + e % CC_TILE;
    rt[e] = r < H && c < W ? root[(size_t)r * W + c] : -1;
  }
  __syncthreads();
  const int dr = tid >> 3, dc0 = (tid & 7) * 4;
  const int r = r0 + dr;
  Stretch s;
  s.root = -1, s.area = 0, s.border = 0, s.lo = INT_MAX, s.hi = 0;
  if (r < H) {
    for (int k = 0; k < 4; ++k) {
      const int dc = dc0 + k, c = c0 + dc;
      if (c >= W) break;
      const int own_root = rt[dr * CC_TILE + dc];
      if (own_root != s.root) {
        if (s.root >= 0) emit(hkey, harea, hborder, hlo, hhi, s);
        s.root = own_root, s.area = 0, s.border = 0, s.lo = INT_MAX, s.hi = 0;
      }
      const int p = (dr + 1) * CC_SIDE + dc + 1;
      const int own = lab[p];
      s.area += 1;
      s.border |= (r == 0 || r == H - 1 || c == 0 || c == W - 1) ? 1 : 0;
      const int nb[4] = {lab[p - CC_SIDE], lab[p + CC_SIDE], lab[p - 1], lab[p + 1]};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool other = nb[j] > 0 && nb[j] != own;      // a labelled pixel of another class; outside the image lab is -1
        s.lo = other && nb[j] < s.lo ? nb[j] : s.lo;
        s.hi = other && nb[j] > s.hi ? nb[j] : s.hi;
      }
    }
    if (s.root >= 0) emit(hkey, harea, hborder, hlo, hhi, s);
  }
  __syncthreads();
  for (int e = tid; e < CC_SLOTS; e += 256) {
    const int key = hkey[e];
    if (key < 0) continue;
    int32_t* __restrict__ row = stats + (size_t)key * 4;
    atomicAdd(&row[0], harea[e]);
    if (hborder[e]) atomicOr(&row[1], 1);
    if (hhi[e] > 0) {
      atomicMin(&row[2], hlo[e]);
      atomicMax(&row[3], hhi[e]);
    }
  }
}

__global__ __launch_bounds__(256) void cc_finish_kernel(const int32_t* __restrict__ root, int n, int32_t* __restrict__ stats) {
  const unsigned q0 = blockIdx.x * 256u + threadIdx.x;
  if (q0 >= (unsigned)n) return;
  const int p = (int)q0;
  if (root[p] == p && stats[(size_t)p * 4 + 3] == 0) stats[(size_t)p * 4 + 2] = 0;
}

__global__ __launch_bounds__(256) void cc_relabel_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ new_label, int n,
                                                         int32_t* __restrict__ out) {
  const unsigned q0 = blockIdx.x * 256u + threadIdx.x;
  if (q0 >= (unsigned)n) return;
  const int p = (int)q0;
  const int r = root[p];
  out[p] = (unsigned)r < (unsigned)n ? new_label[r] : 0;      // a root outside the image names no component: nothing is read through it
}

bool sizes_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_mask_components_ws_bytes(int32_t H, int32_t W) {
  if (!sizes_ok(H, W)) return 0;
  Carver cv(nullptr);
  cv.take<uint8_t>(CC_RESERVED);
  return (int64_t)cv.off;
}

int ribca_mask_components(const int32_t* mask, int32_t H, int32_t W, int32_t* root, int32_t* stats, void* ws, int64_t ws_bytes, void* stream) {
  if (!mask || !root || !stats || !ws) return fail("ribca_mask_components: NULL buffer");
  if (!sizes_ok(H, W)) return fail("ribca_mask_components: needs 1 <= H, W and H W < 2^31");
  const int64_t need = ribca_mask_components_ws_bytes(H, W);
  if (ws_bytes < need) return fail("ribca_mask_components: workspace too small");
  const size_t bytes = (size_t)H * W * sizeof(int32_t);
  if (overlap(mask, bytes, root, bytes) || overlap(mask, bytes, stats, 4 * bytes) || overlap(root, bytes, stats, 4 * bytes) ||
      overlap(ws, (size_t)need, mask, bytes) || overlap(ws, (size_t)need, root, bytes) || overlap(ws, (size_t)need, stats, 4 * bytes))
    return fail("ribca_mask_components: mask, root, stats and ws must not overlap");
  hipStream_t s = (hipStream_t)stream;
  const int n = H * W;
  const int tiles_x = (W + CC_TILE - 1) / CC_TILE, tiles_y = (H + CC_TILE - 1) / CC_TILE;      // tiles_x tiles_y < 2^31 / 1024 + H + W
  const dim3 tiles((unsigned)((long long)tiles_x * tiles_y)), pixels((unsigned)(((long long)n + 255) / 256));
  hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(256), 0, s, mask, H, W, tiles_x, root);
  const long long n_h = (long long)(tiles_y - 1) * W, n_all = n_h + (long long)(tiles_x - 1) * H;      // < 2 H W / 32
  if (n_all > 0) hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, s, mask, H, W, n_h, n_all, root);
  hipLaunchKernelGGL(cc_flatten_kernel, pixels, dim3(256), 0, s, root, n, stats);
  hipLaunchKernelGGL(cc_stats_kernel, tiles, dim3(256), 0, s, mask, root, H, W, tiles_x, stats);
  hipLaunchKernelGGL(cc_finish_kernel, pixels, dim3(256), 0, s, root, n, stats);
  RIBCA_FINISH();
  return 0;
}

int ribca_mask_relabel(const int32_t* root, const int32_t* new_label, int32_t H, int32_t W, int32_t* out, void* stream) {
  if (!root || !new_label || !out) return fail("ribca_mask_relabel: NULL buffer");
  if (!sizes_ok(H, W)) return fail("ribca_mask_relabel: needs 1 <= H, W and H W < 2^31");
  const size_t bytes = (size_t)H * W * sizeof(int32_t);
  if (overlap(out, bytes, root, bytes) || overlap(out, bytes, new_label, bytes)) return fail("ribca_mask_relabel: out must not overlap root or new_label");
  const int n = H * W;
  hipLaunchKernelGGL(cc_relabel_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, root, new_label, n, out);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
