// Per-cell-type statistics and their two plots (Annotator.generate_heatmap, model.py:700-741; Annotator.cell_type_composition, model.py:861-912).
//   group_sums      sums (groups, c) fp64 and counts (groups) of the rows of x (n, c) by their group id, in THE fixed order of ribca_scratch.h:
//                   one workgroup per chunk of kSumChunk rows and tile of GS_COLS columns adds the rows of the chunk in ascending order, every
//                   (group, column) accumulator started at +0.0 and owned by ONE thread (LDS, never shared: no atomics); chunk_total_kernel then
//                   adds the chunks in ascending order.  The result is a pure function of the inputs.
//   heatmap_raster  mean = sum / count per (row, column), min / max over the means that are not NaN, one thread per pixel: colour
//                   lut[min(255, floor((mean - vmin) / (vmax - vmin) * 256))], silver where the mean is NaN, white in the gap around every cell.
//   table_raster    the paint rule of heatmap_raster over a table of values with vmin / vmax given by the caller (values clamped to them).
//   pie_raster      one thread per pixel: the wedge of a pixel of the disc is the number of boundary rays whose angle is <= the pixel's, the angles
//                   compared by half plane and the sign of a cross product (no transcendental on the device).
#include <cmath>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

#pragma clang fp contract(off)

namespace ribca {
namespace {

constexpr int GS_C_MAX = 1024;     // columns: any number of GS_COLS-wide tiles would do; this keeps the grid and the images small
constexpr int GS_GROUPS_MAX = 256;
constexpr int GS_COLS = 16;       // columns of one workgroup
constexpr int GS_SLOTS = 16;      // group slots of one workgroup: the thread (slot, column) owns the groups g with g % GS_SLOTS == slot
constexpr int GS_BATCH = 8;       // rows whose loads are issued together (the additions stay in row order)
constexpr int HM_CELL_MAX = 64;
constexpr int PIE_DIM_MAX = 16384;
constexpr int PIE_RAYS_MAX = 256;

static_assert(GS_COLS * GS_SLOTS == 256, "one thread per (slot, column)");
static_assert(kSumChunk % GS_BATCH == 0, "a batch never straddles two chunks");
// LDS of group_chunk_kernel: 256 * 16 * 8 accumulators + 256 * 4 counts + 1024 * 4 ids = 37 KiB, four workgroups per CU
static_assert(GS_GROUPS_MAX * GS_COLS * 8 + GS_GROUPS_MAX * 4 + kSumChunk * 4 <= 64 * 1024, "static LDS");

int fail(const char* msg) { return api_fail(msg); }

// the workspace of ribca_group_sums; every word of it is written before it is read
struct GroupWs {
  double* part;       // (chunks, groups, c): the sums of each chunk
  int32_t* ipart;     // (chunks, groups + 1): the rows of each chunk per group, then the rows it skipped
  int64_t* skipped;   // the total of the last column
};

GroupWs carve_group(Carver& cv, int n, int c, int groups) {
  GroupWs w;
  const size_t chunks = (size_t)chunks_of(n);
  w.part = cv.take<double>(chunks * groups * c);
  w.ipart = cv.take<int32_t>(chunks * (groups + 1));
  w.skipped = cv.take<int64_t>(1);
  return w;
}

__global__ __launch_bounds__(256) void group_chunk_kernel(const double* __restrict__ x, const int32_t* __restrict__ group, int n, int c, int groups,
                                                          double* __restrict__ part, int32_t* __restrict__ ipart) {
  __shared__ double acc[GS_GROUPS_MAX * GS_COLS];
  __shared__ int32_t cnt[GS_GROUPS_MAX];
  __shared__ int32_t gid[kSumChunk];
  const int ch = blockIdx.x, tile = blockIdx.y;
  const int lc = threadIdx.x % GS_COLS, slot = threadIdx.x / GS_COLS;
  const int col = tile * GS_COLS + lc;
  const int r0 = ch * kSumChunk;
  const int rows = min(kSumChunk, n - r0);
  for (int r = threadIdx.x; r < rows; r += 256) gid[r] = group[r0 + r];
  for (int g = slot; g < groups; g += GS_SLOTS) {
    acc[g * GS_COLS + lc] = 0.0;
    if (lc == 0) cnt[g] = 0;
  }
  __syncthreads();
  int skipped = 0;
  if (col < c) {
    const double* xp = x + (size_t)r0 * c + col;
    for (int b = 0; b < rows; b += GS_BATCH) {
      int g[GS_BATCH];
      double v[GS_BATCH];
#pragma unroll
      for (int u = 0; u < GS_BATCH; ++u) {
        const int r = b + u;
        g[u] = r < rows ? gid[r] : -1;
        const bool mine = g[u] >= 0 && g[u] < groups && g[u] % GS_SLOTS == slot;
        v[u] = mine ? xp[(size_t)r * c] : 0.0;
        if (r < rows && (g[u] < 0 || g[u] >= groups)) ++skipped;
        if (!mine) g[u] = -1;
      }
#pragma unroll
      for (int u = 0; u < GS_BATCH; ++u) {
        if (g[u] < 0) continue;
        acc[g[u] * GS_COLS + lc] = acc[g[u] * GS_COLS + lc] + v[u];
        if (lc == 0) ++cnt[g[u]];
      }
    }
    // the accumulators of this thread leave as it wrote them: no other thread touched them
    for (int gg = slot; gg < groups; gg += GS_SLOTS) {
      part[((size_t)ch * groups + gg) * c + col] = acc[gg * GS_COLS + lc];
      if (tile == 0 && lc == 0) ipart[(size_t)ch * (groups + 1) + gg] = cnt[gg];
    }
    if (tile == 0 && threadIdx.x == 0) ipart[(size_t)ch * (groups + 1) + groups] = skipped;
  }
}

// counts[g] and *skipped as 64-bit totals of the chunks' 32-bit ones, one thread per column of ipart
__global__ __launch_bounds__(256) void group_count_kernel(const int32_t* __restrict__ ipart, int chunks, int groups, int64_t* __restrict__ counts,
                                                          int64_t* __restrict__ skipped) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o > groups) return;
  int64_t s = 0;
  for (int ch = 0; ch < chunks; ++ch) s += ipart[(size_t)ch * (groups + 1) + o];
  if (o < groups) counts[o] = s; else *skipped = s;
}

__device__ __forceinline__ double cell_mean(const double* __restrict__ sums, const int64_t* __restrict__ counts, int row, int cols, int col) {
  const int64_t k = counts[row];
  return k > 0 ? sums[(size_t)row * cols + col] / (double)k : nan("");
}

// range[0] = the smallest, range[1] = the largest mean that is not NaN (NaN both when there is none): one workgroup
__global__ __launch_bounds__(256) void heatmap_range_kernel(const double* __restrict__ sums, const int64_t* __restrict__ counts, int rows, int cols,
                                                            double* __restrict__ range) {
  __shared__ double lo[256], hi[256];
  double a = nan(""), b = nan("");
  for (int i = threadIdx.x; i < rows * cols; i += 256) {
    const double m = cell_mean(sums, counts, i / cols, cols, i % cols);
    if (m == m) {
      a = (a == a) ? fmin(a, m) : m;
      b = (b == b) ? fmax(b, m) : m;
    }
  }
  lo[threadIdx.x] = a;
  hi[threadIdx.x] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      lo[threadIdx.x] = fmin(lo[threadIdx.x], lo[threadIdx.x + s]);      // fmin / fmax return the operand that is a number
      hi[threadIdx.x] = fmax(hi[threadIdx.x], hi[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    range[0] = lo[0];
    range[1] = hi[0];
  }
}

__global__ __launch_bounds__(256) void heatmap_paint_kernel(const double* __restrict__ sums, const int64_t* __restrict__ counts, int rows, int cols,
                                                            const uint8_t* __restrict__ lut, int cell, int gap, const double* __restrict__ range,
                                                            uint8_t* __restrict__ out) {
  const long long W = (long long)cols * cell;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= W * rows * cell) return;
  const int py = (int)(p / W), px = (int)(p % W);
  const int ly = py % cell, lx = px % cell;
  uint8_t r = 255, g = 255, b = 255;
  if (ly >= gap && ly < cell - gap && lx >= gap && lx < cell - gap) {
    const double m = cell_mean(sums, counts, py / cell, cols, px / cell);
    if (m == m) {
      const double vmin = range[0], vmax = range[1];
      int idx = 0;
      if (vmax != vmin) {
        const double d = m - vmin;
        const double w = vmax - vmin;
        const double q = floor(d / w * 256.0);      // three roundings: contraction is off
        idx = q >= 255.0 ? 255 : (q >= 0.0 ? (int)q : 0);      // (q is NaN or below 0 only for infinite means)
      }
      r = lut[3 * idx], g = lut[3 * idx + 1], b = lut[3 * idx + 2];
    } else {
      r = g = b = 192;
    }
  }
  out[3 * p] = r, out[3 * p + 1] = g, out[3 * p + 2] = b;
}

// the paint rule with the scale given by the caller: the value clamped to [vmin, vmax], the middle entry when the scale is a point
__global__ __launch_bounds__(256) void table_paint_kernel(const double* __restrict__ values, int rows, int cols, const uint8_t* __restrict__ lut, int cell,
                                                          int gap, double vmin, double vmax, uint8_t* __restrict__ out) {
  const long long W = (long long)cols * cell;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= W * rows * cell) return;
  const int py = (int)(p / W), px = (int)(p % W);
  const int ly = py % cell, lx = px % cell;
  uint8_t r = 255, g = 255, b = 255;
  if (ly >= gap && ly < cell - gap && lx >= gap && lx < cell - gap) {
    const double v = values[(size_t)(py / cell) * cols + px / cell];
    if (v == v) {
      int idx = 128;
      if (vmax != vmin) {
        const double c = v < vmin ? vmin : (v > vmax ? vmax : v);
        const double d = c - vmin;
        const double w = vmax - vmin;
        const double q = floor(d / w * 256.0);      // three roundings: contraction is off
        idx = q >= 255.0 ? 255 : (q >= 0.0 ? (int)q : 0);
      }
      r = lut[3 * idx], g = lut[3 * idx + 1], b = lut[3 * idx + 2];
    } else {
      r = g = b = 192;
    }
  }
  out[3 * p] = r, out[3 * p + 1] = g, out[3 * p + 2] = b;
}

__device__ __forceinline__ int half_of(double vx, double vy) { return (vy > 0.0 || (vy == 0.0 && vx > 0.0)) ? 0 : 1; }

__global__ __launch_bounds__(256) void pie_paint_kernel(const double* __restrict__ rays, int m, const uint8_t* __restrict__ rgb, int size, int radius,
                                                        uint8_t* __restrict__ out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)size * size) return;
  const int c0 = size / 2;
  const int dx = (int)(p % size) - c0, dy = c0 - (int)(p / size);      // dy grows upwards
  uint8_t r = 255, g = 255, b = 255;
  if ((long long)dx * dx + (long long)dy * dy <= (long long)radius * radius) {
    int wedge = 0;
    if (dx != 0 || dy != 0) {
      const double fx = (double)dx, fy = (double)dy;
      const int hp = half_of(fx, fy);
      for (int k = 0; k < m; ++k) {
        const double ax = rays[2 * k], ay = rays[2 * k + 1];
        const int ha = half_of(ax, ay);
        const double t0 = fx * ay;
        const double t1 = fy * ax;
        const bool pixel_first = hp < ha || (hp == ha && t0 - t1 > 0.0);      // the pixel's angle is below the ray's
        if (!pixel_first) ++wedge;
      }
    }
    r = rgb[3 * wedge], g = rgb[3 * wedge + 1], b = rgb[3 * wedge + 2];
  }
  out[3 * p] = r, out[3 * p + 1] = g, out[3 * p + 2] = b;
}

bool group_args_ok(int n, int c, int groups) { return n >= 0 && n != INT32_MAX && c >= 1 && c <= GS_C_MAX && groups >= 1 && groups <= GS_GROUPS_MAX; }
bool heatmap_args_ok(int rows, int cols, int cell, int gap) {
  return rows >= 1 && rows <= GS_GROUPS_MAX && cols >= 1 && cols <= GS_C_MAX && cell >= 1 && cell <= HM_CELL_MAX && gap >= 0 && 2 * gap < cell;
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_group_sums_ws_bytes(int32_t n, int32_t c, int32_t groups) {
  if (!group_args_ok(n, c, groups)) return 0;
  Carver cv(nullptr);
  carve_group(cv, n, c, groups);
  return (int64_t)cv.off;
}

int ribca_group_sums(const double* x, const int32_t* group, int32_t n, int32_t c, int32_t groups, double* sums, int64_t* counts, int64_t* skipped,
                     void* ws, int64_t ws_bytes, void* stream) {
  if (!sums || !counts || !skipped || !ws || (n > 0 && (!x || !group))) return fail("ribca_group_sums: NULL buffer");
  if (n < 0 || n == INT32_MAX) return fail("ribca_group_sums: needs 0 <= n < 2^31 - 1");
  if (c < 1 || c > GS_C_MAX) return fail("ribca_group_sums: needs 1 <= c <= 1024");
  if (groups < 1 || groups > GS_GROUPS_MAX) return fail("ribca_group_sums: needs 1 <= groups <= 256");
  if (ws_bytes < ribca_group_sums_ws_bytes(n, c, groups)) return fail("ribca_group_sums: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Carver cv(ws);
  const GroupWs w = carve_group(cv, n, c, groups);
  const int chunks = chunks_of(n);
  if (chunks > 0)
    hipLaunchKernelGGL(group_chunk_kernel, dim3((unsigned)chunks, (unsigned)((c + GS_COLS - 1) / GS_COLS)), dim3(256), 0, s, x, group, n, c, groups, w.part,
                       w.ipart);
  launch_chunk_total(w.part, chunks, groups * c, sums, s);
  hipLaunchKernelGGL(group_count_kernel, dim3((unsigned)((groups + 256) / 256)), dim3(256), 0, s, w.ipart, chunks, groups, counts, w.skipped);
  RIBCA_FINISH();
  int64_t host = 0;
  HIP_TRY(hipMemcpyAsync(&host, w.skipped, sizeof(host), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *skipped = host;
  return 0;
}

int64_t ribca_heatmap_raster_ws_bytes(int32_t rows, int32_t cols, int32_t cell, int32_t gap) {
  if (!heatmap_args_ok(rows, cols, cell, gap)) return 0;
  Carver cv(nullptr);
  cv.take<double>(2);
  return (int64_t)cv.off;
}

int ribca_heatmap_raster(const double* sums, const int64_t* counts, int32_t rows, int32_t cols, const uint8_t* lut, int32_t cell, int32_t gap, uint8_t* out,
                         double* vmin, double* vmax, void* ws, int64_t ws_bytes, void* stream) {
  if (!sums || !counts || !lut || !out || !vmin || !vmax || !ws) return fail("ribca_heatmap_raster: NULL buffer");
  if (rows < 1 || rows > GS_GROUPS_MAX || cols < 1 || cols > GS_C_MAX) return fail("ribca_heatmap_raster: needs 1 <= rows <= 256, 1 <= cols <= 1024");
  if (cell < 1 || cell > HM_CELL_MAX || gap < 0 || 2 * gap >= cell) return fail("ribca_heatmap_raster: needs 1 <= cell <= 64, 0 <= 2 gap < cell");
  if (ws_bytes < ribca_heatmap_raster_ws_bytes(rows, cols, cell, gap)) return fail("ribca_heatmap_raster: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Carver cv(ws);
  double* range = cv.take<double>(2);
  const long long pixels = (long long)rows * cell * cols * cell;
  hipLaunchKernelGGL(heatmap_range_kernel, dim3(1), dim3(256), 0, s, sums, counts, rows, cols, range);
  hipLaunchKernelGGL(heatmap_paint_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, sums, counts, rows, cols, lut, cell, gap, range, out);
  RIBCA_FINISH();
  double host[2] = {0.0, 0.0};
  HIP_TRY(hipMemcpyAsync(host, range, sizeof(host), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *vmin = host[0];
  *vmax = host[1];
  return 0;
}

int ribca_table_raster(const double* values, int32_t rows, int32_t cols, const uint8_t* lut, int32_t cell, int32_t gap, double vmin, double vmax,
                       uint8_t* out, void* stream) {
  if (!values || !lut || !out) return fail("ribca_table_raster: NULL buffer");
  if (rows < 1 || rows > GS_GROUPS_MAX || cols < 1 || cols > GS_C_MAX) return fail("ribca_table_raster: needs 1 <= rows <= 256, 1 <= cols <= 1024");
  if (cell < 1 || cell > HM_CELL_MAX || gap < 0 || 2 * gap >= cell) return fail("ribca_table_raster: needs 1 <= cell <= 64, 0 <= 2 gap < cell");
  if (!std::isfinite(vmin) || !std::isfinite(vmax) || vmin > vmax) return fail("ribca_table_raster: needs finite vmin <= vmax");
  const long long pixels = (long long)rows * cell * cols * cell;
  hipLaunchKernelGGL(table_paint_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, values, rows, cols, lut, cell, gap,
                     vmin, vmax, out);
  RIBCA_FINISH();
  return 0;
}

int ribca_pie_raster(const double* rays, int32_t m, const uint8_t* rgb, int32_t size, int32_t radius, uint8_t* out, void* stream) {
  if (!rgb || !out || (m > 0 && !rays)) return fail("ribca_pie_raster: NULL buffer");
  if (m < 0 || m > PIE_RAYS_MAX) return fail("ribca_pie_raster: needs 0 <= m <= 256");
  if (size < 1 || size > PIE_DIM_MAX) return fail("ribca_pie_raster: needs 1 <= size <= 16384");
  if (radius < 0 || radius > size) return fail("ribca_pie_raster: needs 0 <= radius <= size");
  const long long pixels = (long long)size * size;
  hipLaunchKernelGGL(pie_paint_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rays, m, rgb, size, radius, out);
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
