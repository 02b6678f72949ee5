// Scatter plot of 2-D points as filled discs (Annotator.umap_visualization; the reference draws it with one seaborn scatter call, model.py:746-765).
// Painter's order is data order: where discs overlap the point with the higher index shows.
//   scatter_mark   one thread per point: column = rint(x * ax + bx), row = rint(y * ay + by) in fp32, every operation rounded on its own; a point
//                  whose centre is not finite or not on the canvas is counted and skipped; every pixel offset (dx, dy) with |dx|, |dy| <= r
//                  and dx^2 + dy^2 <= r^2 + 1 that lies on the canvas gets atomicMax(point index + 1) in an int32 index image.
//   scatter_paint  one thread per pixel: the colour of point (index - 1), white where the index is 0.
// Integer atomics only: the bytes do not depend on the launch geometry.
#include <cmath>

#include "../../include/ribca_hip.h"
#include "ribca_common.h"
#include "ribca_scratch.h"
#include "ribca_status.h"

#pragma clang fp contract(off)

namespace ribca {
namespace {

constexpr int SC_RMAX = 16;
constexpr int SC_DIM_MAX = 16384;

int fail(const char* msg) { return api_fail(msg); }

// the workspace of ribca_scatter_raster; all of it is zeroed before the kernels run
struct ScatterWs {
  unsigned* count;      // points skipped
  int* index;           // (height, width): 1 + the highest point index that covers the pixel
};

ScatterWs carve_scatter(Carver& c, int height, int width) {
  ScatterWs w;
  w.count = c.take<unsigned>(1);
  w.index = c.take<int>((size_t)height * width);
  return w;
}

__global__ __launch_bounds__(256) void scatter_mark_kernel(const float* __restrict__ pts, int n, float ax, float bx, float ay, float by, int H, int W, int r,
                                                           int* __restrict__ index, unsigned* __restrict__ skipped) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int i = (int)t;
  const float fx = rintf(pts[2 * (size_t)i] * ax + bx);
  const float fy = rintf(pts[2 * (size_t)i + 1] * ay + by);
  if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) {      // false for NaN and either infinity too
    atomicAdd(skipped, 1u);
    return;
  }
  const int cx = (int)fx, cy = (int)fy;
  const int lim = r * r + 1;
  for (int dy = -r; dy <= r; ++dy) {
    const int py = cy + dy;
    if (py < 0 || py >= H) continue;
    for (int dx = -r; dx <= r; ++dx) {
      const int px = cx + dx;
      if (px < 0 || px >= W || dx * dx + dy * dy > lim) continue;
      atomicMax(&index[(size_t)py * W + px], i + 1);
    }
  }
}

__global__ __launch_bounds__(256) void scatter_paint_kernel(const int* __restrict__ index, long long pixels, const uint8_t* __restrict__ rgb, int n,
                                                            uint8_t* __restrict__ out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const int k = index[p];
  const bool hit = k >= 1 && k <= n;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * p + c] = hit ? rgb[3 * (size_t)(k - 1) + c] : (uint8_t)255;
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int64_t ribca_scatter_raster_ws_bytes(int32_t height, int32_t width) {
  if (height < 1 || height > SC_DIM_MAX || width < 1 || width > SC_DIM_MAX) return 0;
  Carver c(nullptr);
  carve_scatter(c, height, width);
  return (int64_t)c.off;
}

int ribca_scatter_raster(const float* points, const uint8_t* rgb, int32_t n, double ax, double bx, double ay, double by, int32_t height, int32_t width,
                         int32_t radius, uint8_t* out, int64_t* skipped, void* ws, int64_t ws_bytes, void* stream) {
  if (!out || !skipped || !ws || (n > 0 && (!points || !rgb))) return fail("ribca_scatter_raster: NULL buffer");
  if (n < 0 || n == INT32_MAX) return fail("ribca_scatter_raster: needs 0 <= n < 2^31 - 1");
  if (height < 1 || height > SC_DIM_MAX || width < 1 || width > SC_DIM_MAX) return fail("ribca_scatter_raster: needs 1 <= height, width <= 16384");
  if (radius < 0 || radius > SC_RMAX) return fail("ribca_scatter_raster: needs 0 <= radius <= 16");
  if (ws_bytes < ribca_scatter_raster_ws_bytes(height, width)) return fail("ribca_scatter_raster: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Carver c(ws);
  const ScatterWs w = carve_scatter(c, height, width);
  const long long pixels = (long long)height * width;
  HIP_TRY(hipMemsetAsync(ws, 0, c.off, s));
  if (n > 0)
    hipLaunchKernelGGL(scatter_mark_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, s, points, n, (float)ax, (float)bx, (float)ay, (float)by, height, width,
                       radius, w.index, w.count);
  hipLaunchKernelGGL(scatter_paint_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, w.index, pixels, rgb, n, out);
  RIBCA_FINISH();
  unsigned host = 0;
  HIP_TRY(hipMemcpyAsync(&host, w.count, sizeof(host), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *skipped = (int64_t)host;
  return 0;
}

}  // extern "C"
