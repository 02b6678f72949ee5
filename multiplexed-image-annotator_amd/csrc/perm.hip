// The two shuffle kernels of the permutation nulls and the refusal their entry points share (ribca_perm.h declares them and states sigma).
//   perm_labels  one thread per (cell, permutation of the batch): row j of the workspace = the n shuffled labels as bytes.  A row of 1e5 cells is
//                100 KB and stays in L2 for the gathers that follow; evaluating sigma for every neighbour or edge end instead of once per cell would
//                cost that many times the hashing.
//   perm_rows    one workgroup per (chunk of kCellChunk cells, permutation of the batch): a thread per cell walks sigma, then the workgroup copies
//                the chunk's rows -- one random row read per cell, coalesced writes -- into rows of ld >= C doubles that never straddle a 128-byte
//                line (row_ld).  With the inverse beside them "sigma(j) == i" is "j == inv[i]" for the reader: a scatter of one int32 per cell.
#include <stdio.h>

#include "ribca_perm.h"
#include "ribca_status.h"

namespace ribca {
namespace {

// grid (ceil(n / 256), batch)
__global__ __launch_bounds__(256) void perm_labels_kernel(const int32_t* __restrict__ cell_type, int n, int T, int h, uint64_t image_key, uint64_t p0,
                                                          uint8_t* __restrict__ labels) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t src = perm_sigma(image_key, p0 + blockIdx.y, (uint32_t)i, (uint32_t)n, h);
  uint8_t lab = kPermSkip;
  if (src < (uint32_t)n) {
    const int32_t t = cell_type[src];
    if ((unsigned)t < (unsigned)T) lab = (uint8_t)t;
  }
  labels[(size_t)blockIdx.y * n + i] = lab;
}

// grid (chunks, batch); INV: the inverse is written as well (a walk that reported no cell -- it cannot -- writes no word of it)
template <bool INV>
__global__ __launch_bounds__(256) void perm_rows_kernel(const double* __restrict__ z, int n, int C, int ld, int h, uint64_t image_key, uint64_t p0,
                                                        double* __restrict__ zp, int32_t* __restrict__ inv) {
  __shared__ uint32_t src[kCellChunk];
  const int first = blockIdx.x * kCellChunk;
  const int cells = min(kCellChunk, n - first);
  if ((int)threadIdx.x < cells) {
    const uint32_t s = perm_sigma(image_key, p0 + blockIdx.y, (uint32_t)(first + threadIdx.x), (uint32_t)n, h);
    src[threadIdx.x] = s;
    if constexpr (INV)
      if (s < (uint32_t)n) inv[(size_t)blockIdx.y * n + s] = first + (int)threadIdx.x;
  }
  __syncthreads();
  double* __restrict__ out = zp + ((size_t)blockIdx.y * n + first) * ld;
  for (int e = threadIdx.x; e < cells * C; e += 256) {
    const int cell = e / C, c = e % C;
    const uint32_t s = src[cell];
    out[cell * ld + c] = s < (uint32_t)n ? z[(size_t)s * C + c] : 0.0;
  }
}

static_assert(kCellChunk == 256, "perm_rows: one thread per cell of the chunk");

}  // namespace

void launch_perm_labels(const int32_t* cell_type, int n, int T, int h, uint64_t image_key, uint64_t p0, int batch, uint8_t* labels, hipStream_t s) {
  hipLaunchKernelGGL(perm_labels_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, s, cell_type, n, T, h, image_key, p0, labels);
}

void launch_perm_rows(const double* z, int n, int C, int ld, int h, uint64_t image_key, uint64_t p0, int batch, double* zp, int32_t* inv,
                      hipStream_t s) {
  const dim3 grid((unsigned)chunks_of_cells(n), (unsigned)batch);
  if (inv)
    hipLaunchKernelGGL(perm_rows_kernel<true>, grid, dim3(256), 0, s, z, n, C, ld, h, image_key, p0, zp, inv);
  else
    hipLaunchKernelGGL(perm_rows_kernel<false>, grid, dim3(256), 0, s, z, n, C, ld, h, image_key, p0, zp, inv);
}

int perm_range_check(const char* who, int32_t image, int64_t p0, int32_t P) {
  if (image >= 0 && p0 >= 0 && P >= 1 && p0 + (int64_t)P <= (1ll << 31)) return 0;
  char msg[128];
  snprintf(msg, sizeof msg, "%s: needs image >= 0, p0 >= 0, 1 <= P, p0 + P <= 2^31", who);
  return api_fail(msg);      // copies its argument
}

}  // namespace ribca
