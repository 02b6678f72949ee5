// Caller-owned scratch, written once: how a workspace is laid out (Carver) and the second half of every fixed-order fp64 sum (chunk_total_kernel).
//
// A layout is ONE function over a Carver&.  Run on Carver(nullptr) it only measures (c.off = the bytes to ask for: what the *_ws_bytes query
// returns and what the entry point's "workspace too small" check compares with); run on Carver(ws) it hands out the pointers.  The two cannot
// disagree.  Every piece starts at a multiple of 256 bytes from the base.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ribca {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Carver {
  char* base; size_t off = 0;
  explicit Carver(void* b) : base(static_cast<char*>(b)) {}
  template <class T> T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = align256(off + count * sizeof(T));
    return p;
  }
};

// THE fixed summation order of regions.hip and spectral.hip (tests/regions_numpy.py and tests/spectral_numpy.py restate it with this chunk): the
// rows of every chunk of kSumChunk added in ascending order, started at 0; then the chunks added in ascending order, started at 0.
constexpr int kSumChunk = 1024;
inline int chunks_of(int n) { return (n + kSumChunk - 1) / kSumChunk; }

// the second half: out[o] = part[0 * width + o] + part[1 * width + o] + ... + part[(chunks - 1) * width + o], in that order, one thread per
// output.  Integer counts that were taken per chunk beside the sums ride along in the same launch: iout[o] = the sum over the chunks of
// ipart[ch * iwidth + o] for o < iwidth <= width (iwidth = 0: none).
static __global__ __launch_bounds__(256) void chunk_total_kernel(const double* __restrict__ part, int chunks, int width, double* __restrict__ out,
                                                                 const int32_t* __restrict__ ipart, int iwidth, int32_t* __restrict__ iout) {
#pragma clang fp contract(off)
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o < width) {
    double s = 0.0;
    for (int ch = 0; ch < chunks; ++ch) s = s + part[(size_t)ch * width + o];
    out[o] = s;
  }
  if (o < iwidth) {
    int c = 0;
    for (int ch = 0; ch < chunks; ++ch) c += ipart[(size_t)ch * iwidth + o];
    iout[o] = c;
  }
}

inline void launch_chunk_total(const double* part, int chunks, int width, double* out, hipStream_t s, const int32_t* ipart = nullptr, int iwidth = 0,
                               int32_t* iout = nullptr) {
  hipLaunchKernelGGL(chunk_total_kernel, dim3((width + 255) / 256), dim3(256), 0, s, part, chunks, width, out, ipart, iwidth, iout);
}

}  // namespace ribca
