// Per-cell marker intensities over the cell's own pixels (Annotator.cell_intensities; steinbock's `measure intensities`): for every cell and
// channel the fp64 sum and sum of squared deviations in a FIXED order (256 strided partials and a halving tree) and the order statistics that
// bracket the requested quantiles, found on the total-order key of the fp32 bit pattern.  include/ribca_hip.h states the contract,
// tests/intensities_numpy.py restates it.
// Two kernels, each launched over every cell; a cell belongs to the one its clipped box selects and the other returns at once:
//   cell_intensities_small   boxes of at most IN_SMALL_BOX pixels (the typical cell), ONE WAVE per cell: the offsets of the cell's pixels are
//                      compacted into LDS with ballots, per channel the values are gathered through them as keys, a lane holds the four partials
//                      lane, lane + 64, lane + 128, lane + 192 in registers (the tree needs no LDS), and the keys are sorted in LDS by a bitonic
//                      network padded to a power of two with the largest key, so that any number of ranks is a lookup.
//   cell_intensities   every larger box, one 256-thread workgroup per cell.  It walks the clipped box in chunks of 256 pixels in row-major order
//                      and compacts the offsets of the cell's pixels into LDS with a ballot scan (no atomics), which also counts the area.
//     resident form    area <= IN_RESIDENT: per channel the values are gathered through the offsets into LDS as keys; thread t adds the elements
//                      t, t + 256, ... (it IS partial t), the tree runs through LDS and one wave's shuffles.
//     streaming form   any larger label: the box is walked again per pass with the compaction rank carried across chunks, so that element j
//                      still reaches partial j mod 256 (through a 256-slot LDS stage).
//     selection        both of its forms: most-significant-digit radix select, four 8-bit passes, every requested rank at once.  A rank follows its own
//                      key prefix; ranks that share a prefix share one LDS histogram (that of the first of them), so an element costs one
//                      integer LDS add per DISTINCT prefix.  Integer counts only: the result does not depend on the order of the adds.
// No floating-point atomics, nothing indexed by a label or a pixel outside LDS, no loop that waits for another thread; every loop is bounded by
// the box or by IN_RESIDENT.  Measured form: DESIGN.md section 21.
#include <stdint.h>

#include "../../include/ribca_hip.h"
#include "ribca_cellbox.h"
#include "ribca_common.h"
#include "ribca_status.h"

#pragma clang fp contract(off)      // sum, mean and squared deviation round one operation at a time, as the restatement does

namespace ribca {
namespace {

constexpr int IN_THREADS = 256;               // threads of a workgroup = partials of the stated sum
constexpr int IN_RESIDENT = 4096;             // pixels of a cell whose offsets and values stay in LDS (ops.INTENSITY_RESIDENT)
constexpr int IN_SMALL_BOX = 1024;            // pixels of a clipped box that one wave takes (ops.INTENSITY_SMALL_BOX); a power of two
constexpr int IN_C_MAX = 64;
constexpr int IN_Q_MAX = 8;
constexpr int IN_RANKS = 2 * IN_Q_MAX;        // lo and hi of every quantile
constexpr int IN_N_MAX = 1 << 21;
constexpr int IN_HW_MAX = 65535;
constexpr uint32_t IN_NAN = 0x7FC00000u;      // order statistics of a cell without a pixel

static_assert(IN_THREADS == 256, "thread t holds partial t of the 256; the tree below is written for four waves");
static_assert(IN_RESIDENT % IN_THREADS == 0, "the compaction keeps whole chunks");
static_assert((IN_SMALL_BOX & (IN_SMALL_BOX - 1)) == 0 && IN_SMALL_BOX >= 64, "the bitonic network pads to a power of two within the LDS array");

int fail(const char* msg) { return api_fail(msg); }

struct Quantiles {
  int32_t num[IN_Q_MAX];
  int32_t Q, den;
};

// the total-order key: all bits of a negative flipped, the sign bit of the rest set
__device__ __forceinline__ uint32_t to_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint32_t key_bits(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

struct Shared {
  int32_t offs[IN_RESIDENT];             // pixel offsets r W + c of the cell, row-major order
  uint32_t keys[IN_RESIDENT];            // one channel's values as keys, same order
  uint32_t hist[IN_RANKS][256];
  double red[IN_THREADS];
  float stage[IN_THREADS];               // streaming sums: the chunk's values at (rank mod 256)
  int wave_tot[2][4];
  uint32_t prefix[IN_RANKS];             // the key bits fixed so far, per requested rank
  uint32_t rank[IN_RANKS];               // the rank among the elements that share the prefix
  int lead[IN_RANKS];                    // the first rank with the same prefix: its histogram is the one in use
  long long want[IN_RANKS];              // the ranks of the cell, the same for every channel
  double result;
};
static_assert(sizeof(Shared) <= 64 * 1024, "LDS of cell_intensities");

// the chunk's ballot scan of ribca_cellbox.h on this kernel's LDS
__device__ __forceinline__ int chunk_rank(Shared& sh, bool flag, int parity, int& m) { return ribca::chunk_rank(sh.wave_tot, flag, parity, m); }

// the stated tree over the 256 partials: s = 128, 64 through LDS, s = 32 .. 1 in wave 0; every thread returns p_0
__device__ __forceinline__ double tree(Shared& sh, double p) {
  const int t = threadIdx.x;
  sh.red[t] = p;
  __syncthreads();
  if (t < 64) {
    double x = (sh.red[t] + sh.red[t + 128]) + (sh.red[t + 64] + sh.red[t + 192]);
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_down(x, s);      // lanes >= s hold values nobody reads
    if (t == 0) sh.result = x;
  }
  __syncthreads();
  return sh.result;
}

// rank r of the two that bracket quantile k of a cell of a pixels (slot = 2 k for lo, 2 k + 1 for hi)
__device__ __forceinline__ long long wanted_rank(const Quantiles& q, int slot, unsigned a) {
  const long long h = (long long)(a - 1) * q.num[slot >> 1];
  return h / q.den + ((slot & 1) && h % q.den != 0 ? 1 : 0);
}

// Radix select of R ranks at once over the keys `each(f)` hands to f (every thread hands over its share; no barrier inside `each`).
// Leaves the selected keys in sh.prefix[0 .. R).
template <typename Each>
__device__ __forceinline__ void select(Shared& sh, int R, Each each) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t fixed = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);      // the bits the earlier passes fixed
    if (t < R) {
      if (pass == 0) sh.prefix[t] = 0u, sh.rank[t] = (uint32_t)sh.want[t], sh.lead[t] = 0;
      else {
        int first = t;
        for (int k = t - 1; k >= 0; --k) first = sh.prefix[k] == sh.prefix[t] ? k : first;
        sh.lead[t] = first;
      }
    }
    for (int e = t; e < R * 256; e += IN_THREADS) (&sh.hist[0][0])[e] = 0u;
    __syncthreads();
    each([&](uint32_t key) {
      for (int k = 0; k < R; ++k)
        if (sh.lead[k] == k && ((key ^ sh.prefix[k]) & fixed) == 0u) atomicAdd(&sh.hist[k][(key >> shift) & 255u], 1u);
    });
    __syncthreads();
    for (int k = wave; k < R; k += 4) {      // a wave per rank: the bin that holds it
      const uint32_t* h = sh.hist[sh.lead[k]];
      const uint32_t c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
      const uint32_t own = c0 + c1 + c2 + c3;
      uint32_t incl = own;
      for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s);
        if (lane >= s) incl += up;
      }
      const uint32_t r = sh.rank[k], below = incl - own;
      if (below <= r && r < incl) {      // exactly one lane: the rank lies among the elements of the prefix
        uint32_t bin = 4 * lane, skipped = below;
        if (r >= skipped + c0) {
          skipped += c0, bin += 1;
          if (r >= skipped + c1) {
            skipped += c1, bin += 1;
            if (r >= skipped + c2) skipped += c2, bin += 1;
          }
        }
        sh.prefix[k] |= bin << shift;
        sh.rank[k] = r - skipped;
      }
    }
    __syncthreads();
  }
}

struct SmallShared {
  int32_t offs[IN_SMALL_BOX];
  uint32_t keys[IN_SMALL_BOX];
};

// one wave per cell; the barriers are those of a one-wave workgroup: they order its LDS writes before the reads of other lanes
__global__ __launch_bounds__(64) void cell_intensities_small_kernel(const float* __restrict__ image, int C, int H, int W,
                                                                   const int32_t* __restrict__ mask, const int32_t* __restrict__ ids,
                                                                   const int32_t* __restrict__ bbox, Quantiles q, int32_t* __restrict__ area,
                                                                   double* __restrict__ sums, uint32_t* __restrict__ order) {
  __shared__ SmallShared sh;
  const int lane = threadIdx.x;
  const size_t cell = blockIdx.x;
  const int32_t id = ids[cell];
  const int R = 2 * q.Q;
  const size_t HW = (size_t)H * W;
  const Box box = clipped_box(bbox + cell * 4, id, H, W);
  if (box.total > (unsigned)IN_SMALL_BOX) return;      // cell_intensities'
  unsigned a = 0;
  for (unsigned base = 0; base < box.total; base += 64) {
    const unsigned e = base + lane;
    bool in = false;
    int off = 0;
    if (e < box.total) {
      off = (box.r0 + (int)(e / (unsigned)box.bw)) * W + box.c0 + (int)(e % (unsigned)box.bw);
      in = mask[off] == id;
    }
    const unsigned long long b = __ballot(in);
    if (in) sh.offs[a + __popcll(b & ((1ull << lane) - 1ull))] = off;      // a + rank < box.total <= IN_SMALL_BOX
    a += (unsigned)__popcll(b);
  }
  if (lane == 0) area[cell] = (int32_t)a;
  double* __restrict__ out_sums = sums + cell * C * 2;
  uint32_t* __restrict__ out_order = order + cell * C * R;
  if (a == 0) {
    for (int e = lane; e < C * 2; e += 64) out_sums[e] = 0.0;
    for (int e = lane; e < C * R; e += 64) out_order[e] = IN_NAN;
    return;
  }
  unsigned padded = 1;      // the first power of two >= a, <= IN_SMALL_BOX
  while (padded < a) padded <<= 1;
  const unsigned want = lane < R ? (unsigned)wanted_rank(q, lane, a) : 0u;
  const double count = (double)a;
  __syncthreads();      // offs is written
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ plane = image + (size_t)c * HW;
    double p[4] = {0.0, 0.0, 0.0, 0.0};      // the partials lane + 64 u
    for (unsigned base = 0; base < a; base += 256) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned j = base + 64 * u + lane;
        if (j < a) {
          const float v = plane[sh.offs[j]];
          sh.keys[j] = to_key(v);
          p[u] += (double)v;
        }
      }
    }
    for (unsigned j = a + lane; j < padded; j += 64) sh.keys[j] = 0xFFFFFFFFu;      // no key is larger: the first a sorted keys are the cell's
    double x = (p[0] + p[2]) + (p[1] + p[3]);      // s = 128, then s = 64
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_down(x, s);
    const double sum = __shfl(x, 0);
    const double mean = sum / count;
    p[0] = p[1] = p[2] = p[3] = 0.0;
    for (unsigned base = 0; base < a; base += 256) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned j = base + 64 * u + lane;
        if (j < a) {
          const double d = (double)__uint_as_float(key_bits(sh.keys[j])) - mean;      // this lane wrote keys[j]
          p[u] += d * d;
        }
      }
    }
    x = (p[0] + p[2]) + (p[1] + p[3]);
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_down(x, s);
    if (lane == 0) out_sums[2 * c] = sum, out_sums[2 * c + 1] = x;
    __syncthreads();
    for (unsigned k = 2; k <= padded; k <<= 1) {
      for (unsigned j = k >> 1; j > 0; j >>= 1) {
        for (unsigned t = lane; t < padded / 2; t += 64) {
          const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), partner = i | j;      // bit j of i is clear
          const uint32_t lo = sh.keys[i], hi = sh.keys[partner];
          if ((lo > hi) == ((i & k) == 0)) sh.keys[i] = hi, sh.keys[partner] = lo;
        }
        __syncthreads();
      }
    }
    if (lane < R) out_order[c * R + lane] = key_bits(sh.keys[want]);
    __syncthreads();      // the next channel overwrites keys
  }
}

__global__ __launch_bounds__(IN_THREADS) void cell_intensities_kernel(const float* __restrict__ image, int C, int H, int W,
                                                                      const int32_t* __restrict__ mask, const int32_t* __restrict__ ids,
                                                                      const int32_t* __restrict__ bbox, Quantiles q, int32_t* __restrict__ area,
                                                                      double* __restrict__ sums, uint32_t* __restrict__ order) {
  __shared__ Shared sh;
  const int t = threadIdx.x;
  const size_t cell = blockIdx.x;
  const int32_t id = ids[cell];
  const int R = 2 * q.Q;
  const size_t HW = (size_t)H * W;
  const Box box = clipped_box(bbox + cell * 4, id, H, W);
  if (box.total <= (unsigned)IN_SMALL_BOX) return;      // cell_intensities_small's

  // the area, and the first IN_RESIDENT offsets
  unsigned a = 0;
  int parity = 0;
  for (unsigned base = 0; base < box.total; base += IN_THREADS, parity ^= 1) {
    const unsigned e = base + t;
    bool in = false;
    int off = 0;
    if (e < box.total) {
      off = (box.r0 + (int)(e / (unsigned)box.bw)) * W + box.c0 + (int)(e % (unsigned)box.bw);
      in = mask[off] == id;
    }
    int m;
    const unsigned at = a + (unsigned)chunk_rank(sh, in, parity, m);
    if (in && at < (unsigned)IN_RESIDENT) sh.offs[at] = off;
    a += (unsigned)m;
  }
  if (t == 0) area[cell] = (int32_t)a;
  double* __restrict__ out_sums = sums + cell * C * 2;
  uint32_t* __restrict__ out_order = order + cell * C * R;
  if (a == 0) {
    for (int e = t; e < C * 2; e += IN_THREADS) out_sums[e] = 0.0;
    for (int e = t; e < C * R; e += IN_THREADS) out_order[e] = IN_NAN;
    return;
  }
  if (t < R) sh.want[t] = wanted_rank(q, t, a);
  __syncthreads();      // offs and want are written
  const double count = (double)a;

  if (a <= (unsigned)IN_RESIDENT) {
    for (int c = 0; c < C; ++c) {
      const float* __restrict__ plane = image + (size_t)c * HW;
      double p = 0.0;
      for (unsigned j = t; j < a; j += IN_THREADS) {
        const float v = plane[sh.offs[j]];
        sh.keys[j] = to_key(v);
        p += (double)v;
      }
      const double sum = tree(sh, p);      // its barriers also publish keys
      const double mean = sum / count;
      p = 0.0;
      for (unsigned j = t; j < a; j += IN_THREADS) {
        const double d = (double)__uint_as_float(key_bits(sh.keys[j])) - mean;
        p += d * d;
      }
      const double ssd = tree(sh, p);
      if (t == 0) out_sums[2 * c] = sum, out_sums[2 * c + 1] = ssd;
      select(sh, R, [&](auto f) {
        for (unsigned j = t; j < a; j += IN_THREADS) f(sh.keys[j]);
      });
      if (t < R) out_order[c * R + t] = key_bits(sh.prefix[t]);
    }
    return;
  }

  // streaming form: element j of the cell goes to partial j mod 256 through sh.stage; `second` adds squared deviations from `mean`
  auto stream_sum = [&](const float* __restrict__ plane, bool second, double mean) {
    double p = 0.0;
    unsigned seen = 0;
    int par = 0;
    for (unsigned base = 0; base < box.total; base += IN_THREADS, par ^= 1) {
      const unsigned e = base + t;
      bool in = false;
      float v = 0.f;
      if (e < box.total) {
        const int off = (box.r0 + (int)(e / (unsigned)box.bw)) * W + box.c0 + (int)(e % (unsigned)box.bw);
        in = mask[off] == id;
        if (in) v = plane[off];
      }
      int m;
      const unsigned at = seen + (unsigned)chunk_rank(sh, in, par, m);
      if (in) sh.stage[at & 255u] = v;
      __syncthreads();
      if (((unsigned)t - seen & 255u) < (unsigned)m) {      // slot t was written in this chunk: the ranks seen .. seen + m - 1, m <= 256
        const double x = (double)sh.stage[t];
        if (second) {
          const double d = x - mean;
          p += d * d;
        } else {
          p += x;
        }
      }
      seen += (unsigned)m;
      // the next write of stage comes behind the barrier of the next chunk_rank
    }
    return tree(sh, p);
  };
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ plane = image + (size_t)c * HW;
    const double sum = stream_sum(plane, false, 0.0);
    const double ssd = stream_sum(plane, true, sum / count);
    if (t == 0) out_sums[2 * c] = sum, out_sums[2 * c + 1] = ssd;
    select(sh, R, [&](auto f) {
      for (unsigned base = 0; base < box.total; base += IN_THREADS) {
        const unsigned e = base + t;
        if (e < box.total) {
          const int off = (box.r0 + (int)(e / (unsigned)box.bw)) * W + box.c0 + (int)(e % (unsigned)box.bw);
          if (mask[off] == id) f(to_key(plane[off]));
        }
      }
    });
    if (t < R) out_order[c * R + t] = key_bits(sh.prefix[t]);
  }
}

}  // namespace
}  // namespace ribca

using namespace ribca;

extern "C" {

int ribca_cell_intensities(const float* image, int32_t C, int32_t H, int32_t W, const int32_t* mask, const int32_t* ids, const int32_t* bbox,
                           int32_t n, const int32_t* q_num, int32_t Q, int32_t q_den, int32_t* area, double* sums, float* order, void* stream) {
  if (n == 0) return 0;
  if (!image || !mask || !ids || !bbox || !q_num || !area || !sums || !order) return fail("ribca_cell_intensities: NULL buffer");
  if (C < 1 || C > IN_C_MAX) return fail("ribca_cell_intensities: needs 1 <= C <= 64");
  if (H < 1 || W < 1 || H > IN_HW_MAX || W > IN_HW_MAX || (long long)H * W >= (1ll << 31))
    return fail("ribca_cell_intensities: needs 1 <= H, W <= 65535 and H W < 2^31");
  if (n < 1 || n > IN_N_MAX) return fail("ribca_cell_intensities: needs 1 <= n <= 2^21");
  if (Q < 1 || Q > IN_Q_MAX) return fail("ribca_cell_intensities: needs 1 <= Q <= 8");
  if (q_den < 1) return fail("ribca_cell_intensities: needs 1 <= q_den");
  Quantiles q;
  q.Q = Q, q.den = q_den;
  for (int k = 0; k < IN_Q_MAX; ++k) {
    q.num[k] = k < Q ? q_num[k] : 0;      // q_num is a HOST array
    if (q.num[k] < 0 || q.num[k] > q_den) return fail("ribca_cell_intensities: needs 0 <= q_num[k] <= q_den");
  }
  hipLaunchKernelGGL(cell_intensities_small_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, image, C, H, W, mask, ids, bbox, q, area, sums,
                     reinterpret_cast<uint32_t*>(order));
  hipLaunchKernelGGL(cell_intensities_kernel, dim3((unsigned)n), dim3(IN_THREADS), 0, (hipStream_t)stream, image, C, H, W, mask, ids, bbox, q, area,
                     sums, reinterpret_cast<uint32_t*>(order));
  RIBCA_FINISH();
  return 0;
}

}  // extern "C"
