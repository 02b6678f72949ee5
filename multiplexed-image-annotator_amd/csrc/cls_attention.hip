// Attention of the CLS query alone, without the K / V product (the last block of a classifier: only token 0 reaches the head).
//
// Per cell, with y_j = (z_j - mean_j) rstd_j the normalised rows (norm1 without gamma / beta), W' = gamma o W_qkv and b' = b + W_qkv beta
// the folded weight and bias, S_h the hd output rows of head h:
//     q_h    = W'_q[S_h,:] y_0 + b'_q[S_h]
//     g_h    = scale * sum_{n in S_h} q_h[n] W'_k[n,:]                 D values
//     p_hj   = softmax_j(g_h . y_j)              (q_h . b_k and (W_k^T q_h) . beta are constant over the keys: they cancel)
//     ybar_h = sum_j p_hj y_j                                          D values
//     o[S_h] = W'_v[S_h,:] ybar_h + b'_v[S_h]    (sum_j p_hj = 1)
// which is exact in real arithmetic (tests/test_cls_attention_algebra.py) and costs 6 D^2 + 48 T D FLOP per cell where K and V for every
// token cost 4 T D^2.  Three launches:
//     cls_qg_kernel    (head, tile of 16 cells): q_h and g_h; every weight is fetched once per tile
//     cls_ybar_kernel  one cell per workgroup: the cell's 101 rows are streamed twice (scores; weighted sum), g and the scores sit in LDS
//     cls_out_kernel   (head, tile of 16 cells): o, written packed-split into row 0 of the cell
// Everything is fp32 on the vector ALU over the stored 22-bit operands (hi + lo is exact in fp32); the D-long dot products add eight
// products in fp32 and the groups of eight in fp64.  No atomics; every sum has a fixed order that depends on nothing but the width, so a
// cell's bits do not depend on its place in the tile, the chunk or the launch.  Only token rows 0 .. T - 1 and columns 0 .. D - 1 are read
// or written.
#include <type_traits>

#include "ribca_common.h"
#include "ribca_kernels.h"

namespace ribca {
namespace {

constexpr int kCT = 16;           // cells per tile of the two head kernels
constexpr int kThreads = 256;
constexpr float kLog2e = 1.44269504088896340736f;

// logical columns k .. k + 3 (k % 4 == 0) of a packed-split row as fp32
__device__ __forceinline__ void ps_load4(const uint16_t* row, int k, float v[4]) {
  const uint16_t* p = row + ps_off(k);
  const uint2 hi = *reinterpret_cast<const uint2*>(p);
  const uint2 lo = *reinterpret_cast<const uint2*>(p + 8);
  v[0] = f16lo_plus_f16lo(hi.x, lo.x);
  v[1] = f16hi_plus_f16hi(hi.x, lo.x);
  v[2] = f16lo_plus_f16lo(hi.y, lo.y);
  v[3] = f16hi_plus_f16hi(hi.y, lo.y);
}
// the same columns of a residual row, normalised: (z - mean) rstd
__device__ __forceinline__ void y_load4(const uint16_t* row, int k, float2 st, float y[4]) {
  ps_load4(row, k, y);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = (y[i] - st.y) * st.x;
}
// one PS group: logical columns k .. k + 7 (k % 8 == 0)
__device__ __forceinline__ void ps_load8(const uint16_t* row, int k, float v[8]) {
  const uint16_t* p = row + 2 * k;
  const u32x4 hi = *reinterpret_cast<const u32x4*>(p);
  const u32x4 lo = *reinterpret_cast<const u32x4*>(p + 8);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = f16lo_plus_f16lo(hi[i], lo[i]);
    v[2 * i + 1] = f16hi_plus_f16hi(hi[i], lo[i]);
  }
}

// acc[i] = W[ng + 16 i][0 .. D) . vec[c][0 .. D) for the thread's cell c and its output rows ng + 16 i < HD.  vec: LDS, kCT rows of D + 4.
// All rows of the thread advance together through k, unrolled, so that several weight loads are in flight (the weights come from L2).
template <int D, int HD>
__device__ __forceinline__ void head_rows_dot(const uint16_t* W, int ldw, const float* vec, int c, int ng, double acc[(HD + 15) / 16]) {
  constexpr int NI = (HD + 15) / 16, UNR = NI >= 3 ? 2 : 4;
  const float* v = vec + c * (D + 4);
  const uint16_t* wr[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    acc[i] = 0.0;
    wr[i] = W + (size_t)(ng + 16 * i < HD ? ng + 16 * i : 0) * ldw;      // (a thread without row i reads row 0 and drops the sum)
  }
#pragma unroll UNR
  for (int k = 0; k < D; k += 8) {
    const float4 a0 = *reinterpret_cast<const float4*>(v + k), a1 = *reinterpret_cast<const float4*>(v + k + 4);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      float w[8];
      ps_load8(wr[i], k, w);
      float s = w[0] * a0.x;
      s = __builtin_fmaf(w[1], a0.y, s);
      s = __builtin_fmaf(w[2], a0.z, s);
      s = __builtin_fmaf(w[3], a0.w, s);
      s = __builtin_fmaf(w[4], a1.x, s);
      s = __builtin_fmaf(w[5], a1.y, s);
      s = __builtin_fmaf(w[6], a1.z, s);
      s = __builtin_fmaf(w[7], a1.w, s);
      acc[i] += (double)s;
    }
  }
}

// row subsets / cell subsets a workgroup of kThreads splits into beside the D / 4 column groups
__host__ __device__ constexpr int col_groups(int D) { return D / 4; }
__host__ __device__ constexpr int cell_split(int D) { return kThreads / col_groups(D) >= 4 ? 4 : kThreads / col_groups(D) >= 2 ? 2 : 1; }
__host__ __device__ constexpr int row_split(int D) { return kThreads / col_groups(D) >= 4 ? 4 : kThreads / col_groups(D); }

// ---- q_h and g_h for (head, cell tile) = blockIdx.x % 12, blockIdx.x / 12.  g: fp32 [cells][12][D]
template <int D>
__global__ __launch_bounds__(kThreads) void cls_qg_kernel(const uint16_t* __restrict__ z, int ldz, const uint16_t* __restrict__ W, int ldw,
                                                          const float* __restrict__ bias2, const float2* __restrict__ rowstat, int cells, float scale,
                                                          float* __restrict__ g) {
  constexpr int HD = D / kHeads, NKG = col_groups(D), S = cell_split(D), CPT = kCT / S, NI = (HD + 15) / 16;
  __shared__ __attribute__((aligned(16))) float ys[kCT * (D + 4)];
  __shared__ float qs[kCT * HD];
  const int h = blockIdx.x % kHeads, c0 = (blockIdx.x / kHeads) * kCT, t = threadIdx.x;
  // y_0 of the tile's cells (zeros behind the last cell)
  for (int idx = t; idx < kCT * NKG; idx += kThreads) {
    const int c = idx / NKG, kg = idx % NKG;
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    if (c0 + c < cells) {
      const size_t row = (size_t)(c0 + c) * kTokens;
      y_load4(z + row * ldz, 4 * kg, rowstat[row], y);
    }
    *reinterpret_cast<float4*>(ys + c * (D + 4) + 4 * kg) = make_float4(y[0], y[1], y[2], y[3]);
  }
  __syncthreads();
  {
    const int c = t % kCT, ng = t / kCT;
    double acc[NI];
    head_rows_dot<D, HD>(W + (size_t)(h * HD) * ldw, ldw, ys, c, ng, acc);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = ng + 16 * i;
      if (n < HD) qs[c * HD + n] = (float)(acc[i] + (double)bias2[h * HD + n]);
    }
  }
  __syncthreads();
  if (t < NKG * S) {
    const int kg = t % NKG, cs = t / NKG;
    float acc[CPT][4];
#pragma unroll
    for (int i = 0; i < CPT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f;
    const uint16_t* wk = W + (size_t)(D + h * HD) * ldw;
#pragma unroll 4
    for (int n = 0; n < HD; ++n) {
      float w[4];
      ps_load4(wk + (size_t)n * ldw, 4 * kg, w);
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const float qv = qs[(cs * CPT + i) * HD + n];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = __builtin_fmaf(qv, w[e], acc[i][e]);
      }
    }
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int cell = c0 + cs * CPT + i;
      if (cell < cells)
        *reinterpret_cast<float4*>(g + ((size_t)cell * kHeads + h) * D + 4 * kg) =
            make_float4(acc[i][0] * scale, acc[i][1] * scale, acc[i][2] * scale, acc[i][3] * scale);
    }
  }
}

// the raw halves of logical columns k .. k + 3 of a packed-split row: loaded early, decoded late (the row loads of the per-cell kernel are
// kept several rows ahead of the arithmetic)
struct Raw4 { uint2 hi, lo; };
__device__ __forceinline__ Raw4 raw_load4(const uint16_t* row, int k) {
  const uint16_t* p = row + ps_off(k);
  return Raw4{*reinterpret_cast<const uint2*>(p), *reinterpret_cast<const uint2*>(p + 8)};
}
__device__ __forceinline__ void y_from_raw(const Raw4& r, float2 st, float y[4]) {
  y[0] = (f16lo_plus_f16lo(r.hi.x, r.lo.x) - st.y) * st.x;
  y[1] = (f16hi_plus_f16hi(r.hi.x, r.lo.x) - st.y) * st.x;
  y[2] = (f16lo_plus_f16lo(r.hi.y, r.lo.y) - st.y) * st.x;
  y[3] = (f16hi_plus_f16hi(r.hi.y, r.lo.y) - st.y) * st.x;
}

template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// sixteen per-lane partial sums (index = head) -> lane l holds the wave's sum of index (l >> 2) & 15.  Each step halves the values a lane
// carries (the upper lane of a pair keeps the upper half); the order of the additions is fixed.  No step goes through the LDS unit's
// bpermute: the 32- and 16-lane exchanges are v_permlane{32,16}_swap (upper half / odd rows of the first operand against lower half / even
// rows of the second: the sum of the two results is the pair sum of the first operand in the lower lanes, of the second in the upper ones),
// the rest DPP and one swizzle.  (The swaps as inline asm, as in gemm_epi.h g4_sum: hipcc folds the two results of the swap builtins into
// one and the ISA then adds a register to itself.  s_nop: the swaps read VALU results of the instruction just before.)
__device__ __forceinline__ float wave_sum16(float v[16], int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float a = v[i], b = v[i + 8];
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    v[i] = a + b;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a = v[i], b = v[i + 4];
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    v[i] = a + b;
  }
  {
    const bool up = (lane & 8) != 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float keep = up ? v[i + 2] : v[i], send = up ? v[i] : v[i + 2];
      v[i] = keep + dpp_move<0x128>(send);      // row_ror:8 = lane ^ 8 inside a row of 16
    }
  }
  {
    const bool up = (lane & 4) != 0;
    const float keep = up ? v[1] : v[0], send = up ? v[0] : v[1];
    v[0] = keep + __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, send), 0x101F));      // lane ^ 4
  }
  float r = v[0];
  r += dpp_move<0x4E>(r);      // quad_perm [2, 3, 0, 1] = lane ^ 2
  r += dpp_move<0xB1>(r);      // quad_perm [1, 0, 3, 2] = lane ^ 1
  return r;
}

// ---- scores, softmax over the keys and ybar for cell blockIdx.x.  g, yb: fp32 [cells][12][D]
// A launch has few workgroups per CU (a chunk of 1024 cells: four), so a workgroup's own chain of load -> use decides the time: in both
// passes over the rows every thread keeps the loads of PF rows in flight ahead of the row it computes on.
template <int D>
__global__ __launch_bounds__(kThreads) void cls_ybar_kernel(const uint16_t* __restrict__ z, int ldz, const float2* __restrict__ rowstat,
                                                            const float* __restrict__ g, float* __restrict__ yb) {
  constexpr int NKG = col_groups(D), S = row_split(D), NIT = (NKG + 63) / 64, HDv = kHeads * D, NW = kThreads / 64, PF = 4;
  constexpr int BUF = (S - 1) * HDv > HDv ? (S - 1) * HDv : HDv;
  __shared__ __attribute__((aligned(16))) float gs[BUF];                 // g; afterwards the sums of the row subsets 1 .. S - 1
  __shared__ __attribute__((aligned(16))) float sc[kTokens * kHeads];    // [key][head]: scores, then probabilities
  __shared__ float2 st[kTokens];
  const int cell = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint16_t* zc = z + (size_t)cell * kTokens * ldz;
  // scores: one wave per key (keys wave, wave + NW, ...), a lane's column groups kg = lane + 64 it
  Raw4 ring[PF][NIT];
  auto load_row = [&](int j, Raw4 r[NIT]) {
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if (lane + 64 * it < NKG) r[it] = raw_load4(zc + (size_t)j * ldz, 4 * (lane + 64 * it));
  };
#pragma unroll
  for (int u = 0; u < PF; ++u) load_row(wave + NW * u, ring[u]);      // (PF * NW <= kTokens)
  for (int i = t; i < HDv / 4; i += kThreads)
    reinterpret_cast<float4*>(gs)[i] = reinterpret_cast<const float4*>(g + (size_t)cell * HDv)[i];
  for (int j = t; j < kTokens; j += kThreads) st[j] = rowstat[(size_t)cell * kTokens + j];
  __syncthreads();
  for (int base = 0; base * NW < kTokens; base += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int j = wave + NW * (base + u);
      if (j < kTokens) {
        Raw4 cur[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) cur[it] = ring[u][it];
        if (j + NW * PF < kTokens) load_row(j + NW * PF, ring[u]);
        float part[16];
#pragma unroll
        for (int h = 0; h < 16; ++h) part[h] = 0.f;
        const float2 sj = st[j];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int kg = lane + 64 * it;
          if (kg < NKG) {
            float y[4];
            y_from_raw(cur[it], sj, y);
#pragma unroll
            for (int h = 0; h < kHeads; ++h) {
              const float4 g4 = *reinterpret_cast<const float4*>(gs + h * D + 4 * kg);
              float s = y[0] * g4.x;
              s = __builtin_fmaf(y[1], g4.y, s);
              s = __builtin_fmaf(y[2], g4.z, s);
              s = __builtin_fmaf(y[3], g4.w, s);
              part[h] += s;
            }
          }
        }
        const float s = wave_sum16(part, lane);
        const int h = (lane >> 2) & 15;
        if ((lane & 3) == 0 && h < kHeads) sc[j * kHeads + h] = s;
      }
    }
  }
  // ybar: thread = (column group, row subset); keys sub, sub + S, ...; the first rows are requested before the softmax
  const int kg = t % NKG, sub = t / NKG;
  Raw4 rb[PF];
  if (sub < S) {
#pragma unroll
    for (int u = 0; u < PF; ++u) rb[u] = raw_load4(zc + (size_t)(sub + S * u) * ldz, 4 * kg);      // (PF * S <= kTokens)
  }
  __syncthreads();
  // softmax over the keys, one wave per head: max, exp2, one reciprocal
  for (int h = wave; h < kHeads; h += NW) {
    const int j0 = lane, j1 = lane + 64;
    const float s0 = sc[j0 * kHeads + h], s1 = j1 < kTokens ? sc[j1 * kHeads + h] : -__builtin_inff();
    const float m = wave_max(fmaxf(s0, s1));
    const float e0 = __builtin_amdgcn_exp2f((s0 - m) * kLog2e), e1 = j1 < kTokens ? __builtin_amdgcn_exp2f((s1 - m) * kLog2e) : 0.f;
    const float inv = 1.0f / wave_sum(e0 + e1);
    sc[j0 * kHeads + h] = e0 * inv;
    if (j1 < kTokens) sc[j1 * kHeads + h] = e1 * inv;
  }
  __syncthreads();      // (also: every wave is done with g -- gs is free)
  float acc[kHeads][4];
#pragma unroll
  for (int h = 0; h < kHeads; ++h) acc[h][0] = acc[h][1] = acc[h][2] = acc[h][3] = 0.f;
  if (sub < S) {
    for (int base = 0; sub + S * base < kTokens; base += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int j = sub + S * (base + u);
        if (j < kTokens) {
          const Raw4 cur = rb[u];
          if (j + S * PF < kTokens) rb[u] = raw_load4(zc + (size_t)(j + S * PF) * ldz, 4 * kg);
          float y[4];
          y_from_raw(cur, st[j], y);
          const float4 p0 = *reinterpret_cast<const float4*>(sc + j * kHeads), p1 = *reinterpret_cast<const float4*>(sc + j * kHeads + 4),
                       p2 = *reinterpret_cast<const float4*>(sc + j * kHeads + 8);
          const float p[kHeads] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
#pragma unroll
          for (int h = 0; h < kHeads; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[h][e] = __builtin_fmaf(p[h], y[e], acc[h][e]);
        }
      }
    }
    if (sub > 0)
#pragma unroll
      for (int h = 0; h < kHeads; ++h)
        *reinterpret_cast<float4*>(gs + ((sub - 1) * kHeads + h) * D + 4 * kg) = make_float4(acc[h][0], acc[h][1], acc[h][2], acc[h][3]);
  }
  if (S > 1) __syncthreads();
  if (sub == 0) {
#pragma unroll
    for (int h = 0; h < kHeads; ++h) {
      for (int s2 = 1; s2 < S; ++s2) {
        const float4 r = *reinterpret_cast<const float4*>(gs + ((s2 - 1) * kHeads + h) * D + 4 * kg);
        acc[h][0] += r.x; acc[h][1] += r.y; acc[h][2] += r.z; acc[h][3] += r.w;
      }
      *reinterpret_cast<float4*>(yb + ((size_t)cell * kHeads + h) * D + 4 * kg) = make_float4(acc[h][0], acc[h][1], acc[h][2], acc[h][3]);
    }
  }
}

// ---- o[S_h] for (head, cell tile), packed-split into columns h hd .. of token row 0 of every cell of `out`
template <int D>
__global__ __launch_bounds__(kThreads) void cls_out_kernel(const float* __restrict__ yb, const uint16_t* __restrict__ W, int ldw,
                                                           const float* __restrict__ bias2, int cells, uint16_t* __restrict__ out, int ldo) {
  constexpr int HD = D / kHeads, NKG = col_groups(D), NI = (HD + 15) / 16;
  __shared__ __attribute__((aligned(16))) float ys[kCT * (D + 4)];
  __shared__ __attribute__((aligned(16))) float os[kCT * HD];
  const int h = blockIdx.x % kHeads, c0 = (blockIdx.x / kHeads) * kCT, t = threadIdx.x;
  for (int idx = t; idx < kCT * NKG; idx += kThreads) {
    const int c = idx / NKG, kg = idx % NKG;
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 + c < cells) y = *reinterpret_cast<const float4*>(yb + ((size_t)(c0 + c) * kHeads + h) * D + 4 * kg);
    *reinterpret_cast<float4*>(ys + c * (D + 4) + 4 * kg) = y;
  }
  __syncthreads();
  {
    const int c = t % kCT, ng = t / kCT;
    double acc[NI];
    head_rows_dot<D, HD>(W + (size_t)(2 * D + h * HD) * ldw, ldw, ys, c, ng, acc);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = ng + 16 * i;
      if (n < HD) os[c * HD + n] = (float)(acc[i] + (double)bias2[2 * D + h * HD + n]);
    }
  }
  __syncthreads();
  for (int idx = t; idx < kCT * (HD / 4); idx += kThreads) {
    const int c = idx / (HD / 4), n4 = 4 * (idx % (HD / 4));
    if (c0 + c < cells) ps_store4(out + (size_t)(c0 + c) * kTokens * ldo, h * HD + n4, os + c * HD + n4);
  }
}

template <class F>
bool for_width(int D, const char* who, F&& f) {
  if (D == 144) f(std::integral_constant<int, 144>{});
  else if (D == 288) f(std::integral_constant<int, 288>{});
  else if (D == 384) f(std::integral_constant<int, 384>{});
  else if (D == 576) f(std::integral_constant<int, 576>{});
  else {
    launch_error("%s: width %d is not one of 144 / 288 / 384 / 576", who, D);
    return false;
  }
  return true;
}
inline unsigned head_tiles(int cells) { return (unsigned)kHeads * (unsigned)((cells + kCT - 1) / kCT); }

}  // namespace

bool cls_attention_supported(int D, int H, int T) { return H == kHeads && T == kTokens && (D == 144 || D == 288 || D == 384 || D == 576); }
int cls_attention_cell_tile() { return kCT; }
size_t cls_attention_scratch_elems(int cells, int D) { return (size_t)cells * kHeads * D; }

void launch_cls_attn_qg(const uint16_t* z, int ldz, const uint16_t* W, int ldw, const float* bias2, const float2* rowstat, int cells, int D,
                        float scale, float* g, hipStream_t s) {
  if (cells <= 0) return;
  for_width(D, "launch_cls_attn_qg", [&](auto d) {
    hipLaunchKernelGGL(cls_qg_kernel<decltype(d)::value>, dim3(head_tiles(cells)), dim3(kThreads), 0, s, z, ldz, W, ldw, bias2, rowstat, cells, scale, g);
  });
}
void launch_cls_attn_ybar(const uint16_t* z, int ldz, const float2* rowstat, const float* g, int cells, int D, float* yb, hipStream_t s) {
  if (cells <= 0) return;
  for_width(D, "launch_cls_attn_ybar", [&](auto d) {
    hipLaunchKernelGGL(cls_ybar_kernel<decltype(d)::value>, dim3(cells), dim3(kThreads), 0, s, z, ldz, rowstat, g, yb);
  });
}
void launch_cls_attn_out(const float* yb, const uint16_t* W, int ldw, const float* bias2, int cells, int D, uint16_t* out, int ldo, hipStream_t s) {
  if (cells <= 0) return;
  for_width(D, "launch_cls_attn_out", [&](auto d) {
    hipLaunchKernelGGL(cls_out_kernel<decltype(d)::value>, dim3(head_tiles(cells)), dim3(kThreads), 0, s, yb, W, ldw, bias2, cells, out, ldo);
  });
}

}  // namespace ribca
