// What the attention kernels share.
//
// * softmax_keys_split: the softmax over the keys of one 16-query tile, in the S^T register layout, and the split of the probabilities into
//   the fp16 hi / lo operand of the P V product -- attention.hip (both kernels), cell_attention.hip, cell_attention_mx.hip.
// * lds_read_tr16: the transposed LDS read of the row-major V images (attention_lds_kernel and the per-cell kernels).
// * CellLdsMap: the LDS map of the per-cell kernels behind their weight ring (K images, V image, column sums and bias), with the padded
//   token and key counts kTP / kVRows -- cell_attention.hip and cell_attention_mx.hip.
//
// The functions are inlined into their kernels: same arithmetic, same order as when each kernel carried its own copy.  The rest of the
// per-cell kernels' common tail (once-per-cell staging, loader loop, folded LayerNorm, q / k / v publication, attention of a head group) is
// NOT here: as function templates it cost the fp16x3 kernel at D = 288 1.4 % and the MX kernel 0.6 % (docs/history.md, "One softmax, one
// LDS map"), so each of the two files keeps it, and tests/test_gpu_cell_attention_mx*.py hold the copies against each other.
#pragma once
#include "gemm_epi.h"
#include "ribca_common.h"

namespace ribca {

typedef __attribute__((__vector_size__(4 * sizeof(_Float16)))) _Float16 f16x4;
typedef __attribute__((__vector_size__(4 * sizeof(short)))) short s16x4;
// ds_read_b64_tr_b16: the 16 lanes of a group receive a 4-row x 16-column block of 16-bit elements column-major (lane 4q + p supplies the
// address of row q, columns 4p .. 4p + 3; lane i receives column i of the four rows)
__device__ __forceinline__ f16x4 lds_read_tr16(const char* p) {
  return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p)));
}

// s[kt][r] = S^T[key 16 kt + 4 g + r][this lane's query], kt < NT.  Keys >= T (only possible in the last tile) are padding.  On return
// phi / plo [t] are the hi / lo fragments of the normalised probabilities of k-step t: key tiles 2t (elements 0..3) and 2t + 1 (4..7);
// the tile behind an odd NT is zero.  s is left holding the unnormalised exponentials.
// (The pad-key mask is a select, not `if (...) s[NT - 1][r] = -INFINITY`: behind a reference the conditional store became a select of the
// whole four-score vector, five v_cndmask more per softmax.)
template <int NT>
__device__ __forceinline__ void softmax_keys_split(f32x4 (&s)[2 * ((NT + 1) / 2)], int T, int g, f16x8 (&phi)[(NT + 1) / 2],
                                                   f16x8 (&plo)[(NT + 1) / 2]) {
  constexpr int KST = (NT + 1) / 2;
#pragma unroll
  for (int r = 0; r < 4; ++r) s[NT - 1][r] = 16 * (NT - 1) + 4 * g + r >= T ? -INFINITY : s[NT - 1][r];
  float mx = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  // exp(s - mx) = exp2(s log2e - mx log2e): ONE packed fma per two scores in front of v_exp_f32 (a subtract and a multiply per
  // score before); probabilities are normalised two at a time and split without the fp16 range clamp (they lie in [0, 1])
  const f32x2v l2 = {1.44269504089f, 1.44269504089f}, moff = {-mx * 1.44269504089f, -mx * 1.44269504089f};
  f32x2v sum2 = {0.f, 0.f};
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    const f32x2v a0 = fma2(f32x2v{s[kt][0], s[kt][1]}, l2, moff);
    const f32x2v a1 = fma2(f32x2v{s[kt][2], s[kt][3]}, l2, moff);
    const f32x2v e0 = {__builtin_amdgcn_exp2f(a0.x), __builtin_amdgcn_exp2f(a0.y)}, e1 = {__builtin_amdgcn_exp2f(a1.x), __builtin_amdgcn_exp2f(a1.y)};
    s[kt] = f32x4{e0.x, e0.y, e1.x, e1.y};
    sum2 += e0;
    sum2 += e1;
  }
  float sum = sum2.x + sum2.y;
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
  const f32x2v inv2 = {inv, inv};
  if (NT & 1) s[NT] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < KST; ++t) {
    const f32x2v pa0 = f32x2v{s[2 * t][0], s[2 * t][1]} * inv2, pa1 = f32x2v{s[2 * t][2], s[2 * t][3]} * inv2;
    const f32x2v pb0 = f32x2v{s[2 * t + 1][0], s[2 * t + 1][1]} * inv2, pb1 = f32x2v{s[2 * t + 1][2], s[2 * t + 1][3]} * inv2;
    const float pa[4] = {pa0.x, pa0.y, pa1.x, pa1.y}, pb[4] = {pb0.x, pb0.y, pb1.x, pb1.y};
    uint2 ha, la, hb, lb;
    split4_unit(pa, ha, la);
    split4_unit(pb, hb, lb);
    phi[t] = __builtin_bit_cast(f16x8, uint4{ha.x, ha.y, hb.x, hb.y});
    plo[t] = __builtin_bit_cast(f16x8, uint4{la.x, la.y, lb.x, lb.y});
  }
}

// ------------------------------------------------------------------------------------------------------- per-cell kernels
// One 512-thread workgroup per cell: waves 0-6 own tokens 16 w .. 16 w + 15, wave 7 streams the weights through an LDS ring.
constexpr int kTP = 112, kVRows = 128;          // token rows of a cell padded to MFMA tiles; keys the P V product runs over

// The LDS map behind the ring: the K images of a head group (one per head), its V image, column sums and folded bias of the whole product.
template <int D_, int HD_, int GD_, int RING_BYTES> struct CellLdsMap {
  static constexpr int D = D_, HD = HD_;
  static constexpr int GD = GD_;                // feature dims per head group
  static constexpr int NTP = GD / 16;           // 16-column tiles per part (q, k, v)
  static constexpr int HPG = GD / HD;           // heads per group
  static constexpr int KIMG = kTP * ROWB;       // one head's K image: 112 tokens x 128 B (fragment order, swizzled like a GEMM tile)
  static constexpr int VROWB = 4 * GD;          // 192 / 256 B: the group's dims packed-split
  static constexpr int VIMG = kVRows * VROWB + 64;
  static constexpr int CB = 2 * 3 * D * 4;      // column sums and folded bias of the whole qkv product
  static constexpr int OFF_K = RING_BYTES;
  static constexpr int OFF_V = OFF_K + HPG * KIMG;
  static constexpr int OFF_CB = OFF_V + (VIMG + 15) / 16 * 16;
  static constexpr int LDS = OFF_CB + CB;
};

}  // namespace ribca
