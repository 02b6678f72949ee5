// The per-cell fusion  norm1 -> attn.qkv -> softmax(q k^T) v  of cell_attention.hip with the QKV phase on the MX products of gemm_mx.hip
// (D = 384, head dim 32; timm Block.norm1 / Attention reached from reference cell_type_annotation/model.py:54-55, 402):
//
//   A W^T  ~=  Ah Wh^T  +  Al' Wh'^T  +  Ah' Wl'^T        per 128 k and accumulator tile: 4 x v_mfma_f32_16x16x32_f16,
//                                                          one scaled MFMA  A lo (e4m3) x W hi (e2m3)  and one  A hi (e2m3) x W lo (e2m3)
//   = 1.75 matrix units per product instead of the three fp16 passes of cell_qkv_attention_kernel, and -- what this kernel is bound by --
//   90 bytes per lane, tile and 128 k read back from the ring instead of 128 (4 hi fragments, 24 bytes of fp6 lo', 2 scale bytes), 23 KB
//   per 128-deep stage of four tiles through the LDS-DMA instead of 32 KB.
//
// Shared with cell_attention.hip through attn_core.h: the softmax (softmax_keys_split), the transposed V read and the LDS map behind the
// ring.  The grid, the once-per-cell staging, the loader wave's loop, the folded LayerNorm, the k / v publication and the loops of the
// attention phase are that file's code, repeated here: moved into shared function templates they compiled to a slower fp16x3 kernel at
// D = 288 (docs/history.md, "One softmax, one LDS map"), and a tail that only one of the two kernels calls would be no gain.  What differs:
// * The token rows stay in registers for the whole cell, so their images are built ONCE per cell: per 128 k the lane (token, g) holds
//   k = 32 s + 8 g + j (s = sub-step 0..3, j = 0..7) -- 32 values that form ONE scale block (a permutation of k inside 128 that the pack
//   kernel applies to W as well: the block of lane g IS the 32 "consecutive" k' = 32 g + 8 s + j the fp6 operand wants in one lane).
//   A hi' is one v_cvt_scalef32_pk32_fp6_f16 of the hi fragments; A lo' is converted to e4m3 with the block's scale (rules of gemm_mx.hip:
//   sl = max(exponent field of the block's largest |hi|, 1) + 93, the fp6 image of hi at sl + 17) and then exchanged between the four lanes
//   of a token: an fp8 operand's lane g holds k' = 16 g .. + 15 and 64 + 16 g .. + 15, i.e. half a block of lane g >> 1 and half a block of
//   lane 2 + (g >> 1) (16 ds_bpermute per 128 k and cell).
// * The weight image (cell_attn_mx_pack_kernel, once per model) is in ring-stage order: stage = (head group, 128 k, part q | k | v) =
//   four 16-column tiles, per tile four 1 KB hi fragments [sub-step], then the fp6 image of lo (16 + 8 bytes per lane) and 16 bytes of
//   scale bytes per lane (sl, sh per tile): every piece is read with lane-linear addresses, free of bank conflicts.  The fp6 image of W hi
//   is NOT stored: the wave has the four hi fragments of a tile in registers and converts them (one v_cvt_scalef32_pk32_fp6_f16 per tile and
//   128 k) -- storing it would add 24 bytes per lane and tile to the very LDS stream the kernel stalls on.
// * 9 ring steps per head group (3 x 128 k x 3 parts) instead of 12, 23 DMA pieces each instead of 24.

#include <type_traits>
#include <utility>

#include "attn_core.h"
#include "gemm_epi.h"
#include "ribca_common.h"
#include "ribca_kernels.h"

namespace ribca {

namespace {

typedef int i32x8m __attribute__((ext_vector_type(8)));
typedef unsigned u32x6m __attribute__((ext_vector_type(6)));
typedef _Float16 h32m __attribute__((ext_vector_type(32)));
typedef short s16x2m __attribute__((ext_vector_type(2)));

template <int... Is, class F>
__device__ __forceinline__ void sfor_impl(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void sfor(F&& f) {
  sfor_impl(std::make_integer_sequence<int, N>{}, f);
}

template <int D, int HD> struct CellMxGeom {
  static constexpr int NK = D / 32;            // 32-deep sub-steps: the token rows' fragments
  static constexpr int NS = D / 128;           // 128-deep MX steps
  static constexpr int GD = 64;                // feature dims per head group: two heads of 32 -> 4 MFMA tiles each of q, k, v
  static constexpr int NTP = GD / 16;          // 16-column tiles per part (q, k, v) = tiles per ring stage
  static constexpr int SPG = 3 * NS;           // ring steps per head group: (128 k, part)
  static constexpr int OFF_L6A = NTP * 4096;   // behind the hi fragments [tile][sub-step][64 x 16]: fp6 lo' dwords 0-3 [tile][64 x 16]
  static constexpr int OFF_L6B = OFF_L6A + NTP * 1024;      // fp6 lo' dwords 4-5 [tile][64 x 8]
  static constexpr int OFF_SC = OFF_L6B + NTP * 512;        // scale bytes [64 x 16]: (sl, sh) of tiles 0..3, 8 bytes of zeros
  static constexpr int WSTAGE = OFF_SC + 1024;              // 23 KB
  static constexpr int GPL = WSTAGE / 1024;                 // DMA instructions (1 KB each) per stage
  static constexpr int GROUPS = D / GD;
  static constexpr int RING = 3;               // stage s + 1 is written while stage s is read; the slot of s - 1 is free by then
  using Map = CellLdsMap<D, HD, GD, RING * WSTAGE>;      // K images, V image, column sums and bias behind the ring (attn_core.h)
  static constexpr int LDS = Map::LDS;
  static constexpr size_t IMAGE = (size_t)GROUPS * SPG * WSTAGE;
  static_assert(D % 128 == 0 && HD == 32 && D % GD == 0 && Map::HPG % 2 == 0, "geometry: whole 128-deep steps, two heads of 32 per group");
  static_assert(WSTAGE % 1024 == 0 && 2 * GPL <= 63, "whole DMA pieces; two stages in flight within the 6-bit vmcnt");
  static_assert(LDS <= 160 * 1024, "LDS of a CU");
};

}  // namespace

// ----------------------------------------------------------------------------------------------------------- weight image
// packed-split gamma o W of qkv [>= 3 D][ldw] -> the stage image; one thread per (stage, tile, lane) = (output column n, 128 k, g): the 32
// values k = 128 S + 32 s + 8 g + j of row n, their fp6 lo' image and both scale bytes (the rules of mx_pack_w_kernel, gemm_mx.hip: either
// image scaled so that the block's largest magnitude lands in [4, 8))
template <int D, int HD>
__global__ void cell_attn_mx_pack_kernel(const uint16_t* __restrict__ W, int ldw, unsigned char* __restrict__ img) {
  using G = CellMxGeom<D, HD>;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G::GROUPS * G::SPG * G::NTP * 64) return;
  const int lane = idx & 63, jt = (idx >> 6) % G::NTP, stage = idx / (64 * G::NTP);
  const int hg = stage / G::SPG, rem = stage - hg * G::SPG, S = rem / 3, part = rem - 3 * S;
  const int r16 = lane & 15, g = lane >> 4;
  const int n = part * D + hg * G::GD + 16 * jt + r16;
  const uint16_t* src = W + (size_t)n * ldw + 256 * S + 16 * g;      // PS group (128 S + 32 s + 8 g) / 8 = 16 S + 4 s + g: + 64 s
  h32m lv;
  unsigned mh = 0, ml = 0;
  uint4 hraw[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    hraw[t] = *reinterpret_cast<const uint4*>(src + 64 * t);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint16_t hb = src[64 * t + e], lb = src[64 * t + 8 + e];
      lv[8 * t + e] = __builtin_bit_cast(_Float16, lb);
      mh = max(mh, (unsigned)(hb & 0x7fff)); ml = max(ml, (unsigned)(lb & 0x7fff));
    }
  }
  int eh = (int)(mh >> 10), el = (int)(ml >> 10);
  eh = eh < 1 ? 1 : eh; el = el < 1 ? 1 : el;
  const int sh = eh + 110, sl = el + 110;      // E - 2 + 127, E = ef - 15
  const u32x6m l6 = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(lv, e8m0_float(sl));
  unsigned char* st = img + (size_t)stage * G::WSTAGE;
#pragma unroll
  for (int t = 0; t < 4; ++t) *reinterpret_cast<uint4*>(st + (jt * 4 + t) * 1024 + lane * 16) = hraw[t];
  *reinterpret_cast<uint4*>(st + G::OFF_L6A + jt * 1024 + lane * 16) = uint4{l6[0], l6[1], l6[2], l6[3]};
  *reinterpret_cast<uint2*>(st + G::OFF_L6B + jt * 512 + lane * 8) = uint2{l6[4], l6[5]};
  unsigned char* sc = st + G::OFF_SC + lane * 16;
  sc[2 * jt] = (unsigned char)sl;
  sc[2 * jt + 1] = (unsigned char)sh;
  if (jt == 0) *reinterpret_cast<uint2*>(sc + 8) = uint2{0u, 0u};
}

// ----------------------------------------------------------------------------------------------------------- kernel
template <int D, int HD>
__global__ __launch_bounds__(512) void cell_qkv_attention_mx_kernel(const uint16_t* __restrict__ z, int ldz, const unsigned char* __restrict__ img,
                                                                    const float* __restrict__ bias2, const float* __restrict__ csum,
                                                                    const float2* __restrict__ rowstat, uint16_t* __restrict__ out, int ldo, int T,
                                                                    float scale) {
  using G = CellMxGeom<D, HD>;
  using M = typename G::Map;
  constexpr int NK = G::NK, NS = G::NS, SPG = G::SPG, GROUPS = G::GROUPS, HPG = M::HPG, kRing = G::RING, kGroupDims = G::GD, NTP = G::NTP,
                kWStage = G::WSTAGE;
  constexpr int NTILES = 3 * NTP;              // accumulator tiles per wave and group: q | k | v
  constexpr int TOTAL = GROUPS * SPG;          // ring steps of the whole cell
  constexpr int GPL = G::GPL;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cell = blockIdx.x;
  const int r16 = lane & 15, g = lane >> 4;

  // ---- once per cell: column sums / folded bias of all 3 D outputs, zero rows behind V
  for (int i = tid; i < 3 * D / 4; i += 512) {
    reinterpret_cast<float4*>(smem + M::OFF_CB)[i] = reinterpret_cast<const float4*>(csum)[i];
    reinterpret_cast<float4*>(smem + M::OFF_CB + 3 * D * 4)[i] = reinterpret_cast<const float4*>(bias2)[i];
  }
  for (int o = kTP * M::VROWB + tid * 16; o < M::VIMG; o += 512 * 16) *reinterpret_cast<uint4*>(smem + M::OFF_V + o) = uint4{0u, 0u, 0u, 0u};
  __syncthreads();

  if (wave == 7) {
    // ------------------------------------------------------------------ loader: the stage image is the stream, two steps ahead (the ring
    // protocol of cell_attention.hip: a slot is refilled only behind the barrier in front of which every consumer's reads of it have returned)
    auto issue = [&](int step) {
      const unsigned char* src = img + (size_t)step * kWStage + lane * 16;
      char* st = smem + (step % kRing) * kWStage;
#pragma unroll
      for (int i = 0; i < GPL; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i * 1024),
                                         (__attribute__((address_space(3))) void*)(st + i * 1024), 16, 0, 0);
    };
    issue(0);
    issue(1);
    for (int step = 0; step < TOTAL; ++step) {
      if (step + 1 < TOTAL) wait_vmcnt<GPL>();
      else wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();                            // stage `step` landed; the slot of step - 1 has been read by everyone
      asm volatile("" ::: "memory");
      if (step + 2 < TOTAL) issue(step + 2);
      if ((step + 1) % SPG == 0) __builtin_amdgcn_s_barrier();  // the group's "k, v published" barrier
    }
    return;
  }

  // -------------------------------------------------------------------- consumers: wave w owns tokens 16 w .. 16 w + 15
  const int tok = wave * 16 + r16;
  const int trow = tok < T ? tok : T - 1;                      // pad rows compute on a copy of the last token; nothing of theirs is stored
  const uint16_t* zr = z + ((size_t)cell * T + trow) * ldz;
  f16x8 ahi[NK];
  i32x8m al8[NS], ah6[NS];                                     // the e4m3 image of lo (exchanged into the fp8 operand's k order) and the fp6 image of hi
  int asc[NS];                                                 // byte 0: the block's lo scale, byte 1: its fp6-hi scale
#pragma unroll
  for (int S = 0; S < NS; ++S) {
    uint4 lo[4];
    unsigned mh = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint4* p = reinterpret_cast<const uint4*>(zr + (4 * (4 * S + t) + g) * 16);
      const uint4 h = p[0];
      lo[t] = p[1];
      ahi[4 * S + t] = __builtin_bit_cast(f16x8, h);
      const unsigned w[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) mh = max(mh, max(w[e] & 0x7fffu, (w[e] >> 16) & 0x7fffu));
    }
    const int sl = mx_sl_byte((int)(mh >> 10));
    const float lscale = e8m0_float(sl);
    unsigned c8[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const unsigned w[4] = {lo[t].x, lo[t].y, lo[t].z, lo[t].w};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const f32x2 a = unpack_f16(w[2 * e]), b = unpack_f16(w[2 * e + 1]);
        s16x2m r = {0, 0};
        r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, a[0], a[1], lscale, false);
        r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, b[0], b[1], lscale, true);
        c8[2 * t + e] = __builtin_bit_cast(unsigned, r);
      }
    }
    // fp8 operand order: dwords 0-3 = k' 16 g .. + 15 = sub-steps 2 (g & 1), + 1 of lane g >> 1; dwords 4-7 = the same of lane 2 + (g >> 1)
    const int srcA = r16 + 16 * (g >> 1), srcB = srcA + 32;
    unsigned d8[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned a0 = __shfl(c8[i], srcA, 64), a1 = __shfl(c8[4 + i], srcA, 64);
      const unsigned b0 = __shfl(c8[i], srcB, 64), b1 = __shfl(c8[4 + i], srcB, 64);
      d8[i] = (g & 1) ? a1 : a0;
      d8[4 + i] = (g & 1) ? b1 : b0;
    }
    al8[S] = i32x8m{(int)d8[0], (int)d8[1], (int)d8[2], (int)d8[3], (int)d8[4], (int)d8[5], (int)d8[6], (int)d8[7]};
    h32m hv;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) hv[8 * t + e] = ahi[4 * S + t][e];
    const u32x6m h6 = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(hv, e8m0_float(sl + kMxShDelta));
    ah6[S] = i32x8m{(int)h6[0], (int)h6[1], (int)h6[2], (int)h6[3], (int)h6[4], (int)h6[5], 0, 0};      // (dwords 6, 7 are not read by an fp6 operand)
    asc[S] = sl | ((sl + kMxShDelta) << 8);
  }
  const float2 rs = rowstat[(size_t)cell * T + trow];
  const float rstd = rs.x, nm = -rs.y * rs.x;
  const char* cb = smem + M::OFF_CB;
  uint16_t* orow = out + ((size_t)cell * T + tok) * ldo;
  const int k_wr = lds_off(tok, 2 * g);                        // this lane's 32 bytes (hi | lo) of a K image row
  constexpr int KST = 4, NT = 7;

  int step = 0;
  for (int hg = 0; hg < GROUPS; ++hg) {
    f32x4 acc[NTILES];
#pragma unroll
    for (int j = 0; j < NTILES; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    sfor<SPG>([&](auto sp_c) {
      constexpr int SP = decltype(sp_c)::value, S = SP / 3, PART = SP % 3;
      // Every fragment read of the PREVIOUS stage must have RETURNED before this barrier: behind it the loader refills that very slot
      // (ring of 3, two stages ahead) -- cell_attention.hip, DESIGN.md section 3.2.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const char* st = smem + (step % kRing) * kWStage + lane * 16;
      ++step;
      const uint2 wsc = *reinterpret_cast<const uint2*>(st + G::OFF_SC);      // bytes: sl0 sh0 sl1 sh1 | sl2 sh2 sl3 sh3
      sfor<NTP / 2>([&](auto jp_c) {
        constexpr int JP = decltype(jp_c)::value;
        const int scw = (int)(JP == 0 ? wsc.x : wsc.y);
        f16x8 whi[2][4];
        i32x8m wl6[2], wh6[2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          constexpr int dummy = 0; (void)dummy;
          const int jt = 2 * JP + jj;
#pragma unroll
          for (int t = 0; t < 4; ++t) whi[jj][t] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(st + (jt * 4 + t) * 1024));
          const uint4 la = *reinterpret_cast<const uint4*>(st + G::OFF_L6A + jt * 1024);
          const uint2 lb = *reinterpret_cast<const uint2*>(st + G::OFF_L6B + jt * 512 - lane * 8);
          wl6[jj] = i32x8m{(int)la.x, (int)la.y, (int)la.z, (int)la.w, (int)lb.x, (int)lb.y, 0, 0};
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          // the fp6 image of this tile's W hi, from the four fragments the wave holds anyway; scale byte = the packer's sh of (tile, lane)
          h32m hv;
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) hv[8 * t + e] = whi[jj][t][e];
          const unsigned shb = ((unsigned)scw >> (16 * jj + 8)) & 0xffu;
          const u32x6m c = __builtin_amdgcn_cvt_scalef32_pk32_fp6_f16(hv, e8m0_float((int)shb));
          wh6[jj] = i32x8m{(int)c[0], (int)c[1], (int)c[2], (int)c[3], (int)c[4], (int)c[5], 0, 0};
        }
        constexpr int J0 = PART * NTP + 2 * JP;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc[J0] = mfma_f16(whi[0][t], ahi[4 * S + t], acc[J0]);
          acc[J0 + 1] = mfma_f16(whi[1][t], ahi[4 * S + t], acc[J0 + 1]);
        }
        // W hi' (fp6, its sh byte) x A lo' (fp8, byte 0);  W lo' (fp6, its sl byte) x A hi' (fp6, byte 1)
        acc[J0] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wh6[0], al8[S], acc[J0], 2, 0, 1, scw, 0, asc[S]);
        acc[J0 + 1] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wh6[1], al8[S], acc[J0 + 1], 2, 0, 3, scw, 0, asc[S]);
        acc[J0] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wl6[0], ah6[S], acc[J0], 2, 2, 0, scw, 1, asc[S]);
        acc[J0 + 1] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wl6[1], ah6[S], acc[J0 + 1], 2, 2, 2, scw, 1, asc[S]);
      });
    });
    // ---- folded LayerNorm + bias: tile j of part `which` holds output columns which D + 48 hg + 16 (j % 3) + 4 g .. + 3 of this token
#pragma unroll
    for (int j = 0; j < NTILES; ++j) {
      const int n = (j / NTP) * D + hg * kGroupDims + 16 * (j % NTP) + 4 * g;
      const float4 c4 = *reinterpret_cast<const float4*>(cb + n * 4), b4 = *reinterpret_cast<const float4*>(cb + 3 * D * 4 + n * 4);
      // two columns per instruction (v_pk_fma_f32); the same two fused multiply-adds per value as ln_fold4 (gemm_epi.h)
      const f32x2v r2 = {rstd, rstd}, n2 = {nm, nm};
      const f32x2v lo2 = fma2(r2, f32x2v{acc[j][0], acc[j][1]}, fma2(n2, f32x2v{c4.x, c4.y}, f32x2v{b4.x, b4.y}));
      const f32x2v hi2 = fma2(r2, f32x2v{acc[j][2], acc[j][3]}, fma2(n2, f32x2v{c4.z, c4.w}, f32x2v{b4.z, b4.w}));
      acc[j] = f32x4{lo2.x, lo2.y, hi2.x, hi2.y};
    }
    // ---- publish k (fragment order, one image per head) and v (row-major packed-split rows of 48 dims)
    f16x8 qhi[HPG], qlo[HPG];
#pragma unroll
    for (int h = 0; h < HPG; ++h) {
      constexpr int dummy = 0; (void)dummy;
      const int d_lo = h * HD, d_hi = d_lo + HD;               // dims of this head inside the group
      const int tA = d_lo / 16, tB = (d_hi - 1) / 16;
      // a lane's 4 columns of a tile lie wholly inside or outside the head (HD % 4 == 0)
      const bool inA = 16 * tA + 4 * g >= d_lo && 16 * tA + 4 * g < d_hi;
      const bool inB = tB != tA && 16 * tB + 4 * g >= d_lo && 16 * tB + 4 * g < d_hi;
      float qa[4], qb[4], ka[4], kb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        qa[r] = inA ? acc[tA][r] * scale : 0.f;
        qb[r] = inB ? acc[tB][r] * scale : 0.f;
        ka[r] = inA ? acc[NTP + tA][r] : 0.f;
        kb[r] = inB ? acc[NTP + tB][r] : 0.f;
      }
      uint2 h0, l0, h1, l1;
      split4(qa, h0, l0);
      split4(qb, h1, l1);
      qhi[h] = __builtin_bit_cast(f16x8, uint4{h0.x, h0.y, h1.x, h1.y});
      qlo[h] = __builtin_bit_cast(f16x8, uint4{l0.x, l0.y, l1.x, l1.y});
      split4(ka, h0, l0);
      split4(kb, h1, l1);
      char* kimg = smem + M::OFF_K + h * M::KIMG;
      *reinterpret_cast<uint4*>(kimg + k_wr) = uint4{h0.x, h0.y, h1.x, h1.y};
      *reinterpret_cast<uint4*>(kimg + (k_wr ^ 16)) = uint4{l0.x, l0.y, l1.x, l1.y};
    }
    {
      uint16_t* vrow = reinterpret_cast<uint16_t*>(smem + M::OFF_V + tok * M::VROWB);
#pragma unroll
      for (int j = 0; j < NTP; ++j) {
        const float v4[4] = {acc[2 * NTP + j][0], acc[2 * NTP + j][1], acc[2 * NTP + j][2], acc[2 * NTP + j][3]};
        // 256-byte V rows (64-dim groups) would put the 8 rows of a transposed read on the same banks: the 16-dim pair index is
        // XORed with the low two bits of the row on both sides (write here, read below)
        const int jj = kGroupDims == 64 ? (j ^ (tok & 3)) : j;
        ps_store4_pair<16>(vrow, 16 * jj + 4 * g, v4);         // lanes g and g ^ 1 complete an 8-dim group: 16 bytes each
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                              // k, v of every token are in LDS
    asm volatile("" ::: "memory");

    // ---- attention of the group's heads for this wave's 16 queries, TWO heads at a time: the S^T MFMAs of one head cover the softmax
    // VALU of the other, and the two P V products interleave (a wave is in-order: without a second independent chain every
    // exp / split waits behind the MFMAs that feed it)
    constexpr int DT = (HD + 15) / 16;
    const char* vimg = smem + M::OFF_V;
#pragma unroll
    for (int hp = 0; hp < HPG; hp += 2) {
      f32x4 s[2][2 * KST];
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        const int ko = lds_off(16 * kt + r16, 2 * g);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const char* kimg = smem + M::OFF_K + (hp + e) * M::KIMG;
          const f16x8 kh = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(kimg + ko));
          const f16x8 kl = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(kimg + (ko ^ 16)));
          s[e][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
          s[e][kt] = mfma_f16(kl, qhi[hp + e], s[e][kt]);
          s[e][kt] = mfma_f16(kh, qlo[hp + e], s[e][kt]);
          s[e][kt] = mfma_f16(kh, qhi[hp + e], s[e][kt]);
        }
      }
      f16x8 phi[2][KST], plo[2][KST];
#pragma unroll
      for (int e = 0; e < 2; ++e) softmax_keys_split<NT>(s[e], T, g, phi[e], plo[e]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int t = 0; t < KST; ++t) {
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int dcol0 = (hp + e) * HD + 16 * dt + 4 * (r16 & 3);    // first of the 4 dims this lane addresses for the transposed read
            const int dcol = kGroupDims == 64 ? ((((dcol0 >> 4) ^ (r16 >> 2)) << 4) | (dcol0 & 15)) : dcol0;      // (row & 3 == r16 >> 2)
            const int voff = (dcol >> 3) * 32 + (dcol & 7) * 2;           // byte offset of their hi halves inside a V row; + 16: lo halves
            const char* va = vimg + (32 * t + 4 * g + (r16 >> 2)) * M::VROWB + voff;
            const f16x4 h0 = lds_read_tr16(va), l0 = lds_read_tr16(va + 16);
            const f16x4 h1 = lds_read_tr16(va + 16 * M::VROWB), l1 = lds_read_tr16(va + 16 * M::VROWB + 16);
            const f16x8 vhi = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
            const f16x8 vlo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
            o[e] = mfma_f16(vlo, phi[e][t], o[e]);
            o[e] = mfma_f16(vhi, plo[e][t], o[e]);
            o[e] = mfma_f16(vhi, phi[e][t], o[e]);
          }
        }
        const int d = 16 * dt + 4 * g;                         // o[r] = O[query tok][head dim d + r]
        if (tok < T && d < HD) {
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float v4[4] = {o[e][0], o[e][1], o[e][2], o[e][3]};
            ps_store4(orow, (hg * HPG + hp + e) * HD + d, v4);
          }
        }
      }
    }
  }
}

bool cell_attention_mx_supported(int D, int H, int T) { return H == kHeads && T == kTokens && D == 384; }
size_t cell_attention_mx_image_bytes(int D) { return D == 384 ? CellMxGeom<384, 32>::IMAGE : 0; }

void launch_cell_attention_mx_pack(const uint16_t* W, int ldw, int D, unsigned char* img, hipStream_t s) {
  if (D != 384) { launch_error("launch_cell_attention_mx_pack: no stage image for D = %d", D); return; }
  using G = CellMxGeom<384, 32>;
  constexpr int total = G::GROUPS * G::SPG * G::NTP * 64;
  hipLaunchKernelGGL((cell_attn_mx_pack_kernel<384, 32>), dim3((total + 255) / 256), dim3(256), 0, s, W, ldw, img);
}

void launch_cell_qkv_attention_mx(const uint16_t* z, int ldz, const unsigned char* img, const float* bias2, const float* csum, const float2* rowstat,
                                  uint16_t* out, int ldo, int cells, int D, float scale, hipStream_t s) {
  if (cells <= 0) return;
  if (D != 384) { launch_error("launch_cell_qkv_attention_mx: no kernel for D = %d", D); return; }
  static unsigned long long attr_done = 0ull;
  const auto kern = cell_qkv_attention_mx_kernel<384, 32>;
  constexpr int lds = CellMxGeom<384, 32>::LDS;
  if (!ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds, attr_done)) return;
  hipLaunchKernelGGL(kern, dim3(cells), dim3(512), lds, s, z, ldz, img, bias2, csum, rowstat, out, ldo, (int)kTokens, scale);
}

}  // namespace ribca
