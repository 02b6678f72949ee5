// Second half of a 144-wide classifier block in ONE kernel, the token rows stationary in registers (timm Block: attn.proj + residual,
// norm2, mlp.fc1, GELU, mlp.fc2 + residual; reached from reference cell_type_annotation/model.py:54-55, 402):
//
//     z  <- fl(z + xa Wp^T + bp - mean1)                     (stored-row convention of EpiResidZK: re-centred, clamped, split;
//     h   = gelu(rstd2 (z (g2 o W1)^T) - rstd2 mean2 c1 + b1')   (ln_fold4, gelu_erf1)     the sums of the updates and of the statistics in fp64, one rounding)
//     z  <- fl(z + h W2^T + b2 - mean2),    rs <- (rstd, mean) of the new rows: final, no partials and no finaliser
//
// Why: at D = 144 every product of this half is tiny (K, N = 144 or 576) and the three GEMM launches it replaces move 8.8 KB per row,
// more than half of it the 576-wide h written by fc1 and read back by fc2.  A wave can own whole rows at this width -- 16 rows x 160
// columns as split fp16 operands are 40 registers, 16 x 144 fp32 accumulators 36 -- so only the weights stream (as in
// cell_attention.hip) and nothing but the new rows and their 8 bytes of statistics leaves the CU.
//
// * grid = ceil(M / 64), 256 threads, two workgroups per CU: wave w owns rows 64 b + 16 w .. + 15 (rows >= M compute on a copy of row
//   M - 1 and store nothing).  A row's bits depend on nothing but the row: not on M, its tile or its wave.
// * transposed tiles as in cell_attention.hip: a lane (r16, g) holds output columns 16 j + 4 g .. + 3 of token r16.  Two such tiles ARE one
//   32-deep operand fragment of the next product under the permutation  slot 8 g + p  <->  column (p < 4 ? 4 g + p : 16 + 4 g + p - 4)
//   of the 32-block, which cell_mlp_pack_kernel applies to the K order of fc1's and fc2's weights once at create: no transpose through LDS.
// * fc1 runs in six slices of 96 columns; each slice's GELU output is split in registers and multiplied straight into the fc2
//   accumulators (three K steps of fc2 per slice).  h never exists outside registers.
// * the weights of the whole half are ONE image of 53 stages in the order they are consumed (5 x proj, then per slice 5 x fc1 + 3 x fc2),
//   each stage the LDS image itself (XOR-swizzled 128-byte rows as gemm_split16.hip): the ring of three slots is filled by linear
//   LDS-DMA copies issued by the four waves themselves, two stages ahead, counted vmcnt, one s_barrier per stage with every fragment
//   read returned in front of it (tests/test_cell_mlp_resources.py).
// * per product and K step the three passes and their order are those of the GEMM family: lo * hi, hi * lo, hi * hi, fp32 accumulate.

#include "gemm_epi.h"
#include "ribca_common.h"
#include "ribca_kernels.h"

namespace ribca {

namespace {

constexpr int kD = 144, kDp = 160, kH4 = 576;
constexpr int kSlice = 96, kSlices = kH4 / kSlice;          // fc1 column slices
constexpr int kStageBig = kD * ROWB;                        // 18 KB: 144 weight rows of one 32-deep K step (proj, fc2)
constexpr int kStageFc1 = kSlice * ROWB;                    // 12 KB
constexpr int kNkD = kDp / 32;                              // 5 K steps over a residual row
constexpr int kNkS = kSlice / 32;                           // 3 K steps of fc2 per slice
constexpr int kProjBytes = kNkD * kStageBig;
constexpr int kSliceBytes = kNkD * kStageFc1 + kNkS * kStageBig;
constexpr int kImageBytes = kProjBytes + kSlices * kSliceBytes;      // 792 576
constexpr int kRing = 3;
constexpr int kOffC = kRing * kStageBig;                    // fc1c | fc1b2 | projb | fc2b
constexpr int kOffC1 = kOffC, kOffB1 = kOffC1 + kH4 * 4, kOffBp = kOffB1 + kH4 * 4, kOffB2 = kOffBp + kD * 4;
constexpr int kLds = kOffB2 + kD * 4;                       // 61 056 B: two workgroups per CU
constexpr float kEps = 1e-6f;

template <int OFF>
__device__ __forceinline__ void lds_rd16(f16x8& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_rd16(f32x4& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}

// logical column inside a 32-block of operand slot 8 g + p of a fragment built from two accumulator tiles
__device__ __host__ __forceinline__ int chain_col(int gq, int p) { return p < 4 ? 4 * gq + p : 16 + 4 * gq + (p - 4); }

}  // namespace

// projw [>= 144][320], fc1w (gamma o W) [>= 576][320], fc2w [>= 144][1152], all packed-split  ->  the stage image; one thread per 16 bytes
__global__ __launch_bounds__(256) void cell_mlp_pack_kernel(const uint16_t* __restrict__ projw, const uint16_t* __restrict__ fc1w,
                                                            const uint16_t* __restrict__ fc2w, uint16_t* __restrict__ img) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= kImageBytes / 16) return;
  const int byte = idx * 16;
  const uint16_t* W;
  int ldw, nbase, s, within;
  bool perm;
  if (byte < kProjBytes) {
    W = projw; ldw = 2 * kDp; nbase = 0; s = byte / kStageBig; within = byte % kStageBig; perm = false;
  } else {
    const int rem = byte - kProjBytes, q = rem / kSliceBytes, r2 = rem % kSliceBytes;
    if (r2 < kNkD * kStageFc1) {
      W = fc1w; ldw = 2 * kDp; nbase = kSlice * q; s = r2 / kStageFc1; within = r2 % kStageFc1; perm = true;
    } else {
      const int r3 = r2 - kNkD * kStageFc1;
      W = fc2w; ldw = 2 * kH4; nbase = 0; s = kNkS * q + r3 / kStageBig; within = r3 % kStageBig; perm = true;
    }
  }
  const int row = within / ROWB, pc = (within % ROWB) / 16;
  const int lc = pc ^ swz_f(row), gq = lc >> 1, part = lc & 1;
  const uint16_t* src = W + (size_t)(nbase + row) * ldw + 8 * part;
  uint16_t v[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) v[p] = src[ps_off(32 * s + (perm ? chain_col(gq, p) : 8 * gq + p))];
  uint4 o;
  o.x = v[0] | ((uint32_t)v[1] << 16); o.y = v[2] | ((uint32_t)v[3] << 16); o.z = v[4] | ((uint32_t)v[5] << 16); o.w = v[6] | ((uint32_t)v[7] << 16);
  reinterpret_cast<uint4*>(img)[idx] = o;
}

__global__ __launch_bounds__(256, 2) void cell_mlp_kernel(const uint16_t* __restrict__ xa, int ldx, const char* __restrict__ img,
                                                          const float* __restrict__ projb, const float* __restrict__ fc1c,
                                                          const float* __restrict__ fc1b2, const float* __restrict__ fc2b, uint16_t* z, int ldz,
                                                          float2* rs, int M) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int m = blockIdx.x * 64 + wave * 16 + r16;
  const bool ok = m < M;
  const int mrow = ok ? m : M - 1;

  // ---- everything this wave reads from global memory besides the weights: requested first and waited for with the constants below, in
  // front of the first ring stage (the counted waits of the ring then see LDS-DMA pieces only)
  const uint16_t* xr = xa + (size_t)mrow * ldx;
  f16x8 ahi[kNkD], alo[kNkD];
#pragma unroll
  for (int s = 0; s < kNkD; ++s) {
    const uint4* p = reinterpret_cast<const uint4*>(xr + (4 * s + g) * 16);
    ahi[s] = __builtin_bit_cast(f16x8, p[0]);
    alo[s] = __builtin_bit_cast(f16x8, p[1]);
  }
  uint16_t* zr = z + (size_t)mrow * ldz;
  uint2 zoh[kD / 16], zol[kD / 16];
#pragma unroll
  for (int j = 0; j < kD / 16; ++j) {
    const uint16_t* p = zr + ps_off(16 * j + 4 * g);
    zoh[j] = *reinterpret_cast<const uint2*>(p);
    zol[j] = *reinterpret_cast<const uint2*>(p + 8);
  }
  const float pm1 = rs[mrow].y;
  for (int i = tid; i < kH4 / 4; i += 256) {
    reinterpret_cast<float4*>(smem + kOffC1)[i] = reinterpret_cast<const float4*>(fc1c)[i];
    reinterpret_cast<float4*>(smem + kOffB1)[i] = reinterpret_cast<const float4*>(fc1b2)[i];
  }
  if (tid < kD / 4) {
    reinterpret_cast<float4*>(smem + kOffBp)[tid] = reinterpret_cast<const float4*>(projb)[tid];
    reinterpret_cast<float4*>(smem + kOffB2)[tid] = reinterpret_cast<const float4*>(fc2b)[tid];
  }
  // the loaded values are USED here, in front of the first LDS-DMA: hipcc places its own wait for them at their first use, and behind the
  // ring's first pieces that wait would cover the pieces as well
  float pm1u = pm1;
#pragma unroll
  for (int s = 0; s < kNkD; ++s) asm volatile("" : "+v"(ahi[s]), "+v"(alo[s]));
#pragma unroll
  for (int j = 0; j < kD / 16; ++j) asm volatile("" : "+v"(zoh[j].x), "+v"(zoh[j].y), "+v"(zol[j].x), "+v"(zol[j].y));
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(pm1u)::"memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // ---- the weight ring: stage = NP pieces of 1 KB, wave w copies pieces w, w + 4, ...
  const char* gsrc = img + wave * 1024 + lane * 16;
  auto issue = [&](auto np_c, int off, int slot) {
    constexpr int NP = decltype(np_c)::value;
    char* st = smem + slot * kStageBig + wave * 1024;
#pragma unroll
    for (int i = 0; i < (NP + 3) / 4; ++i) {
      if (4 * i + 3 < NP || wave + 4 * i < NP)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc + off + i * 4096),
                                         (__attribute__((address_space(3))) void*)(st + i * 4096), 16, 0, 0);
    }
  };
  constexpr std::integral_constant<int, kStageBig / 1024> kBig{};
  constexpr std::integral_constant<int, kStageFc1 / 1024> kFc1{};
  // what may stay in flight when a stage is waited for: the NEXT stage's pieces of the wave that has the fewest (4 of 18, 3 of 12)
  constexpr int kFlyBig = 4, kFlyFc1 = 3;

  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const unsigned w_rd = lds_base + (unsigned)lds_off(r16, 2 * g);      // + 2048 per tile, + kStageBig per slot; lo: ^ 16
  const unsigned c_rd = lds_base + (unsigned)(16 * g);                  // constants: + 4 n0

  // NT output tiles of one K step from ring slot `slot`: acc[j] += W[16 j ..][step] . (bhi, blo), three passes, fragment reads one
  // group of three tiles ahead of their MFMAs
  auto kstep = [&](auto nt_c, int slot, const f16x8& bhi, const f16x8& blo, f32x4* acc) {
    constexpr int NT = decltype(nt_c)::value, NG = NT / 3;
    const unsigned ah = w_rd + (unsigned)(slot * kStageBig), al = ah ^ 16u;
    f16x8 wh[2][3], wl[2][3];
    lds_rd16<0>(wh[0][0], ah); lds_rd16<0>(wl[0][0], al);
    lds_rd16<2048>(wh[0][1], ah); lds_rd16<2048>(wl[0][1], al);
    lds_rd16<4096>(wh[0][2], ah); lds_rd16<4096>(wl[0][2], al);
    auto group = [&](auto jb_c) {
      constexpr int jb = decltype(jb_c)::value, cur = jb & 1, nxt = cur ^ 1;
      if constexpr (jb + 1 < NG) {
        lds_rd16<(3 * jb + 3) * 2048>(wh[nxt][0], ah); lds_rd16<(3 * jb + 3) * 2048>(wl[nxt][0], al);
        lds_rd16<(3 * jb + 4) * 2048>(wh[nxt][1], ah); lds_rd16<(3 * jb + 4) * 2048>(wl[nxt][1], al);
        lds_rd16<(3 * jb + 5) * 2048>(wh[nxt][2], ah); lds_rd16<(3 * jb + 5) * 2048>(wl[nxt][2], al);
        asm volatile("s_waitcnt lgkmcnt(6)"
                     : "+v"(wh[cur][0]), "+v"(wh[cur][1]), "+v"(wh[cur][2]), "+v"(wl[cur][0]), "+v"(wl[cur][1]), "+v"(wl[cur][2])::"memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(wh[cur][0]), "+v"(wh[cur][1]), "+v"(wh[cur][2]), "+v"(wl[cur][0]), "+v"(wl[cur][1]), "+v"(wl[cur][2])::"memory");
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * jb + j] = mfma_f16(wl[cur][j], bhi, acc[3 * jb + j]);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * jb + j] = mfma_f16(wh[cur][j], blo, acc[3 * jb + j]);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * jb + j] = mfma_f16(wh[cur][j], bhi, acc[3 * jb + j]);
    };
    group(std::integral_constant<int, 0>{});
    if constexpr (NG > 1) group(std::integral_constant<int, 1>{});
    if constexpr (NG > 2) group(std::integral_constant<int, 2>{});
  };
  // top of a stage: its pieces have landed (FLY younger ones may stay in flight), every read of the previous stage has returned (kstep
  // ends on lgkmcnt(0); stated again for the ring rule), and behind the barrier the slot of the stage before is free
  auto stage_top = [&](auto fly_c) {
    wait_vmcnt<decltype(fly_c)::value>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  constexpr std::integral_constant<int, kFlyBig> fBig{};
  constexpr std::integral_constant<int, kFlyFc1> fFc1{};
  constexpr std::integral_constant<int, 0> fNone{};
  constexpr std::integral_constant<int, 9> t9{};
  constexpr std::integral_constant<int, 6> t6{};

  // mean and rstd of a row from the lane's 36 clamped fp32 values, summed in fp64 (the row's four lanes in a fixed order).  A row's values
  // can differ by three decades (one massive activation beside 143 small ones): fp32 sums then lose the small ones' bits twice over, in the
  // mean and again in the centred squares, and the rstd's relative error multiplies every fc1 output of the row.  36 + 36 conversions and
  // adds per lane and row, beside 144 GELU evaluations: not on the kernel's critical path.
  auto dsum4 = [&](double v) { v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64); return v; };
  auto row_stats = [&](const f32x4* x, float& mean, float& rstd) {
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < kD / 16; ++j) sum += ((double)x[j][0] + (double)x[j][1]) + ((double)x[j][2] + (double)x[j][3]);
    const double md = dsum4(sum) / (double)kD;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < kD / 16; ++j) {
      const double d0 = x[j][0] - md, d1 = x[j][1] - md, d2 = x[j][2] - md, d3 = x[j][3] - md;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    mean = (float)md;
    rstd = (float)(1.0 / sqrt(dsum4(q) / (double)kD + (double)kEps));
  };

  // ------------------------------------------------------------------------------------------------ proj + residual + norm2 statistics
  int slot = 0;                                                         // ring slot of the current stage
  issue(kBig, 0, 0);
  issue(kBig, kStageBig, 1);
  f32x4 acc[kD / 16];
#pragma unroll
  for (int j = 0; j < kD / 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < kNkD; ++s) {
    if (s + 1 < kNkD) stage_top(fBig); else stage_top(fFc1);
    const int nslot = slot == 0 ? 2 : slot - 1;                          // (slot + 2) % 3
    if (s + 2 < kNkD) issue(kBig, (s + 2) * kStageBig, nslot);
    else issue(kFc1, kProjBytes + (s + 2 - kNkD) * kStageFc1, nslot);    // the first slice's fc1 stages 0, 1
    kstep(t9, slot, ahi[s], alo[s], acc);
    slot = slot == 2 ? 0 : slot + 1;
  }
  // the row as stored: x = clamp(z + acc + bias - previous mean), split; zhi / zlo are the operand of fc1 AND the residual of fc2.
  // The four terms are added in fp64 and rounded ONCE: three fp32 additions cost up to three half-ulps at the magnitude of the
  // largest partial sum, which is what the stored row's error was made of wherever z and the product nearly cancel.
  f16x8 zhi[kNkD], zlo[kNkD];
  float mean2, rstd2;
  {
    f32x4 b4[kD / 16];
    lds_rd16<kOffBp + 0 * 64>(b4[0], c_rd); lds_rd16<kOffBp + 1 * 64>(b4[1], c_rd); lds_rd16<kOffBp + 2 * 64>(b4[2], c_rd);
    lds_rd16<kOffBp + 3 * 64>(b4[3], c_rd); lds_rd16<kOffBp + 4 * 64>(b4[4], c_rd); lds_rd16<kOffBp + 5 * 64>(b4[5], c_rd);
    lds_rd16<kOffBp + 6 * 64>(b4[6], c_rd); lds_rd16<kOffBp + 7 * 64>(b4[7], c_rd); lds_rd16<kOffBp + 8 * 64>(b4[8], c_rd);
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(b4[0]), "+v"(b4[1]), "+v"(b4[2]), "+v"(b4[3]), "+v"(b4[4]), "+v"(b4[5]), "+v"(b4[6]), "+v"(b4[7]), "+v"(b4[8])::"memory");
    uint2 xh[kD / 16 + 1], xl[kD / 16 + 1];
#pragma unroll
    for (int j = 0; j < kD / 16; ++j) {
      const float zo[4] = {f16lo_plus_f16lo(zoh[j].x, zol[j].x), f16hi_plus_f16hi(zoh[j].x, zol[j].x), f16lo_plus_f16lo(zoh[j].y, zol[j].y),
                           f16hi_plus_f16hi(zoh[j].y, zol[j].y)};
      float x[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = clamp_f16_range((float)((double)zo[r] + ((double)acc[j][r] + ((double)b4[j][r] - (double)pm1u))));
      acc[j] = f32x4{x[0], x[1], x[2], x[3]};
      split4_unit(x, xh[j], xl[j]);                                     // already inside the fp16 range
    }
    xh[kD / 16] = uint2{0u, 0u}; xl[kD / 16] = uint2{0u, 0u};            // columns 144 .. 159: the K pad
    row_stats(acc, mean2, rstd2);
#pragma unroll
    for (int s = 0; s < kNkD; ++s) {
      zhi[s] = __builtin_bit_cast(f16x8, uint4{xh[2 * s].x, xh[2 * s].y, xh[2 * s + 1].x, xh[2 * s + 1].y});
      zlo[s] = __builtin_bit_cast(f16x8, uint4{xl[2 * s].x, xl[2 * s].y, xl[2 * s + 1].x, xl[2 * s + 1].y});
    }
  }
  const float nm2 = -mean2 * rstd2;

  // ------------------------------------------------------------------------------------------------ fc1 -> GELU -> fc2, slice by slice
#pragma unroll
  for (int j = 0; j < kD / 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < kSlices; ++q) {
    const int base = kProjBytes + q * kSliceBytes;                       // this slice's stages in the image
    const bool more = q + 1 < kSlices;
    f32x4 hacc[kSlice / 16];
#pragma unroll
    for (int j = 0; j < kSlice / 16; ++j) hacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < kNkD; ++s) {
      if (s + 1 < kNkD) stage_top(fFc1); else stage_top(fBig);
      const int nslot = slot == 0 ? 2 : slot - 1;
      if (s + 2 < kNkD) issue(kFc1, base + (s + 2) * kStageFc1, nslot);
      else issue(kBig, base + kNkD * kStageFc1 + (s + 2 - kNkD) * kStageBig, nslot);
      kstep(t6, slot, zhi[s], zlo[s], hacc);
      slot = slot == 2 ? 0 : slot + 1;
    }
    // folded LayerNorm + GELU, split in registers: two tiles are one operand fragment of fc2
    f16x8 hhi[kNkS], hlo[kNkS];
    {
      f32x4 c4[kSlice / 16], b4[kSlice / 16];
      const unsigned cq = c_rd + (unsigned)(q * kSlice * 4);
      lds_rd16<kOffC1 + 0 * 64>(c4[0], cq); lds_rd16<kOffB1 + 0 * 64>(b4[0], cq);
      lds_rd16<kOffC1 + 1 * 64>(c4[1], cq); lds_rd16<kOffB1 + 1 * 64>(b4[1], cq);
      lds_rd16<kOffC1 + 2 * 64>(c4[2], cq); lds_rd16<kOffB1 + 2 * 64>(b4[2], cq);
      lds_rd16<kOffC1 + 3 * 64>(c4[3], cq); lds_rd16<kOffB1 + 3 * 64>(b4[3], cq);
      lds_rd16<kOffC1 + 4 * 64>(c4[4], cq); lds_rd16<kOffB1 + 4 * 64>(b4[4], cq);
      lds_rd16<kOffC1 + 5 * 64>(c4[5], cq); lds_rd16<kOffB1 + 5 * 64>(b4[5], cq);
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(c4[0]), "+v"(c4[1]), "+v"(c4[2]), "+v"(c4[3]), "+v"(c4[4]), "+v"(c4[5]), "+v"(b4[0]), "+v"(b4[1]), "+v"(b4[2]),
                     "+v"(b4[3]), "+v"(b4[4]), "+v"(b4[5])::"memory");
      uint2 hh[kSlice / 16], hl[kSlice / 16];
#pragma unroll
      for (int j = 0; j < kSlice / 16; ++j) {
        float x[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = gelu_erf1(fmaf(rstd2, hacc[j][r], fmaf(nm2, c4[j][r], b4[j][r])));
        split4(x, hh[j], hl[j]);
      }
#pragma unroll
      for (int s = 0; s < kNkS; ++s) {
        hhi[s] = __builtin_bit_cast(f16x8, uint4{hh[2 * s].x, hh[2 * s].y, hh[2 * s + 1].x, hh[2 * s + 1].y});
        hlo[s] = __builtin_bit_cast(f16x8, uint4{hl[2 * s].x, hl[2 * s].y, hl[2 * s + 1].x, hl[2 * s + 1].y});
      }
    }
#pragma unroll
    for (int s = 0; s < kNkS; ++s) {
      // behind this stage: another fc2 stage, or the next slice's first fc1 stage, or nothing
      if (s + 1 < kNkS) stage_top(fBig);
      else if (more) stage_top(fFc1);
      else stage_top(fNone);
      const int nslot = slot == 0 ? 2 : slot - 1;
      if (s + 2 < kNkS) issue(kBig, base + kNkD * kStageFc1 + (s + 2) * kStageBig, nslot);
      else if (more) issue(kFc1, base + kSliceBytes + (s + 2 - kNkS) * kStageFc1, nslot);
      kstep(t9, slot, hhi[s], hlo[s], acc);
      slot = slot == 2 ? 0 : slot + 1;
    }
  }

  // ------------------------------------------------------------------------------------------------ residual, store, final statistics
  {
    f32x4 b4[kD / 16];
    lds_rd16<kOffB2 + 0 * 64>(b4[0], c_rd); lds_rd16<kOffB2 + 1 * 64>(b4[1], c_rd); lds_rd16<kOffB2 + 2 * 64>(b4[2], c_rd);
    lds_rd16<kOffB2 + 3 * 64>(b4[3], c_rd); lds_rd16<kOffB2 + 4 * 64>(b4[4], c_rd); lds_rd16<kOffB2 + 5 * 64>(b4[5], c_rd);
    lds_rd16<kOffB2 + 6 * 64>(b4[6], c_rd); lds_rd16<kOffB2 + 7 * 64>(b4[7], c_rd); lds_rd16<kOffB2 + 8 * 64>(b4[8], c_rd);
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(b4[0]), "+v"(b4[1]), "+v"(b4[2]), "+v"(b4[3]), "+v"(b4[4]), "+v"(b4[5]), "+v"(b4[6]), "+v"(b4[7]), "+v"(b4[8])::"memory");
#pragma unroll
    for (int j = 0; j < kD / 16; ++j) {
      const uint4 h = __builtin_bit_cast(uint4, zhi[j >> 1]), l = __builtin_bit_cast(uint4, zlo[j >> 1]);
      const uint32_t h0 = (j & 1) ? h.z : h.x, h1 = (j & 1) ? h.w : h.y, l0 = (j & 1) ? l.z : l.x, l1 = (j & 1) ? l.w : l.y;
      const float zo[4] = {f16lo_plus_f16lo(h0, l0), f16hi_plus_f16hi(h0, l0), f16lo_plus_f16lo(h1, l1), f16hi_plus_f16hi(h1, l1)};
      float x[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = clamp_f16_range((float)((double)zo[r] + ((double)acc[j][r] + ((double)b4[j][r] - (double)mean2))));
      acc[j] = f32x4{x[0], x[1], x[2], x[3]};
      // the partner lane (g ^ 1, same row, same guard) holds the other four columns of the packed-split group
      if (ok) ps_store4_pair<16>(z + (size_t)m * ldz, 16 * j + 4 * g, x);
    }
    float mean, rstd;
    row_stats(acc, mean, rstd);
    if (ok && g == 0) rs[m] = float2{rstd, mean};
  }
}

bool cell_mlp_supported(int D) { return D == kD; }
size_t cell_mlp_image_bytes(int D) { return D == kD ? (size_t)kImageBytes : 0; }

void launch_cell_mlp_pack(const uint16_t* projw, const uint16_t* fc1w, const uint16_t* fc2w, int D, uint16_t* img, hipStream_t s) {
  if (D != kD) { launch_error("cell_mlp: no form for D = %d", D); return; }
  hipLaunchKernelGGL(cell_mlp_pack_kernel, dim3((kImageBytes / 16 + 255) / 256), dim3(256), 0, s, projw, fc1w, fc2w, img);
}

void launch_cell_mlp(const uint16_t* xa, int ldx, const uint16_t* img, const float* projb, const float* fc1c, const float* fc1b2, const float* fc2b,
                     uint16_t* z, int ldz, float2* rs, int M, int D, hipStream_t s) {
  if (M <= 0) return;
  if (D != kD || ldx < 2 * kDp || ldz < 2 * kDp) { launch_error("cell_mlp: no form for D = %d, ldx = %d, ldz = %d", D, ldx, ldz); return; }
  static unsigned long long attr_done = 0ull;
  if (!ensure_dynamic_lds(reinterpret_cast<const void*>(cell_mlp_kernel), kLds, attr_done)) return;
  hipLaunchKernelGGL(cell_mlp_kernel, dim3((M + 63) / 64), dim3(256), kLds, s, xa, ldx, reinterpret_cast<const char*>(img), projb, fc1c, fc1b2, fc2b, z,
                     ldz, rs, M);
}

}  // namespace ribca
