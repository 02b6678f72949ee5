"""What tests/test_gpu_cell_attention_mx.py and tests/test_mx_format.py share: the token rows of the per-cell MX kernel's input families as
fp32 on the host (before the packed-split encoding), the host statement of that encoding, and the emulated QKV product of either kernel.
Plain numpy / CPU torch: nothing here needs a device.

Families (rows [m][384]; m = cells * 101):
    uniform    N(0, 1) + 0.5                                     (ln_case(m, D, 90, dev, 0.5, 1.0))
    heavy      N(0, 1) + 0.5 under another seed                  (ln_case(m, D, 95, dev, 0.5, 1.0); the family's edge is in its weights)
    mean30     N(0, 1) + 30: |mean| / std = 30                   (ln_case(m, D, 90, dev, 30.0, 1.0))
    edge_rows  the rows of `uniform`, then per row: a scale out of logspace(-2, 1, m) in a seeded shuffled order (the 16 tokens of a wave
               differ); in every fourth row the columns k = 5, 13, 21, 29 (mod 32) x 4096 (four outliers in every scale block of either
               kernel; values beyond the fp16 range saturate at 65504 with lo = 0); in rows = 3 (mod 16) the columns k = 5, 13, 21, 29
               (mod 128) x 4096 -- all four inside ONE block of 32 consecutive k, one in each of the four blocks k = 128 S + 32 s + 8 g + j
               of this kernel: the rows on which the two groupings really differ; in rows = 1 (mod 16) columns 128 .. 255 exactly zero
               (every block of the 128-k step S = 1 has exponent field 0: the scale rule's clamp); rows = 2 (mod 16) x 1e-4 (hi an fp16
               subnormal).  Rows 0 and T - 1 of cell 0 stay as they were: the last token is the one the kernel's pad rows copy."""
import numpy as np
import torch

import mx_emulation as mx
from kernel_harness import rnd

D, T = 384, 101
ROW_FAMILIES = ["uniform", "heavy", "mean30", "edge_rows"]
_SEED = {"uniform": 90, "heavy": 95, "mean30": 90, "edge_rows": 90}
OUTLIER_COLS = [k for k in range(D) if k % 32 in (5, 13, 21, 29)]
OUTLIER_COLS_128 = [k for k in range(D) if k % 128 in (5, 13, 21, 29)]


def rows_f32(name, m):
    """the family's rows as ln_case draws them (fp32, host), edited for edge_rows"""
    z = rnd((m, D), _SEED[name], "cpu", 1.0) + (30.0 if name == "mean30" else 0.5)
    if name != "edge_rows":
        return z
    keep = z[[0, T - 1]].clone()
    order = np.random.RandomState(4211).permutation(m)
    scales = torch.from_numpy(np.logspace(-2.0, 1.0, m)[order].astype(np.float32))
    z = z * scales[:, None]
    z[0::4, OUTLIER_COLS] *= 4096.0
    z[3::16, OUTLIER_COLS_128] *= 4096.0
    z[1::16, 128:256] = 0.0
    z[2::16] *= 1.0e-4
    z[[0, T - 1]] = keep
    return z


def split_host(x32):
    """the packed-split encoding of fp32 values as the library's packer states it (clamp to the fp16 range, hi = fp16(x), lo =
    fp16(x - hi)): (hi float16, lo float16) numpy arrays"""
    x = np.clip(np.asarray(x32, dtype=np.float32), -65504.0, 65504.0)
    hi = x.astype(np.float16)
    return hi, (x - hi.astype(np.float32)).astype(np.float16)


def lo_codes(hi16, lo16, cell_blocks):
    """A lo / scale before the e4m3 rounding, per element, under the scale blocks of the per-cell kernel (cell_blocks) or the 32 consecutive
    k of gemm_mx.hip"""
    m, k = hi16.shape
    cols = np.arange(k)
    if cell_blocks:
        src = np.empty(k, dtype=np.int64)
        src[mx.hi_pos(cols)] = cols
        hi16, lo16 = hi16[:, src], lo16[:, src]
    ef = mx.f16_exp_field(np.abs(hi16.reshape(m, k // 32, 32))).max(axis=2)
    scale = 2.0 ** (np.maximum(ef, 1).astype(np.float64) + 93 - 127)
    return lo16.astype(np.float64).reshape(m, k // 32, 32) / scale[:, :, None], ef


def qkv_products(z_hi, z_lo16, w_hi, w_lo16):
    """(per-cell kernel's emulated product, unfused pair's emulated product) in float64: cell_gemm with that kernel's blocks, gemm with
    pack_act's 32 consecutive k"""
    lo = z_lo16.astype(np.float64)
    _, lo_q, _, _ = mx.pack_act(z_hi, lo)
    return mx.cell_gemm(z_hi, lo, w_hi, w_lo16), mx.gemm(z_hi, lo_q, w_hi, w_lo16)
