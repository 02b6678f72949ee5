"""What the kernel-level GPU tests share: the packed-split encoding through the library's own packer, seeded operands, a LayerNorm case with its
row statistics and folded weight, the report of a measured error, and the guard-band arena.  A plain module: the tests import what they use by
name."""
import os

import numpy as np
import torch

from multiplexed_image_annotator_amd import synth

BAND = 8192      # bytes on either side of every operand: more than a 128-row tile of 48-byte rows, a 4 KB page and a 1 KB DMA piece


def ps_encode(x: torch.Tensor, kp: int, rows_pad: int = None) -> torch.Tensor:
    """fp32 [R, K] -> packed-split fp16 bits [Rp, 2*Kp] (int16 storage) via the library's own packer."""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    r, k = x.shape
    rp = rows_pad or r
    out = torch.zeros((rp, 2 * kp), dtype=torch.int16, device=x.device)
    check(lib().ribca_test_pack_weight(ptr(x.contiguous()), r, k, ptr(out), rp, kp, stream_ptr()), "pack")
    return out


def ps_decode(buf: torch.Tensor, k: int) -> torch.Tensor:
    """packed-split [R, 2*Kp] int16 -> fp64 [R, K] (hi + lo)."""
    r = buf.shape[0]
    f = buf.view(torch.float16).view(r, -1, 2, 8)
    hi, lo = f[:, :, 0, :].reshape(r, -1), f[:, :, 1, :].reshape(r, -1)
    return (hi.double() + lo.double())[:, :k]


def note_err(tag, err):
    """RIBCA_TEST_REPORT=1: print the measured error next to each bound (how the bounds of the tests were checked on hardware)."""
    if os.environ.get("RIBCA_TEST_REPORT"):
        import sys
        print(f"[measured] {tag}: {err:.3e}", file=sys.__stdout__, flush=True)      # past pytest's capture: the log of a run carries the values


def rnd(shape, seed, dev, scale=1.0):
    n = int(np.prod(shape))
    return (synth.approx_normal(synth.stream_key(seed, "t"), n).reshape(shape) * scale).to(torch.float32).to(dev)


def junk(nbytes, dev):
    return torch.full((max(int(nbytes), 1),), 255, dtype=torch.uint8, device=dev)      # as doubles: NaN


def ln_case(m, d, seed, dev, mean=0.5, std=3.0, row_scale=False):
    """rows of a packed-split residual stream with a chosen mean / spread, their exact (fp64) decode, LayerNorm parameters"""
    z = rnd((m, d), seed, dev, std) + mean
    if row_scale:      # spread the row scales over three decades (background tokens of a real patch sit at |z| ~ 0.02)
        z = z * torch.logspace(-2, 1, m, device=dev, dtype=torch.float32)[:, None]
    dp = (d + 31) // 32 * 32
    z_ps = ps_encode(z, dp)
    zq = ps_decode(z_ps, d)
    g = rnd((d,), seed + 1, dev, 0.1) + 1.0
    b = rnd((d,), seed + 2, dev, 0.1)
    return z_ps, zq, g, b, dp


def row_stats(z_ps, dp, m, d, dev, recentre=False):
    """(rstd, mean) per row of a packed-split buffer; recentre rewrites the rows as z - mean first"""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    rs = torch.zeros((m, 2), dtype=torch.float32, device=dev)
    check(lib().ribca_test_row_stats(ptr(z_ps), 2 * dp, m, d, ptr(rs), 1 if recentre else 0, stream_ptr()), "row_stats")
    return rs


def stats_err(rs, rows):
    """relative error of (rstd, mean) against the fp64 statistics of `rows`; the mean is measured on the scale of the row's spread"""
    mu = rows.mean(1)
    rstd = 1.0 / torch.sqrt(rows.var(1, unbiased=False) + 1e-6)
    amp = 1.0 + mu.abs() * rstd
    e1 = ((rs[:, 0].double() - rstd).abs() / (rstd * amp)).max().item()
    e2 = ((rs[:, 1].double() - mu).abs() * rstd / amp).max().item()
    return e1, e2


def fold_weight(w, g, b, bias, kp, dev):
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    n, k = w.shape
    npad = lib().ribca_gemm_padded_n(n)
    w_ps = torch.zeros((npad, 2 * kp), dtype=torch.int16, device=dev)
    csum = torch.zeros(n, dtype=torch.float32, device=dev)
    bias2 = torch.zeros(n, dtype=torch.float32, device=dev)
    check(lib().ribca_test_fold_weight(ptr(w), n, k, ptr(g), ptr(b), ptr(bias), ptr(w_ps), npad, kp, ptr(csum), ptr(bias2), stream_ptr()), "fold")
    return w_ps, csum, bias2


def umap_graph(n, seed, n_epochs=500):
    """the pruned fuzzy graph of n random points in 6 dimensions, its epochs per sample and its reverse edges"""
    import umap_restatement as R
    from multiplexed_image_annotator_amd import manifold
    x = np.random.RandomState(seed).randn(n, 6).astype(np.float32)
    idx, dist = R.knn(x, 15)
    sigma, rho = R.smooth_knn_dist(dist)
    g = manifold.prune_graph(manifold.fuzzy_union(idx, R.membership(idx, dist, sigma, rho), n), n_epochs)
    return g, manifold.epochs_per_sample(g.data, n_epochs), manifold.reverse_edges(g)


class Arena:
    """operands carved out of ONE device buffer with a band of `fill` bytes before and after each"""

    def __init__(self, dev, fill, capacity=96 << 20):
        self.buf = torch.full((capacity,), fill, dtype=torch.uint8, device=dev)
        self.fill, self.off, self.spans = fill, BAND, []

    def put(self, t: torch.Tensor) -> torch.Tensor:
        """a copy of t inside the arena"""
        v = self.empty(t.shape, t.dtype)
        v.copy_(t)
        return v

    def zeros(self, shape, dtype):
        v = self.empty(shape, dtype)
        v.zero_()
        return v

    def empty(self, shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        start = (self.off + 255) // 256 * 256
        assert start + nbytes + BAND <= self.buf.numel(), "arena too small"
        self.spans.append((start, nbytes))
        self.off = start + nbytes + BAND
        return self.buf[start:start + nbytes].view(dtype).view(shape)

    def bands_intact(self):
        """every byte outside the carved spans still holds the fill pattern"""
        mask = torch.ones(self.off, dtype=torch.bool, device=self.buf.device)
        for s, n in self.spans:
            mask[s:s + n] = False
        return bool(torch.all(self.buf[:self.off][mask] == self.fill))
