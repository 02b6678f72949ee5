"""numpy oracles of the co-occurrence by distance, written from the rules include/ribca_hip.h states: the ordered cell pairs per (radius band,
cell type, neighbour type) of csrc/cooccurrence.hip by a chunked O(n^2) count with the same fp64 operation order (dx = x_i - x_j, d = dx * dx,
d += dy * dy: numpy rounds every elementwise operation on its own), and the lift of multiplexed_image_annotator_amd/cooccurrence.py restated with
fractions.Fraction, one entry at a time."""
from fractions import Fraction

import numpy as np


def pair_counts(x, y, labels, t, r2, chunk=512):
    """(B, t, t) int64: for every ordered pair i != j with both labels in [0, t), one count in the band b with r2[b - 1] < d2 <= r2[b] (band 0:
    d2 <= r2[0]); beyond r2[-1] nothing.  b = the number of thresholds strictly below d2."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    r2 = np.asarray(r2, dtype=np.float64)
    n, nb = len(x), len(r2)
    ok = (lab >= 0) & (lab < t)
    out = np.zeros(nb * t * t, dtype=np.int64)
    cols = np.arange(n)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        dx = x[i0:i1, None] - x[None, :]
        dy = y[i0:i1, None] - y[None, :]
        d = dx * dx
        d = d + dy * dy
        keep = (d <= r2[-1]) & ok[i0:i1, None] & ok[None, :] & (np.arange(i0, i1)[:, None] != cols[None, :])
        rows, js = np.nonzero(keep)
        band = np.searchsorted(r2, d[rows, js], side="left")
        out += np.bincount((band * t + lab[i0 + rows]) * t + lab[js], minlength=nb * t * t)
    return out.reshape(nb, t, t)


def lift(counts):
    """(B, T, T) fp64: Fraction(N S, R[a] R[c]) rounded once; NaN where R[a] R[c] is 0"""
    n = np.asarray(counts)
    out = np.full(n.shape, np.nan)
    for b in range(n.shape[0]):
        rows = [sum(int(v) for v in n[b, a]) for a in range(n.shape[1])]
        total = sum(rows)
        for a in range(n.shape[1]):
            for c in range(n.shape[2]):
                if rows[a] * rows[c]:
                    out[b, a, c] = float(Fraction(int(n[b, a, c]) * total, rows[a] * rows[c]))
    return out


def cumulative(counts):
    """running sums over the bands as Python integers"""
    n = np.asarray(counts).astype(object)
    out = n.copy()
    for b in range(1, n.shape[0]):
        out[b] = out[b - 1] + n[b]
    return out


def table_csv(names, radii, counts):
    """the long table, line by line"""
    n = np.asarray(counts).astype(object)
    cum = cumulative(counts)
    band, total = lift(n), lift(cum)
    text = "band,r_lo,r_hi,cell_type,neighbor_type,count,lift,cum_count,cum_lift\n"
    for b in range(n.shape[0]):
        for a in range(n.shape[1]):
            for c in range(n.shape[2]):
                text += ",".join([str(b), repr(0.0 if b == 0 else float(radii[b - 1])), repr(float(radii[b])), str(names[a]), str(names[c]), str(int(n[b, a, c])),
                                  repr(float(band[b, a, c])), str(int(cum[b, a, c])), repr(float(total[b, a, c]))]) + "\n"
    return text
