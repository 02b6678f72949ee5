"""Host side of the local indicators of spatial association (Annotator.local_autocorrelation): the seed, local Moran's I and Getis-Ord Gi* per
cell from the neighbour sums of ops.local_lag, the two-sided pseudo-p-value and the class of every cell from the conditional-permutation counts of
ops.local_perm_counts (csrc/local_autocorr.hip), and the two CSVs.  The statistics are those of PySAL's ``esda.Moran_Local`` / ``G_Local`` over a
k-NN graph with unit weights: with m neighbours per cell, n cells, z the centred values of a channel, lag_i the sum of z over the neighbours of i
and D = sum_i z_i^2,
    I_i = n z_i lag_i / (m D)                                                        (their mean is the global Moran's I of autocorr.py)
    Gi*_i = (lag_i + z_i) / (sqrt(D / n) sqrt((n w - w^2) / (n - 1))),  w = m + 1       (the analytic z-score, the cell included)
With z_i fixed the lag is the only random part of either, so one pair of counts (ge, le: the permutations with a lag at or above / at or below
the observed one) serves both.  NO MULTIPLE-TESTING CORRECTION IS APPLIED: at alpha = 0.05 about one cell in twenty of an unstructured channel
is flagged.  No torch here.  DESIGN.md section 17."""
from __future__ import annotations

import os
from fractions import Fraction
from typing import Dict, Sequence, Tuple

import numpy as np

#: class index -> name: the quadrant of (z, lag) of a significant cell
CLASSES = ("not_significant", "HH", "LH", "LL", "HL")
FIELDS = ("z", "lag", "local_i", "gi_star", "n_ge", "n_le", "p", "class")


def default_seed() -> int:
    """RIBCA_LOCAL_SEED overrides the default seed 0; read at every call."""
    v = os.environ.get("RIBCA_LOCAL_SEED")
    return int(v) if v not in (None, "") else 0


def alpha_fraction(alpha) -> Tuple[int, int]:
    """alpha = num / den exactly, from its decimal text (0.05 -> 1 / 20); 0 < alpha <= 1"""
    f = Fraction(str(alpha))
    if not 0 < f <= 1:
        raise ValueError(f"alpha must lie in (0, 1], got {alpha}")
    return f.numerator, f.denominator


def statistics(z, lag, ge, le, m2, m: int, n_perms: int, alpha=0.05) -> Dict[str, np.ndarray]:
    """z, lag (n, C) fp64; ge, le (n, C) integer counts over n_perms permutations; m2 (C) = D, the sum of z^2 per channel; m = the width of the
    neighbour list.  Returns (n, C) arrays: ``local_i`` (NaN where D == 0), ``gi_star`` (NaN where D == 0 or n <= m + 1), ``p`` =
    min(1, 2 (min(ge, le) + 1) / (P + 1)), the two-sided pseudo-p-value, and ``class`` (uint8): 0 unless the cell is significant -- in integers,
    2 (min(ge, le) + 1) den <= num (P + 1) with alpha = num / den -- and then 1 HH (z > 0, lag > 0), 2 LH (z < 0, lag > 0), 3 LL (z < 0,
    lag < 0), 4 HL (z > 0, lag < 0); a z or lag of exactly 0 stays 0.  No multiple-testing correction."""
    z = np.asarray(z, dtype=np.float64)
    lag = np.asarray(lag, dtype=np.float64)
    ge = np.asarray(ge).astype(np.int64)
    le = np.asarray(le).astype(np.int64)
    d = np.asarray(m2, dtype=np.float64)
    if z.ndim != 2 or lag.shape != z.shape or ge.shape != z.shape or le.shape != z.shape or d.shape != z.shape[1:]:
        raise ValueError(f"statistics takes (n, C) values, lags and two counts and (C) sums of squares, got {z.shape}, {lag.shape}, {ge.shape}, "
                         f"{le.shape} and {d.shape}")
    n, m, p = len(z), int(m), int(n_perms)
    if n < 1 or m < 1 or p < 1:
        raise ValueError(f"statistics needs at least one cell, one neighbour and one permutation, got {n}, {m} and {p}")
    num, den = alpha_fraction(alpha)
    w = float(m + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        local_i = np.where(d == 0.0, np.nan, (float(n) * z * lag) / (float(m) * d))
        if n > m + 1:
            scale = np.sqrt(d / float(n)) * np.sqrt((float(n) * w - w * w) / float(n - 1))
            gi = np.where(d == 0.0, np.nan, (lag + z) / scale)
        else:
            gi = np.full(z.shape, np.nan)
    low = np.minimum(ge, le)
    pval = np.minimum(1.0, (2.0 * (low + 1).astype(np.float64)) / float(p + 1))
    significant = 2 * (low + 1) * den <= num * (p + 1)
    cls = np.zeros(z.shape, dtype=np.uint8)
    cls[significant & (z > 0) & (lag > 0)] = 1
    cls[significant & (z < 0) & (lag > 0)] = 2
    cls[significant & (z < 0) & (lag < 0)] = 3
    cls[significant & (z > 0) & (lag < 0)] = 4
    return {"z": z, "lag": lag, "local_i": local_i, "gi_star": gi, "n_ge": ge, "n_le": le, "p": pval, "class": cls}


def table_csv(cell_ids: Sequence[int], markers: Sequence[str], stats: Dict[str, np.ndarray]) -> str:
    """one line per cell: cell_id, then per marker z, lag, local_i, gi_star, n_ge, n_le, p, class; the floats with 17 significant digits (the
    text parses back to the same doubles)"""
    lines = ["cell_id," + ",".join(f"{name}_{f}" for name in markers for f in FIELDS)]
    for r, cell in enumerate(cell_ids):
        cols = [str(int(cell))]
        for k in range(len(markers)):
            cols += [f"{float(stats[f][r, k]):.17g}" for f in ("z", "lag", "local_i", "gi_star")]
            cols += [str(int(stats["n_ge"][r, k])), str(int(stats["n_le"][r, k])), f"{float(stats['p'][r, k]):.17g}", str(int(stats["class"][r, k]))]
        lines.append(",".join(cols))
    return "\n".join(lines) + "\n"


def class_counts(cls) -> np.ndarray:
    """(C, 5): the cells of every channel in each of the five classes"""
    cls = np.asarray(cls)
    return np.stack([np.bincount(cls[:, k], minlength=len(CLASSES))[:len(CLASSES)] for k in range(cls.shape[1])]).astype(np.int64)


def summary_csv(markers: Sequence[str], cls) -> str:
    """one line per marker: the cells in each class, in the order of CLASSES"""
    counts = class_counts(cls)
    lines = ["marker,cells," + ",".join(CLASSES)]
    for k, name in enumerate(markers):
        lines.append(",".join([str(name), str(int(len(cls)))] + [str(int(v)) for v in counts[k]]))
    return "\n".join(lines) + "\n"
