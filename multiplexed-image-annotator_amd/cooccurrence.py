"""Host side of the co-occurrence by distance (Annotator.cooccurrence_by_distance): from the (B, T, T) integer counts N_b[a][c] of ordered cell
pairs per radius band (ops.radial_pair_counts; csrc/cooccurrence.hip) the lift of every (band, cell type, neighbour type), its cumulative form,
the long table and the values of the figures.  lift_b[a][c] = N_b[a][c] S_b / (R_b[a] R_b[c]) with the row totals R_b[a] = sum_c N_b[a][c] and the
band total S_b = sum_a R_b[a]: the observed count over the count expected if the two types of a pair in that ring were independent (every band
matrix is symmetric, so the row totals are the column totals).  In the spirit of squidpy's ``co_occurrence``, not numerically identical to it: that
one is cumulative with its own choice of intervals.  No torch here.  DESIGN.md section 15."""
from __future__ import annotations

import re
from typing import Dict, Sequence

import numpy as np


def default_radii(cell_size, bands: int = 16) -> np.ndarray:
    """cell_size, 2 cell_size, ... bands cell_size pixels"""
    return float(cell_size) * np.arange(1, int(bands) + 1, dtype=np.float64)


def check_radii(radii, max_bands: int) -> np.ndarray:
    """the radii as a 1-d fp64 array; ValueError unless there are 1 .. max_bands of them, finite, non-negative and strictly increasing"""
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if not 1 <= r.size <= max_bands:
        raise ValueError(f"the co-occurrence takes 1 to {max_bands} radii, got {r.size}")
    if not np.isfinite(r).all() or (r < 0.0).any() or (np.diff(r) <= 0.0).any():
        raise ValueError(f"the radii must be finite, non-negative and strictly increasing, got {r.tolist()}")
    with np.errstate(over="ignore"):
        r2 = r * r
    if not np.isfinite(r2).all() or (np.diff(r2) <= 0.0).any():
        raise ValueError(f"the squares of the radii must be finite and strictly increasing, got {r.tolist()}")
    return r


def slug(name) -> str:
    """a cell-type name as part of a file name: every character outside [A-Za-z0-9] becomes ``_``"""
    return re.sub(r"[^A-Za-z0-9]", "_", str(name))


def _exact(counts) -> np.ndarray:
    n = np.asarray(counts)
    if n.ndim != 3 or n.shape[1] != n.shape[2] or n.dtype.kind not in "iu":
        raise ValueError(f"the co-occurrence takes (B, T, T) integer counts, got {n.dtype} {n.shape}")
    return n.astype(object)      # Python integers from here on


def _lift_of(exact: np.ndarray) -> np.ndarray:
    """numerator N S and denominator R[a] R[c] as Python integers, then ONE true division: correctly rounded, whatever the size of the counts"""
    out = np.full(exact.shape, np.nan, dtype=np.float64)
    for b in range(exact.shape[0]):
        rows = [sum(int(v) for v in exact[b, a]) for a in range(exact.shape[1])]
        total = sum(rows)
        for a in range(exact.shape[1]):
            for c in range(exact.shape[2]):
                den = rows[a] * rows[c]
                if den > 0:
                    out[b, a, c] = (int(exact[b, a, c]) * total) / den
    return out


def lift(counts) -> np.ndarray:
    """(B, T, T) fp64: the lift of every band; NaN where a marginal is zero"""
    return _lift_of(_exact(counts))


def cumulative_counts(counts) -> np.ndarray:
    """(B, T, T) Python integers: the pairs with d <= r_hi of each band, the running sums over the bands"""
    return np.cumsum(_exact(counts), axis=0)


def cumulative_lift(counts) -> np.ndarray:
    """the same lift over every pair with d <= r_hi of the band"""
    return _lift_of(cumulative_counts(counts))


def band_totals(counts) -> Dict[str, np.ndarray]:
    """``rows`` (B, T) and ``total`` (B) as arrays of Python integers"""
    exact = _exact(counts)
    rows = exact.sum(axis=2)
    return {"rows": rows, "total": rows.sum(axis=1)}


def figure_values(counts, lifts) -> np.ndarray:
    """log2 of the lift where the count is positive, NaN elsewhere (a zero count has lift 0 or none)"""
    n = np.asarray(counts)
    out = np.full(n.shape, np.nan, dtype=np.float64)
    ok = n > 0
    out[ok] = np.log2(np.asarray(lifts, dtype=np.float64)[ok])
    return out


def table_csv(names: Sequence[str], radii, counts) -> str:
    """long form, one line per (band, cell type, neighbour type); the floats with ``repr`` (the text parses back to the same doubles)"""
    exact = _exact(counts)
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if r.size != exact.shape[0] or len(names) != exact.shape[1]:
        raise ValueError(f"{r.size} radii and {len(names)} names for counts of shape {exact.shape}")
    cum = np.cumsum(exact, axis=0)
    band, total = _lift_of(exact), _lift_of(cum)
    lines = ["band,r_lo,r_hi,cell_type,neighbor_type,count,lift,cum_count,cum_lift"]
    for b in range(exact.shape[0]):
        lo, hi = (0.0 if b == 0 else float(r[b - 1])), float(r[b])
        for a, first in enumerate(names):
            for c, second in enumerate(names):
                lines.append(f"{b},{lo!r},{hi!r},{first},{second},{int(exact[b, a, c])},{float(band[b, a, c])!r},{int(cum[b, a, c])},"
                             f"{float(total[b, a, c])!r}")
    return "\n".join(lines) + "\n"
