"""Host side of the neighbourhood enrichment (Annotator.neighborhood_enrichment): the seed, the z-scores of the observed co-occurrence counts
against their permutation null (ops.nhood_perm_counts; csrc/enrichment.hip) and the two CSVs.  The statistic is histoCAT's / squidpy's
``nhood_enrichment``: z = (observed - mean of the null) / population std of the null, the k-NN graph fixed and the labels shuffled within each
image.  DESIGN.md section 14."""
from __future__ import annotations

import math
import os
from typing import Dict, Sequence

import numpy as np


def default_seed() -> int:
    """RIBCA_ENRICH_SEED overrides the default seed 0; read at every call."""
    v = os.environ.get("RIBCA_ENRICH_SEED")
    return int(v) if v not in (None, "") else 0


def z_scores(observed, perm_counts) -> Dict[str, np.ndarray]:
    """observed (T, T) and perm_counts (P, T, T) integer counts -> ``mean``, ``std``, ``z`` (T, T) fp64 and ``n_ge``, ``n_le`` (T, T) int64.
    S1 = sum of the null counts and S2 = sum of their squares are exact Python integers (P S2 passes 2^63 for counts near 2^27 at P = 1000):
    mean = S1 / P, std = sqrt(P S2 - S1^2) / P (the population std), z = (observed - mean) / std and NaN where std is 0; n_ge / n_le = the
    permutations whose count is >= / <= the observed one."""
    obs = np.asarray(observed)
    perm = np.asarray(perm_counts)
    if perm.ndim != 3 or perm.shape[0] < 1 or obs.shape != perm.shape[1:]:
        raise ValueError(f"z_scores takes (T, T) observed counts and (P, T, T) permutation counts with P >= 1, got {obs.shape} and {perm.shape}")
    if obs.dtype.kind not in "iu" or perm.dtype.kind not in "iu":
        raise ValueError("z_scores takes integer counts")
    p = int(perm.shape[0])
    exact = perm.astype(object)      # Python integers from here on
    s1 = exact.sum(axis=0)
    s2 = (exact * exact).sum(axis=0)
    mean = np.empty(obs.shape, dtype=np.float64)
    std = np.empty(obs.shape, dtype=np.float64)
    for pos in np.ndindex(*obs.shape):
        a, b = int(s1[pos]), int(s2[pos])
        mean[pos] = a / p
        std[pos] = math.sqrt(p * b - a * a) / p
    z = np.full(obs.shape, np.nan)
    ok = std > 0.0
    z[ok] = (obs[ok].astype(np.float64) - mean[ok]) / std[ok]
    target = obs.astype(object)[None]      # compared as Python integers: int64 against uint64 would go through float64 in numpy
    return {"mean": mean, "std": std, "z": z, "n_ge": (exact >= target).sum(axis=0).astype(np.int64),
            "n_le": (exact <= target).sum(axis=0).astype(np.int64)}


def colour_limit(z: np.ndarray) -> float:
    """the symmetric colour scale of the figure: +- the largest |z| that is finite, +- 1 when there is none (or it is 0)"""
    finite = np.abs(z[np.isfinite(z)])
    lim = float(finite.max()) if finite.size else 0.0
    return lim if lim > 0.0 else 1.0


def matrix_csv(names: Sequence[str], z: np.ndarray) -> str:
    """the layout of the reference's neighbourhood CSV (spatial_methods.py:117-128: a trailing comma on every line), z with three decimals, ``nan``
    where it is NaN"""
    lines = ["cell_type," + "".join(f"{c}," for c in names)]
    for r, c in enumerate(names):
        lines.append(f"{c}," + "".join(f"{float(z[r][j]):.3f}," for j in range(len(names))))
    return "\n".join(lines) + "\n"


def table_csv(names: Sequence[str], observed: np.ndarray, stats: Dict[str, np.ndarray]) -> str:
    """long form, one line per (cell type, neighbour type): the floats with 17 significant digits (the text parses back to the same doubles)"""
    lines = ["cell_type,neighbour,observed,null_mean,null_std,z,n_ge,n_le"]
    for r, a in enumerate(names):
        for j, b in enumerate(names):
            lines.append(f"{a},{b},{int(observed[r][j])},{float(stats['mean'][r][j]):.17g},{float(stats['std'][r][j]):.17g},{float(stats['z'][r][j]):.17g},"
                         f"{int(stats['n_ge'][r][j])},{int(stats['n_le'][r][j])}")
    return "\n".join(lines) + "\n"
