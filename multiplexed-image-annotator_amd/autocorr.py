"""Host side of the spatial autocorrelation of the markers (Annotator.spatial_autocorrelation): the seed, Moran's I and Geary's C from the
numerators of ops.autocorr_observed / ops.autocorr_perm (csrc/autocorr.hip), their permutation null and the CSV.  The statistics are those of
squidpy's ``spatial_autocorr`` over a k-NN graph with unit weights: with m neighbours per cell, n cells, z the centred values of a channel,
N = sum_i z_i sum_j z_j and G = sum_i sum_j (z_i - z_j)^2 over the neighbours j of i, and D = sum_i z_i^2,
    I = N / (m D),      C = (n - 1) G / (2 n m D).
DESIGN.md section 16."""
from __future__ import annotations

import math
import os
from typing import Dict, Sequence

import numpy as np

COLUMNS = "marker,cells,morans_i,i_null_mean,i_null_std,i_z,i_n_ge,i_n_le,gearys_c,c_null_mean,c_null_std,c_z,c_n_ge,c_n_le"


def default_seed() -> int:
    """RIBCA_AUTOCORR_SEED overrides the default seed 0; read at every call."""
    v = os.environ.get("RIBCA_AUTOCORR_SEED")
    return int(v) if v not in (None, "") else 0


def _against_null(observed: np.ndarray, null: np.ndarray, prefix: str, out: Dict[str, np.ndarray]) -> None:
    """observed (C), null (P, C): mean and population std of the null through math.fsum (exactly rounded sums: the order of the permutations
    does not matter), z = (observed - mean) / std and NaN where std is 0 or not a number; n_ge / n_le = the permutations at or above / at or
    below the observed value (a NaN compares false: 0)."""
    p, c = null.shape
    mean, std, z = np.empty(c), np.empty(c), np.full(c, np.nan)
    for k in range(c):
        col = [float(v) for v in null[:, k]]
        mean[k] = math.fsum(col) / p
        std[k] = math.sqrt(math.fsum([(v - mean[k]) * (v - mean[k]) for v in col]) / p)
        if std[k] > 0.0:
            z[k] = (observed[k] - mean[k]) / std[k]
    out[prefix] = observed
    out[prefix + "_null_mean"], out[prefix + "_null_std"], out[prefix + "_z"] = mean, std, z
    out[prefix + "_n_ge"] = (null >= observed[None]).sum(axis=0).astype(np.int64)
    out[prefix + "_n_le"] = (null <= observed[None]).sum(axis=0).astype(np.int64)


def statistics(obs, null, m2, cells: int, m: int) -> Dict[str, np.ndarray]:
    """obs (2, C) and null (P, 2, C): the numerators N (row 0) and G (row 1), observed and per permutation; m2 (C) = D, the sum of z^2 per
    channel; cells = n; m = the neighbours per cell.  Returns, per channel, ``i`` = N / (m D) and ``c`` = ((n - 1) G) / (2 n m D) (NaN where
    D == 0: a constant channel), and for each of the two the null's ``_null_mean`` and ``_null_std`` (population), ``_z`` and ``_n_ge`` /
    ``_n_le``.  No p-value is formed."""
    obs = np.asarray(obs, dtype=np.float64)
    null = np.asarray(null, dtype=np.float64)
    d = np.asarray(m2, dtype=np.float64)
    if obs.ndim != 2 or obs.shape[0] != 2 or null.ndim != 3 or null.shape[0] < 1 or null.shape[1:] != obs.shape or d.shape != obs.shape[1:]:
        raise ValueError(f"statistics takes (2, C) observed and (P, 2, C) permuted numerators with P >= 1 and (C) sums of squares, got {obs.shape}, "
                         f"{null.shape} and {d.shape}")
    n, m = int(cells), int(m)
    if n < 1 or m < 1:
        raise ValueError(f"statistics needs at least one cell and one neighbour, got {cells} and {m}")
    both = np.concatenate([obs[None], null])      # (1 + P, 2, C): the observed values and the null go through the same arithmetic
    with np.errstate(divide="ignore", invalid="ignore"):
        moran = np.where(d == 0.0, np.nan, both[:, 0] / (float(m) * d))
        geary = np.where(d == 0.0, np.nan, (float(n - 1) * both[:, 1]) / (2.0 * float(n) * float(m) * d))
    out: Dict[str, np.ndarray] = {}
    _against_null(moran[0], moran[1:], "i", out)
    _against_null(geary[0], geary[1:], "c", out)
    return out


def figure_values(stats: Dict[str, np.ndarray]) -> np.ndarray:
    """(C, 2): Moran's I and 1 - Geary's C per marker -- both positive for a structured channel, near 0 for salt and pepper"""
    return np.ascontiguousarray(np.stack([stats["i"], 1.0 - stats["c"]], axis=1))


def table_csv(markers: Sequence[str], cells: int, stats: Dict[str, np.ndarray]) -> str:
    """one line per marker; the floats with 17 significant digits (the text parses back to the same doubles)"""
    lines = [COLUMNS]
    for k, name in enumerate(markers):
        cols = [str(name), str(int(cells))]
        for s in ("i", "c"):
            cols += [f"{float(stats[s + t][k]):.17g}" for t in ("", "_null_mean", "_null_std", "_z")]
            cols += [str(int(stats[s + "_n_ge"][k])), str(int(stats[s + "_n_le"][k]))]
        lines.append(",".join(cols))
    return "\n".join(lines) + "\n"
