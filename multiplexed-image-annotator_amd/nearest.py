"""Host side of the nearest cell of every type (Annotator.nearest_type_distances): from the (n, T) table of squared distances to the nearest
other cell of each type (ops.nearest_by_type; csrc/nearest.hip) the counts of cells per (radius band, anchor type, target type), the cross-type
nearest-neighbour distribution G_ab(r) = the fraction of a-cells whose nearest b-cell lies within r (spatstat's ``Gcross`` without edge
correction, scimap's ``spatial_distance`` summarised), its z-score against the label-permutation null of ops.nearest_perm_counts, and the two
CSVs.  No p-value is formed: the permutations at or above / at or below the observed count are reported as they are, as the neighbourhood
enrichment reports them.  No torch here.  DESIGN.md section 18."""
from __future__ import annotations

import math
import os
from typing import Dict, Optional, Sequence

import numpy as np

from .cooccurrence import slug


def default_seed() -> int:
    """RIBCA_NEAREST_SEED overrides the default seed 0; read at every call."""
    v = os.environ.get("RIBCA_NEAREST_SEED")
    return int(v) if v not in (None, "") else 0


def observed_counts(near2, types, n_types: int, r2) -> np.ndarray:
    """(B, T, T) int64: counts[band][a][b] = the cells of type a whose squared distance to the nearest b-cell lies in r2[band - 1] < m <= r2[band]
    (band 0: m <= r2[0]); beyond r2[-1], or +inf, nothing; a label outside [0, T) is no anchor.  Plain comparisons on the very doubles the
    kernel wrote: what ops.nearest_perm_counts counts under the identity labelling."""
    m = np.asarray(near2, dtype=np.float64)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    edges = np.asarray(r2, dtype=np.float64).reshape(-1)
    t = int(n_types)
    if m.shape != (len(lab), t):
        raise ValueError(f"observed_counts takes an (n, T) table for n labels, got {m.shape} for {len(lab)} labels and T = {t}")
    out = np.zeros((len(edges), t, t), dtype=np.int64)
    anchor = (lab >= 0) & (lab < t)
    for band in range(len(edges)):
        inside = m <= edges[band]
        if band > 0:
            inside &= m > edges[band - 1]
        inside &= anchor[:, None]
        for a in np.unique(lab[anchor]):
            out[band, a] = inside[lab == a].sum(axis=0)
    return out


def statistics(observed, null, anchors_present) -> Dict[str, np.ndarray]:
    """observed (B, T, T) integer counts per band, null (P, B, T, T) or None, anchors_present (T) = the cells of each type ->
    ``cumulative`` (B, T, T) int64, the running sums over the bands, and ``G`` = cumulative / n_a, NaN where n_a is 0.  With a null, on ITS
    running sums: ``mean`` = fsum(v) / P, ``std`` = sqrt(fsum((v - mean)^2) / P) (the population std), ``z`` = (cumulative - mean) / std and
    NaN where std is 0, ``n_ge`` / ``n_le`` = the permutations whose cumulative count is >= / <= the observed one."""
    obs = np.asarray(observed)
    present = np.asarray(anchors_present).reshape(-1)
    if obs.ndim != 3 or obs.shape[1] != obs.shape[2] or obs.dtype.kind not in "iu" or present.shape != (obs.shape[1],):
        raise ValueError(f"statistics takes (B, T, T) integer counts and T anchor counts, got {obs.dtype} {obs.shape} and {present.shape}")
    cum = np.cumsum(obs.astype(np.int64), axis=0)
    g = np.full(obs.shape, np.nan, dtype=np.float64)
    for a in range(obs.shape[1]):
        if int(present[a]) > 0:
            g[:, a, :] = cum[:, a, :] / float(int(present[a]))
    out = {"cumulative": cum, "G": g}
    if null is None:
        return out
    perm = np.asarray(null)
    if perm.ndim != 4 or perm.shape[0] < 1 or perm.shape[1:] != obs.shape or perm.dtype.kind not in "iu":
        raise ValueError(f"statistics takes (P, B, T, T) integer permutation counts with P >= 1, got {perm.dtype} {perm.shape}")
    p = int(perm.shape[0])
    pc = np.cumsum(perm.astype(np.int64), axis=1)
    mean = np.empty(obs.shape, dtype=np.float64)
    std = np.empty(obs.shape, dtype=np.float64)
    for pos in np.ndindex(*obs.shape):
        vals = [float(v) for v in pc[(slice(None),) + pos]]
        mu = math.fsum(vals) / p
        mean[pos] = mu
        std[pos] = math.sqrt(math.fsum((v - mu) * (v - mu) for v in vals) / p)
    z = np.full(obs.shape, np.nan)
    ok = std > 0.0
    z[ok] = (cum[ok].astype(np.float64) - mean[ok]) / std[ok]
    out.update({"mean": mean, "std": std, "z": z, "n_ge": (pc >= cum[None]).sum(axis=0).astype(np.int64),
                "n_le": (pc <= cum[None]).sum(axis=0).astype(np.int64)})
    return out


def cells_csv(cell_ids, types, names: Sequence[str], near2, arg) -> str:
    """one line per cell: ``cell_id``, ``cell_type`` and per target type ``d_{slug}`` = sqrt(near2) with 17 significant digits (the text parses
    back to the same double; ``inf`` where there is no such cell) and ``id_{slug}`` = the id of that nearest cell (empty where there is none)"""
    ids = np.asarray(cell_ids).reshape(-1)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    m = np.asarray(near2, dtype=np.float64)
    who = np.asarray(arg).astype(np.int64)
    t = len(names)
    if m.shape != (len(ids), t) or who.shape != m.shape or len(lab) != len(ids):
        raise ValueError(f"cells_csv takes (n, T) tables for n cells and T names, got {m.shape}, {who.shape}, {len(ids)} cells, {t} names")
    d = np.sqrt(m)
    slugs = [slug(c) for c in names]
    lines = ["cell_id,cell_type," + ",".join(f"d_{s},id_{s}" for s in slugs)]
    for i in range(len(ids)):
        name = names[lab[i]] if 0 <= lab[i] < t else ""
        cols = ",".join(f"{float(d[i, b]):.17g},{int(ids[who[i, b]]) if who[i, b] >= 0 else ''}" for b in range(t))
        lines.append(f"{int(ids[i])},{name},{cols}")
    return "\n".join(lines) + "\n"


def table_csv(names: Sequence[str], radii, observed, anchors_present, stats: Optional[Dict[str, np.ndarray]] = None) -> str:
    """long form, one line per (anchor type, target type, band): the anchor cells, the outer radius, the count of the band, the cumulative count
    and G; with a null (``stats`` of ``statistics`` holding ``z``) its mean, std, z and the permutations at or above / at or below.  The floats
    with 17 significant digits."""
    obs = np.asarray(observed)
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    present = np.asarray(anchors_present).reshape(-1)
    if obs.ndim != 3 or r.size != obs.shape[0] or len(names) != obs.shape[1] or obs.shape[1] != obs.shape[2] or present.shape != (len(names),):
        raise ValueError(f"{r.size} radii, {len(names)} names and {present.shape} anchor counts for counts of shape {obs.shape}")
    if stats is None:
        stats = statistics(obs, None, present)
    with_null = "z" in stats
    head = "anchor,target,anchor_cells,r,count,cum_count,G"
    lines = [head + (",null_mean,null_std,z,n_ge,n_le" if with_null else "")]
    for a, first in enumerate(names):
        for b, second in enumerate(names):
            for k in range(r.size):
                pos = (k, a, b)
                line = (f"{first},{second},{int(present[a])},{float(r[k]):.17g},{int(obs[pos])},{int(stats['cumulative'][pos])},"
                        f"{float(stats['G'][pos]):.17g}")
                if with_null:
                    line += (f",{float(stats['mean'][pos]):.17g},{float(stats['std'][pos]):.17g},{float(stats['z'][pos]):.17g},"
                             f"{int(stats['n_ge'][pos])},{int(stats['n_le'][pos])}")
                lines.append(line)
    return "\n".join(lines) + "\n"


def distance_colour_index(near2_column, r_max: float) -> np.ndarray:
    """(n) uint8: the entry of the colour table for every cell of a distance map, int(min(d / r_max, 1) * 255) with d = sqrt(near2)"""
    d = np.sqrt(np.asarray(near2_column, dtype=np.float64))
    ratio = d / float(r_max) if r_max > 0 else np.where(d > 0.0, 1.0, 0.0)      # a single radius of 0: the duplicates against the rest
    return (np.minimum(ratio, 1.0) * 255.0).astype(np.int64).astype(np.uint8)
