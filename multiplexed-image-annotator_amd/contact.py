"""Host side of the cell contact graph (Annotator.contact_analysis): from the directed edge list of ops.contact_graph (csrc/contact.hip: two
cells are in contact when pixels of their masks lie within a few pixels of each other; ``pairs`` = the ordered pixel pairs within that reach) the
observed type-pair counts, the CSVs of the edges, the cells and the type pairs, and the colour index of the degree map.  The z-scores against
the label-permutation null of ops.edge_perm_counts are enrichment.z_scores, unchanged: histoCAT's neighbourhood analysis on the graph it was
defined on.  No p-value is formed: the permutations at or above / at or below the observed count are reported as they are.  No torch here.
DESIGN.md section 19."""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .cooccurrence import slug

#: the degree at which the degree map saturates: a fixed scale, so that maps compare across images
DEGREE_SCALE = 12

#: offsets of the Euclidean disk of radius d, the pixel itself excluded, for d = 1 .. 8
DISK_OFFSETS = (4, 12, 28, 48, 80, 112, 148, 196)


def default_seed() -> int:
    """RIBCA_CONTACT_SEED overrides the default seed 0; read at every call."""
    v = os.environ.get("RIBCA_CONTACT_SEED")
    return int(v) if v not in (None, "") else 0


def _edge_arrays(src, dst, pairs):
    s = np.asarray(src).astype(np.int64).reshape(-1)
    d = np.asarray(dst).astype(np.int64).reshape(-1)
    w = np.asarray(pairs).astype(np.int64).reshape(-1)
    if d.shape != s.shape or w.shape != s.shape:
        raise ValueError(f"an edge list takes three arrays of one length, got {s.shape}, {d.shape}, {w.shape}")
    return s, d, w


def observed(src, dst, pairs, types, n_types: int) -> Tuple[np.ndarray, np.ndarray]:
    """(edges, pixel_pairs), both (T, T) int64: the directed edges and the sum of their pixel pairs by (type of src, type of dst); an edge with
    an end whose label lies outside [0, T) is skipped, as ops.edge_perm_counts skips it"""
    s, d, w = _edge_arrays(src, dst, pairs)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    t = int(n_types)
    a, b = lab[s], lab[d]
    ok = (a >= 0) & (a < t) & (b >= 0) & (b < t)
    flat = a[ok] * t + b[ok]
    edges = np.bincount(flat, minlength=t * t).astype(np.int64).reshape(t, t)
    total = np.zeros(t * t, dtype=np.int64)
    np.add.at(total, flat, w[ok])      # bincount's weights are doubles; these sums stay integers
    return edges, total.reshape(t, t)


def neighbours_by_type(src, dst, types, n_cells: int, n_types: int) -> np.ndarray:
    """(n, T) int64: the contact neighbours of every cell by their type"""
    s = np.asarray(src).astype(np.int64).reshape(-1)
    d = np.asarray(dst).astype(np.int64).reshape(-1)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    t = int(n_types)
    b = lab[d]
    ok = (b >= 0) & (b < t)
    return np.bincount(s[ok] * t + b[ok], minlength=int(n_cells) * t).astype(np.int64).reshape(int(n_cells), t)


def _name(names: Sequence[str], label: int) -> str:
    return str(names[label]) if 0 <= label < len(names) else ""


def edges_csv(cell_ids, types, names: Sequence[str], src, dst, pairs) -> str:
    """every undirected contact once, the lower mask label first: ``cell_id_a,cell_id_b,cell_type_a,cell_type_b,pixel_pairs`` in (a, b) order"""
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    s, d, w = _edge_arrays(src, dst, pairs)
    keep = ids[s] < ids[d]
    rows = sorted(zip(ids[s[keep]].tolist(), ids[d[keep]].tolist(), lab[s[keep]].tolist(), lab[d[keep]].tolist(), w[keep].tolist()))
    lines = ["cell_id_a,cell_id_b,cell_type_a,cell_type_b,pixel_pairs"]
    lines += [f"{a},{b},{_name(names, ta)},{_name(names, tb)},{p}" for a, b, ta, tb, p in rows]
    return "\n".join(lines) + "\n"


def cells_csv(cell_ids, types, names: Sequence[str], src, dst, pairs, degree) -> str:
    """one line per cell in ``cell_ids`` order: ``cell_id,cell_type,degree,pixel_pairs`` (the sum over its contacts) and one ``n_{slug}`` per
    cell type, the contact neighbours of that type"""
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    deg = np.asarray(degree).astype(np.int64).reshape(-1)
    s, d, w = _edge_arrays(src, dst, pairs)
    n, t = len(ids), len(names)
    if lab.shape != (n,) or deg.shape != (n,):
        raise ValueError(f"cells_csv takes n labels and n degrees for n cells, got {lab.shape} and {deg.shape} for {n}")
    total = np.zeros(n, dtype=np.int64)
    np.add.at(total, s, w)
    by_type = neighbours_by_type(s, d, lab, n, t)
    lines = ["cell_id,cell_type,degree,pixel_pairs" + "".join(f",n_{slug(c)}" for c in names)]
    for i in range(n):
        lines.append(f"{int(ids[i])},{_name(names, int(lab[i]))},{int(deg[i])},{int(total[i])}" + "".join(f",{int(v)}" for v in by_type[i]))
    return "\n".join(lines) + "\n"


def table_csv(names: Sequence[str], edges, pixel_pairs, stats: Optional[Dict[str, np.ndarray]] = None) -> str:
    """long form, one line per (cell type, neighbour type): the directed edges and their pixel pairs; with a null (``stats`` of
    enrichment.z_scores over the edge counts) its mean, std, z and the permutations at or above / at or below.  Floats with 17 significant
    digits."""
    e = np.asarray(edges)
    w = np.asarray(pixel_pairs)
    t = len(names)
    if e.shape != (t, t) or w.shape != (t, t):
        raise ValueError(f"table_csv takes two (T, T) tables for T names, got {e.shape} and {w.shape} for {t}")
    lines = ["cell_type,neighbour,edges,pixel_pairs" + (",null_mean,null_std,z,n_ge,n_le" if stats is not None else "")]
    for r, a in enumerate(names):
        for j, b in enumerate(names):
            line = f"{a},{b},{int(e[r][j])},{int(w[r][j])}"
            if stats is not None:
                line += (f",{float(stats['mean'][r][j]):.17g},{float(stats['std'][r][j]):.17g},{float(stats['z'][r][j]):.17g},"
                         f"{int(stats['n_ge'][r][j])},{int(stats['n_le'][r][j])}")
            lines.append(line)
    return "\n".join(lines) + "\n"


def nan_stats(n_types: int) -> Dict[str, np.ndarray]:
    """the statistics of a group without an edge: nothing was permuted, every float is NaN and the two counts are 0"""
    shape = (int(n_types), int(n_types))
    nan = np.full(shape, np.nan)
    return {"mean": nan, "std": nan.copy(), "z": nan.copy(), "n_ge": np.zeros(shape, dtype=np.int64), "n_le": np.zeros(shape, dtype=np.int64)}


def row_normalised(pixel_pairs) -> np.ndarray:
    """(T, T) fp64: every row of the pixel-pair matrix over its sum -- the share of a type's contact surface that faces each type; a row
    without contact stays 0"""
    w = np.asarray(pixel_pairs).astype(np.float64)
    sums = w.sum(axis=1, keepdims=True)
    return np.divide(w, sums, out=np.zeros_like(w), where=sums > 0)


def degree_colour_index(degree) -> np.ndarray:
    """(n) uint8: the entry of the colour table for every cell of the degree map, int(min(degree / 12, 1) * 255)"""
    ratio = np.asarray(degree).astype(np.float64) / float(DEGREE_SCALE)
    return (np.minimum(ratio, 1.0) * 255.0).astype(np.int64).astype(np.uint8)
