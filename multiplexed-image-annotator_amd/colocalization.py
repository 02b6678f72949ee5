"""Host side of the marker colocalisation table (Annotator.marker_colocalization): from the area, the counts above both gates, the fp64 sums,
the centred cross products and the gated sums of ops.cell_coloc (csrc/colocalization.hip; include/ribca_hip.h states the pixel set, the gates
and the summation order) Pearson's r, the Manders overlap coefficient, the Manders fractions M1 and M2, the share of the cell above both gates
and the Jaccard index of the two gated pixel sets, per cell and marker pair; the per-type summary; the matrix of median r.  What CellProfiler's
MeasureColocalization reports per object.  Everything in fp64; no torch here.  DESIGN.md section 27."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import intensities, localization

#: the default gate, CellProfiler's "15 % of the maximum", taken here of the normalised scale u = (x + 1) / 2 of ``intensity_full``
THRESHOLD = 0.15
#: the most markers one call correlates (ops.COLOC_MAX_MARKERS: a gate word of the kernel is 32 bits)
MAX_MARKERS = 32
#: the per-cell and per-pair columns of ``features``, in the order of ``pairs_csv``
STATS = ("r", "overlap", "m1", "m2", "both", "both_fraction", "jaccard")
#: the columns of ``summary``
SUMMARY = ("n", "n_valid", "mean_r", "median_r", "median_overlap", "median_m1", "median_m2", "mean_both_fraction")
#: the scale of the r map and of the median-r figures
LIMIT = localization.LIMIT


def all_pairs(k: int) -> List[Tuple[int, int]]:
    """the pairs (a, b), a <= b, in the column order of ops.cell_coloc: (0,0), (0,1) .. (0,k-1), (1,1) .."""
    return [(a, b) for a in range(int(k)) for b in range(a, int(k))]


def off_pairs(k: int) -> List[Tuple[int, int]]:
    """the pairs a < b in the same order: the columns of every table here, P' = k (k - 1) / 2 of them"""
    return [(a, b) for a in range(int(k)) for b in range(a + 1, int(k))]


def pair_names(markers: Sequence[str]) -> List[str]:
    """``{A}~{B}`` for every pair of ``off_pairs``"""
    return [f"{markers[a]}~{markers[b]}" for a, b in off_pairs(len(markers))]


def check_threshold(threshold) -> float:
    """``threshold`` as a float; ValueError unless 0 <= threshold < 1 (a number, no bool)"""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not 0.0 <= float(threshold) < 1.0:
        raise ValueError(f"threshold must be a number T with 0 <= T < 1 on the normalised scale, got {threshold!r}")
    return float(threshold)


def gates(threshold, k: int) -> np.ndarray:
    """(k) fp32: the gate T of the scale u = (x + 1) / 2 on the image's own scale x, ``np.float32(2 T - 1)``, once per selected channel"""
    t = check_threshold(threshold)
    return np.full(int(k), np.float32(2.0 * t - 1.0), dtype=np.float32)


def parse_pairs(pairs, markers: Sequence[str]) -> List[int]:
    """the columns (indices into ``off_pairs``) of the named pairs ``"A:B"``, in the order given, each once; ``B:A`` names the column of
    ``A~B``.  ValueError for a name that is not two different markers of ``markers`` joined by one colon, or for a pair named twice"""
    names = [str(m) for m in markers]
    cols = {q: j for j, q in enumerate(off_pairs(len(names)))}
    out: List[int] = []
    for item in ([] if pairs is None else list(pairs)):
        parts = str(item).split(":")
        if len(parts) != 2 or not parts[0] or not parts[1]:
            raise ValueError(f"a pair is two marker names joined by a colon, A:B, got {item!r}")
        for name in parts:
            if names.count(name) != 1:
                raise ValueError(f"pair {item!r}: {name!r} is not one of the markers {names}")
        a, b = names.index(parts[0]), names.index(parts[1])
        if a == b:
            raise ValueError(f"pair {item!r} names one marker twice")
        col = cols[(min(a, b), max(a, b))]
        if col in out:
            raise ValueError(f"pair {item!r} is named twice")
        out.append(col)
    return out


def features(area, both, sums, cross, gated) -> Dict[str, np.ndarray]:
    """From ``area`` (n), ``both`` (n, P), ``sums`` (n, K), ``cross`` (n, P) and ``gated`` (n, K, K) of ops.cell_coloc, P = K (K + 1) / 2 in the
    order of ``all_pairs``.  With a = area, S = sums, X = cross, G = gated, B = both of one cell, for every pair k < l of ``off_pairs`` (the
    columns of every array returned, (n, K (K - 1) / 2) fp64, ``both`` int64):

    * ``r`` = X_kl / sqrt(X_kk X_ll), clamped to [-1, 1]: Pearson's r over the cell's pixels, the same on the image's scale x and on the
      reported scale u = (x + 1) / 2.  NaN when a < 2 or X_kk or X_ll is 0 (a marker constant over the cell);
    * ``overlap`` = R_kl / sqrt(R_kk R_ll) with R_kl = (X_kl + S_k S_l / a + S_k + S_l + a) / 4, the raw second moment sum u_k u_l: the Manders
      overlap coefficient.  NaN when a = 0 or R_kk or R_ll is <= 0;
    * ``m1`` = ((G[k][l] + B_ll) / 2) / ((S_k + a) / 2): the share of marker k's intensity (on the u scale) that lies on the pixels where
      marker l is above its gate; ``m2`` = ((G[l][k] + B_kk) / 2) / ((S_l + a) / 2) is the mirror image.  Each is NaN when a = 0 or its
      denominator is <= 0;
    * ``both`` = B_kl, ``both_fraction`` = B_kl / a (NaN when a = 0), ``jaccard`` = B_kl / (B_kk + B_ll - B_kl) (NaN at 0 / 0)."""
    a_int = np.asarray(area).astype(np.int64).reshape(-1)
    b = np.asarray(both).astype(np.int64)
    s = np.asarray(sums, dtype=np.float64)
    x = np.asarray(cross, dtype=np.float64)
    g = np.asarray(gated, dtype=np.float64)
    n = len(a_int)
    if s.ndim != 2 or len(s) != n:
        raise ValueError(f"features takes sums (n, K) for n = {n} cells, got {s.shape}")
    k = s.shape[1]
    p = k * (k + 1) // 2
    if b.shape != (n, p) or x.shape != (n, p) or g.shape != (n, k, k):
        raise ValueError(f"features takes both and cross (n, {p}) and gated (n, {k}, {k}) for n = {n} cells, got {b.shape}, {x.shape} and {g.shape}")
    at = {q: j for j, q in enumerate(all_pairs(k))}
    off = off_pairs(k)
    a = a_int.astype(np.float64)
    out = {key: np.full((n, len(off)), np.nan) for key in STATS if key != "both"}
    out["both"] = np.zeros((n, len(off)), dtype=np.int64)
    some = a_int > 0
    with np.errstate(all="ignore"):
        for j, (kk, ll) in enumerate(off):
            xkl, xkk, xll = x[:, at[(kk, ll)]], x[:, at[(kk, kk)]], x[:, at[(ll, ll)]]
            sk, sl = s[:, kk], s[:, ll]
            bkl, bkk, bll = b[:, at[(kk, ll)]], b[:, at[(kk, kk)]], b[:, at[(ll, ll)]]
            out["both"][:, j] = bkl
            ok = (a_int >= 2) & (xkk > 0.0) & (xll > 0.0)
            out["r"][ok, j] = np.minimum(1.0, np.maximum(-1.0, xkl[ok] / np.sqrt(xkk[ok] * xll[ok])))
            rkl = (xkl + sk * sl / a + sk + sl + a) / 4.0
            rkk = (xkk + sk * sk / a + sk + sk + a) / 4.0
            rll = (xll + sl * sl / a + sl + sl + a) / 4.0
            ok = some & (rkk > 0.0) & (rll > 0.0)
            out["overlap"][ok, j] = rkl[ok] / np.sqrt(rkk[ok] * rll[ok])
            den = (sk + a) / 2.0
            ok = some & (den > 0.0)
            out["m1"][ok, j] = ((g[ok, kk, ll] + bll[ok].astype(np.float64)) / 2.0) / den[ok]
            den = (sl + a) / 2.0
            ok = some & (den > 0.0)
            out["m2"][ok, j] = ((g[ok, ll, kk] + bkk[ok].astype(np.float64)) / 2.0) / den[ok]
            out["both_fraction"][some, j] = bkl[some].astype(np.float64) / a[some]
            union = bkk + bll - bkl
            ok = union > 0
            out["jaccard"][ok, j] = bkl[ok].astype(np.float64) / union[ok].astype(np.float64)
    return out


_name = intensities._name
_num = intensities._num


def cells_csv(cell_ids, types, names: Sequence[str], markers: Sequence[str], area, r) -> str:
    """one line per cell in ``cell_ids`` order: ``id``, ``cell type``, ``area`` and ``{A}~{B}_r`` for every pair of ``off_pairs``; floats with
    17 significant digits, NaN as ``nan``, as intensities.cells_csv"""
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    ar = np.asarray(area).astype(np.int64).reshape(-1)
    n, cols = len(ids), pair_names(markers)
    table = np.asarray(r, dtype=np.float64).reshape(n, -1) if n else np.zeros((0, len(cols)))
    if lab.shape != (n,) or ar.shape != (n,) or table.shape != (n, len(cols)):
        raise ValueError(f"cells_csv takes n labels, n areas and an (n, {len(cols)}) table for n = {n} cells, got {table.shape}")
    lines = [",".join(["id", "cell type", "area"] + [c + "_r" for c in cols])]
    for i in range(n):
        lines.append(",".join([str(int(ids[i])), _name(names, int(lab[i])), str(int(ar[i]))] + [_num(v) for v in table[i]]))
    return "\n".join(lines) + "\n"


def pairs_csv(cell_ids, types, names: Sequence[str], markers: Sequence[str], columns: Sequence[int], area, feat: Dict[str, np.ndarray]) -> str:
    """one line per cell: ``id``, ``cell type``, ``area`` and, per named pair (``columns`` from ``parse_pairs``), ``{A}~{B}_{stat}`` for every
    stat of STATS; ``both`` as an integer"""
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    ar = np.asarray(area).astype(np.int64).reshape(-1)
    n, cols = len(ids), pair_names(markers)
    if lab.shape != (n,) or ar.shape != (n,) or any(np.asarray(feat[s]).shape != (n, len(cols)) for s in STATS):
        raise ValueError(f"pairs_csv takes n labels, n areas and (n, {len(cols)}) tables for n = {n} cells")
    lines = [",".join(["id", "cell type", "area"] + [f"{cols[c]}_{s}" for c in columns for s in STATS])]
    for i in range(n):
        cells = [str(int(feat[s][i, c])) if s == "both" else _num(feat[s][i, c]) for c in columns for s in STATS]
        lines.append(",".join([str(int(ids[i])), _name(names, int(lab[i])), str(int(ar[i]))] + cells))
    return "\n".join(lines) + "\n"


def _median(v: np.ndarray) -> float:
    v = v[~np.isnan(v)]
    return float(np.median(v)) if len(v) else float("nan")


def summary(types, n_types: int, feat: Dict[str, np.ndarray]) -> np.ndarray:
    """(T, P', 8) fp64, SUMMARY per cell type and pair: the cells of the type, those of them with a valid (not NaN) r, the mean and the median
    of r over these, the medians of overlap, m1 and m2 and the mean of both_fraction, each over the type's cells where it is not NaN; NaN
    where none is left"""
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    r = np.asarray(feat["r"], dtype=np.float64)
    if r.ndim != 2 or len(r) != len(lab):
        raise ValueError(f"summary takes (n, P') tables for n = {len(lab)} labels, got {r.shape}")
    t = int(n_types)
    out = np.full((t, r.shape[1], len(SUMMARY)), np.nan)
    for a in range(t):
        of_type = lab == a
        for j in range(r.shape[1]):
            x = r[of_type, j]
            ok = x[~np.isnan(x)]
            out[a, j, 0], out[a, j, 1] = of_type.sum(), len(ok)
            if len(ok):
                out[a, j, 2], out[a, j, 3] = ok.mean(), np.median(ok)
            out[a, j, 4], out[a, j, 5], out[a, j, 6] = (_median(np.asarray(feat[s], dtype=np.float64)[of_type, j]) for s in ("overlap", "m1", "m2"))
            f = np.asarray(feat["both_fraction"], dtype=np.float64)[of_type, j]
            f = f[~np.isnan(f)]
            if len(f):
                out[a, j, 7] = f.mean()
    return out


def summary_csv(names: Sequence[str], markers: Sequence[str], table) -> str:
    """long form, one line per (cell type, pair): ``cell_type,marker_a,marker_b,`` and SUMMARY"""
    s = np.asarray(table)
    off = off_pairs(len(markers))
    if s.shape != (len(names), len(off), len(SUMMARY)):
        raise ValueError(f"summary_csv takes a (T, {len(off)}, {len(SUMMARY)}) table for T names, got {s.shape}")
    lines = ["cell_type,marker_a,marker_b," + ",".join(SUMMARY)]
    for a, cell_type in enumerate(names):
        for j, (k, l) in enumerate(off):
            lines.append(f"{cell_type},{markers[k]},{markers[l]},{int(s[a, j, 0])},{int(s[a, j, 1])}," + ",".join(_num(v) for v in s[a, j, 2:]))
    return "\n".join(lines) + "\n"


def median_matrix(r, k: int, rows=None) -> np.ndarray:
    """(K, K) fp64, symmetric: the median of r over the cells ``rows`` (a boolean (n) array; None: all cells) where it is not NaN, per pair;
    NaN where no cell is left; 1.0 on the diagonal"""
    x = np.asarray(r, dtype=np.float64)
    off = off_pairs(k)
    if x.ndim != 2 or x.shape[1] != len(off):
        raise ValueError(f"median_matrix takes an (n, {len(off)}) table of r for {k} markers, got {x.shape}")
    if rows is not None:
        x = x[np.asarray(rows, dtype=bool)]
    out = np.full((k, k), np.nan)
    for j, (a, b) in enumerate(off):
        out[a, b] = out[b, a] = _median(x[:, j])
    out[np.arange(k), np.arange(k)] = 1.0
    return out


def matrix_csv(markers: Sequence[str], matrix) -> str:
    """the median-r matrix: ``marker`` and one column per marker, one line per marker"""
    return intensities.matrix_csv(markers, markers, matrix).replace("cell_type,", "marker,", 1)


def colour_index(r) -> np.ndarray:
    """uint8, same shape: the entry of the diverging colour table of a pair's map, int(clip((r + 1) / 2, 0, 1) * 255); NaN -> 0"""
    return localization.colour_index(r)
