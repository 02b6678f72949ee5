"""Host side of the per-cell marker intensity table (Annotator.cell_intensities): from the area, the fp64 ``[sum, ssd]`` and the bracketing
order statistics of ops.cell_intensities (csrc/intensities.hip; include/ribca_hip.h states the summation order and the ranks) the columns
steinbock's ``measure intensities`` writes -- mean, spread, min, quartiles, max of every marker over the cell's OWN pixels -- the per-type
summary, the robustly standardised type medians and the comparison with the window table ``ImageProcessor.intensity_full``.  Everything in fp64;
no torch here.  DESIGN.md section 21."""
from __future__ import annotations

import re
from typing import List, Sequence

import numpy as np

#: the quantiles Annotator.cell_intensities asks for: min, quartiles, max
Q_NUM = (0, 1, 2, 3, 4)
Q_DEN = 4
#: the columns of ``type_summary``
SUMMARY = ("n", "mean_of_means", "median_of_means", "median_of_medians")
#: the standardised-medians figure saturates at this many robust standard deviations: a fixed scale
Z_LIMIT = 3.0
#: MAD -> standard deviation of a normal distribution
MAD_SCALE = 1.4826


def statistic_names(q_num: Sequence[int] = Q_NUM, q_den: int = Q_DEN) -> List[str]:
    """the statistics of ``features`` in column order: ``mean``, ``std`` and one name per quantile -- ``min`` for 0, ``max`` for 1, ``median``,
    ``q25``, ``q75`` for 1/2, 1/4, 3/4, and ``q{num}of{den}`` for any other"""
    names = ["mean", "std"]
    den = int(q_den)
    for num in (int(v) for v in q_num):
        if num == 0:
            names.append("min")
        elif num == den:
            names.append("max")
        elif 2 * num == den:
            names.append("median")
        elif 4 * num == den:
            names.append("q25")
        elif 4 * num == 3 * den:
            names.append("q75")
        else:
            names.append(f"q{num}of{den}")
    return names


def features(area, sums, order, q_num: Sequence[int] = Q_NUM, q_den: int = Q_DEN) -> np.ndarray:
    """(n, C, 2 + Q) fp64, the columns of ``statistic_names``, from ``area`` (n), ``sums`` (n, C, 2) and ``order`` (n, C, Q, 2).  With a = the
    area, (sum, ssd) = sums[i, c] and (lo, hi) = order[i, c, k] widened to fp64:

    * ``mean = sum / a``; ``std = sqrt(ssd / a)`` (population, as ``np.std``);
    * quantile k, with ``h = (a - 1) q_num[k]`` in integers: ``lo + (hi - lo) * (h % q_den) / q_den`` -- numpy's linear interpolation at
      ``q_num[k] / q_den``; exactly ``lo`` where the rank is whole;
    * every value is reported on the scale of ``ImageProcessor.intensity_full``: ``(x + 1) / 2`` for the mean and the quantiles, ``x / 2`` for the
      std, unconditionally, as preprocess.py does.

    A cell without a pixel (a = 0) has NaN in every column."""
    a = np.asarray(area).astype(np.int64).reshape(-1)
    n = len(a)
    q = np.asarray(q_num).astype(np.int64).reshape(-1)
    den = int(q_den)
    s = np.asarray(sums, dtype=np.float64)
    o = np.asarray(order).astype(np.float64)
    if s.ndim != 3 or s.shape[0] != n or s.shape[2] != 2 or o.shape != (n, s.shape[1], len(q), 2):
        raise ValueError(f"features takes sums (n, C, 2) and order (n, C, {len(q)}, 2) for n = {n} cells, got {s.shape} and {o.shape}")
    out = np.full((n, s.shape[1], 2 + len(q)), np.nan)
    full = a > 0
    count = a[full].astype(np.float64)[:, None]
    out[full, :, 0] = (s[full, :, 0] / count + 1.0) / 2.0
    out[full, :, 1] = np.sqrt(s[full, :, 1] / count) / 2.0
    rest = ((a[full] - 1)[:, None] * q[None, :]) % den      # (cells, Q), exact in int64
    lo, hi = o[full, :, :, 0], o[full, :, :, 1]
    with np.errstate(invalid="ignore"):      # inf - inf of an infinite pixel: NaN, as numpy's own quantile gives
        value = lo + (hi - lo) * rest[:, None, :].astype(np.float64) / float(den)
    value = np.where(rest[:, None, :] == 0, lo, value)
    out[full, :, 2:] = (value + 1.0) / 2.0
    return out


def _name(names: Sequence[str], label: int) -> str:
    return str(names[label]) if 0 <= label < len(names) else ""


def _num(v) -> str:
    return f"{float(v):.17g}"


def cells_csv(cell_ids, types, names: Sequence[str], area, markers: Sequence[str], stats: Sequence[str], feat) -> str:
    """one line per cell in ``cell_ids`` order: ``id``, ``cell type``, ``area`` and ``{marker}_{stat}`` per marker and statistic; floats with 17
    significant digits, NaN as ``nan``"""
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    a = np.asarray(area).astype(np.int64).reshape(-1)
    f = np.asarray(feat, dtype=np.float64)
    n = len(ids)
    if lab.shape != (n,) or a.shape != (n,) or f.shape != (n, len(markers), len(stats)):
        raise ValueError(f"cells_csv takes n labels, n areas and an (n, {len(markers)}, {len(stats)}) table for n = {n} cells, got {f.shape}")
    lines = ["id,cell type,area," + ",".join(f"{m}_{s}" for m in markers for s in stats)]
    for i in range(n):
        lines.append(f"{int(ids[i])},{_name(names, int(lab[i]))},{int(a[i])}," + ",".join(_num(v) for v in f[i].reshape(-1)))
    return "\n".join(lines) + "\n"


def type_summary(types, n_types: int, means, medians) -> np.ndarray:
    """(T, C, 4) fp64, SUMMARY per cell type and marker over the type's cells with a finite mean: their number, the mean and the median of the
    per-cell means, the median of the per-cell medians; NaN where a type has no such cell"""
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    m = np.asarray(means, dtype=np.float64)
    d = np.asarray(medians, dtype=np.float64)
    if m.ndim != 2 or m.shape != d.shape or len(m) != len(lab):
        raise ValueError(f"type_summary takes (n, C) means and medians for n = {len(lab)} labels, got {m.shape} and {d.shape}")
    t = int(n_types)
    out = np.full((t, m.shape[1], len(SUMMARY)), np.nan)
    for a in range(t):
        for c in range(m.shape[1]):
            ok = (lab == a) & np.isfinite(m[:, c])
            out[a, c, 0] = ok.sum()
            if ok.any():
                out[a, c, 1:] = (m[ok, c].mean(), np.median(m[ok, c]), np.median(d[ok, c]))
    return out


def summary_csv(names: Sequence[str], markers: Sequence[str], table) -> str:
    """long form, one line per (cell type, marker): ``cell_type,marker,n,mean_of_means,median_of_means,median_of_medians``"""
    s = np.asarray(table)
    if s.shape != (len(names), len(markers), len(SUMMARY)):
        raise ValueError(f"summary_csv takes a (T, C, {len(SUMMARY)}) table for T names and C markers, got {s.shape}")
    lines = ["cell_type,marker," + ",".join(SUMMARY)]
    for a, cell_type in enumerate(names):
        for c, marker in enumerate(markers):
            lines.append(f"{cell_type},{marker},{int(s[a, c, 0])}," + ",".join(_num(v) for v in s[a, c, 1:]))
    return "\n".join(lines) + "\n"


def standardised_medians(types, n_types: int, means) -> np.ndarray:
    """(T, C) fp64: ``(median_t - median_all) / (1.4826 MAD_all)`` of the per-cell means of every marker -- median_t over the type's cells,
    median_all and ``MAD_all = median |x - median_all|`` over all cells, each over the cells with a finite mean; 0 where MAD_all is 0, NaN for a
    type without such a cell"""
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    m = np.asarray(means, dtype=np.float64)
    if m.ndim != 2 or len(m) != len(lab):
        raise ValueError(f"standardised_medians takes (n, C) means for n = {len(lab)} labels, got {m.shape}")
    t = int(n_types)
    out = np.full((t, m.shape[1]), np.nan)
    for c in range(m.shape[1]):
        ok = np.isfinite(m[:, c])
        if not ok.any():
            continue
        centre = np.median(m[ok, c])
        spread = MAD_SCALE * np.median(np.abs(m[ok, c] - centre))
        for a in range(t):
            x = m[ok & (lab == a), c]
            if len(x):
                out[a, c] = (np.median(x) - centre) / spread if spread > 0.0 else 0.0
    return out


def matrix_csv(names: Sequence[str], markers: Sequence[str], z) -> str:
    """the standardised medians as a matrix: ``cell_type`` and one column per marker"""
    m = np.asarray(z)
    if m.shape != (len(names), len(markers)):
        raise ValueError(f"matrix_csv takes a (T, C) matrix for T names and C markers, got {m.shape}")
    lines = ["cell_type," + ",".join(str(c) for c in markers)]
    for a, cell_type in enumerate(names):
        lines.append(f"{cell_type}," + ",".join(_num(v) for v in m[a]))
    return "\n".join(lines) + "\n"


def vs_window(mask_means, intensity_full) -> np.ndarray:
    """(C, 3) fp64: per marker Pearson's r between the exact mask mean and the window table, and the mean and the max of ``|mask mean - window|``,
    over the cells where both are finite; r is NaN where either column is constant, everything NaN where no cell is left"""
    x = np.asarray(mask_means, dtype=np.float64)
    y = np.asarray(intensity_full, dtype=np.float64)
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError(f"vs_window takes two (n, C) tables, got {x.shape} and {y.shape}")
    out = np.full((x.shape[1], 3), np.nan)
    for c in range(x.shape[1]):
        ok = np.isfinite(x[:, c]) & np.isfinite(y[:, c])
        if not ok.any():
            continue
        u, v = x[ok, c], y[ok, c]
        du, dv = u - u.mean(), v - v.mean()
        suu, svv = float((du * du).sum()), float((dv * dv).sum())
        if suu > 0.0 and svv > 0.0:
            out[c, 0] = float((du * dv).sum()) / np.sqrt(suu * svv)
        diff = np.abs(u - v)
        out[c, 1], out[c, 2] = diff.mean(), diff.max()
    return out


def vs_window_csv(markers: Sequence[str], table) -> str:
    """``marker,pearson_r,mean_abs_difference,max_abs_difference``, one line per marker"""
    t = np.asarray(table)
    if t.shape != (len(markers), 3):
        raise ValueError(f"vs_window_csv takes a (C, 3) table for C markers, got {t.shape}")
    lines = ["marker,pearson_r,mean_abs_difference,max_abs_difference"]
    for c, marker in enumerate(markers):
        lines.append(f"{marker}," + ",".join(_num(v) for v in t[c]))
    return "\n".join(lines) + "\n"


def colour_index(mean) -> np.ndarray:
    """uint8, same shape: the entry of the colour table of a marker's map, int(clip(mean, 0, 1) * 255); NaN -> 0"""
    v = np.nan_to_num(np.asarray(mean, dtype=np.float64), nan=0.0)
    return (np.clip(v, 0.0, 1.0) * 255.0).astype(np.int64).astype(np.uint8)


def file_slug(marker: str) -> str:
    """a marker name as part of a file name: every character outside [A-Za-z0-9] becomes ``_``"""
    return re.sub(r"[^A-Za-z0-9]", "_", str(marker))
