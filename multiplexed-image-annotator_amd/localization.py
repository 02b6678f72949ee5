"""Host side of the marker localisation table (Annotator.marker_localization): from the pixel counts, the deepest pixel and the fp64 sums per
depth shell of ops.cell_shell_sums (csrc/localization.hip; include/ribca_hip.h states the depth, the shells and the summation order) the mean of
every marker over the edge compartment and over the inner compartment of each cell, their contrast, the inscribed radius, the pooled profile
over the shells per cell type, and the per-type summary.  What CellProfiler's MeasureObjectIntensityDistribution reports, and the "membrane vs
interior" check of the MIBI pipelines.  Everything in fp64; no torch here.  DESIGN.md section 26."""
from __future__ import annotations

import math
from typing import Dict, List, Sequence

import numpy as np

from . import intensities

#: the outer edge of every shell but the last, in pixels of depth below the cell's edge: shell k holds EDGES[k-1] < depth <= EDGES[k], the last
#: shell everything deeper than EDGES[-1]
EDGES = (1, 2, 3, 4, 6, 8)
#: how far ops.mask_depth searches: beyond it a pixel is "deeper than DEPTH" (depth2 == -1) and lies in the last shell
DEPTH = 8
#: the columns of ``summary``
SUMMARY = ("n", "n_nan", "mean_contrast", "median_contrast")
#: the scale of the contrast map and of the median-contrast figure
LIMIT = 1.0

assert EDGES[-1] == DEPTH and all(a < b for a, b in zip(EDGES[:-1], EDGES[1:]))


def edges2() -> np.ndarray:
    """the squares of EDGES as int32: what ops.cell_shell_sums compares depth2 with"""
    return np.array([e * e for e in EDGES], dtype=np.int32)


def shell_names() -> List[str]:
    """``<=1``, ``<=2``, ... and ``>8``: the depth range of every shell, in pixels"""
    return [f"<={e}" for e in EDGES] + [f">{EDGES[-1]}"]


def check_band(band) -> int:
    """``band`` as an int; ValueError unless it is one of EDGES (an integer, no bool)"""
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or int(band) not in EDGES:
        raise ValueError(f"band must be one of the shell edges {EDGES} (pixels), got {band!r}")
    return int(band)


def features(count, deepest, sums, band) -> Dict[str, np.ndarray]:
    """From ``count`` (n, S), ``deepest`` (n) and ``sums`` (n, C, S), S = len(EDGES) + 1, for the band width ``band`` (one of EDGES, else
    ValueError).  With e = EDGES.index(band), the EDGE compartment of a cell is its shells 0 .. e -- the pixels at most ``band`` pixels below the
    cell's edge -- and the INNER compartment the shells e + 1 .. S - 1.  Returns

    * ``edge_area``, ``inner_area`` (n) int64: the counts of the compartment's shells added up; ``area`` their sum;
    * ``inradius`` (n): ``sqrt(deepest)``, the radius of the largest disc around a pixel of the cell that stays inside it; ``inf`` where
      deepest == -1 (deeper than DEPTH: the writers print ``>8``), NaN for a cell without a pixel (printed empty);
    * ``edge``, ``inner`` (n, C): the compartment's mean.  ``total`` starts at 0.0 and adds the sums of the compartment's shells in shell order;
      the mean is ``total / pixels`` and is reported as ``(mean + 1) / 2``, the scale of ``ImageProcessor.intensity_full`` and of
      intensities.features, unconditionally.  NaN for an empty compartment;
    * ``contrast`` (n, C): ``(edge - inner) / (edge + inner)`` of the two reported means: +1 all of the marker on the rim, -1 all inside, 0
      evenly spread.  NaN when either compartment is empty or ``edge + inner <= 0``."""
    b = check_band(band)
    cnt = np.asarray(count).astype(np.int64)
    deep = np.asarray(deepest).astype(np.int64).reshape(-1)
    s = np.asarray(sums, dtype=np.float64)
    n, shells = len(deep), len(EDGES) + 1
    if cnt.shape != (n, shells) or s.ndim != 3 or s.shape[0] != n or s.shape[2] != shells:
        raise ValueError(f"features takes count (n, {shells}) and sums (n, C, {shells}) for n = {n} cells, got {cnt.shape} and {s.shape}")
    cut = EDGES.index(b) + 1
    parts = {}
    for name, lo, hi in (("edge", 0, cut), ("inner", cut, shells)):
        pixels = cnt[:, lo:hi].sum(axis=1)
        total = np.zeros((n, s.shape[1]))
        for k in range(lo, hi):
            total = total + s[:, :, k]
        mean = np.full((n, s.shape[1]), np.nan)
        full = pixels > 0
        mean[full] = (total[full] / pixels[full].astype(np.float64)[:, None] + 1.0) / 2.0
        parts[name + "_area"], parts[name] = pixels, mean
    area = parts["edge_area"] + parts["inner_area"]
    inradius = np.full(n, np.nan)
    inradius[area > 0] = np.sqrt(np.maximum(deep[area > 0], 0).astype(np.float64))
    inradius[(area > 0) & (deep == -1)] = np.inf
    num, den = parts["edge"] - parts["inner"], parts["edge"] + parts["inner"]
    contrast = np.full(num.shape, np.nan)
    ok = np.isfinite(num) & (den > 0.0)      # NaN where a compartment is empty: both comparisons are False there
    contrast[ok] = num[ok] / den[ok]
    return {"area": area, "edge_area": parts["edge_area"], "inner_area": parts["inner_area"], "inradius": inradius, "edge": parts["edge"],
            "inner": parts["inner"], "contrast": contrast}


_name = intensities._name
_num = intensities._num


def _radius(v: float) -> str:
    """the inradius column: 17 significant digits, ``>8`` beyond the depth search, empty for a cell without a pixel"""
    if math.isnan(v):
        return ""
    return f">{DEPTH}" if math.isinf(v) else _num(v)


def cells_csv(cell_ids, types, names: Sequence[str], markers: Sequence[str], feat: Dict[str, np.ndarray]) -> str:
    """one line per cell in ``cell_ids`` order: ``id``, ``cell type``, ``area``, ``inradius``, ``edge_area``, ``inner_area`` and per marker
    ``{marker}_edge``, ``{marker}_inner``, ``{marker}_contrast``; floats with 17 significant digits, NaN as ``nan``, as intensities.cells_csv"""
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    n = len(ids)
    table = np.stack([np.asarray(feat[k], dtype=np.float64) for k in ("edge", "inner", "contrast")], axis=2) if n else np.zeros((0, len(markers), 3))
    if lab.shape != (n,) or table.shape != (n, len(markers), 3) or len(feat["area"]) != n:
        raise ValueError(f"cells_csv takes n labels and (n, {len(markers)}) tables for n = {n} cells, got {table.shape}")
    lines = ["id,cell type,area,inradius,edge_area,inner_area," + ",".join(f"{m}_{s}" for m in markers for s in ("edge", "inner", "contrast"))]
    for i in range(n):
        lines.append(f"{int(ids[i])},{_name(names, int(lab[i]))},{int(feat['area'][i])},{_radius(float(feat['inradius'][i]))},"
                     f"{int(feat['edge_area'][i])},{int(feat['inner_area'][i])}," + ",".join(_num(v) for v in table[i].reshape(-1)))
    return "\n".join(lines) + "\n"


def profile(types, n_types: int, count, sums):
    """(pixels (T, S) int64, mean (T, C, S) fp64): per cell type the pixels of every shell and the POOLED mean of every marker over them -- the
    shell sums of the type's cells added from 0.0 in row order, over the counts added up, reported as ``(mean + 1) / 2`` like every mean of
    ``features``; NaN where a type has no pixel in a shell"""
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    cnt = np.asarray(count).astype(np.int64)
    s = np.asarray(sums, dtype=np.float64)
    if cnt.ndim != 2 or s.ndim != 3 or len(cnt) != len(lab) or len(s) != len(lab) or s.shape[2] != cnt.shape[1]:
        raise ValueError(f"profile takes count (n, S) and sums (n, C, S) for n = {len(lab)} labels, got {cnt.shape} and {s.shape}")
    t = int(n_types)
    pixels = np.zeros((t, cnt.shape[1]), dtype=np.int64)
    total = np.zeros((t,) + s.shape[1:])
    for i in range(len(lab)):
        if 0 <= lab[i] < t:
            pixels[lab[i]] += cnt[i]
            total[lab[i]] = total[lab[i]] + s[i]
    mean = np.full(total.shape, np.nan)
    full = pixels > 0
    for c in range(s.shape[1]):
        mean[:, c, :][full] = (total[:, c, :][full] / pixels[full].astype(np.float64) + 1.0) / 2.0
    return pixels, mean


def profile_csv(names: Sequence[str], markers: Sequence[str], pixels, mean) -> str:
    """long form, one line per (cell type, marker, shell): ``cell_type,marker,shell,pixels,mean`` with the shells named by ``shell_names``"""
    px, m = np.asarray(pixels), np.asarray(mean)
    shells = shell_names()
    if px.shape != (len(names), len(shells)) or m.shape != (len(names), len(markers), len(shells)):
        raise ValueError(f"profile_csv takes (T, {len(shells)}) pixels and a (T, C, {len(shells)}) table, got {px.shape} and {m.shape}")
    lines = ["cell_type,marker,shell,pixels,mean"]
    for a, cell_type in enumerate(names):
        for c, marker in enumerate(markers):
            for k, shell in enumerate(shells):
                lines.append(f"{cell_type},{marker},{shell},{int(px[a, k])},{_num(m[a, c, k])}")
    return "\n".join(lines) + "\n"


def summary(types, n_types: int, contrast) -> np.ndarray:
    """(T, C, 4) fp64, SUMMARY per cell type and marker: the cells of the type, those of them with a NaN contrast, and the mean and the median
    of the contrast over the others; NaN where a type has none"""
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    x = np.asarray(contrast, dtype=np.float64)
    if x.ndim != 2 or len(x) != len(lab):
        raise ValueError(f"summary takes an (n, C) contrast for n = {len(lab)} labels, got {x.shape}")
    t = int(n_types)
    out = np.full((t, x.shape[1], len(SUMMARY)), np.nan)
    for a in range(t):
        for c in range(x.shape[1]):
            of_type = lab == a
            ok = of_type & ~np.isnan(x[:, c])
            out[a, c, 0], out[a, c, 1] = of_type.sum(), of_type.sum() - ok.sum()
            if ok.any():
                out[a, c, 2:] = (x[ok, c].mean(), np.median(x[ok, c]))
    return out


def summary_csv(names: Sequence[str], markers: Sequence[str], table) -> str:
    """long form, one line per (cell type, marker): ``cell_type,marker,n,n_nan,mean_contrast,median_contrast``"""
    s = np.asarray(table)
    if s.shape != (len(names), len(markers), len(SUMMARY)):
        raise ValueError(f"summary_csv takes a (T, C, {len(SUMMARY)}) table for T names and C markers, got {s.shape}")
    lines = ["cell_type,marker," + ",".join(SUMMARY)]
    for a, cell_type in enumerate(names):
        for c, marker in enumerate(markers):
            lines.append(f"{cell_type},{marker},{int(s[a, c, 0])},{int(s[a, c, 1])}," + ",".join(_num(v) for v in s[a, c, 2:]))
    return "\n".join(lines) + "\n"


def matrix_csv(names: Sequence[str], markers: Sequence[str], median) -> str:
    """the median contrast (``summary[:, :, 3]``) as a matrix: ``cell_type`` and one column per marker"""
    return intensities.matrix_csv(names, markers, median)


def colour_index(contrast) -> np.ndarray:
    """uint8, same shape: the entry of the diverging colour table of a marker's map, int(clip((contrast + 1) / 2, 0, 1) * 255); NaN -> 0"""
    v = np.nan_to_num((np.asarray(contrast, dtype=np.float64) + LIMIT) / (2.0 * LIMIT), nan=0.0)
    return (np.clip(v, 0.0, 1.0) * 255.0).astype(np.int64).astype(np.uint8)
