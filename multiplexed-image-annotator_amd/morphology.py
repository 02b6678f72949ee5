"""Host side of the per-cell morphology table (Annotator.cell_morphology): from the integer sums and the bounding boxes of ops.mask_morphology
(csrc/morphology.hip; include/ribca_hip.h states the sixteen columns) the features steinbock's ``measure regionprops`` and MCMICRO's
quantification write -- area, centroid, axes, eccentricity, orientation, perimeter, extent -- and three this project adds: the Euler number of
every label (fragments and holes), the share of a cell's outline that faces other cells, and the share of the cell inside the window its
classifiers saw.  Everything in fp64 from exact integers; pixel units; no torch here.  DESIGN.md section 20."""
from __future__ import annotations

import math
from typing import Dict, Sequence

import numpy as np

#: the columns of the per-cell table after ``cell_id,cell_type``, in file order
FEATURES = ("area", "centroid_r", "centroid_c", "bbox_h", "bbox_w", "extent", "equivalent_diameter", "major_axis", "minor_axis", "eccentricity",
            "orientation", "perimeter", "circularity", "euler", "contact_fraction", "on_image_edge", "patch_coverage")
#: those written as integers
INTEGER_FEATURES = ("area", "bbox_h", "bbox_w", "euler", "on_image_edge")
#: the columns of ``summary``
STATISTICS = ("n", "mean", "std", "min", "q25", "median", "q75", "max")
#: the standardised-means figure saturates at this many standard deviations: a fixed scale
Z_LIMIT = 3.0


def patch_rect(bbox, height: int, width: int, patch_size: int) -> np.ndarray:
    """(n, 4) int32 ``r0, r1, c0, c1`` (half open): the window ribca_extract_patches[_scaled] crops for a cell with the bounding box ``rmin, rmax,
    cmin, cmax`` (csrc/preprocess.hip, the reference's arithmetic): ``rmid = (rmin + rmax) // 2``, ``r0 = max(rmid - (P + 1) // 2, 0)``,
    ``r1 = min(r0 + P, H)``, columns likewise -- for an odd P the kernel truncates ``rmid - P / 2``, which is the same number wherever the
    maximum does not take over."""
    b = np.asarray(bbox).astype(np.int64).reshape(-1, 4)
    p = int(patch_size)
    half = (p + 1) // 2
    r0 = np.maximum((b[:, 0] + b[:, 1]) // 2 - half, 0)
    c0 = np.maximum((b[:, 2] + b[:, 3]) // 2 - half, 0)
    return np.stack([r0, np.minimum(r0 + p, int(height)), c0, np.minimum(c0 + p, int(width))], axis=1).astype(np.int32)


def features(sums, bbox) -> Dict[str, np.ndarray]:
    """A dict of (n) arrays, one per name of FEATURES, from ``sums`` (n, 16) and ``bbox`` (n, 4).  With A = the area, S_r, S_c, S_rr, S_cc, S_rc
    the raw moments (columns 1 .. 5), e_cell, e_bg, e_img the leaving pixel edges (6 .. 8), p_a, p_b, p_c the perimeter classes (9 .. 11), q1, q3,
    qd the bit quads (12 .. 14) and ``in_rect`` column 15:

    * ``area`` = A; ``centroid_r`` = S_r / A, ``centroid_c`` = S_c / A; ``bbox_h`` = rmax - rmin + 1, ``bbox_w`` = cmax - cmin + 1;
      ``extent`` = A / (bbox_h bbox_w); ``equivalent_diameter`` = sqrt(4 A / pi);
    * the central second moments from exact integers (Python integers: the products pass 2^64, and int / int rounds correctly):
      ``N_rr = A S_rr - S_r^2``, ``m_rr = N_rr / A^2``, likewise ``m_cc`` and ``N_rc = A S_rc - S_r S_c``, ``m_rc = N_rc / A^2``;
    * ``lambda_1,2 = (m_rr + m_cc) / 2 +- sqrt(((m_rr - m_cc) / 2)^2 + m_rc^2)``; ``major_axis = 4 sqrt(lambda_1)``,
      ``minor_axis = 4 sqrt(max(lambda_2, 0))``, ``eccentricity = sqrt(1 - lambda_2 / lambda_1)`` (0 when lambda_1 = 0; lambda_2 clamped at 0),
      ``orientation = atan2(2 m_rc, m_rr - m_cc) / 2``, the angle of the major axis from the row axis, in (-pi / 2, pi / 2];
    * ``perimeter = p_a + p_b sqrt 2 + p_c (1 + sqrt 2) / 2`` (scikit-image's 4-neighbourhood perimeter);
      ``circularity = 4 pi A / perimeter^2`` (NaN at perimeter 0);
    * ``euler = (q1 - q3 - 2 qd) / 4``: the components at 8-connectivity minus the holes at 4-connectivity (1 for one solid blob);
    * ``contact_fraction = e_cell / (e_cell + e_bg + e_img)``; ``on_image_edge`` = 1 when e_img > 0, else 0;
      ``patch_coverage = in_rect / A``.

    A cell without a pixel (A = 0) has area, bbox_h, bbox_w, euler and on_image_edge 0 and NaN everywhere else."""
    s = np.asarray(sums).astype(np.int64).reshape(-1, 16)      # every column stays below 2^63
    b = np.asarray(bbox).astype(np.int64).reshape(-1, 4)
    n = len(s)
    if len(b) != n:
        raise ValueError(f"features takes one bounding box per row of sums, got {len(b)} for {n}")
    out = {name: np.full(n, np.nan) for name in FEATURES}
    for name in INTEGER_FEATURES:
        out[name] = np.zeros(n, dtype=np.int64)
    root2 = math.sqrt(2.0)
    for i in range(n):
        a, sr, sc, srr, scc, src, e_cell, e_bg, e_img, pa, pb, pc, q1, q3, qd, inside = (int(v) for v in s[i])
        if a == 0:
            continue
        height, width = int(b[i, 1] - b[i, 0] + 1), int(b[i, 3] - b[i, 2] + 1)
        out["area"][i] = a
        out["centroid_r"][i] = sr / a
        out["centroid_c"][i] = sc / a
        out["bbox_h"][i], out["bbox_w"][i] = height, width
        out["extent"][i] = a / (height * width)
        out["equivalent_diameter"][i] = math.sqrt(4.0 * a / math.pi)
        m_rr, m_cc, m_rc = (a * srr - sr * sr) / (a * a), (a * scc - sc * sc) / (a * a), (a * src - sr * sc) / (a * a)
        mid, half = (m_rr + m_cc) / 2.0, math.sqrt(((m_rr - m_cc) / 2.0) ** 2 + m_rc * m_rc)
        l1, l2 = mid + half, max(mid - half, 0.0)
        out["major_axis"][i] = 4.0 * math.sqrt(l1)
        out["minor_axis"][i] = 4.0 * math.sqrt(l2)
        out["eccentricity"][i] = math.sqrt(max(1.0 - l2 / l1, 0.0)) if l1 > 0.0 else 0.0
        out["orientation"][i] = 0.5 * math.atan2(2.0 * m_rc, m_rr - m_cc)
        perimeter = pa + pb * root2 + pc * (1.0 + root2) / 2.0
        out["perimeter"][i] = perimeter
        out["circularity"][i] = 4.0 * math.pi * a / (perimeter * perimeter) if perimeter > 0.0 else math.nan
        out["euler"][i] = (q1 - q3 - 2 * qd) // 4      # the numerator is a multiple of four
        edges = e_cell + e_bg + e_img
        out["contact_fraction"][i] = e_cell / edges if edges else math.nan
        out["on_image_edge"][i] = 1 if e_img > 0 else 0
        out["patch_coverage"][i] = inside / a
    return out


def feature_matrix(feat: Dict[str, np.ndarray]) -> np.ndarray:
    """(n, F) fp64, the columns in FEATURES order: what a tile-per-rank run gathers"""
    return np.stack([np.asarray(feat[name], dtype=np.float64) for name in FEATURES], axis=1) if len(feat["area"]) else np.zeros((0, len(FEATURES)))


def from_matrix(rows) -> Dict[str, np.ndarray]:
    """the inverse of feature_matrix (the integer features are exact in fp64)"""
    m = np.asarray(rows, dtype=np.float64).reshape(-1, len(FEATURES))
    return {name: (m[:, k].astype(np.int64) if name in INTEGER_FEATURES else m[:, k].copy()) for k, name in enumerate(FEATURES)}


def _name(names: Sequence[str], label: int) -> str:
    return str(names[label]) if 0 <= label < len(names) else ""


def _text(name: str, value) -> str:
    return str(int(value)) if name in INTEGER_FEATURES else f"{float(value):.17g}"


def cells_csv(cell_ids, types, names: Sequence[str], feat: Dict[str, np.ndarray]) -> str:
    """one line per cell in ``cell_ids`` order: ``cell_id,cell_type`` and every name of FEATURES; integers as integers, floats with 17
    significant digits"""
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    n = len(ids)
    if lab.shape != (n,) or any(len(feat[name]) != n for name in FEATURES):
        raise ValueError(f"cells_csv takes n labels and n values of every feature for n = {n} cells")
    lines = ["cell_id,cell_type," + ",".join(FEATURES)]
    for i in range(n):
        lines.append(f"{int(ids[i])},{_name(names, int(lab[i]))}," + ",".join(_text(name, feat[name][i]) for name in FEATURES))
    return "\n".join(lines) + "\n"


def summary(types, n_types: int, feat: Dict[str, np.ndarray]) -> np.ndarray:
    """(T, F, 8) fp64, STATISTICS of every feature over the cells of every type whose value is finite: their number, mean, population std,
    min, the quartiles (numpy's linear interpolation) and max; NaN where a type has no such cell"""
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    t = int(n_types)
    out = np.full((t, len(FEATURES), len(STATISTICS)), np.nan)
    for k, name in enumerate(FEATURES):
        v = np.asarray(feat[name], dtype=np.float64)
        for a in range(t):
            x = v[(lab == a) & np.isfinite(v)]
            out[a, k, 0] = len(x)
            if len(x):
                out[a, k, 1:] = (x.mean(), x.std(), x.min(), np.quantile(x, 0.25), np.quantile(x, 0.5), np.quantile(x, 0.75), x.max())
    return out


def summary_csv(names: Sequence[str], table) -> str:
    """long form, one line per (cell type, feature): ``cell_type,feature,n,mean,std,min,q25,median,q75,max``; floats with 17 significant digits"""
    s = np.asarray(table)
    if s.shape != (len(names), len(FEATURES), len(STATISTICS)):
        raise ValueError(f"summary_csv takes a (T, {len(FEATURES)}, {len(STATISTICS)}) table for T names, got {s.shape} for {len(names)}")
    lines = ["cell_type,feature," + ",".join(STATISTICS)]
    for a, cell_type in enumerate(names):
        for k, name in enumerate(FEATURES):
            lines.append(f"{cell_type},{name},{int(s[a, k, 0])}," + ",".join(f"{float(v):.17g}" for v in s[a, k, 1:]))
    return "\n".join(lines) + "\n"


def standardised_means(types, n_types: int, feat: Dict[str, np.ndarray]) -> np.ndarray:
    """(T, F) fp64: ``(mean_t - mean_all) / std_all`` of every feature, the means and the population std over the cells with a finite value
    (mean_all and std_all over those with a label in [0, T)); NaN for a type without such a cell or a feature without spread"""
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    t = int(n_types)
    out = np.full((t, len(FEATURES)), np.nan)
    for k, name in enumerate(FEATURES):
        v = np.asarray(feat[name], dtype=np.float64)
        ok = np.isfinite(v) & (lab >= 0) & (lab < t)
        if not ok.any():
            continue
        mean, std = v[ok].mean(), v[ok].std()
        if not std > 0.0:
            continue
        for a in range(t):
            x = v[ok & (lab == a)]
            if len(x):
                out[a, k] = (x.mean() - mean) / std
    return out


def matrix_csv(names: Sequence[str], z) -> str:
    """the standardised means as a matrix: ``cell_type`` and one column per feature; floats with 17 significant digits"""
    m = np.asarray(z)
    if m.shape != (len(names), len(FEATURES)):
        raise ValueError(f"matrix_csv takes a (T, {len(FEATURES)}) matrix for T names, got {m.shape} for {len(names)}")
    lines = ["cell_type," + ",".join(FEATURES)]
    for a, cell_type in enumerate(names):
        lines.append(f"{cell_type}," + ",".join(f"{float(v):.17g}" for v in m[a]))
    return "\n".join(lines) + "\n"


def diameter_colour_index(equivalent_diameter, cell_size: float) -> np.ndarray:
    """(n) uint8: the entry of the colour table of the diameter map, int(min(equivalent_diameter / (2 cell_size), 1) * 255); NaN -> 0"""
    ratio = np.nan_to_num(np.asarray(equivalent_diameter, dtype=np.float64) / (2.0 * float(cell_size)), nan=0.0)
    return (np.clip(ratio, 0.0, 1.0) * 255.0).astype(np.int64).astype(np.uint8)


def coverage_colour_index(patch_coverage) -> np.ndarray:
    """(n) uint8: the entry of the colour table of the coverage map, int(patch_coverage * 255) with patch_coverage in [0, 1]; NaN -> 0"""
    ratio = np.nan_to_num(np.asarray(patch_coverage, dtype=np.float64), nan=0.0)
    return (np.clip(ratio, 0.0, 1.0) * 255.0).astype(np.int64).astype(np.uint8)
