"""Matching a second mask to the cells (Annotator.mask_matching): the host side, int64 and fp64 only.  Mask A holds the CELLS the run works on,
mask B the OBJECTS of a second segmentation of the same image -- nuclei beside whole cells, or another tool's cells.  Everything here is a
function of the sparse contingency table ops.overlap_pairs returns: ``cell``, ``obj`` (indices into ``ids_a`` / ``ids_b``) and ``inter`` (the
pixels the pair shares), sorted by (cell, obj), with ``area_a`` and ``area_b``.  tests/overlap_numpy.py restates every rule with plain loops.

OWNER of an object: the cell with the largest ``inter``, a tie to the lowest cell index; accepted when ``inter * 100 >= min_overlap * area_b``
in integers, else the object is an ORPHAN (owner -1).  AGREEMENT of the two masks: a pair is a true positive at the threshold t percent when
``inter * 100 > t * union`` (``union = area_a + area_b - inter``), STRICTLY and in integers, for t = 50, 55, .., 95 (THRESHOLDS).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .intensities import _num

THRESHOLDS = tuple(range(50, 100, 5))      # percent: above one half the matching needs no assignment solver (agreement_counts)
CELL_STATUS = ("none", "single", "multi")
OBJECT_STATUS = ("matched", "split", "orphan")
AGREEMENT = ("cells", "objects", "tp", "unmatched_cells", "unmatched_objects", "precision", "recall", "f1", "mean_matched_iou", "panoptic_quality")


def check_min_overlap(min_overlap) -> int:
    """``min_overlap`` as an int, ValueError unless it is an integer (no bool) percent in 1 .. 100"""
    if isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, np.integer)) or not 1 <= int(min_overlap) <= 100:
        raise ValueError(f"min_overlap must be an integer percent from 1 to 100, got {min_overlap!r}")
    return int(min_overlap)


def _pairs(cell, obj, inter) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    c = np.asarray(cell).astype(np.int64).reshape(-1)
    o = np.asarray(obj).astype(np.int64).reshape(-1)
    w = np.asarray(inter).astype(np.int64).reshape(-1)
    if not len(c) == len(o) == len(w):
        raise ValueError(f"the pair table takes cell, obj and inter of one length, got {len(c)}, {len(o)} and {len(w)}")
    return c, o, w


def owners(cell, obj, inter, area_b, min_overlap: int = 50) -> Tuple[np.ndarray, np.ndarray]:
    """(owner (m) int32, inside (m) int64): for every object the cell that owns it, or -1, and the pixels it shares with that cell (0 for an
    orphan).  The candidate is the cell with the largest ``inter``, a tie to the lowest cell index; it is accepted when
    ``inter * 100 >= min_overlap * area_b[j]``, compared in int64."""
    p = check_min_overlap(min_overlap)
    c, o, w = _pairs(cell, obj, inter)
    area = np.asarray(area_b).astype(np.int64).reshape(-1)
    m = len(area)
    owner, inside = np.full(m, -1, dtype=np.int32), np.zeros(m, dtype=np.int64)
    if len(c):
        order = np.lexsort((c, -w, o))                  # by object, the largest share first, the lowest cell first among equals
        first = order[np.concatenate([[True], o[order][1:] != o[order][:-1]])]
        ok = w[first] * 100 >= p * area[o[first]]
        owner[o[first][ok]] = c[first][ok]
        inside[o[first][ok]] = w[first][ok]
    return owner, inside


def cell_rows(cell, obj, inter, area_a, ids_b, owner) -> Dict[str, np.ndarray]:
    """Per cell, int64 unless said: ``area``; ``objects``, the objects it owns; ``object_id``, the label of the owned object with the largest
    ``inter`` (a tie to the lowest label; 0 without one); ``inner_area``, the sum of ``inter`` over its owned objects; ``outer_area`` =
    area - inner_area; ``inner_fraction`` = inner_area / area in fp64, 0 for a cell without a pixel; ``foreign_area``, the sum of ``inter`` over
    the objects it overlaps and does not own; ``status``, an index into CELL_STATUS: none, single or multi by ``objects`` = 0, 1, more."""
    c, o, w = _pairs(cell, obj, inter)
    area = np.asarray(area_a).astype(np.int64).reshape(-1)
    labels = np.asarray(ids_b).astype(np.int64).reshape(-1)
    own = np.asarray(owner).astype(np.int64).reshape(-1)
    n = len(area)
    mine = own[o] == c if len(c) else np.zeros(0, dtype=bool)
    objects = np.bincount(c[mine], minlength=n).astype(np.int64)
    inner = np.bincount(c[mine], weights=w[mine].astype(np.float64), minlength=n).astype(np.int64)      # exact: sums of pixels below 2^31
    foreign = np.bincount(c[~mine], weights=w[~mine].astype(np.float64), minlength=n).astype(np.int64)
    object_id = np.zeros(n, dtype=np.int64)
    if mine.any():
        cm, om, wm = c[mine], o[mine], w[mine]
        order = np.lexsort((om, -wm, cm))               # ids_b ascends: the lowest object index is the lowest label
        first = order[np.concatenate([[True], cm[order][1:] != cm[order][:-1]])]
        object_id[cm[first]] = labels[om[first]]
    fraction = np.zeros(n, dtype=np.float64)
    fraction[area > 0] = inner[area > 0].astype(np.float64) / area[area > 0].astype(np.float64)
    return {"area": area, "objects": objects, "object_id": object_id, "inner_area": inner, "outer_area": area - inner, "inner_fraction": fraction,
            "foreign_area": foreign, "status": np.minimum(objects, 2)}


def object_rows(cell, obj, inter, area_b, ids_a, owner, inside) -> Dict[str, np.ndarray]:
    """Per object, int64 unless said: ``area``; ``cells``, the cells it overlaps; ``owner_id``, the label of its owner, 0 for an orphan;
    ``inside``, the pixels it shares with its owner; ``fraction`` = inside / area in fp64 (0 for an object without a pixel); ``uncovered`` =
    area minus the sum of its ``inter``, its pixels on no cell; ``status``, an index into OBJECT_STATUS: orphan without an owner, else split
    when it overlaps more than one cell, else matched."""
    c, o, w = _pairs(cell, obj, inter)
    area = np.asarray(area_b).astype(np.int64).reshape(-1)
    labels = np.asarray(ids_a).astype(np.int64).reshape(-1)
    own = np.asarray(owner).astype(np.int64).reshape(-1)
    ins = np.asarray(inside).astype(np.int64).reshape(-1)
    m = len(area)
    cells = np.bincount(o, minlength=m).astype(np.int64)
    covered = np.bincount(o, weights=w.astype(np.float64), minlength=m).astype(np.int64)
    owner_id = np.zeros(m, dtype=np.int64)
    owner_id[own >= 0] = labels[own[own >= 0]]
    fraction = np.zeros(m, dtype=np.float64)
    fraction[area > 0] = ins[area > 0].astype(np.float64) / area[area > 0].astype(np.float64)
    status = np.where(own < 0, 2, np.where(cells > 1, 1, 0)).astype(np.int64)
    return {"area": area, "cells": cells, "owner_id": owner_id, "inside": ins, "fraction": fraction, "uncovered": area - covered, "status": status}


def pair_rows(cell, obj, inter, area_a, area_b) -> Tuple[np.ndarray, np.ndarray]:
    """(union int64, iou fp64) of every pair: ``union = area_a[cell] + area_b[obj] - inter`` and ``iou = inter / union``"""
    c, o, w = _pairs(cell, obj, inter)
    union = np.asarray(area_a).astype(np.int64).reshape(-1)[c] + np.asarray(area_b).astype(np.int64).reshape(-1)[o] - w
    return union, w.astype(np.float64) / union.astype(np.float64)


def agreement_counts(cell, obj, inter, area_a, area_b) -> Tuple[np.ndarray, np.ndarray]:
    """stardist's ``matching`` restricted to the thresholds where it needs no assignment solver.  Returns (counts (len(THRESHOLDS), 3) int64,
    iou_sum (len(THRESHOLDS)) fp64) of one image: column 0 the cells and column 1 the objects with area > 0 -- the same at every threshold --
    column 2 the true positives, and the sum of the IoU of the true positives, added one after another in (cell, obj) order.  A pair is a true
    positive at t percent when ``inter * 100 > t * union``, strictly, in int64.  With IoU above one half each of the two shapes shares more
    than half of its pixels with the other; the objects are disjoint, and so are the cells, so no cell and no object is in two such pairs:
    the matching is unique by construction and the true positives ARE the optimal assignment."""
    c, o, w = _pairs(cell, obj, inter)
    union, iou = pair_rows(c, o, w, area_a, area_b)
    counts, sums = np.zeros((len(THRESHOLDS), 3), dtype=np.int64), np.zeros(len(THRESHOLDS), dtype=np.float64)
    counts[:, 0] = int((np.asarray(area_a).reshape(-1) > 0).sum())
    counts[:, 1] = int((np.asarray(area_b).reshape(-1) > 0).sum())
    for k, t in enumerate(THRESHOLDS):
        tp = w * 100 > t * union
        counts[k, 2] = int(tp.sum())
        if tp.any():
            sums[k] = np.cumsum(iou[tp])[-1]            # a running sum: one addition after another
    return counts, sums


def add_agreement(per_image: Sequence[Tuple[np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, np.ndarray]:
    """the counts and IoU sums of a group: those of its images added up in image order"""
    counts, sums = np.zeros((len(THRESHOLDS), 3), dtype=np.int64), np.zeros(len(THRESHOLDS), dtype=np.float64)
    for c, s in per_image:
        counts = counts + np.asarray(c, dtype=np.int64)
        sums = sums + np.asarray(s, dtype=np.float64)
    return counts, sums


def agreement_table(counts, iou_sum) -> np.ndarray:
    """(len(THRESHOLDS), len(AGREEMENT)) fp64: cells, objects, tp, unmatched_cells = cells - tp, unmatched_objects = objects - tp, precision
    tp / objects, recall tp / cells, f1 = 2 tp / (2 tp + unmatched_cells + unmatched_objects), the mean matched IoU = iou_sum / tp, and the
    panoptic quality iou_sum / (tp + unmatched_cells / 2 + unmatched_objects / 2); a zero denominator gives 0"""
    counts = np.asarray(counts, dtype=np.int64).reshape(len(THRESHOLDS), 3)
    sums = np.asarray(iou_sum, dtype=np.float64).reshape(len(THRESHOLDS))
    out = np.zeros((len(THRESHOLDS), len(AGREEMENT)), dtype=np.float64)

    def ratio(a: float, b: float) -> float:
        return a / b if b != 0 else 0.0

    for k in range(len(THRESHOLDS)):
        cells, objects, tp = (int(v) for v in counts[k])
        fn, fp = cells - tp, objects - tp
        out[k] = (cells, objects, tp, fn, fp, ratio(float(tp), float(objects)), ratio(float(tp), float(cells)), ratio(2.0 * tp, float(2 * tp + fn + fp)),
                  ratio(float(sums[k]), float(tp)), ratio(float(sums[k]), tp + fn / 2.0 + fp / 2.0))
    return out


def type_summary(types, n_types: int, status, inner_fraction) -> np.ndarray:
    """(T + 1, 6) fp64: per cell type, and in the last row over ALL cells, the number of cells, of those with status none, single and multi,
    and the mean and the median of ``inner_fraction`` (NaN without a cell).  A label outside [0, T) counts in the last row only."""
    lab = np.asarray(types).astype(np.int64).reshape(-1)
    st = np.asarray(status).astype(np.int64).reshape(-1)
    fr = np.asarray(inner_fraction, dtype=np.float64).reshape(-1)
    t = int(n_types)
    out = np.full((t + 1, 6), np.nan)
    for a in range(t + 1):
        sel = lab == a if a < t else np.ones(len(lab), dtype=bool)
        out[a, :4] = (sel.sum(), (sel & (st == 0)).sum(), (sel & (st == 1)).sum(), (sel & (st == 2)).sum())
        if sel.any():
            out[a, 4:] = (np.cumsum(fr[sel])[-1] / float(sel.sum()), np.median(fr[sel]))      # the mean: a running sum in row order
    return out


def fraction_colour_index(inner_fraction) -> np.ndarray:
    """the viridis entry of the fraction map: int(clip(inner_fraction, 0, 1) * 255)"""
    return (np.clip(np.asarray(inner_fraction, dtype=np.float64), 0.0, 1.0) * 255).astype(np.int64)


# ---- text ------------------------------------------------------------------------------------------------------------------------------------------
def cells_csv(cell_ids, rows: Dict[str, np.ndarray], types=None, names: Optional[Sequence[str]] = None) -> str:
    """one line per cell in ``cell_ids`` order; ``cell type`` is empty without ``types`` (before predict()) and for a label outside ``names``"""
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    lab = None if types is None else np.asarray(types).astype(np.int64).reshape(-1)
    lines = ["id,cell type,area,objects,object_id,inner_area,outer_area,inner_fraction,foreign_area,status"]
    for i in range(len(ids)):
        kind = str(names[int(lab[i])]) if lab is not None and names is not None and 0 <= int(lab[i]) < len(names) else ""
        lines.append(f"{int(ids[i])},{kind},{int(rows['area'][i])},{int(rows['objects'][i])},{int(rows['object_id'][i])},{int(rows['inner_area'][i])},"
                     f"{int(rows['outer_area'][i])},{_num(rows['inner_fraction'][i])},{int(rows['foreign_area'][i])},{CELL_STATUS[int(rows['status'][i])]}")
    return "\n".join(lines) + "\n"


def objects_csv(object_ids, rows: Dict[str, np.ndarray]) -> str:
    ids = np.asarray(object_ids).astype(np.int64).reshape(-1)
    lines = ["id,area,cells,owner_id,inside,fraction,uncovered,status"]
    for j in range(len(ids)):
        lines.append(f"{int(ids[j])},{int(rows['area'][j])},{int(rows['cells'][j])},{int(rows['owner_id'][j])},{int(rows['inside'][j])},"
                     f"{_num(rows['fraction'][j])},{int(rows['uncovered'][j])},{OBJECT_STATUS[int(rows['status'][j])]}")
    return "\n".join(lines) + "\n"


def pairs_csv(cell_ids, object_ids, cell, obj, inter, union, iou) -> str:
    """one line per pair that shares a pixel, in (cell, object) order"""
    a, b = np.asarray(cell_ids).astype(np.int64).reshape(-1), np.asarray(object_ids).astype(np.int64).reshape(-1)
    c, o, w = _pairs(cell, obj, inter)
    lines = ["cell_id,object_id,intersection,union,iou"]
    for k in range(len(c)):
        lines.append(f"{int(a[c[k]])},{int(b[o[k]])},{int(w[k])},{int(union[k])},{_num(iou[k])}")
    return "\n".join(lines) + "\n"


def agreement_csv(table) -> str:
    """one line per threshold: the threshold in percent, five integer columns, five fp64 columns"""
    t = np.asarray(table, dtype=np.float64).reshape(len(THRESHOLDS), len(AGREEMENT))
    lines = ["threshold_percent," + ",".join(AGREEMENT)]
    for k, thr in enumerate(THRESHOLDS):
        lines.append(f"{thr}," + ",".join(str(int(v)) for v in t[k, :5]) + "," + ",".join(_num(v) for v in t[k, 5:]))
    return "\n".join(lines) + "\n"


def summary_csv(names: Sequence[str], table) -> str:
    """one line per cell type and a last line ``all``"""
    s = np.asarray(table, dtype=np.float64).reshape(len(names) + 1, 6)
    lines = ["cell_type,n,none,single,multi,mean_inner_fraction,median_inner_fraction"]
    for a, name in enumerate(list(names) + ["all"]):
        lines.append(f"{name}," + ",".join(str(int(v)) for v in s[a, :4]) + "," + ",".join(_num(v) for v in s[a, 4:]))
    return "\n".join(lines) + "\n"
