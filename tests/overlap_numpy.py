"""The restatement of csrc/overlap.hip, ops.overlap_pairs / mask_compartments and every rule of multiplexed_image_annotator_amd/matching.py,
written independently of all three: one pixel at a time into a dict of pairs, plain Python loops and integers over that dict, Python floats
added one after another.  Nothing here calls into the package."""
import numpy as np

THRESHOLDS = (50, 55, 60, 65, 70, 75, 80, 85, 90, 95)
CELL_STATUS = ("none", "single", "multi")


def index_image(mask, table, count):
    """(H, W) int64: table[mask] where the label is inside the table and the entry inside [0, count), else -1"""
    mask = np.asarray(mask).astype(np.int64)
    table = np.asarray(table).astype(np.int64)
    out = np.full(mask.shape, -1, dtype=np.int64)
    for r in range(mask.shape[0]):
        for c in range(mask.shape[1]):
            lab = int(mask[r, c])
            if 0 <= lab < len(table) and 0 <= int(table[lab]) < count:
                out[r, c] = int(table[lab])
    return out


def id_table(ids):
    """label -> index for ascending labels, label 0 never: what ops._cell_table builds"""
    ids = [int(v) for v in ids]
    table = np.full(max(ids) + 1 if ids else 1, -1, dtype=np.int32)
    for k, v in enumerate(ids):
        table[v] = k
    table[0] = -1
    return table


def labels_of(mask):
    return sorted(set(int(v) for v in np.asarray(mask).reshape(-1) if v > 0))


def overlap(mask_a, tab_a, n, mask_b, tab_b, m):
    """({(i, j): shared pixels}, area_a (n) int64, area_b (m) int64)"""
    ca, cb = index_image(mask_a, tab_a, n), index_image(mask_b, tab_b, m)
    pairs, area_a, area_b = {}, np.zeros(n, dtype=np.int64), np.zeros(m, dtype=np.int64)
    for r in range(ca.shape[0]):
        for c in range(ca.shape[1]):
            i, j = int(ca[r, c]), int(cb[r, c])
            if i >= 0:
                area_a[i] += 1
            if j >= 0:
                area_b[j] += 1
            if i >= 0 and j >= 0:
                pairs[(i, j)] = pairs.get((i, j), 0) + 1
    return pairs, area_a, area_b


def table(pairs, n, slots):
    """(partner (n, S) int32, inter (n, S) int64, degree (n) int32) as ribca_mask_overlap writes them when every row fits"""
    partner = np.full((n, slots), -1, dtype=np.int32)
    inter = np.zeros((n, slots), dtype=np.int64)
    degree = np.zeros(n, dtype=np.int32)
    for (i, j) in sorted(pairs):
        partner[i, degree[i]], inter[i, degree[i]] = j, pairs[(i, j)]
        degree[i] += 1
    return partner, inter, degree


def pair_arrays(pairs):
    keys = sorted(pairs)
    return (np.array([k[0] for k in keys], dtype=np.int32), np.array([k[1] for k in keys], dtype=np.int32),
            np.array([pairs[k] for k in keys], dtype=np.int64))


def compartments(mask_a, tab_a, n, mask_b, tab_b, m, owner):
    mask_a = np.asarray(mask_a)
    ca, cb = index_image(mask_a, tab_a, n), index_image(mask_b, tab_b, m)
    inner, outer = np.zeros(mask_a.shape, dtype=np.int32), np.zeros(mask_a.shape, dtype=np.int32)
    for r in range(ca.shape[0]):
        for c in range(ca.shape[1]):
            i, j = int(ca[r, c]), int(cb[r, c])
            if i < 0:
                continue
            if j >= 0 and int(owner[j]) == i:
                inner[r, c] = mask_a[r, c]
            else:
                outer[r, c] = mask_a[r, c]
    return inner, outer


# ---- the rules of matching.py ------------------------------------------------------------------------------------------------------------------------
def owners(pairs, area_b, min_overlap=50):
    """(owner, inside) lists: the cell with the most shared pixels, the lowest cell among equals, accepted at >= min_overlap percent of the object"""
    m = len(area_b)
    owner, inside = [-1] * m, [0] * m
    for j in range(m):
        best, share = -1, 0
        for (i, jj) in sorted(pairs):
            if jj == j and pairs[(i, jj)] > share:      # strictly more: the first (lowest) cell keeps a tie
                best, share = i, pairs[(i, jj)]
        if best >= 0 and share * 100 >= min_overlap * int(area_b[j]):
            owner[j], inside[j] = best, share
    return owner, inside


def cell_rows(pairs, area_a, ids_b, owner):
    rows = []
    for i in range(len(area_a)):
        owned = sorted((j, w) for (ii, j), w in pairs.items() if ii == i and owner[j] == i)
        foreign = sum(w for (ii, j), w in pairs.items() if ii == i and owner[j] != i)
        inner = sum(w for _, w in owned)
        top, top_w = 0, 0
        for j, w in owned:
            if w > top_w:
                top, top_w = int(ids_b[j]), w
        area = int(area_a[i])
        rows.append({"area": area, "objects": len(owned), "object_id": top, "inner_area": inner, "outer_area": area - inner,
                     "inner_fraction": inner / area if area else 0.0, "foreign_area": foreign, "status": CELL_STATUS[min(len(owned), 2)]})
    return rows


def object_rows(pairs, area_b, ids_a, owner, inside):
    rows = []
    for j in range(len(area_b)):
        shares = [w for (i, jj), w in pairs.items() if jj == j]
        area = int(area_b[j])
        status = "orphan" if owner[j] < 0 else ("split" if len(shares) > 1 else "matched")
        rows.append({"area": area, "cells": len(shares), "owner_id": int(ids_a[owner[j]]) if owner[j] >= 0 else 0, "inside": inside[j],
                     "fraction": inside[j] / area if area else 0.0, "uncovered": area - sum(shares), "status": status})
    return rows


def pair_rows(pairs, area_a, area_b):
    out = []
    for (i, j) in sorted(pairs):
        w = pairs[(i, j)]
        union = int(area_a[i]) + int(area_b[j]) - w
        out.append((i, j, w, union, w / union))
    return out


def true_positives(pairs, area_a, area_b, t):
    return [(i, j, w / u) for i, j, w, u, _ in pair_rows(pairs, area_a, area_b) if w * 100 > t * u]


def agreement_counts(pairs, area_a, area_b):
    """per threshold [cells, objects, tp] and the IoU sum of the true positives in (cell, object) order"""
    cells, objects = sum(1 for a in area_a if a > 0), sum(1 for a in area_b if a > 0)
    counts, sums = [], []
    for t in THRESHOLDS:
        total = 0.0
        tps = true_positives(pairs, area_a, area_b, t)
        for _, _, iou in tps:
            total = total + iou
        counts.append([cells, objects, len(tps)])
        sums.append(total)
    return counts, sums


def add_agreement(per_image):
    counts, sums = [[0, 0, 0] for _ in THRESHOLDS], [0.0 for _ in THRESHOLDS]
    for c, s in per_image:
        for k in range(len(THRESHOLDS)):
            counts[k] = [counts[k][q] + int(c[k][q]) for q in range(3)]
            sums[k] = sums[k] + float(s[k])
    return counts, sums


def agreement_rows(counts, sums):
    rows = []
    for k in range(len(THRESHOLDS)):
        cells, objects, tp = counts[k]
        fn, fp = cells - tp, objects - tp
        div = lambda a, b: a / b if b else 0.0      # noqa: E731
        rows.append([cells, objects, tp, fn, fp, div(tp, objects), div(tp, cells), div(2 * tp, 2 * tp + fn + fp), div(sums[k], tp),
                     div(sums[k], tp + fn / 2 + fp / 2)])
    return rows


def type_summary(types, n_types, cells):
    """per type and for all cells: n, none, single, multi, mean and median of inner_fraction"""
    rows = []
    for a in list(range(n_types)) + [None]:
        mine = [c for k, c in enumerate(cells) if a is None or int(types[k]) == a]
        counts = [len(mine)] + [sum(1 for c in mine if c["status"] == s) for s in CELL_STATUS]
        if mine:
            total = 0.0
            for c in mine:
                total = total + c["inner_fraction"]
            fr = sorted(c["inner_fraction"] for c in mine)
            mid = len(fr) // 2
            median = fr[mid] if len(fr) % 2 else (fr[mid - 1] + fr[mid]) / 2
            rows.append(counts + [total / len(mine), median])
        else:
            rows.append(counts + [float("nan"), float("nan")])
    return rows


def num(v):
    return "%.17g" % float(v)


def cells_csv(ids_a, cells, types=None, names=None):
    lines = ["id,cell type,area,objects,object_id,inner_area,outer_area,inner_fraction,foreign_area,status"]
    for k, c in enumerate(cells):
        kind = names[int(types[k])] if types is not None and 0 <= int(types[k]) < len(names) else ""
        lines.append(",".join([str(int(ids_a[k])), kind, str(c["area"]), str(c["objects"]), str(c["object_id"]), str(c["inner_area"]), str(c["outer_area"]),
                               num(c["inner_fraction"]), str(c["foreign_area"]), c["status"]]))
    return "\n".join(lines) + "\n"


def objects_csv(ids_b, objects):
    lines = ["id,area,cells,owner_id,inside,fraction,uncovered,status"]
    for k, o in enumerate(objects):
        lines.append(",".join([str(int(ids_b[k])), str(o["area"]), str(o["cells"]), str(o["owner_id"]), str(o["inside"]), num(o["fraction"]),
                               str(o["uncovered"]), o["status"]]))
    return "\n".join(lines) + "\n"


def pairs_csv(ids_a, ids_b, rows):
    lines = ["cell_id,object_id,intersection,union,iou"]
    for i, j, w, u, iou in rows:
        lines.append(",".join([str(int(ids_a[i])), str(int(ids_b[j])), str(w), str(u), num(iou)]))
    return "\n".join(lines) + "\n"


def agreement_csv(rows):
    lines = ["threshold_percent,cells,objects,tp,unmatched_cells,unmatched_objects,precision,recall,f1,mean_matched_iou,panoptic_quality"]
    for t, r in zip(THRESHOLDS, rows):
        lines.append(",".join([str(t)] + [str(int(v)) for v in r[:5]] + [num(v) for v in r[5:]]))
    return "\n".join(lines) + "\n"


def summary_csv(names, rows):
    lines = ["cell_type,n,none,single,multi,mean_inner_fraction,median_inner_fraction"]
    for name, r in zip(list(names) + ["all"], rows):
        lines.append(",".join([name] + [str(int(v)) for v in r[:4]] + [num(v) for v in r[4:]]))
    return "\n".join(lines) + "\n"


def image_texts(mask_a, mask_b, min_overlap=50, types=None, names=None):
    """everything Annotator.mask_matching derives from one image's two masks: the three texts, the per-cell rows, the agreement counts, the split"""
    ids_a, ids_b = labels_of(mask_a), labels_of(mask_b)
    tab_a, tab_b = id_table(ids_a), id_table(ids_b)
    n, m = len(ids_a), len(ids_b)
    pairs, area_a, area_b = overlap(mask_a, tab_a, n, mask_b, tab_b, m)
    owner, inside = owners(pairs, area_b, min_overlap)
    cells = cell_rows(pairs, area_a, ids_b, owner)
    objects = object_rows(pairs, area_b, ids_a, owner, inside)
    inner, outer = compartments(mask_a, tab_a, n, mask_b, tab_b, m, owner)
    return {"ids_a": ids_a, "ids_b": ids_b, "pairs": pairs, "cells": cells, "objects": objects, "owner": owner, "inner": inner, "outer": outer,
            "agreement": agreement_counts(pairs, area_a, area_b),
            "cells_csv": cells_csv(ids_a, cells, types, names), "objects_csv": objects_csv(ids_b, objects),
            "pairs_csv": pairs_csv(ids_a, ids_b, pair_rows(pairs, area_a, area_b))}


def shifted_second_mask(mask, shift=2, zeroed=3, merged=2):
    """B of the end-to-end case: the mask moved ``shift`` columns to the right, its first ``zeroed`` labels set to 0 and the next ``merged``
    labels made one"""
    mask = np.asarray(mask).astype(np.int32)
    out = np.zeros_like(mask)
    out[:, shift:] = mask[:, :mask.shape[1] - shift]
    ids = labels_of(mask)
    for v in ids[:zeroed]:
        out[out == v] = 0
    for v in ids[zeroed + 1:zeroed + merged]:
        out[out == v] = ids[zeroed]
    return out
