"""Host side of the mask repair (ImageProcessor(repair_mask=A), ops.repair_labels, csrc/components.hip): the decisions between the kernels, over
the compacted component rows of ribca_mask_components -- about as many as the mask has cells, not as many as it has pixels.  The rules:

1. of the components of a label v in the mask as read, the MAIN one is the one of the largest area, the smallest root among equal areas;
2. a foreground component of fewer than ``min_area`` pixels is DROPPED (its pixels become 0), main or not;
3. a component that is neither main nor dropped is SPLIT off: it gets the id ``largest label + 1 + k``, k its rank among the split components by
   ascending root;
4. in the components of THAT mask, a background component that touches no image border and is bordered by exactly one label (lo == hi > 0) is a
   HOLE and takes that label;
5. a background component that is enclosed but bordered by several labels stays background and is counted as ``holes_left``.

Integers only; no torch here.  DESIGN.md section 23."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

INT32_MAX = 2 ** 31 - 1
#: the columns of {batch_id}_repair_{image number}.csv and of the component rows ops.repair_labels returns (action as its index in ACTIONS)
COLUMNS = ("source_id", "row", "col", "area", "action", "id", "filled")
ACTIONS = ("kept", "split", "dropped")
KEPT, SPLIT, DROPPED = 0, 1, 2


def check_min_area(min_area, what: str = "min_area", allow_zero: bool = False) -> int:
    """``min_area`` as an int, ValueError unless it is an integer (no bool) >= 1 and <= INT32_MAX, or 0 where that means "do not repair" """
    low = 0 if allow_zero else 1
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or not low <= int(min_area) <= INT32_MAX:
        raise ValueError(f"{what} must be an integer from {low} pixels up, got {min_area!r}")
    return int(min_area)


def decide(roots, labels, areas, min_area: int) -> Tuple[np.ndarray, np.ndarray]:
    """Rules 1 to 3 over the FOREGROUND components of the mask as read, given in ascending order of their roots: (action (n,) int64 -- an index
    into ACTIONS --, id (n,) int64 -- the label of the component in the repaired mask, 0 where dropped).  ValueError where a new id would pass
    INT32_MAX."""
    roots = np.asarray(roots, dtype=np.int64).reshape(-1)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    areas = np.asarray(areas, dtype=np.int64).reshape(-1)
    a = check_min_area(min_area)
    n = len(roots)
    if len(labels) != n or len(areas) != n:
        raise ValueError(f"decide takes one label and one area per component, got {len(labels)} and {len(areas)} for {n} components")
    if n and ((labels <= 0).any() or (areas <= 0).any() or (np.diff(roots) <= 0).any()):
        raise ValueError("decide takes foreground components (label > 0, area > 0) in ascending order of their roots")
    action = np.zeros(n, dtype=np.int64)
    new_id = labels.copy()
    if n == 0:
        return action, new_id
    order = np.lexsort((roots, -areas, labels))      # by label, then the largest area, then the smallest root
    first = np.ones(n, dtype=bool)
    first[1:] = labels[order][1:] != labels[order][:-1]
    main = np.zeros(n, dtype=bool)
    main[order[first]] = True
    dropped = areas < a
    split = ~main & ~dropped
    action[split] = SPLIT
    action[dropped] = DROPPED
    new_id[dropped] = 0
    k = int(split.sum())
    if k:
        top = int(labels.max())
        if top + k > INT32_MAX:
            raise ValueError(f"repair would split off {k} components above the largest label {top}: the new ids pass INT32_MAX")
        new_id[split] = top + 1 + np.arange(k, dtype=np.int64)      # the rows are in ascending order of their roots
    return action, new_id


def fill(labels, border, lo, hi) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Rules 4 and 5 over ALL components of the mask that rules 1 to 3 gave (``labels``: the value of the mask at each root): (the label every
    component takes (m,) int64 -- 0 for background that stays --, hole (m,) bool, left (m,) bool)"""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    border = np.asarray(border, dtype=np.int64).reshape(-1)
    lo = np.asarray(lo, dtype=np.int64).reshape(-1)
    hi = np.asarray(hi, dtype=np.int64).reshape(-1)
    enclosed = (labels <= 0) & (border == 0)
    hole = enclosed & (lo == hi) & (lo > 0)
    left = enclosed & ~hole
    new = np.where(labels > 0, labels, 0)
    new[hole] = lo[hole]
    return new, hole, left


def rows(roots, labels, areas, action, new_id, width: int, hole_labels, hole_areas) -> np.ndarray:
    """(n, 7) int64 in the order of COLUMNS, one row per foreground component of the mask as read, sorted by (source id, root).  ``hole_labels``
    and ``hole_areas``: the label and the pixels of every hole that was filled; a label of the repaired mask is one component, which takes them"""
    roots = np.asarray(roots, dtype=np.int64).reshape(-1)
    new_id = np.asarray(new_id, dtype=np.int64).reshape(-1)
    out = np.zeros((len(roots), len(COLUMNS)), dtype=np.int64)
    out[:, 0] = np.asarray(labels, dtype=np.int64).reshape(-1)
    out[:, 1], out[:, 2] = roots // int(width), roots % int(width)
    out[:, 3] = np.asarray(areas, dtype=np.int64).reshape(-1)
    out[:, 4] = np.asarray(action, dtype=np.int64).reshape(-1)
    out[:, 5] = new_id
    hole_labels = np.asarray(hole_labels, dtype=np.int64).reshape(-1)
    if len(hole_labels):
        ids, inverse = np.unique(hole_labels, return_inverse=True)
        added = np.zeros(len(ids), dtype=np.int64)
        np.add.at(added, inverse, np.asarray(hole_areas, dtype=np.int64).reshape(-1))
        at = np.searchsorted(ids, new_id)
        at[at == len(ids)] = 0
        hit = (ids[at] == new_id) & (new_id > 0)
        out[hit, 6] = added[at[hit]]
    return out[np.lexsort((roots, out[:, 0]))]


def cells_csv(table) -> str:
    """one line per foreground component of the mask as read, ordered by (source id, root); every column an integer but ``action``"""
    lines = [",".join(COLUMNS)]
    for row in np.asarray(table, dtype=np.int64).reshape(-1, len(COLUMNS)).tolist():
        lines.append(",".join(ACTIONS[v] if k == 4 else str(v) for k, v in enumerate(row)))
    return "\n".join(lines) + "\n"


def stats(table, min_area: int, holes_filled: int, hole_pixels: int, holes_left: int, repair_ms: float = 0.0) -> Dict[str, float]:
    """the record of Annotator.repair_stats for one image"""
    table = np.asarray(table, dtype=np.int64).reshape(-1, len(COLUMNS))
    dropped = table[:, 4] == DROPPED
    ids_in = np.unique(table[:, 0])
    survivors = np.unique(table[~dropped, 0])
    return {"min_area": int(min_area), "labels_in": int(len(ids_in)), "labels_out": int(len(np.unique(table[~dropped, 5]))),
            "components_split": int((table[:, 4] == SPLIT).sum()), "components_dropped": int(dropped.sum()),
            "dropped_pixels": int(table[dropped, 3].sum()), "labels_removed": int(len(ids_in) - len(survivors)),
            "holes_filled": int(holes_filled), "hole_pixels": int(hole_pixels), "holes_left": int(holes_left), "repair_ms": float(repair_ms)}
