"""Host side of the mask expansion (ImageProcessor(expand_mask=D), ops.expand_labels, csrc/expand.hip): the per-cell table of what the
expansion did, from the label table of the mask as read (the core: a nucleus) and of the mask as grown (the cell) -- both are
ops.label_table's (n, 7) rows ``rmin, rmax, cmin, cmax, sum r, sum c, area`` over the same ascending ids, since expansion makes and removes no
label.  Integers only; no torch here.  DESIGN.md section 22."""
from __future__ import annotations

from typing import Dict

import numpy as np

#: the columns of {batch_id}_expansion_{image number}.csv
COLUMNS = ("id", "area_core", "area_cell", "grown", "rmin", "rmax", "cmin", "cmax")


def rows(cell_ids, core_table, cell_table) -> np.ndarray:
    """(n, 8) int64 in the order of COLUMNS: the id, the pixels of the label before and after, their difference, and the box of the grown cell"""
    ids = np.asarray(cell_ids, dtype=np.int64).reshape(-1)
    core = np.asarray(core_table, dtype=np.int64).reshape(-1, 7)
    cell = np.asarray(cell_table, dtype=np.int64).reshape(-1, 7)
    if len(core) != len(ids) or len(cell) != len(ids):
        raise ValueError(f"rows takes one row of either label table per cell, got {len(core)} and {len(cell)} for {len(ids)} cells")
    out = np.zeros((len(ids), len(COLUMNS)), dtype=np.int64)
    out[:, 0] = ids
    out[:, 1], out[:, 2] = core[:, 6], cell[:, 6]
    out[:, 3] = cell[:, 6] - core[:, 6]
    out[:, 4:8] = cell[:, :4]
    return out


def cells_csv(table) -> str:
    """one line per cell in id order, every column an integer"""
    lines = [",".join(COLUMNS)]
    for row in np.asarray(table, dtype=np.int64).reshape(-1, len(COLUMNS)).tolist():
        lines.append(",".join(str(v) for v in row))
    return "\n".join(lines) + "\n"


def stats(table, distance: int, expand_ms: float) -> Dict[str, float]:
    """the record of Annotator.expansion_stats for one image"""
    table = np.asarray(table, dtype=np.int64).reshape(-1, len(COLUMNS))
    return {"n": int(len(table)), "D": int(distance), "pixels_grown": int(table[:, 3].sum()), "cells_unchanged": int((table[:, 3] == 0).sum()),
            "expand_ms": float(expand_ms)}
