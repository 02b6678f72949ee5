"""The host side of the cell outlines (Annotator.cell_outlines): the rings ops.mask_rings traced -- rows ``cell, start, vertices, edges, area2,
saddles`` sorted by (cell, start), ``first`` and the kept ``vertices`` [r, c] -- grouped into polygons with holes, and the text of the two files
of an image: a GeoJSON FeatureCollection in the layout QuPath documents for its own export (one detection per cell) and a per-cell CSV.  No GPU
and no float: everything here is integer arithmetic on the rows.  include/ribca_hip.h states the lattice, the ring row and the saddle rule; by that
rule a ring may touch itself or another ring of its cell at a saddle vertex, which strict validators call invalid -- the ``saddles`` column of the
CSV says for which cells that can happen."""
from __future__ import annotations

import json
from typing import List, Optional, Sequence, Tuple

import numpy as np

CELL, START, VERTICES, EDGES, AREA2, SADDLES = range(6)


def _check(rings, first, vertices):
    rings = np.asarray(rings, dtype=np.int64).reshape(-1, 6)
    first = np.asarray(first, dtype=np.int64).reshape(-1)
    vertices = np.asarray(vertices, dtype=np.int64).reshape(-1, 2)
    if len(first) != len(rings) + 1 or first[0] != 0 or not np.array_equal(np.diff(first), rings[:, VERTICES]) or first[-1] != len(vertices):
        raise ValueError("outlines: first is not the prefix sum of the rings' vertex counts over the vertices given")
    key = rings[:, :2].tolist()
    if key != sorted(key):
        raise ValueError("outlines: the rings are not sorted by (cell, start)")
    return rings, first, vertices


def _inside(points: np.ndarray, r: int, c: int) -> bool:
    """is the centre of pixel (r, c) inside the ring ``points``: an even-odd count of the ring's vertical edges to the left of it that span its row"""
    nxt = np.roll(points, -1, axis=0)
    vertical = points[:, 1] == nxt[:, 1]
    lo, hi = np.minimum(points[:, 0], nxt[:, 0]), np.maximum(points[:, 0], nxt[:, 0])
    return bool(int((vertical & (points[:, 1] <= c) & (lo <= r) & (r < hi)).sum()) & 1)


def polygons(rings, first, vertices, n: int) -> List[List[Tuple[int, List[int]]]]:
    """The rings of each of the ``n`` cells grouped into polygons: per cell a list of ``(exterior, holes)``, ring indices into ``rings``, the
    polygons in the order of their exteriors' ``start`` and the holes of each by ``start``; a cell without a pixel has an empty list.  A ring with
    area2 > 0 is an exterior, one with area2 < 0 a hole.  A hole of a cell with one exterior belongs to it; with several, the pixel at the hole's
    start vertex -- it lies inside the hole -- is tested against every exterior (``_inside``, exact), and because an exterior may lie inside the
    hole of another the hole goes to the containing exterior of smallest area2."""
    rings, first, vertices = _check(rings, first, vertices)
    if len(rings) and (rings[:, CELL].min() < 0 or rings[:, CELL].max() >= n):
        raise ValueError(f"outlines: a ring names a cell outside 0 .. {n - 1}")
    out: List[List[Tuple[int, List[int]]]] = [[] for _ in range(n)]
    by_cell: List[List[int]] = [[] for _ in range(n)]
    for k in range(len(rings)):
        by_cell[int(rings[k, CELL])].append(k)
    for i, members in enumerate(by_cell):
        exteriors = [k for k in members if rings[k, AREA2] > 0]
        parts = {k: [] for k in exteriors}
        for k in members:
            if rings[k, AREA2] > 0:
                continue
            if len(exteriors) == 1:
                parts[exteriors[0]].append(k)
                continue
            r, c = (int(v) for v in vertices[first[k]])
            around = [e for e in exteriors if _inside(vertices[first[e]:first[e + 1]], r, c)]
            if not around:
                raise ValueError(f"outlines: the hole of cell {i} at vertex ({r}, {c}) lies in none of its exterior rings")
            parts[min(around, key=lambda e: int(rings[e, AREA2]))].append(k)
        out[i] = [(e, parts[e]) for e in exteriors]      # members are sorted by start, so both lists are
    return out


def cell_table(rings, n: int) -> np.ndarray:
    """(n, 6) int64 per cell: area in pixels, exterior rings, hole rings, kept vertices, boundary edges, saddle passes"""
    rings = np.asarray(rings, dtype=np.int64).reshape(-1, 6)
    table = np.zeros((n, 6), dtype=np.int64)
    cell = rings[:, CELL]
    for col, values in enumerate((rings[:, AREA2], rings[:, AREA2] > 0, rings[:, AREA2] < 0, rings[:, VERTICES], rings[:, EDGES], rings[:, SADDLES])):
        np.add.at(table[:, col], cell, values.astype(np.int64))
    if (table[:, 0] & 1).any():
        raise ValueError("outlines: the rings of a cell do not close (odd area2)")
    table[:, 0] //= 2
    return table


def _ring_text(points: np.ndarray) -> str:
    """[[c,r],...] closed by its first vertex"""
    pts = points.tolist()
    return "[" + ",".join(f"[{c},{r}]" for r, c in pts + pts[:1]) + "]"


def geojson(rings, first, vertices, cell_ids, types=None, names: Optional[Sequence[str]] = None, colours=None, confidence: Optional[Sequence[str]] = None) -> str:
    """The GeoJSON text of one image: one FeatureCollection, one Feature per line in ``cell_ids`` order (a cell without a pixel has none), no
    spaces.  A cell with one exterior ring is a ``Polygon``, a cell with several a ``MultiPolygon`` whose polygons follow their exteriors'
    ``start``; in a polygon the exterior comes first, then its holes by ``start``.  Coordinates are integers ``[c, r]`` = [x, y] in pixel
    units with the origin at the top-left corner of the image and y downwards (vertex (r, c) is the top-left corner of pixel (r, c)), every ring
    closed by repeating its first vertex.  The WINDING STAYS AS TRACED: exterior rings run clockwise on the screen (x to the right, y down),
    holes counter-clockwise -- in a y-up reading that is the counter-clockwise exterior RFC 7946 recommends; nothing is re-oriented.
    ``properties``: ``"objectType":"detection"``, ``"name"`` = the cell id as a string, with ``types`` (an index into ``names`` per cell) also
    ``"classification":{"name":...,"color":[r,g,b]}`` (``colours``: one RGB row per entry of ``names``), and ``"measurements"``: ``id``, ``area``
    (pixels) and, with ``confidence`` (one JSON number as text per cell), ``confidence``.  Without ``types`` the classification and the confidence are absent."""
    rings, first, vertices = _check(rings, first, vertices)
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    n = len(ids)
    parts = polygons(rings, first, vertices, n)
    area = cell_table(rings, n)[:, 0]
    if types is not None:
        lab = np.asarray(types).astype(np.int64).reshape(-1)
        rgb = np.asarray(colours).astype(np.int64).reshape(-1, 3)
        if lab.shape != (n,) or names is None or len(rgb) < len(names) or (n and (lab.min() < 0 or lab.max() >= len(names))):
            raise ValueError("geojson takes one cell-type index per cell, the names they index and one colour per name")
        if confidence is not None and len(confidence) != n:
            raise ValueError("geojson takes one confidence per cell")
    features = []
    for i in range(n):
        if not parts[i]:
            continue
        shapes = ["[" + ",".join(_ring_text(vertices[first[k]:first[k + 1]]) for k in [e] + holes) + "]" for e, holes in parts[i]]
        if len(shapes) == 1:
            geometry = '{"type":"Polygon","coordinates":' + shapes[0] + "}"
        else:
            geometry = '{"type":"MultiPolygon","coordinates":[' + ",".join(shapes) + "]}"
        props = '"objectType":"detection","name":' + json.dumps(str(int(ids[i])))
        measurements = f'"id":{int(ids[i])},"area":{int(area[i])}'
        if types is not None:
            t = int(lab[i])
            props += ',"classification":{"name":' + json.dumps(str(names[t])) + f',"color":[{int(rgb[t, 0])},{int(rgb[t, 1])},{int(rgb[t, 2])}]' + "}"
            if confidence is not None:
                measurements += f',"confidence":{confidence[i]}'
        features.append('{"type":"Feature","geometry":' + geometry + ',"properties":{' + props + ',"measurements":{' + measurements + "}}}")
    return '{"type":"FeatureCollection","features":[\n' + ",\n".join(features) + "\n]}\n"


def cells_csv(rings, cell_ids, types=None, names: Optional[Sequence[str]] = None) -> str:
    """one line per cell in ``cell_ids`` order: ``id``, with ``types`` ``cell type``, then ``area,exteriors,holes,vertices,boundary_edges,saddles``"""
    ids = np.asarray(cell_ids).astype(np.int64).reshape(-1)
    n = len(ids)
    table = cell_table(rings, n)
    lab = None if types is None else np.asarray(types).astype(np.int64).reshape(-1)
    if lab is not None and (lab.shape != (n,) or names is None):
        raise ValueError("cells_csv takes one cell-type index per cell and the names they index")
    lines = ["id," + ("cell type," if lab is not None else "") + "area,exteriors,holes,vertices,boundary_edges,saddles"]
    for i in range(n):
        kind = "" if lab is None else (str(names[int(lab[i])]) if 0 <= int(lab[i]) < len(names) else "") + ","
        lines.append(f"{int(ids[i])},{kind}" + ",".join(str(int(v)) for v in table[i]))
    return "\n".join(lines) + "\n"


def image_stats(rings, n: int) -> dict:
    """the counts of one image's record in ``outline_stats``"""
    rings = np.asarray(rings, dtype=np.int64).reshape(-1, 6)
    table = cell_table(rings, n)
    return {"n": int(n), "rings": int(len(rings)), "holes": int(table[:, 2].sum()), "multi_part": int((table[:, 1] > 1).sum()),
            "vertices": int(table[:, 3].sum()), "saddles": int(table[:, 5].sum()), "longest_ring": int(rings[:, EDGES].max()) if len(rings) else 0}
