"""Python restatement of the cell outlines, written from the definitions include/ribca_hip.h states for ribca_mask_rings and
ribca_mask_ring_vertices, in plain loops and NOT in the form of the kernels (no candidates, no walkers that abort): every boundary edge of every
cell goes into a set, the successor of an edge is looked up among the cell's outgoing edges at the vertex it ends in (the left turn where there
are two), the set is taken apart into cycles, and every cycle is turned so that it begins at its smallest vertex.  Also ``rasterise``, the
even-odd fill that gives the pixels back, the label -> cell table as ops.mask_rings builds it, and the masks of the tests."""
import numpy as np

import components_numpy as CN

STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))      # east, south, west, north as (dr, dc)


def label_table(mask):
    """(label_to_cell int32, ids ascending int64) as ops.contact_graph builds them: cell k = the k-th label > 0"""
    mask = np.asarray(mask)
    ids = np.unique(mask[mask > 0]).astype(np.int64)
    table = np.full(int(ids.max()) + 1 if len(ids) else 1, -1, dtype=np.int32)
    table[ids] = np.arange(len(ids), dtype=np.int32)
    table[0] = -1
    return table, ids


def owners(mask, label_to_cell, n):
    """(H, W) int64: the cell every pixel belongs to, -1 for none"""
    mask = np.asarray(mask, dtype=np.int64)
    table = np.asarray(label_to_cell, dtype=np.int64)
    inside = (mask >= 0) & (mask < len(table))
    cell = np.where(inside, table[np.where(inside, mask, 0)], -1)
    return np.where((cell >= 0) & (cell < n), cell, -1)


def boundary_edges(own):
    """cell -> set of (r, c, d): the directed unit edge that leaves vertex (r, c) in direction d with a pixel of the cell on its right"""
    h, w = own.shape
    pad = np.full((h + 2, w + 2), -1, dtype=np.int64)
    pad[1:-1, 1:-1] = own
    pad = pad.tolist()
    edges = {}
    for r in range(h):
        for c in range(w):
            i = pad[r + 1][c + 1]
            if i < 0:
                continue
            mine = edges.setdefault(i, set())
            if pad[r][c + 1] != i:
                mine.add((r, c, 0))              # top
            if pad[r + 1][c + 2] != i:
                mine.add((r, c + 1, 1))          # right
            if pad[r + 2][c + 1] != i:
                mine.add((r + 1, c + 1, 2))      # bottom
            if pad[r + 1][c] != i:
                mine.add((r + 1, c, 3))          # left
    return edges


def cycles(edge_set):
    """the rings of one cell: lists of edges (r, c, d), each beginning at the edge that leaves the ring's smallest vertex, with the number of
    saddle passes beside it"""
    out = []
    left = set(edge_set)
    while left:
        first = min(left)
        ring, saddles = [], 0
        e = first
        while True:
            ring.append(e)
            left.remove(e)
            r, c, d = e
            r, c = r + STEP[d][0], c + STEP[d][1]
            onward = [k for k in range(4) if (r, c, k) in edge_set]
            assert len(onward) in (1, 2)
            if len(onward) == 2:                 # a saddle: the left turn
                saddles += 1
                assert (d + 3) % 4 in onward
                e = (r, c, (d + 3) % 4)
            else:
                e = (r, c, onward[0])
            if e == first:
                break
        k = min(range(len(ring)), key=lambda j: ring[j][:2])
        assert [x[:2] for x in ring].count(ring[k][:2]) == 1      # a ring passes its smallest vertex once
        out.append((ring[k:] + ring[:k], saddles))
    return out


def trace(mask, label_to_cell, n):
    """(rings (R, 6) int64 sorted by (cell, start), first (R + 1) int64, vertices (first[R], 2) int32) of the mask"""
    mask = np.asarray(mask, dtype=np.int32)
    h, w = mask.shape
    own = owners(mask, label_to_cell, n)
    rows = []
    for i, edge_set in boundary_edges(own).items():
        for ring, saddles in cycles(edge_set):
            kept = [ring[j][:2] for j in range(len(ring)) if ring[j][2] != ring[j - 1][2]]
            assert kept[0] == ring[0][:2]        # the start is a vertex at which the direction changes
            area2 = 0
            for j in range(len(kept)):
                (r0, c0), (r1, c1) = kept[j], kept[(j + 1) % len(kept)]
                area2 += c0 * r1 - c1 * r0
            rows.append(((i, ring[0][0] * (w + 1) + ring[0][1], len(kept), len(ring), area2, saddles), kept, ring[0][2]))
    rows.sort(key=lambda x: x[0][:2])
    rings = np.array([x[0] for x in rows], dtype=np.int64).reshape(-1, 6)
    first = np.zeros(len(rows) + 1, dtype=np.int64)
    first[1:] = np.cumsum(rings[:, 2])
    vertices = np.array([v for x in rows for v in x[1]], dtype=np.int32).reshape(-1, 2)
    return rings, first, vertices


def leaving(rings, first, vertices):
    """the direction every ring leaves its start in: 0 east, 1 south"""
    out = []
    for k in range(len(rings)):
        (r0, c0), (r1, c1) = vertices[first[k]], vertices[first[k] + 1]
        out.append(0 if (r1 == r0 and c1 > c0) else 1 if (c1 == c0 and r1 > r0) else -1)
    return np.array(out, dtype=np.int64)


def rasterise(rings, first, vertices, h, w):
    """(H, W) int64, the cell of every pixel by the even-odd rule over the rings of each cell, -1 for none: a pixel is inside when the ray from
    its centre to the left crosses an odd number of the cell's vertical edges"""
    out = np.full((h, w), -1, dtype=np.int64)
    cells = np.unique(rings[:, 0]) if len(rings) else []
    for i in cells:
        fill = np.zeros((h, w), dtype=bool)
        for k in np.flatnonzero(rings[:, 0] == i):
            pts = vertices[first[k]:first[k + 1]].astype(np.int64)
            for j in range(len(pts)):
                (r0, c0), (r1, c1) = pts[j], pts[(j + 1) % len(pts)]
                assert (r0 == r1) != (c0 == c1)      # axis-parallel, never of length 0
                if c0 == c1:
                    fill[min(r0, r1):max(r0, r1), c0:] ^= True
        assert (out[fill] == -1).all()               # no pixel is inside two cells
        out[fill] = i
    return out


# ---- the masks of the tests ---------------------------------------------------------------------------------------------------------------------
def seam_discs():
    """the ``discs`` fixture of tests/test_gpu_components.py: 67 x 131, damaged discs and bars across every seam of 32 x 32 tiles"""
    mask = CN.damaged_discs(67, 131, 40, 11)
    mask[31:33, 40:60] = 41
    mask[5:20, 63:65] = 42
    mask[30:36, 128:131] = 43
    mask[63:66, 10:120] = 44
    mask[2:66, 95:98] = 45
    return mask


def ranked(mask):
    """the mask with every label > 0 replaced by its rank 1, 2, ... among the labels; everything else stays"""
    mask = np.asarray(mask, dtype=np.int32)
    ids = np.unique(mask[mask > 0])
    out = mask.copy()
    out[mask > 0] = (np.searchsorted(ids, mask[mask > 0]) + 1).astype(np.int32)
    return out


def special_masks(tile):
    """CN.special_masks(tile) for the outlines.  A cell is named through label_to_cell, whose length L is an int32, so the label INT32_MAX of
    ``near_int32_max`` can own no pixel under any table (and a table up to its neighbour would hold 2^31 - 1 entries): that shape is traced
    with its labels ranked, 1 and 2, and ``near_int32_max_as_read`` is what the tests trace with a short table, where both labels lie at
    or above L and the mask has no ring."""
    out = dict(CN.special_masks(tile))
    out["near_int32_max"] = ranked(out["near_int32_max"])
    return out


def checkerboard():
    rr, cc = np.mgrid[0:8, 0:8]
    return (((rr + cc) % 2) * 3).astype(np.int32)


def nested_ring():
    """a 7 x 7 frame of label 4 in a 9 x 9 image, hollowed to 5 x 5, and one pixel of 4 at the centre"""
    mask = np.zeros((9, 9), dtype=np.int32)
    mask[1:8, 1:8] = 4
    mask[2:7, 2:7] = 0
    mask[4, 4] = 4
    return mask


def small_masks():
    """name -> mask: thin, tiny and uniform ones, the checkerboard and the nested ring"""
    line = np.zeros(50, dtype=np.int32)
    line[[3, 4, 20, 49]] = (5, 5, 2, 5)
    lone = np.zeros((33, 33), dtype=np.int32)
    lone[32, 32] = 77
    return {"row": line.reshape(1, 50), "column": line.reshape(50, 1), "pixel": np.full((1, 1), 5, dtype=np.int32), "lone": lone,
            "uniform": np.full((40, 70), 9, dtype=np.int32), "background": np.zeros((40, 70), dtype=np.int32), "checkerboard": checkerboard(),
            "nested": nested_ring()}
