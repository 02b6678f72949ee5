"""numpy restatement of the per-cell morphology sums, written from the rules include/ribca_hip.h states for ribca_mask_morphology: which pixels
belong to which cell (contact_numpy.cell_image), the sixteen columns and the bounding box in two forms -- a plain loop over the definition and
shifted arrays -- and the seeded mask generator of the tests: Voronoi discs with punched holes and scattered fragments."""
import numpy as np

import contact_numpy as CN

COLS = 16
INT32_MAX = 2 ** 31 - 1
FOUR = ((-1, 0), (1, 0), (0, -1), (0, 1))
DIAGONAL = ((-1, -1), (-1, 1), (1, -1), (1, 1))
P_A, P_B, P_C = (5, 7, 15, 17, 25, 27), (21, 33), (13, 23)


def _empty(n):
    sums = np.zeros((n, COLS), dtype=np.int64)
    bbox = np.tile(np.array([INT32_MAX, -1, INT32_MAX, -1], dtype=np.int32), (n, 1))
    return sums, bbox


def sums_loop(mask, label_to_cell, n, rect=None):
    """(sums (n, 16) int64, bbox (n, 4) int32) by the definition, one pixel and one window at a time"""
    cell = CN.cell_image(mask, label_to_cell, n)
    h, w = cell.shape
    sums, bbox = _empty(n)

    def at(r, c):
        return int(cell[r, c]) if 0 <= r < h and 0 <= c < w else -1

    def border(r, c, i):      # (r, c) is a border pixel of cell i
        return at(r, c) == i and any(at(r + dr, c + dc) != i for dr, dc in FOUR)

    for r in range(h):
        for c in range(w):
            i = at(r, c)
            if i < 0:
                continue
            row = sums[i]
            row[0] += 1
            row[1] += r
            row[2] += c
            row[3] += r * r
            row[4] += c * c
            row[5] += r * c
            for dr, dc in FOUR:
                rr, cc = r + dr, c + dc
                if not (0 <= rr < h and 0 <= cc < w):
                    row[8] += 1
                elif at(rr, cc) != i:
                    row[6 if at(rr, cc) >= 0 else 7] += 1
            if border(r, c, i):
                a = sum(border(r + dr, c + dc, i) for dr, dc in FOUR)
                b = sum(border(r + dr, c + dc, i) for dr, dc in DIAGONAL)
                v = 1 + 2 * a + 10 * b
                if v in P_A:
                    row[9] += 1
                elif v in P_B:
                    row[10] += 1
                elif v in P_C:
                    row[11] += 1
            if rect is not None:
                q = rect[i]
                if int(q[0]) <= r < int(q[1]) and int(q[2]) <= c < int(q[3]):
                    row[15] += 1
            bbox[i] = (min(bbox[i, 0], r), max(bbox[i, 1], r), min(bbox[i, 2], c), max(bbox[i, 3], c))
    for r in range(h + 1):      # the window whose lower right pixel is (r, c)
        for c in range(w + 1):
            four = (at(r - 1, c - 1), at(r - 1, c), at(r, c - 1), at(r, c))
            for i in set(four):
                if i < 0:
                    continue
                where = [k for k in range(4) if four[k] == i]
                if len(where) == 1:
                    sums[i, 12] += 1
                elif len(where) == 3:
                    sums[i, 13] += 1
                elif where in ([0, 3], [1, 2]):
                    sums[i, 14] += 1
    return sums, bbox


def _shift(a, dr, dc, fill):
    """b[r, c] = a[r + dr, c + dc], ``fill`` where that leaves the array"""
    h, w = a.shape
    b = np.full_like(a, fill)
    if abs(dr) >= h or abs(dc) >= w:
        return b
    b[max(0, -dr):h - max(0, dr), max(0, -dc):w - max(0, dc)] = a[max(0, dr):h - max(0, -dr), max(0, dc):w - max(0, -dc)]
    return b


def _add(sums, col, cells, values=None):
    """sums[cells, col] += values in integers (bincount's weights are doubles)"""
    np.add.at(sums[:, col], cells, 1 if values is None else values)


def sums_arrays(mask, label_to_cell, n, rect=None):
    """the same by shifted arrays"""
    cell = CN.cell_image(mask, label_to_cell, n)
    h, w = cell.shape
    sums, bbox = _empty(n)
    rr, cc = np.mgrid[0:h, 0:w].astype(np.int64)
    own = cell >= 0
    i = cell[own]
    r, c = rr[own], cc[own]
    _add(sums, 0, i)
    for col, v in ((1, r), (2, c), (3, r * r), (4, c * c), (5, r * c)):
        _add(sums, col, i, v)
    inside = np.ones((h, w), dtype=bool)
    is_border = np.zeros((h, w), dtype=bool)
    for dr, dc in FOUR:
        other = _shift(cell, dr, dc, -1)
        there = _shift(inside, dr, dc, False)
        leaves = own & (other != cell)
        is_border |= leaves
        _add(sums, 6, cell[leaves & there & (other >= 0)])
        _add(sums, 7, cell[leaves & there & (other < 0)])
        _add(sums, 8, cell[leaves & ~there])
    a = sum((_shift(cell, dr, dc, -1) == cell) & _shift(is_border, dr, dc, False) for dr, dc in FOUR)
    b = sum((_shift(cell, dr, dc, -1) == cell) & _shift(is_border, dr, dc, False) for dr, dc in DIAGONAL)
    v = 1 + 2 * a + 10 * b
    for col, values in ((9, P_A), (10, P_B), (11, P_C)):
        _add(sums, col, cell[is_border & np.isin(v, values)])
    ring = np.full((h + 2, w + 2), -1, dtype=np.int64)
    ring[1:-1, 1:-1] = cell
    four = (ring[:-1, :-1], ring[:-1, 1:], ring[1:, :-1], ring[1:, 1:])
    for k, x in enumerate(four):
        first = x >= 0
        for earlier in four[:k]:
            first &= earlier != x
        count = sum((y == x).astype(np.int64) for y in four)
        partner = four[3 - k]      # the pixel on the diagonal
        _add(sums, 12, x[first & (count == 1)])
        _add(sums, 13, x[first & (count == 3)])
        _add(sums, 14, x[first & (count == 2) & (partner == x)])
    if rect is not None:
        q = np.asarray(rect).astype(np.int64)[i]
        _add(sums, 15, i[(q[:, 0] <= r) & (r < q[:, 1]) & (q[:, 2] <= c) & (c < q[:, 3])])
    if len(i):
        lo_r, hi_r = np.full(n, INT32_MAX, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        lo_c, hi_c = lo_r.copy(), hi_r.copy()
        np.minimum.at(lo_r, i, r)
        np.maximum.at(hi_r, i, r)
        np.minimum.at(lo_c, i, c)
        np.maximum.at(hi_c, i, c)
        bbox = np.stack([lo_r, hi_r, lo_c, hi_c], axis=1).astype(np.int32)
    return sums, bbox


def generated_mask(h=96, w=80, cells=60, seed=7, radius=9.0):
    """(h, w) int32 with the labels 1 .. cells: Voronoi discs (contact_numpy.random_mask), then in two cells out of three a punched hole of one
    to four pixels at a pixel of the cell that has all its eight neighbours in the cell, and for half of the cells one to three fragments of
    one or two pixels at random places of the image (over the background or over other cells)"""
    rng = np.random.RandomState(seed)
    mask = CN.random_mask(h, w, cells, seed, radius)
    base = mask.copy()
    for label in range(1, cells + 1):
        if label % 3 == 0:
            continue
        solid = base == label
        for dr, dc in FOUR + DIAGONAL:
            solid &= _shift(base, dr, dc, 0) == label
        spots = np.argwhere(solid)
        if len(spots) == 0:
            continue
        r, c = spots[rng.randint(len(spots))]
        mask[r, c] = 0
        for dr, dc in FOUR[:rng.randint(0, 4)]:
            if base[r + dr, c + dc] == label:
                mask[r + dr, c + dc] = 0
    for label in range(1, cells + 1, 2):
        for _ in range(rng.randint(1, 4)):
            r, c = rng.randint(0, h), rng.randint(0, w - 1)
            mask[r, c:c + rng.randint(1, 3)] = label
    return mask


def windows_and_others(bbox, h, w, patch, seed):
    """(n, 4) int32 rectangles: the crop window (rmid = (rmin + rmax) // 2, r0 = max(rmid - (patch + 1) // 2, 0), r1 = min(r0 + patch, h), columns
    likewise) for the even cells, arbitrary rows -- some empty, some negative, some past the image -- for the odd ones"""
    rng = np.random.RandomState(seed)
    n = len(bbox)
    rect = np.zeros((n, 4), dtype=np.int32)
    for i in range(n):
        if i % 2 == 0:
            rmid, cmid = (int(bbox[i, 0]) + int(bbox[i, 1])) // 2, (int(bbox[i, 2]) + int(bbox[i, 3])) // 2
            r0, c0 = max(rmid - (patch + 1) // 2, 0), max(cmid - (patch + 1) // 2, 0)
            rect[i] = (r0, min(r0 + patch, h), c0, min(c0 + patch, w))
        else:
            a, b = rng.randint(-5, h + 5, 2)
            c, d = rng.randint(-5, w + 5, 2)
            rect[i] = (a, b, c, d)      # empty when b <= a or d <= c
    return rect
