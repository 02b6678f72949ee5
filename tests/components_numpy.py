"""Python restatement of the connected components of a mask and of the mask repair, written from the rules include/ribca_hip.h states for
ribca_mask_components and repair.py states for the repair: a flood fill in raster order -- the first pixel a fill starts from is the smallest
index of its component --, the repair as plain loops over labels, and the text of the repair CSV.  Also the damaged masks of the tests: random
discs with holes, specks and duplicated labels, and the special shapes (serpentine, comb, diagonal ring) in units of the kernel's pixel tile."""
import numpy as np

import expand_numpy as EN

INT32_MAX = 2 ** 31 - 1
N4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def components(mask):
    """(root (H, W) int32, stats (H W, 4) int32) of ``mask``"""
    mask = np.asarray(mask, dtype=np.int32)
    h, w = mask.shape
    cls = np.where(mask > 0, mask, 0).tolist()
    root = [[-1] * w for _ in range(h)]
    stats = np.zeros((h * w, 4), dtype=np.int32)
    for r0 in range(h):
        for c0 in range(w):
            if root[r0][c0] >= 0:
                continue
            p = r0 * w + c0
            v = cls[r0][c0]
            steps = N8 if v > 0 else N4
            root[r0][c0] = p
            stack = [(r0, c0)]
            area, border, lo, hi = 0, 0, 0, 0
            while stack:
                r, c = stack.pop()
                area += 1
                if r == 0 or r == h - 1 or c == 0 or c == w - 1:
                    border = 1
                for dr, dc in N4:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < h and 0 <= cc < w and cls[rr][cc] > 0 and cls[rr][cc] != v:
                        u = cls[rr][cc]
                        lo = u if lo == 0 or u < lo else lo
                        hi = u if u > hi else hi
                for dr, dc in steps:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < h and 0 <= cc < w and cls[rr][cc] == v and root[rr][cc] < 0:
                        root[rr][cc] = p
                        stack.append((rr, cc))
            stats[p] = (area, border, lo, hi)
    return np.array(root, dtype=np.int32), stats


def repair(mask, min_area):
    """(the repaired mask (H, W) int32, the text of the repair CSV, the counts) by the five rules"""
    mask = np.asarray(mask, dtype=np.int32)
    h, w = mask.shape
    root, stats = components(mask)
    flat = mask.reshape(-1)
    by_label = {}
    for p in np.flatnonzero(stats[:, 0] > 0).tolist():
        if flat[p] > 0:
            by_label.setdefault(int(flat[p]), []).append(p)
    comps = {}      # root -> [source id, area, action, id, filled]
    split = []
    for v, roots in by_label.items():
        main = min(roots, key=lambda p: (-int(stats[p, 0]), p))
        for p in roots:
            area = int(stats[p, 0])
            if area < min_area:
                comps[p] = [v, area, "dropped", 0, 0]
            elif p == main:
                comps[p] = [v, area, "kept", v, 0]
            else:
                comps[p] = [v, area, "split", None, 0]
                split.append(p)
    top = max(by_label) if by_label else 0
    if split and top + len(split) > INT32_MAX:
        raise ValueError("the new ids pass INT32_MAX")
    for k, p in enumerate(sorted(split)):
        comps[p][3] = top + 1 + k
    mid = np.zeros(h * w, dtype=np.int32)
    rflat = root.reshape(-1)
    for p, rec in comps.items():
        mid[rflat == p] = rec[3]
    mid = mid.reshape(h, w)
    root2, stats2 = components(mid)
    out = mid.copy()
    owner = {rec[3]: p for p, rec in comps.items() if rec[3] > 0}
    holes_filled = hole_pixels = holes_left = 0
    for p in np.flatnonzero(stats2[:, 0] > 0).tolist():
        if mid.reshape(-1)[p] > 0 or stats2[p, 1]:
            continue
        area, _, lo, hi = (int(x) for x in stats2[p])
        if lo == hi and lo > 0:
            out[root2 == p] = lo
            comps[owner[lo]][4] += area
            holes_filled += 1
            hole_pixels += area
        else:
            holes_left += 1
    lines = ["source_id,row,col,area,action,id,filled"]
    for p in sorted(comps, key=lambda p: (comps[p][0], p)):
        v, area, action, new, filled = comps[p]
        lines.append("%d,%d,%d,%d,%s,%d,%d" % (v, p // w, p % w, area, action, new, filled))
    dropped = [rec for rec in comps.values() if rec[2] == "dropped"]
    alive = {rec[0] for rec in comps.values() if rec[2] != "dropped"}
    counts = {"min_area": int(min_area), "labels_in": len(by_label), "labels_out": len(owner), "components_split": len(split),
              "components_dropped": len(dropped), "dropped_pixels": sum(rec[1] for rec in dropped), "labels_removed": len(by_label) - len(alive),
              "holes_filled": holes_filled, "hole_pixels": hole_pixels, "holes_left": holes_left}
    return out, "\n".join(lines) + "\n", counts


def damaged_discs(h, w, cells, seed):
    """random discs, then the faults of a stitched or hand-edited mask: labels used twice, holes of one to six pixels, specks of one to four
    pixels of an existing label elsewhere -- some of them inside a hole of another cell"""
    rng = np.random.RandomState(seed + 1000)
    mask = EN.random_discs(h, w, cells, seed, rmin=3.0, rmax=7.0)
    ids = np.unique(mask[mask > 0])
    for _ in range(max(2, cells // 8)):                      # duplicated labels
        a, b = rng.choice(ids, 2, replace=False)
        mask[mask == a] = b
    inner = np.argwhere(mask > 0)
    for _ in range(cells // 2):                              # holes
        r, c = inner[rng.randint(len(inner))]
        hh, ww = rng.randint(1, 3), rng.randint(1, 4)
        mask[r:r + hh, c:c + ww] = 0
    for k in range(cells // 2):                              # specks
        r, c = rng.randint(0, h), rng.randint(0, w)
        if k % 3 == 0:
            r, c = inner[rng.randint(len(inner))]            # over a cell: a foreign speck, or one inside a hole
        hh, ww = rng.randint(1, 3), rng.randint(1, 3)
        mask[r:r + hh, c:c + ww] = rng.choice(ids)
    return mask


def serpentine(tile, value, ground):
    """a one-pixel-wide path of ``value`` on ``ground`` that winds through 3 x 3 tiles: every second row is full, joined to the next full row at
    alternating ends, so that the path crosses every vertical seam in every full row"""
    n = 3 * tile
    mask = np.full((n, n), ground, dtype=np.int32)
    for k, r in enumerate(range(0, n, 2)):
        mask[r, :] = value
        if r + 1 < n:
            mask[r + 1, n - 1 if k % 2 == 0 else 0] = value
    return mask


def comb(tile, value=3):
    """teeth that run down through two tiles and meet only in the last row, in the third tile"""
    n = 3 * tile
    mask = np.zeros((n, n), dtype=np.int32)
    mask[0:n, 1:n:3] = value
    mask[n - 1, :] = value
    return mask


def special_masks(tile):
    """name -> mask: the shapes whose components the tests state in words"""
    t = tile
    out = {}
    for name, (a, b) in {"diagonal_down": ((t - 1, t - 1), (t, t)), "diagonal_up": ((t, t - 1), (t - 1, t))}.items():
        m = np.zeros((2 * t, 2 * t), dtype=np.int32)
        m[a], m[b] = 5, 5
        out[name] = m
    m = np.zeros((2 * t, 2 * t), dtype=np.int32)      # a background pixel at a tile corner inside a diagonal ring of label 7
    for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        m[t + dr, t + dc] = 7
    out["diagonal_ring"] = m
    m = np.zeros((t + 8, 2 * t), dtype=np.int32)
    m[4:12, t - 6:t], m[4:12, t:t + 6] = 2, 9         # two labels side by side across a seam
    out["side_by_side"] = m
    m = np.zeros((t + 3, 3 * t), dtype=np.int32)
    m[2:7, 2:7], m[t - 2:t + 2, 3 * t - 6:3 * t - 1] = 4, 4      # one label in two distant blobs
    out["two_blobs"] = m
    out["serpentine"] = serpentine(t, 6, 0)
    out["channel"] = serpentine(t, 0, 6)
    out["comb"] = comb(t)
    m = np.zeros((t + 5, t + 9), dtype=np.int32)
    m[3:9, 3:9], m[3:9, 9:14], m[t:t + 4, t - 2:t + 6] = INT32_MAX, INT32_MAX - 1, INT32_MAX
    out["near_int32_max"] = m
    m = EN.random_discs(t + 9, 2 * t + 3, 12, 3)
    neg = (np.arange(m.size).reshape(m.shape) % 3 == 0) & (m == 0)
    m[neg] = -4
    m[0, 0] = -(2 ** 31)
    out["negative"] = m
    return out
