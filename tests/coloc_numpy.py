"""numpy restatement of ribca_cell_coloc, written from the rules include/ribca_hip.h states: per cell the K selected channels over the cell's
pixels in row-major order, the 256 strided partials and the halving tree for the sums, the centred cross products and the gated sums -- a
closed gate skips the element, it does not add a zero --, the strict fp32 gate, and the formulas of colocalization.features as plain loops
over cells and pairs.  ``variant`` breaks the summation order on purpose, for the tests that show their inputs can tell the orders apart."""
import math

import numpy as np

from intensities_numpy import PARTIALS, clipped_box
from localization_numpy import tree


def pairs(k):
    """(0,0), (0,1) .. (0,k-1), (1,1) ..: the order of the ``both`` and ``cross`` columns"""
    return [(a, b) for a in range(k) for b in range(a, k)]


def _tree_sum(values, keep=None, partials=PARTIALS, plain=False):
    """values (R, a) fp64, keep (R, a) bool or None: per row the stated tree over the kept elements; element e belongs to partial
    e mod ``partials`` whatever ``keep`` says.  ``plain``: np.sum's own order instead"""
    rows_n, a = values.shape
    if plain:
        return np.where(keep, values, 0.0).sum(axis=1) if keep is not None else values.sum(axis=1)
    p = np.zeros((rows_n, PARTIALS))
    for r in range(-(-a // partials)):      # row r holds the elements partials r .. partials r + partials - 1: one candidate per partial
        e = slice(r * partials, min((r + 1) * partials, a))
        width = e.stop - e.start
        if keep is None:
            p[:, :width] = p[:, :width] + values[:, e]
        else:
            p[:, :width] = np.where(keep[:, e], p[:, :width] + values[:, e], p[:, :width])      # skipped, not added as zeros
    return tree(p)


def coloc(image, mask, ids, bbox, chan, thr, variant=None):
    """area (n) int32, both (n, P) int32, sums (n, K) fp64, cross (n, P) fp64, gated (n, K, K) fp64.  ``variant``: None for the contract,
    "plain" for np.sum's order, "mod64" for element e in partial e mod 64"""
    image = np.asarray(image, dtype=np.float32)
    _, h, w = image.shape
    chan = [int(c) for c in chan]
    gates = np.asarray(thr, dtype=np.float32).reshape(-1)
    n, k = len(ids), len(chan)
    pr = pairs(k)
    kw = {"plain": variant == "plain", "partials": 64 if variant == "mod64" else PARTIALS}
    area, both = np.zeros(n, dtype=np.int32), np.zeros((n, len(pr)), dtype=np.int32)
    sums, cross, gated = np.zeros((n, k)), np.zeros((n, len(pr))), np.zeros((n, k, k))
    for i in range(n):
        box = clipped_box(bbox[i], h, w)
        if int(ids[i]) <= 0 or box is None:
            continue
        r0, r1, c0, c1 = box
        inside = mask[r0:r1 + 1, c0:c1 + 1] == int(ids[i])
        a = int(inside.sum())
        area[i] = a
        if a == 0:
            continue
        v32 = image[chan][:, r0:r1 + 1, c0:c1 + 1][:, inside]      # (K, a) fp32, row-major order
        with np.errstate(invalid="ignore"):
            g = v32 > gates[:, None]                               # the fp32 comparison, strict
        v = v32.astype(np.float64)
        with np.errstate(all="ignore"):      # non-finite pixels: only area and both are specified
            sums[i] = _tree_sum(v, **kw)
            d = v - (sums[i] / float(a))[:, None]
            prod = np.stack([d[x] * d[y] for x, y in pr])
            cross[i] = _tree_sum(prod, **kw)
            for l in range(k):
                gated[i, :, l] = _tree_sum(v, np.broadcast_to(g[l], v.shape), **kw)
        both[i] = [int((g[x] & g[y]).sum()) for x, y in pr]
    return area, both, sums, cross, gated


def features(area, both, sums, cross, gated):
    """colocalization.features as loops over cells and pairs k < l: the dictionary of its (n, P') arrays"""
    n, k = sums.shape
    pr = pairs(k)
    at = {q: j for j, q in enumerate(pr)}
    off = [q for q in pr if q[0] < q[1]]
    out = {key: np.full((n, len(off)), math.nan) for key in ("r", "overlap", "m1", "m2", "both_fraction", "jaccard")}
    out["both"] = np.zeros((n, len(off)), dtype=np.int64)
    for i in range(n):
        a = float(area[i])
        for j, (x, y) in enumerate(off):
            xkl, xkk, xll = float(cross[i][at[(x, y)]]), float(cross[i][at[(x, x)]]), float(cross[i][at[(y, y)]])
            sk, sl = float(sums[i][x]), float(sums[i][y])
            bkl, bkk, bll = int(both[i][at[(x, y)]]), int(both[i][at[(x, x)]]), int(both[i][at[(y, y)]])
            out["both"][i, j] = bkl
            if area[i] >= 2 and xkk > 0.0 and xll > 0.0:
                out["r"][i, j] = min(1.0, max(-1.0, xkl / math.sqrt(xkk * xll)))
            if area[i] > 0:
                rkl = (xkl + sk * sl / a + sk + sl + a) / 4.0
                rkk = (xkk + sk * sk / a + sk + sk + a) / 4.0
                rll = (xll + sl * sl / a + sl + sl + a) / 4.0
                if rkk > 0.0 and rll > 0.0:
                    out["overlap"][i, j] = rkl / math.sqrt(rkk * rll)
                if (sk + a) / 2.0 > 0.0:
                    out["m1"][i, j] = ((float(gated[i][x][y]) + bll) / 2.0) / ((sk + a) / 2.0)
                if (sl + a) / 2.0 > 0.0:
                    out["m2"][i, j] = ((float(gated[i][y][x]) + bkk) / 2.0) / ((sl + a) / 2.0)
                out["both_fraction"][i, j] = bkl / a
            if bkk + bll - bkl > 0:
                out["jaccard"][i, j] = bkl / float(bkk + bll - bkl)
    return out


# ---- the images and cells the GPU test and the host test share ---------------------------------------------------------------------------------
GATES = (-0.5, 0.0, 0.25, -0.125, 0.5, 0.75)      # one per channel of the six-channel images, exact in fp32


def generated_image(c: int, h: int, w: int, seed: int, gates=GATES) -> np.ndarray:
    """(c, h, w) fp32: random values in [-1, 1], and about 3 % of every channel exactly AT the channel's gate (``gates[k % len(gates)]``), so
    that only a strict comparison counts them as closed.  fp32 values of one magnitude add exactly in fp64 in any order, so half of the
    values are scaled by a random power of two down to 2^-44: their low bits fall below the last place of the running sums, and the sums
    depend on the order"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-1.0, 1.0, size=(c, h, w)).astype(np.float32)
    img = img * np.where(rng.random((c, h, w)) < 0.5, np.exp2(-rng.integers(0, 45, size=(c, h, w))), 1.0).astype(np.float32)
    ties = rng.random((c, h, w)) < 0.03
    for k in range(c):
        img[k][ties[k]] = np.float32(gates[k % len(gates)])
    return np.ascontiguousarray(img)


def small_cells(small_box: int = 1024):
    """(mask (96, 128) int32, ids, bbox): cells of 1, 2, 255, 256 and 257 pixels; a solid box of exactly ``small_box`` pixels and one of one
    pixel more; a box that leaves out part of its label; a label in two blobs with another cell and background between them; a cell on the
    last row and column whose box reaches out of the image; then rows that are no cell: ids 0 and -3, an empty box, a box outside the image"""
    assert small_box == 1024
    m = np.zeros((96, 128), dtype=np.int32)
    m[0:32, 0:32] = 6                               # 1024
    m[0:25, 34:75] = 7                              # 25 x 41 = 1025
    m[0:16, 78:94] = 4                              # 256
    m[0:16, 96:112] = 3
    m[15, 111] = 0                                  # 255
    m[34:50, 0:16] = 5
    m[50, 0] = 5                                    # 257
    m[34, 20] = 1
    m[34, 24:26] = 2
    m[36:48, 30:50] = 8
    m[36:42, 56:64] = 9
    m[60:67, 90:100] = 9
    m[50:55, 70:76] = 11
    m[88:96, 118:128] = 10
    ids = np.array([6, 7, 4, 3, 5, 1, 2, 8, 9, 11, 10, 0, -3, 4, 4], dtype=np.int32)
    bbox = np.array([[0, 31, 0, 31], [0, 24, 34, 74], [0, 15, 78, 93], [0, 15, 96, 111], [34, 50, 0, 15], [34, 34, 20, 20], [34, 34, 24, 25],
                     [38, 45, 33, 46], [36, 66, 56, 99], [50, 54, 70, 75], [88, 100, 118, 140], [0, 31, 0, 31], [0, 31, 0, 31],
                     [10, 9, 78, 93], [200, 230, 300, 340]], dtype=np.int32)
    return m, ids, bbox


def large_cells(resident: int = 4096):
    """(mask (128, 160) int32, ids, bbox): labels of ``resident``, ``resident`` + 1 and 9000 pixels"""
    assert resident == 4096
    m = np.zeros((128, 160), dtype=np.int32)
    m[0:64, 0:64] = 1
    m[0:64, 66:130] = 2
    m[64, 66] = 2
    m[66:126, 0:150] = 3
    ids = np.array([1, 2, 3], dtype=np.int32)
    bbox = np.array([[0, 63, 0, 63], [0, 64, 66, 129], [66, 125, 0, 149]], dtype=np.int32)
    return m, ids, bbox


def wide_cells():
    """(mask (40, 40) int32, ids, bbox) for the 32-channel image: three cells, one of them with one element per partial at most"""
    m = np.zeros((40, 40), dtype=np.int32)
    m[2:12, 3:20] = 1      # 170
    m[14:36, 5:30] = 2     # 550
    m[37:40, 36:40] = 3    # 12, in the corner
    ids = np.array([1, 2, 3], dtype=np.int32)
    bbox = np.array([[2, 11, 3, 19], [14, 35, 5, 29], [37, 39, 36, 39]], dtype=np.int32)
    return m, ids, bbox


#: the channel selections every six-channel image is run with: K = 2, K = 3, and K = 6 as a permutation that is not monotone
SELECTIONS = ((4, 1), (0, 5, 2), (3, 0, 5, 1, 4, 2))
