"""numpy restatement of ribca_cell_intensities (include/ribca_hip.h states the contract): per cell and channel the fp64 sum and sum of squared
deviations in the stated order -- 256 strided partials, then the halving tree -- and the order statistics that bracket the requested quantiles
on the total-order key of the fp32 bit pattern.  Two forms: ``direct`` (boolean indexing per cell, np.sort on the key, the tree in a plain loop)
and ``arrays`` (all channels of a cell at once, for the larger cases).  Also the generated image and mask the tests share."""
import numpy as np

NAN_BITS = 0x7FC00000
PARTIALS = 256


def to_key(values) -> np.ndarray:
    """uint32: all bits of a negative flipped, the sign bit of the rest set"""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def from_key(keys) -> np.ndarray:
    """fp32 with the bit patterns the keys were made of"""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def tree_sum_loop(values) -> float:
    """partial j adds v_j, v_{j+256}, ... in that order from 0.0; then p_j += p_{j+s} for j < s, s = 128 .. 1; p_0"""
    p = [0.0] * PARTIALS
    for j, v in enumerate(values):
        p[j % PARTIALS] = p[j % PARTIALS] + float(v)
    s = PARTIALS // 2
    while s >= 1:
        for j in range(s):
            p[j] = p[j] + p[j + s]
        s //= 2
    return p[0]


def tree_sum_arrays(values) -> np.ndarray:
    """the same over the last axis of an (..., a) fp64 array"""
    v = np.asarray(values, dtype=np.float64)
    a = v.shape[-1]
    rows = -(-a // PARTIALS)
    padded = np.zeros(v.shape[:-1] + (rows * PARTIALS,))      # a partial that starts at +0.0 is never -0.0, so + 0.0 changes no bit
    padded[..., :a] = v
    padded = padded.reshape(v.shape[:-1] + (rows, PARTIALS))
    p = np.zeros(v.shape[:-1] + (PARTIALS,))
    for r in range(rows):
        p = p + padded[..., r, :]
    s = PARTIALS // 2
    while s >= 1:
        p = p[..., :s] + p[..., s:2 * s]
        s //= 2
    return p[..., 0]


def ranks(a: int, q_num, q_den: int):
    """[(lo, hi)] per quantile: h = (a - 1) q_num[k]; lo = h // q_den; hi = lo + (h % q_den != 0)"""
    out = []
    for num in q_num:
        h = (int(a) - 1) * int(num)
        lo = h // int(q_den)
        out.append((lo, lo + (1 if h % int(q_den) else 0)))
    return out


def clipped_box(box, h: int, w: int):
    r0, r1, c0, c1 = max(int(box[0]), 0), min(int(box[1]), h - 1), max(int(box[2]), 0), min(int(box[3]), w - 1)
    return (r0, r1, c0, c1) if r0 <= r1 and c0 <= c1 else None


def _outputs(n, c, q):
    order = np.full((n, c, q, 2), NAN_BITS, dtype=np.uint32).view(np.float32)
    return np.zeros(n, dtype=np.int32), np.zeros((n, c, 2), dtype=np.float64), order


def direct(image, mask, ids, bbox, q_num=(0, 1, 2, 3, 4), q_den=4):
    """area (n) int32, sums (n, C, 2) fp64, order (n, C, Q, 2) fp32 -- the plain form"""
    image = np.asarray(image, dtype=np.float32)
    c_img, h, w = image.shape
    n = len(ids)
    area, sums, order = _outputs(n, c_img, len(q_num))
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
        for c in range(c_img):
            v = image[c, r0:r1 + 1, c0:c1 + 1][inside]      # row-major order
            total = tree_sum_loop(v)
            mean = total / float(a)
            dev = [(float(x) - mean) * (float(x) - mean) for x in v]
            sums[i, c] = (total, tree_sum_loop(dev))
            ordered = from_key(np.sort(to_key(v)))
            for k, (lo, hi) in enumerate(ranks(a, q_num, q_den)):
                order[i, c, k] = (ordered[lo], ordered[hi])
    return area, sums, order


def arrays(image, mask, ids, bbox, q_num=(0, 1, 2, 3, 4), q_den=4):
    """the same, every channel of a cell at once"""
    image = np.asarray(image, dtype=np.float32)
    c_img, h, w = image.shape
    n = len(ids)
    area, sums, order = _outputs(n, c_img, len(q_num))
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
        v = image[:, r0:r1 + 1, c0:c1 + 1][:, inside]      # (C, a)
        v64 = v.astype(np.float64)
        with np.errstate(all="ignore"):      # non-finite pixels: only the order statistics are specified
            total = tree_sum_arrays(v64)
            dev = v64 - (total / float(a))[:, None]
            sums[i, :, 0], sums[i, :, 1] = total, tree_sum_arrays(dev * dev)
        ordered = from_key(np.sort(to_key(v), axis=1))
        for k, (lo, hi) in enumerate(ranks(a, q_num, q_den)):
            order[i, :, k, 0], order[i, :, k, 1] = ordered[:, lo], ordered[:, hi]
    return area, sums, order


def boxes_of(mask, ids) -> np.ndarray:
    """(n, 4) int32 rmin, rmax, cmin, cmax of every id; (0, -1, 0, -1), an empty box, for an id the mask does not hold"""
    out = np.zeros((len(ids), 4), dtype=np.int32)
    for i, v in enumerate(ids):
        rr, cc = np.nonzero(mask == int(v))
        out[i] = (rr.min(), rr.max(), cc.min(), cc.max()) if len(rr) else (0, -1, 0, -1)
    return out


def boxes_of_all(mask, ids) -> np.ndarray:
    """the same for many ids in one pass over the mask (every id must occur)"""
    rr, cc = np.nonzero(mask > 0)
    lab = mask[rr, cc]
    top = int(lab.max()) + 1
    rmin, cmin = np.full(top, mask.shape[0]), np.full(top, mask.shape[1])
    rmax, cmax = np.full(top, -1), np.full(top, -1)
    np.minimum.at(rmin, lab, rr), np.maximum.at(rmax, lab, rr), np.minimum.at(cmin, lab, cc), np.maximum.at(cmax, lab, cc)
    pick = np.asarray(ids, dtype=np.int64)
    return np.stack([rmin[pick], rmax[pick], cmin[pick], cmax[pick]], axis=1).astype(np.int32)


def generated_image(c: int, h: int, w: int, seed: int = 5) -> np.ndarray:
    """(c, h, w) fp32 with many exact ties: values quantised to a few levels of both signs, -0.0 and +0.0, denormals, and a few values of full
    precision between them"""
    rng = np.random.default_rng(seed)
    levels = np.array([-1.0, -0.75, -0.5, -0.0, 0.0, 0.125, 0.5, 1.0, 1e-40, -1e-40, 3e-45, 0.3, -0.3], dtype=np.float32)
    img = levels[rng.integers(0, len(levels), size=(c, h, w))]
    fine = rng.random((c, h, w)) < 0.2
    img[fine] = (rng.standard_normal((c, h, w)).astype(np.float32))[fine]
    return np.ascontiguousarray(img)


def generated_mask(resident: int = 4096) -> np.ndarray:
    """(100, 130) int32.  Label 1: a square of exactly ``resident`` pixels; label 2: a square of ``resident`` pixels and one more below it; label
    3: a single pixel; label 4: two distant blobs (its box holds labels 5 and 6 and background); labels 7 ..: a grid of small cells of odd sizes,
    label 39 touching the last row and column; label 40 is absent."""
    side = int(round(resident ** 0.5))
    assert side * side == resident and side <= 64
    m = np.zeros((100, 130), dtype=np.int32)
    m[0:side, 0:side] = 1
    m[0:side, 64:64 + side] = 2
    m[side, 64] = 2
    m[70, 2] = 3
    m[68:73, 10:15] = 4
    m[90:97, 100:104] = 4
    m[75:80, 30:41] = 5
    m[82:88, 60:70] = 6
    label = 7
    for r in range(66, 98, 8):
        for c in range(16, 128, 9):
            if m[r:r + 7, c:c + 8].any() or label >= 39:
                continue
            m[r:r + 3 + label % 5, c:c + 2 + label % 7] = label
            label += 1
    m[97:100, 125:130] = 39
    return m
