"""numpy restatement of label expansion, written from the rules include/ribca_hip.h states for ribca_expand_labels: a brute-force loop over the
offsets of the disk dr^2 + dc^2 <= D^2 that keeps, per pixel, the lexicographic minimum of (squared distance, label) over the labelled pixels in
reach -- and, beside it, the largest label at that distance, which tells the TIE pixels: grown pixels whose nearest labelled pixels carry more
than one distinct label, the only pixels where scipy's scan-order rule may differ.  Also the seeded masks of the tests (random discs of radius
2 .. 6) and the text of the expansion CSV restated from the two masks."""
import numpy as np

BIG = np.int64(1) << 40


def expand(mask, distance):
    """(out (H, W) int32, dist2 (H, W) int32, ties (H, W) bool) of ``mask`` grown by ``distance`` pixels"""
    mask = np.asarray(mask, dtype=np.int32)
    d = int(distance)
    h, w = mask.shape
    pad = np.zeros((h + 2 * d, w + 2 * d), dtype=np.int64)      # nothing outside the image carries a label
    pad[d:d + h, d:d + w] = np.where(mask > 0, mask, 0)
    best = np.full((h, w), BIG, dtype=np.int64)
    low = np.zeros((h, w), dtype=np.int64)
    high = np.zeros((h, w), dtype=np.int64)
    for dr in range(-d, d + 1):
        for dc in range(-d, d + 1):
            d2 = dr * dr + dc * dc
            if d2 > d * d:
                continue
            v = pad[d + dr:d + dr + h, d + dc:d + dc + w]
            has = v > 0
            closer = has & (d2 < best)
            same = has & (d2 == best)
            low = np.where(closer, v, np.where(same, np.minimum(low, v), low))
            high = np.where(closer, v, np.where(same, np.maximum(high, v), high))
            best = np.where(closer, d2, best)
    found = best < BIG
    grown = found & (mask <= 0)
    out = np.where(found, low, mask).astype(np.int32)      # a labelled pixel finds itself at distance 0
    dist2 = np.where(found, best, -1).astype(np.int32)
    return out, dist2, grown & (low != high)


def random_discs(h, w, cells, seed, rmin=2.0, rmax=6.0, first_label=1):
    """``cells`` discs of radius rmin .. rmax at random centres anywhere in the image, so that some are cut by every border; a later disc
    paints over an earlier one, and a label may end up without a pixel"""
    rng = np.random.RandomState(seed)
    mask = np.zeros((h, w), dtype=np.int32)
    rr, cc = np.mgrid[0:h, 0:w]
    for k in range(cells):
        r, c = rng.uniform(-1, h), rng.uniform(-1, w)
        rad = rng.uniform(rmin, rmax)
        mask[(rr - r) ** 2 + (cc - c) ** 2 <= rad * rad] = first_label + k
    return mask


def label_rows(mask):
    """(ids ascending, area, box rmin rmax cmin cmax) of the labels > 0 of a mask"""
    mask = np.asarray(mask)
    ids = np.unique(mask[mask > 0]).astype(np.int64)
    area = np.zeros(len(ids), dtype=np.int64)
    box = np.zeros((len(ids), 4), dtype=np.int64)
    for k, i in enumerate(ids):
        r, c = np.nonzero(mask == i)
        area[k] = len(r)
        box[k] = (r.min(), r.max(), c.min(), c.max())
    return ids, area, box


def expansion_csv(core, grown_mask):
    """the text of {batch_id}_expansion_{image number}.csv from the mask as read and the mask as grown"""
    ids, area_core, _ = label_rows(core)
    ids2, area_cell, box = label_rows(grown_mask)
    assert np.array_equal(ids, ids2)
    lines = ["id,area_core,area_cell,grown,rmin,rmax,cmin,cmax"]
    for k, i in enumerate(ids):
        lines.append("%d,%d,%d,%d,%d,%d,%d,%d" % (i, area_core[k], area_cell[k], area_cell[k] - area_core[k], box[k, 0], box[k, 1], box[k, 2], box[k, 3]))
    return "\n".join(lines) + "\n"
