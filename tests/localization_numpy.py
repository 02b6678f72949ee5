"""numpy restatement of ribca_mask_depth and ribca_cell_shell_sums, written from the rules include/ribca_hip.h states: the depth by a plain search
over the offsets of the disk dr^2 + dc^2 <= D^2, the shell sums with the 256 strided partials per shell and the halving tree written out, and
``features`` of localization.py as plain loops over cells and markers."""
import math

import numpy as np

from intensities_numpy import PARTIALS, clipped_box

BIG = np.int64(1) << 40


def depth(mask, distance):
    """depth2 (H, W) int32: for a labelled pixel the smallest squared distance, at most D D, to a pixel inside the image whose max(label, 0)
    differs, -1 without one; 0 on the background"""
    mask = np.asarray(mask, dtype=np.int32)
    d = int(distance)
    h, w = mask.shape
    lab = np.where(mask > 0, mask, 0).astype(np.int64)
    pad = np.full((h + 2 * d, w + 2 * d), -1, dtype=np.int64)      # -1: outside the image, never "a different pixel"
    pad[d:d + h, d:d + w] = lab
    best = np.full((h, w), BIG, dtype=np.int64)
    for dr in range(-d, d + 1):
        for dc in range(-d, d + 1):
            d2 = dr * dr + dc * dc
            if d2 > d * d or d2 == 0:
                continue
            v = pad[d + dr:d + dr + h, d + dc:d + dc + w]
            best = np.where((v >= 0) & (v != lab) & (d2 < best), d2, best)
    return np.where(lab == 0, 0, np.where(best < BIG, best, -1)).astype(np.int32)


def shell_of(depth2, edges2):
    """the shell of every pixel: S - 1 where depth2 is -1, else #{j : depth2 > edges2[j]}"""
    d = np.asarray(depth2).astype(np.int64)
    e = np.asarray(edges2).astype(np.int64).reshape(-1)
    return np.where(d == -1, len(e), (d[..., None] > e).sum(axis=-1))


def tree(p):
    """p (..., 256): p_j += p_{j+s} for j < s, s = 128 .. 1; p_0"""
    s = PARTIALS // 2
    while s >= 1:
        p = p[..., :s] + p[..., s:2 * s]
        s //= 2
    return p[..., 0]


def shell_sums(image, mask, depth2, ids, bbox, edges2):
    """count (n, S) int32, deepest (n) int32, sums (n, C, S) fp64.  Element e of a cell, its e-th pixel in row-major order whatever its shell,
    belongs to partial e mod 256; partial p[k][j] adds, in increasing e, its elements of shell k and skips the others; then the tree."""
    image = np.asarray(image, dtype=np.float32)
    c_img, h, w = image.shape
    n, shells = len(ids), len(edges2) + 1
    count = np.zeros((n, shells), dtype=np.int32)
    deepest = np.zeros(n, dtype=np.int32)
    sums = np.zeros((n, c_img, shells), dtype=np.float64)
    for i in range(n):
        box = clipped_box(bbox[i], h, w)
        if int(ids[i]) <= 0 or box is None:
            continue
        r0, r1, c0, c1 = box
        inside = mask[r0:r1 + 1, c0:c1 + 1] == int(ids[i])
        a = int(inside.sum())
        if a == 0:
            continue
        d = depth2[r0:r1 + 1, c0:c1 + 1][inside].astype(np.int64)      # row-major order
        shell = shell_of(d, edges2)
        count[i] = np.bincount(shell, minlength=shells)
        deepest[i] = -1 if (d == -1).any() else d.max()
        v = image[:, r0:r1 + 1, c0:c1 + 1][:, inside].astype(np.float64)      # (C, a)
        rows = -(-a // PARTIALS)
        for k in range(shells):
            p = np.zeros((c_img, PARTIALS))
            for r in range(rows):      # row r holds the elements 256 r .. 256 r + 255: one candidate per partial
                e = slice(r * PARTIALS, min((r + 1) * PARTIALS, a))
                mine = shell[e] == k
                width = e.stop - e.start
                p[:, :width] = np.where(mine[None, :], p[:, :width] + v[:, e], p[:, :width])      # skipped, not added as zeros
            sums[i, :, k] = tree(p)
    return count, deepest, sums


def features(count, deepest, sums, band, edges):
    """localization.features as loops: the dictionary of its arrays"""
    n, c_img, shells = sums.shape
    cut = list(edges).index(band) + 1
    out = {"area": np.zeros(n, dtype=np.int64), "edge_area": np.zeros(n, dtype=np.int64), "inner_area": np.zeros(n, dtype=np.int64),
           "inradius": np.full(n, np.nan), "edge": np.full((n, c_img), np.nan), "inner": np.full((n, c_img), np.nan),
           "contrast": np.full((n, c_img), np.nan)}
    for i in range(n):
        ea = sum(int(count[i][k]) for k in range(cut))
        ia = sum(int(count[i][k]) for k in range(cut, shells))
        out["edge_area"][i], out["inner_area"][i], out["area"][i] = ea, ia, ea + ia
        if ea + ia:
            out["inradius"][i] = math.inf if int(deepest[i]) == -1 else math.sqrt(float(deepest[i]))
        for c in range(c_img):
            means = []
            for pixels, ks in ((ea, range(cut)), (ia, range(cut, shells))):
                total = 0.0
                for k in ks:
                    total = total + float(sums[i][c][k])
                means.append((total / float(pixels) + 1.0) / 2.0 if pixels else math.nan)
            out["edge"][i, c], out["inner"][i, c] = means
            if ea and ia and means[0] + means[1] > 0.0:
                out["contrast"][i, c] = (means[0] - means[1]) / (means[0] + means[1])
    return out
