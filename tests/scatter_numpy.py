"""Numpy twin of csrc/scatter.hip, written from include/ribca_hip.h: filled discs in data order (a later point paints over an earlier one), the
affine map applied in fp32 with every operation rounded on its own, white background."""
import numpy as np


def disc_offsets(radius):
    """(dx, dy) with |dx|, |dy| <= radius and dx^2 + dy^2 <= radius^2 + 1"""
    return [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if dx * dx + dy * dy <= radius * radius + 1]


def affine(points, height, width, margin=0.05):
    """column = ax x + bx, row = ay y + by: [min - margin span, max + margin span] of x onto [0, width - 1], of y onto [height - 1, 0]"""
    pts = np.asarray(points, dtype=np.float64)
    pts = pts[np.isfinite(pts).all(axis=1)]
    xlo, xhi = pts[:, 0].min(), pts[:, 0].max()
    ylo, yhi = pts[:, 1].min(), pts[:, 1].max()
    xs = (xhi - xlo) if xhi > xlo else 1.0
    ys = (yhi - ylo) if yhi > ylo else 1.0
    xlo, xhi, ylo, yhi = xlo - margin * xs, xhi + margin * xs, ylo - margin * ys, yhi + margin * ys
    ax = (width - 1) / (xhi - xlo)
    ay = (height - 1) / (yhi - ylo)
    return ax, -ax * xlo, -ay, ay * yhi


def centres(points, aff):
    """fp32 centre (column, row) of every point, rint-ed; NaN where not finite"""
    p = np.asarray(points, dtype=np.float32)
    ax, bx, ay, by = (np.float32(v) for v in aff)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.rint((p[:, 0] * ax).astype(np.float32) + bx).astype(np.float32)
        fy = np.rint((p[:, 1] * ay).astype(np.float32) + by).astype(np.float32)
    return fx, fy


def raster(points, rgb, height, width, aff, radius=2):
    """-> ((height, width, 3) uint8, number of skipped points, (height, width) int32 index image: point + 1, 0 = background)"""
    fx, fy = centres(points, aff)
    with np.errstate(invalid="ignore"):
        ok = (fx >= 0) & (fx < np.float32(width)) & (fy >= 0) & (fy < np.float32(height))
    index = np.zeros((height, width), dtype=np.int32)
    live = np.flatnonzero(ok)
    cx, cy = fx[live].astype(np.int64), fy[live].astype(np.int64)
    for dx, dy in disc_offsets(radius):
        px, py = cx + dx, cy + dy
        on = (px >= 0) & (px < width) & (py >= 0) & (py < height)
        np.maximum.at(index, (py[on], px[on]), (live[on] + 1).astype(np.int32))
    out = np.full((height, width, 3), 255, dtype=np.uint8)
    hit = index > 0
    out[hit] = np.asarray(rgb, dtype=np.uint8)[index[hit] - 1]
    return out, int((~ok).sum()), index
