"""numpy oracles of csrc/celltype_stats.hip, written from the rules include/ribca_hip.h states: the summation tree of ribca_group_sums, the pixels
of ribca_heatmap_raster and of ribca_pie_raster.  numpy rounds every operation on its own, as the kernels do (fma contraction off)."""
import numpy as np

R = 1024      # rows per chunk of the summation tree
SILVER = 192


def group_sums(x, group, groups):
    """sums (groups, c), counts (groups), skipped: rows added in ascending order within each chunk of R from +0.0, chunks added in ascending order
    from +0.0"""
    x = np.asarray(x, dtype=np.float64)
    group = np.asarray(group)
    n, c = x.shape
    chunks = (n + R - 1) // R
    part = np.zeros((chunks, groups, c), dtype=np.float64)
    counts = np.zeros(groups, dtype=np.int64)
    skipped = 0
    for r in range(n):
        g = int(group[r])
        if g < 0 or g >= groups:
            skipped += 1
            continue
        part[r // R, g] = part[r // R, g] + x[r]
        counts[g] += 1
    sums = np.zeros((groups, c), dtype=np.float64)
    for k in range(chunks):
        sums = sums + part[k]
    return sums, counts, skipped


def means_of(sums, counts):
    """sum / count in fp64, NaN rows where the count is 0"""
    sums = np.asarray(sums, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.int64)
    out = np.full(sums.shape, np.nan)
    ok = counts > 0
    out[ok] = sums[ok] / counts[ok][:, None].astype(np.float64)
    return out


def colour_index(means, vmin, vmax):
    """the index rule on an array of means that are numbers"""
    means = np.asarray(means, dtype=np.float64)
    if vmax == vmin:
        return np.zeros(means.shape, dtype=np.int64)
    q = np.floor(((means - vmin) / (vmax - vmin)) * 256.0)
    return np.where(q >= 255.0, 255, np.where(q >= 0.0, q, 0)).astype(np.int64)


def heatmap_raster(means, lut, cell, gap):
    """(T cell, C cell, 3) uint8, vmin, vmax from the (T, C) means (NaN = no cells)"""
    means = np.asarray(means, dtype=np.float64)
    t, c = means.shape
    good = ~np.isnan(means)
    vmin = means[good].min() if good.any() else np.nan
    vmax = means[good].max() if good.any() else np.nan
    rgb = np.full((t, c, 3), SILVER, dtype=np.uint8)
    if good.any():
        rgb[good] = np.asarray(lut, dtype=np.uint8)[colour_index(means[good], vmin, vmax)]
    img = np.repeat(np.repeat(rgb, cell, axis=0), cell, axis=1)
    ly, lx = np.arange(t * cell) % cell, np.arange(c * cell) % cell
    inside = ((ly >= gap) & (ly < cell - gap))[:, None] & ((lx >= gap) & (lx < cell - gap))[None, :]
    img[~inside] = 255
    return img, vmin, vmax


def _half(vx, vy):
    return np.where((vy > 0) | ((vy == 0) & (vx > 0)), 0, 1)


def pie_wedge_index(rays, size, radius):
    """(size, size) int64: the wedge of every pixel of the disc by the half-plane / cross-product order, -1 outside"""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 2)
    c0 = size // 2
    fx = (np.arange(size) - c0).astype(np.float64)[None, :] * np.ones((size, 1))
    fy = (c0 - np.arange(size)).astype(np.float64)[:, None] * np.ones((1, size))
    hp = _half(fx, fy)
    wedge = np.zeros((size, size), dtype=np.int64)
    for ax, ay in rays:
        ha = int(_half(np.float64(ax), np.float64(ay)))
        t0 = fx * ay
        t1 = fy * ax
        pixel_first = (hp < ha) | ((hp == ha) & ((t0 - t1) > 0.0))
        wedge += ~pixel_first
    wedge[c0, c0] = 0
    wedge[fx * fx + fy * fy > float(radius) * float(radius)] = -1
    return wedge


def pie_raster(rays, rgb, size, radius):
    wedge = pie_wedge_index(rays, size, radius)
    img = np.full((size, size, 3), 255, dtype=np.uint8)
    img[wedge >= 0] = np.asarray(rgb, dtype=np.uint8)[wedge[wedge >= 0]]
    return img


def pie_wedge_index_by_angle(counts, size, radius):
    """the same image from the definition: the angle of the pixel (arctan2, counter-clockwise from 3 o'clock) against the cumulated fractions of
    the counts; empty wedges take no angle, so the index counts the wedges that are not empty"""
    counts = np.asarray([c for c in counts if c > 0], dtype=np.float64)
    bounds = 2.0 * np.pi * np.cumsum(counts)[:-1] / counts.sum()
    c0 = size // 2
    dx = (np.arange(size) - c0)[None, :] * np.ones((size, 1))
    dy = (c0 - np.arange(size))[:, None] * np.ones((1, size))
    ang = np.mod(np.arctan2(dy, dx), 2.0 * np.pi)
    wedge = np.searchsorted(bounds, ang.reshape(-1), side="right").reshape(size, size).astype(np.int64)
    wedge[dx * dx + dy * dy > radius * radius] = -1
    return wedge
