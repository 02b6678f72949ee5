"""numpy oracles of the nearest cell of every type, written from the rules include/ribca_hip.h states: the (n, T) table of squared distances and
indices of csrc/nearest.hip by a chunked O(n^2) search with the same fp64 operation order (dx = x_i - x_j, d = dx * dx + dy * dy: numpy rounds
every elementwise operation on its own), the band counts of the nearest distances under the keyed label permutations (sigma_p from
tests/enrichment_numpy.py), and the host statistics of multiplexed_image_annotator_amd/nearest.py restated one entry at a time."""
import math

import numpy as np

import enrichment_numpy as EN


def nearest_by_type(x, y, labels, t, chunk=512):
    """near2 (n, t) fp64 and arg (n, t) int64: the least d2 to another cell of each type and the lowest index that attains it; +inf / -1 where
    there is none.  A label outside [0, t) is never a target."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    n = len(x)
    near2 = np.full((n, t), np.inf)
    arg = np.full((n, t), -1, dtype=np.int64)
    members = [np.nonzero(lab == b)[0] for b in range(t)]      # ascending: argmin returns the first, the lowest index
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        rows = np.arange(i0, i1)
        for b, js in enumerate(members):
            if len(js) == 0:
                continue
            dx = x[i0:i1, None] - x[None, js]
            dy = y[i0:i1, None] - y[None, js]
            d = dx * dx + dy * dy
            d[rows[:, None] == js[None, :]] = np.inf      # the cell itself
            k = np.argmin(d, axis=1)
            m = d[np.arange(i1 - i0), k]
            found = np.isfinite(m)
            near2[i0:i1, b] = m
            arg[i0:i1, b] = np.where(found, js[k], -1)
    return near2, arg


def band_counts(near2, labels, t, r2):
    """(B, t, t) int64: per anchor type a = labels[i] in [0, t) and target type b the cells whose near2[i][b] lies in each band, band = the number
    of thresholds strictly below it; beyond r2[-1] (or +inf) nothing"""
    near2 = np.asarray(near2, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    r2 = np.asarray(r2, dtype=np.float64)
    keep = (near2 <= r2[-1]) & ((lab >= 0) & (lab < t))[:, None]
    rows, cols = np.nonzero(keep)
    band = np.searchsorted(r2, near2[rows, cols], side="left")
    return np.bincount((band * t + lab[rows]) * t + cols, minlength=len(r2) * t * t).reshape(len(r2), t, t)


def perm_labels(cell_type, seed, image, p):
    """label_p(i) = cell_type[sigma_p(i)]"""
    cell_type = np.asarray(cell_type)
    return cell_type[EN.sigma(len(cell_type), seed, image, p)]


def perm_counts(x, y, cell_type, t, r2, seed, image, p0, n_perms):
    """(P, B, t, t) int64: the positions stay, the labels move"""
    return np.stack([band_counts(nearest_by_type(x, y, lab, t)[0], lab, t, r2)
                     for lab in (perm_labels(cell_type, seed, image, p0 + j) for j in range(n_perms))])


def statistics(observed, null, anchors_present):
    """the dictionary of nearest.statistics, entry by entry on Python numbers"""
    obs = np.asarray(observed)
    nb, t, _ = obs.shape
    cum = np.zeros(obs.shape, dtype=np.int64)
    g = np.full(obs.shape, np.nan)
    for a in range(t):
        for b in range(t):
            run = 0
            for k in range(nb):
                run += int(obs[k, a, b])
                cum[k, a, b] = run
                if int(anchors_present[a]) > 0:
                    g[k, a, b] = run / int(anchors_present[a])
    out = {"cumulative": cum, "G": g}
    if null is None:
        return out
    null = np.asarray(null)
    p = null.shape[0]
    mean, std, z = np.zeros(obs.shape), np.zeros(obs.shape), np.full(obs.shape, np.nan)
    n_ge, n_le = np.zeros(obs.shape, dtype=np.int64), np.zeros(obs.shape, dtype=np.int64)
    for a in range(t):
        for b in range(t):
            runs = [0] * p
            for k in range(nb):
                runs = [runs[j] + int(null[j, k, a, b]) for j in range(p)]
                mu = math.fsum(float(v) for v in runs) / p
                sd = math.sqrt(math.fsum((float(v) - mu) * (float(v) - mu) for v in runs) / p)
                mean[k, a, b], std[k, a, b] = mu, sd
                if sd > 0.0:
                    z[k, a, b] = (float(cum[k, a, b]) - mu) / sd
                n_ge[k, a, b] = sum(v >= cum[k, a, b] for v in runs)
                n_le[k, a, b] = sum(v <= cum[k, a, b] for v in runs)
    out.update({"mean": mean, "std": std, "z": z, "n_ge": n_ge, "n_le": n_le})
    return out
