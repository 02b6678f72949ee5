"""numpy oracle of the tissue-region arithmetic (csrc/regions.hip, multiplexed_image_annotator_amd/regions.py), written as
plain loops in the stated summation orders so that the GPU results can be compared bit for bit.  numpy only (scipy's k-d tree builds the
planted count tables; it is not part of the arithmetic).  Not a test module."""
import math

import numpy as np

CHUNK = 1024
MASK64 = 0xFFFFFFFFFFFFFFFF
SIZES = (10, 20, 30, 50, 75, 100, 150, 200)


# ------------------------------------------------------------------------------------------------------------------------ inputs
def planted_counts(n, n_types, n_bands, seed, sizes=SIZES):
    """(n, len(sizes), n_types) int16 count table of synth.planted_bands through an exact k-d tree query, and the planted band of every cell"""
    from scipy.spatial import cKDTree
    from multiplexed_image_annotator_amd import synth
    x, y, types, band = synth.planted_bands(n, n_types, n_bands, seed)
    pts = np.stack([x, y], axis=1)
    _, idx = cKDTree(pts).query(pts, k=max(sizes) + 1)
    nb = types[idx[:, 1:]]
    counts = np.zeros((n, len(sizes), n_types), dtype=np.int16)
    for l, s in enumerate(sizes):
        for t in range(n_types):
            counts[:, l, t] = (nb[:, :s] == t).sum(axis=1)
    return counts, band


def size_columns(sizes, n_types):
    return np.repeat(np.asarray(sizes, dtype=np.float64), n_types)


# --------------------------------------------------------------------------------------------------------------------------- PCA
def gram(counts2d):
    c = counts2d.astype(np.int64)
    return c.sum(axis=0), c.T @ c


def pca_from_gram(g, colsum, n, size_col, var=0.99):
    size = np.asarray(size_col, dtype=np.float64)
    mean = colsum.astype(np.float64) / size / float(n)
    cov = (g.astype(np.float64) / (size[:, None] * size[None, :]) - float(n) * (mean[:, None] * mean[None, :])) / float(n - 1)
    lam, vec = np.linalg.eigh(cov)
    lam = lam[::-1].copy()
    vt = np.ascontiguousarray(vec[:, ::-1].T)
    lam[lam < 0.0] = 0.0
    for j in range(vt.shape[0]):
        if vt[j, np.argmax(np.abs(vt[j]))] < 0:
            vt[j] = -vt[j]
    d = int(np.searchsorted(np.cumsum(lam / lam.sum()), var, side="right")) + 1
    d = min(d, vt.shape[0])
    return mean, np.ascontiguousarray(vt[:d]), lam, d


def project(counts2d, size_col, mean, comps):
    """y[i, j] = sum over f ascending of (c[i, f] / size[f] - mean[f]) * v[j, f], every operation rounded on its own"""
    n, f_all = counts2d.shape
    y = np.zeros((n, comps.shape[0]), dtype=np.float64)
    for f in range(f_all):
        x = counts2d[:, f].astype(np.float64) / size_col[f] - mean[f]
        y = y + x[:, None] * comps[None, :, f]
    return y


# ----------------------------------------------------------------------------------------------------------------------- k-means
def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed, step, trial):
    h = splitmix64(splitmix64(splitmix64(seed & MASK64) ^ step) ^ trial)
    return (h >> 11) * 2.0 ** -53


def dist2(y, centres):
    """(n, k): sums of squared differences in dimension order"""
    out = np.zeros((y.shape[0], centres.shape[0]), dtype=np.float64)
    for f in range(y.shape[1]):
        e = y[:, f:f + 1] - centres[None, :, f]
        out = out + e * e
    return out


def seq_sum_rows(a):
    """sum of the rows of a (m, ...) in ascending order, starting from +0"""
    return np.cumsum(np.concatenate([np.zeros((1,) + a.shape[1:], dtype=np.float64), a], axis=0), axis=0)[-1]


def chunked_sum(v):
    """rows of every chunk of 1024 in ascending order, then the chunks in ascending order"""
    parts = np.array([seq_sum_rows(v[r:r + CHUNK]) for r in range(0, len(v), CHUNK)])
    return seq_sum_rows(parts)


def kmeans_plusplus(y, k, seed):
    n = y.shape[0]
    trials = 2 + int(math.log(k))
    first = min(int(draw(seed, 0, 0) * n), n - 1)
    picks = [first]
    closest = dist2(y, y[[first]])[:, 0]
    for c in range(1, k):
        prefix = np.cumsum(closest)
        cand = []
        for t in range(trials):
            target = draw(seed, c, t) * prefix[-1]
            cand.append(min(int(np.searchsorted(prefix, target, side="left")), n - 1))
        d2 = np.minimum(closest[:, None], dist2(y, y[cand]))
        pot = [chunked_sum(d2[:, t]) for t in range(trials)]
        best = int(np.argmin(pot))
        picks.append(cand[best])
        closest = d2[:, best].copy()
    return picks, closest


def assign(y, centres):
    d2 = dist2(y, centres)
    labels = np.argmin(d2, axis=1)      # the first minimum: the least (d2, j)
    return labels.astype(np.int64), d2[np.arange(len(labels)), labels]


def centre_sums(y, labels, k):
    """THE summation order: per chunk of 1024 rows and per cluster the rows in ascending order, then the chunks in ascending order"""
    d = y.shape[1]
    sums = np.zeros((k, d), dtype=np.float64)
    counts = np.zeros(k, dtype=np.int64)
    for r in range(0, len(y), CHUNK):
        part = np.zeros((k, d), dtype=np.float64)
        lab = labels[r:r + CHUNK]
        for c in range(k):
            rows = y[r:r + CHUNK][lab == c]
            part[c] = seq_sum_rows(rows)
            counts[c] += len(rows)
        sums = sums + part
    return sums, counts


def finalize(sums, counts, old):
    new = old.copy()
    for c in range(len(counts)):
        if counts[c] > 0:
            new[c] = sums[c] / float(counts[c])
    e = new - old
    shift = np.array([seq_sum_rows((e[c] * e[c])[:, None])[0] for c in range(len(counts))])
    return new, shift


def relocate(y, labels, mind2, sums, counts):
    empty = np.flatnonzero(counts == 0)
    far = np.lexsort((np.arange(len(y)), -mind2))[:len(empty)]
    for m in range(len(empty)):
        src = labels[far[m]]
        sums[src] = sums[src] - y[far[m]]
        sums[empty[m]] = y[far[m]]
        counts[empty[m]] = 1
        counts[src] -= 1
    return far


def lloyd(y, centres, max_iter=300, tol_factor=1e-4, trace=None):
    """-> labels, centres, iterations, inertia"""
    k = centres.shape[0]
    tol = float(np.mean(np.var(y, axis=0)) * tol_factor)
    centres = centres.copy()
    old_labels = np.full(len(y), -1, dtype=np.int64)
    strict = False
    it = 0
    for it in range(max_iter):
        labels, mind2 = assign(y, centres)
        sums, counts = centre_sums(y, labels, k)
        if (counts == 0).any():
            relocate(y, labels, mind2, sums, counts)
        centres, shift = finalize(sums, counts, centres)
        if trace is not None:
            trace.append((labels.copy(), centres.copy()))
        if np.array_equal(labels, old_labels):
            strict = True
            break
        total = 0.0
        for v in shift.tolist():
            total = total + v
        if total <= tol:
            break
        old_labels = labels
    if not strict:
        labels, mind2 = assign(y, centres)
    return labels, centres, it + 1, float(np.cumsum(mind2)[-1])


def kmeans(y, k, seed=0, trace=None):
    picks, _ = kmeans_plusplus(y, k, seed)
    labels, centres, iters, inertia = lloyd(y, y[picks], trace=trace)
    return labels, centres, iters, inertia, picks
