"""numpy oracle of the spatial autocorrelation, written from the rules include/ribca_hip.h states for ribca_autocorr_observed and
ribca_autocorr_perm: the neighbour sums in list order, THE tree over chunks of 256 cells, the rows moved by the bijection sigma_p of
tests/enrichment_numpy.py.  numpy's float64 element-wise operations round every operation on its own (no fma), as the kernels do."""
import numpy as np

import enrichment_numpy as EN

CHUNK = 256

#: (n, C, m) of the kernel tests: the smallest cases; both sides of the chunk of 256 cells; a second chunk of one cell; a channel count across
#: the tile of 16; the widest panel; 17 chunks
SHAPES = [(2, 1, 1), (5, 3, 4), (255, 1, 24), (256, 2, 31), (257, 15, 24), (300, 17, 8), (1000, 64, 3), (4097, 15, 24)]


def random_table(n, c, m, seed=0):
    """a centred-looking table with channels of very different scale, and a random neighbour list (any cell may stand in any list)"""
    rng = np.random.RandomState(n + c + m + seed)
    z = rng.randn(n, c) * 10.0 ** rng.uniform(-3, 3, c)
    return z - z.mean(axis=0), rng.randint(0, n, (n, m))


def tree(v):
    """(n, C) -> (C): chunks of 256 cells padded with +0.0, eight rounds of adjacent pairs, then the chunks added from +0.0 in ascending order"""
    v = np.asarray(v, dtype=np.float64)
    n, c = v.shape
    chunks = (n + CHUNK - 1) // CHUNK
    v = np.concatenate([v, np.zeros((chunks * CHUNK - n, c))]).reshape(chunks, CHUNK, c)
    for _ in range(8):
        v = v[:, 0::2] + v[:, 1::2]
    total = np.zeros(c)
    for k in range(chunks):
        total = total + v[k, 0]
    return total


def numerators(zp, idx):
    """(2, C): TREE(a) and TREE(g) of the (n, C) table over the (n, m) list; entries of idx outside [0, n) are skipped"""
    zp = np.asarray(zp, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64)
    n = zp.shape[0]
    s, g = np.zeros(zp.shape), np.zeros(zp.shape)
    for q in range(idx.shape[1]):
        j = idx[:, q]
        ok = ((j >= 0) & (j < n))[:, None]
        v = zp[np.where(ok[:, 0], j, 0)]
        d = zp - v
        s = np.where(ok, s + v, s)
        g = np.where(ok, g + d * d, g)
    return np.stack([tree(zp * s), tree(g)])


def observed(z, idx):
    return numerators(z, idx)


def perm(z, idx, seed, image, p0, n_perms):
    """(P, 2, C): permutation p0 + j gives cell i the row z[sigma(i)]"""
    z = np.asarray(z, dtype=np.float64)
    return np.stack([numerators(z[EN.sigma(len(z), seed, image, p0 + j)], idx) for j in range(n_perms)])


def centred(x):
    """the table the Annotator hands to the kernels, restated: the column sums in the order of ribca_group_sums (one group; chunks of 1024 rows
    added in row order, then the chunks in order), divided by n, subtracted; and the sums of squares of the result in the same order"""
    x = np.asarray(x, dtype=np.float64)
    z = x - ordered_sum(x) / float(len(x))
    return z, ordered_sum(z * z)


def ordered_sum(x):
    total = np.zeros(x.shape[1])
    for k in range(0, len(x), 1024):
        part = np.zeros(x.shape[1])
        for row in x[k:k + 1024]:
            part = part + row
        total = total + part
    return total


def dense_moran(z, idx):
    """I = (n / S0) z'Wz / z'z per channel from a dense W with W[i, j] = the number of times j stands in the list of i; S0 = the sum of W"""
    z = np.asarray(z, dtype=np.float64)
    n = len(z)
    w = np.zeros((n, n))
    np.add.at(w, (np.repeat(np.arange(n), idx.shape[1]), np.asarray(idx).reshape(-1)), 1.0)
    return np.array([(n / w.sum()) * (z[:, c] @ w @ z[:, c]) / (z[:, c] @ z[:, c]) for c in range(z.shape[1])])
