"""Plain numpy restatement of the GPU part of HDBSCAN (include/ribca_hip.h: ribca_core_distance, ribca_mreach_mst), written from its
description: the oracle of tests/test_hdbscan_host.py and tests/test_gpu_hdbscan.py.

    d2(i, j)      fp32 sum of squared differences in dimension order (every product and sum rounds on its own)
    core2(i)      the min_samples-th smallest d2(i, .), the point itself counted
    mreach2(i, j) max(core2(i), core2(j), d2(i, j))
    tree          Kruskal over all pairs in the total order (mreach2, min(i, j), max(i, j)); weights sqrt(mreach2) in fp32

The n x n matrix is formed: a few thousand points at most.
"""
import numpy as np

# (seed, n, min_cluster_size): the planted inputs the feature was specified on
PLANTED = [(0, 1500, 10), (1, 1500, 25), (2, 3000, 50), (3, 3000, 10), (4, 2000, 5), (5, 3000, 20), (6, 2500, 15)]
# after the best one-to-one renaming at most 0.5 % of the points may differ from sklearn.cluster.HDBSCAN (ties between equal
# mutual-reachability weights are broken by index here, by Prim's visiting order there)
CAP = 0.005


def planted(seed, n, dim=5, centres=8):
    """8 centres uniform in [0, 10]^5; 95 % of the points a random centre + N(0, 0.25^2), 5 % uniform in [0, 10]^5; float32"""
    rng = np.random.RandomState(seed)
    c = rng.uniform(0, 10, size=(centres, dim))
    n_noise = int(round(0.05 * n))
    n_blob = n - n_noise
    which = rng.randint(centres, size=n_blob)
    blob = c[which] + 0.25 * rng.randn(n_blob, dim)
    noise = rng.uniform(0, 10, size=(n_noise, dim))
    x = np.concatenate([blob, noise]).astype(np.float32)
    truth = np.concatenate([which, np.full(n_noise, -1)])
    perm = rng.permutation(n)
    return np.ascontiguousarray(x[perm]), truth[perm]


def lattice(seed, n, dim=5, side=3):
    """points of a small integer lattice drawn with replacement: duplicated rows and massive ties of every distance"""
    rng = np.random.RandomState(seed)
    return rng.randint(side, size=(n, dim)).astype(np.float32)


def two_groups(seed, n, dim=5, gap=1000.0):
    """two Gaussian groups far apart: the last Boruvka round joins them by one long edge"""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, dim)
    x[n // 3:, 0] += gap
    return x.astype(np.float32)


def dist2(x):
    x = np.asarray(x, dtype=np.float32)
    n, dim = x.shape
    s = np.zeros((n, n), dtype=np.float32)
    for d in range(dim):
        e = x[:, None, d] - x[None, :, d]
        s = s + e * e
    return s


def core2(d2, min_samples):
    return np.partition(d2, min_samples - 1, axis=1)[:, min_samples - 1].copy()


def mreach2(d2, c2):
    return np.maximum(np.maximum(c2[:, None], c2[None, :]), d2)


def kruskal(n, u, v):
    """positions (into the sorted edge list u, v) of the spanning forest's edges.  The edges are taken in blocks: a block is first
    thinned with the components known before it (vectorised), the survivors go through a union-find one by one."""
    parent = np.arange(n)
    taken = []
    block = 1 << 16
    for s in range(0, len(u), block):
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        bu, bv = u[s:s + block], v[s:s + block]
        cand = np.flatnonzero(parent[bu] != parent[bv])
        pl = parent.tolist()
        for e in cand.tolist():
            a, b = int(bu[e]), int(bv[e])
            while pl[a] != a:
                a = pl[a]
            while pl[b] != b:
                b = pl[b]
            if a != b:
                pl[b] = a
                taken.append(s + e)
        parent = np.asarray(pl)
        if len(taken) == n - 1:
            break
    return np.asarray(taken, dtype=np.int64)


def mst(x, min_samples):
    """(u, v, w, core2): the unique minimum spanning tree under the total order, u < v, in that order; w = sqrt(mreach2) fp32"""
    d2 = dist2(x)
    c2 = core2(d2, min_samples)
    m2 = mreach2(d2, c2)
    n = len(x)
    iu, iv = np.triu_indices(n, 1)
    w2 = m2[iu, iv]
    order = np.lexsort((iv, iu, w2))
    iu, iv, w2 = iu[order], iv[order], w2[order]
    pos = kruskal(n, iu, iv)
    assert len(pos) == n - 1
    return iu[pos].astype(np.int32), iv[pos].astype(np.int32), np.sqrt(w2[pos]).astype(np.float32), c2


def best_renaming_mismatches(a, b):
    """points labelled differently after the best one-to-one renaming of b's clusters to a's (noise maps to noise only)"""
    from scipy.optimize import linear_sum_assignment
    a, b = np.asarray(a), np.asarray(b)
    ka, kb = int(a.max()) + 1, int(b.max()) + 1
    agree = int(((a < 0) & (b < 0)).sum())
    if ka > 0 and kb > 0:
        both = (a >= 0) & (b >= 0)
        table = np.zeros((ka, kb), dtype=np.int64)
        np.add.at(table, (a[both], b[both]), 1)
        r, c = linear_sum_assignment(-table)
        agree += int(table[r, c].sum())
    return len(a) - agree
