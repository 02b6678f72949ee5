"""numpy oracle of the local indicators of spatial association, written from the rules include/ribca_hip.h states for ribca_local_lag and
ribca_local_perm_counts: the neighbour sums in list order, the conditional permutation (cell i keeps its row, the others move with the bijection
sigma_p of tests/enrichment_numpy.py and the swap that fixes i), the two counts.  numpy's float64 element-wise operations round every operation on
its own (no fma), as the kernels do."""
import numpy as np

import enrichment_numpy as EN


def _ordered_sum(z, src, ok):
    """(n, C): (((+0.0 + z[src[:, 0]]) + z[src[:, 1]]) + ...) over the entries with ok"""
    s = np.zeros(z.shape)
    for q in range(src.shape[1]):
        s = np.where(ok[:, q, None], s + z[np.where(ok[:, q], src[:, q], 0)], s)
    return s


def _valid(idx, n):
    idx = np.asarray(idx).astype(np.int64)
    return idx, (idx >= 0) & (idx < n)


def lag(z, idx):
    z = np.asarray(z, dtype=np.float64)
    idx, ok = _valid(idx, len(z))
    return _ordered_sum(z, idx, ok)


def sources(idx, sg):
    """(n, m): the source row of every list entry under sigma = sg: i if j == i; sg[i] if sg[j] == i; sg[j] otherwise (entries that are
    not valid: 0, never read)"""
    n = len(sg)
    idx, ok = _valid(idx, n)
    j = np.where(ok, idx, 0)
    own = np.arange(n)[:, None]
    return np.where(j == own, own, np.where(sg[j] == own, sg[own], sg[j]))


def perm_sums(z, idx, seed, image, p):
    """(n, C): s_p, the neighbour sums under the conditional permutation p"""
    z = np.asarray(z, dtype=np.float64)
    idx, ok = _valid(idx, len(z))
    return _ordered_sum(z, sources(idx, EN.sigma(len(z), seed, image, p)), ok)


def perm_counts(z, idx, observed, seed, image, p0, n_perms):
    """(ge, le), two (n, C) int64 arrays over the permutations p0 .. p0 + n_perms - 1"""
    observed = np.asarray(observed, dtype=np.float64)
    ge, le = np.zeros(observed.shape, dtype=np.int64), np.zeros(observed.shape, dtype=np.int64)
    for j in range(n_perms):
        s = perm_sums(z, idx, seed, image, p0 + j)
        ge += s >= observed
        le += s <= observed
    return ge, le
