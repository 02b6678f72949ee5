"""Numpy twin of csrc/spectral.hip, written from include/ribca_hip.h: the same sums in the same order, every product and sum rounded on its own
(numpy never contracts), so each primitive agrees with the kernel bit for bit -- and so does manifold.spectral_component_gpu run over
NumpyPrims, because the solver's host part is shared.  Also the planted graphs of the spectral tests and the derived bounds they assert.

The loops run over the position inside a row (spmm), the row inside a chunk (gram) and the column of u (combine) and are vectorised over
everything else; the order of the additions that reach one output is the kernel's.
"""
import numpy as np
import scipy.sparse

import umap_restatement as R

CHUNK = 1024


def spmm(indptr, indices, weights, dinv, x, alpha=1.0, beta=0.0, gamma=0.0, z=None):
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    dinv = np.asarray(dinv, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n, m = x.shape
    acc = np.zeros((n, m))
    length = np.diff(indptr)
    for k in range(int(length.max()) if n else 0):      # the k-th entry of every row that has one: per row, CSR order
        rows = np.flatnonzero(length > k)
        e = indptr[rows] + k
        j = indices[e]
        coef = (dinv[rows] * w[e]) * dinv[j]
        acc[rows] = acc[rows] + coef[:, None] * x[j]
    y = alpha * acc
    if beta != 0.0:
        y = y + beta * x
    if z is not None:
        y = y + gamma * np.asarray(z, dtype=np.float64)
    return y


def spmm_loop(indptr, indices, weights, dinv, x, alpha=1.0, beta=0.0, gamma=0.0, z=None):
    """the same, one scalar at a time: the plain statement the vectorised form above is checked against"""
    n, m = x.shape
    y = np.zeros((n, m))
    for i in range(n):
        for c in range(m):
            acc = 0.0
            for e in range(int(indptr[i]), int(indptr[i + 1])):
                j = int(indices[e])
                acc = acc + ((dinv[i] * np.float64(weights[e])) * dinv[j]) * x[j, c]
            v = alpha * acc
            if beta != 0.0:
                v = v + beta * x[i, c]
            if z is not None:
                v = v + gamma * z[i, c]
            y[i, c] = v
    return y


def gram(u, v):
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n, p = u.shape
    q = v.shape[1]
    chunks = (n + CHUNK - 1) // CHUNK
    up = np.zeros((chunks * CHUNK, p))
    vp = np.zeros((chunks * CHUNK, q))
    up[:n], vp[:n] = u, v
    up, vp = up.reshape(chunks, CHUNK, p), vp.reshape(chunks, CHUNK, q)
    live = np.minimum(n - np.arange(chunks) * CHUNK, CHUNK)
    part = np.zeros((chunks, p, q))
    for r in range(min(n, CHUNK)):      # row r of every chunk that has one
        on = live > r
        part[on] = part[on] + up[on, r, :, None] * vp[on, r, None, :]
    g = np.zeros((p, q))
    for ch in range(chunks):
        g = g + part[ch]
    return g


def combine(u, c, x=None, add=False):
    u, c = np.asarray(u, dtype=np.float64), np.asarray(c, dtype=np.float64)
    acc = np.array(x, dtype=np.float64, copy=True) if add else np.zeros((u.shape[0], c.shape[1]))
    for k in range(u.shape[1]):
        acc = acc + u[:, k, None] * c[None, k, :]
    return acc


class NumpyPrims:
    """the interface of manifold.GpuSpectralPrims over the functions above; a block is an (n, m) numpy array written in place"""

    def graph(self, g, dinv):
        return g.indptr.astype(np.int64), g.indices.astype(np.int32), g.data.astype(np.float32), np.asarray(dinv, dtype=np.float64)

    def upload(self, a):
        return np.array(a, dtype=np.float64, order="C")

    def download(self, h):
        return h.copy()

    def empty(self, n, m):
        return np.zeros((n, m))

    def spmm(self, graph, x, out, alpha=1.0, beta=0.0, gamma=0.0, z=None):
        assert out is not x
        out[...] = spmm(*graph, x, alpha, beta, gamma, z)
        return out

    def gram(self, u, v):
        return gram(u, v)

    def combine(self, u, c, out, add=False):
        assert out is not u
        out[...] = combine(u, c, out, add)
        return out


# ------------------------------------------------------------------------------------------------------------------- planted graphs
def blob_graph(sizes, norm, dim=15, seed=0):
    """the pruned fuzzy graph (umap_restatement, 15 neighbours, 500 epochs) of unit-noise blobs around normal centres scaled to ``norm``"""
    rng = np.random.RandomState(seed)
    centres = rng.normal(size=(len(sizes), dim))
    centres *= norm / np.linalg.norm(centres, axis=1, keepdims=True)
    x = np.concatenate([centres[c] + rng.normal(size=(m, dim)) for c, m in enumerate(sizes)])
    x = x[rng.permutation(len(x))].astype(np.float32)
    idx, dist = R.knn(x, 15)
    sigma, rho = R.smooth_knn_dist(dist)
    return R.prune(R.union(idx, R.membership(idx, dist, sigma, rho), len(x)), 500)


def fixture_a():
    return blob_graph((150, 200, 250), 4.0), 2


def fixture_b():
    return blob_graph((100, 150, 200, 250), 3.0), 3


def ring_graph(n=64):
    i = np.arange(n)
    a = scipy.sparse.coo_matrix((np.ones(2 * n, dtype=np.float32), (np.concatenate([i, i]), np.concatenate([(i + 1) % n, (i - 1) % n]))), shape=(n, n))
    g = a.tocsr()
    g.sort_indices()
    return g


def dense_normalised(g):
    """S = D^-1/2 A D^-1/2 in fp64, dense, and the eigenpairs of L = I - S ascending"""
    a = np.asarray(g.todense(), dtype=np.float64)
    dinv = 1.0 / np.sqrt(a.sum(axis=1))
    s = dinv[:, None] * a * dinv[None, :]
    lam, vec = np.linalg.eigh(np.eye(len(a)) - (s + s.T) / 2)
    return s, lam, vec


def check_against_dense(g, dim, out, tol, degenerate=False):
    """The derived bounds (none tuned).  With theta_j = x_j^T S x_j and r_j = S x_j - theta_j x_j of the returned unit columns:
    ||r_j|| <= tol (the solver's stopping rule); an eigenvalue of S lies within ||r_j|| of theta_j (the residual bound for a Rayleigh
    quotient of a symmetric matrix) -- the j-th one, unless the spectrum is degenerate; and the sine of the largest principal angle between
    span(out) and the exact invariant subspace is at most ||R||_F / delta, delta = lambda_{dim+1} - max(1 - theta) (Davis-Kahan sin-theta)."""
    s, lam, vec = dense_normalised(g)
    assert out.shape == (g.shape[0], dim) and out.dtype == np.float64
    assert np.allclose(np.linalg.norm(out, axis=0), 1.0, rtol=0, atol=1e-12)
    theta = np.einsum("ij,ij->j", out, s @ out)
    res = s @ out - out * theta[None, :]
    rn = np.linalg.norm(res, axis=0)
    assert (rn <= tol).all(), rn
    mu = 1.0 - theta      # eigenvalue estimates of L
    if not degenerate:
        assert (np.abs(mu - lam[1:dim + 1]) <= rn).all(), (mu, lam[1:dim + 1], rn)
    else:
        assert (np.abs(mu[:, None] - lam[None, 1:dim + 1]).min(axis=1) <= rn).all()
    delta = lam[dim + 1] - mu.max()
    assert delta > 0
    exact = vec[:, 1:dim + 1]
    qo, _ = np.linalg.qr(out)
    sine = np.linalg.norm(qo - exact @ (exact.T @ qo), 2)      # ||(I - E E^T) Q||_2 = the sine of the largest principal angle
    bound = np.linalg.norm(res) / delta
    # the measured sine carries the rounding of a dense eigh and a QR (a few n eps): far below any bound a residual of 1e-5 gives
    assert sine <= bound + 1e-12, (sine, bound)
    # sign rule
    for j in range(dim):
        k = int(np.argmax(np.abs(out[:, j])))
        assert out[k, j] > 0
    return {"residuals": rn, "eigenvalues": mu, "sine": sine, "bound": bound, "exact": lam[:dim + 2]}
