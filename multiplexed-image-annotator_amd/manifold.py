"""GPU UMAP embedding and HDBSCAN for the extra-cell-types step (reference Annotator._find_extra_cell_types, model.py:642-675, which calls
``umap.UMAP(n_components=5).fit_transform``).  umap-learn 0.5's ``fit_transform`` defaults restated: the k-NN search, the fuzzy
membership weights and the layout SGD run in the HIP library (csrc/umap.hip); the graph union, the pruning, the (a, b) fit and the
spectral start are small host steps in scipy, as in umap itself.  DESIGN.md section "Extra cell types" lists the two deliberate
deviations of the SGD (Jacobi epochs, hashed negative samples): same input and seed, same bits.

``hdbscan`` restates ``sklearn.cluster.HDBSCAN(min_cluster_size).fit(x).labels_`` with sklearn's defaults: the core distances and the minimum
spanning tree of the mutual-reachability graph -- the O(n^2) part -- run in the HIP library (csrc/hdbscan.hip); the tree part (single linkage,
condensing, stabilities, excess-of-mass selection, labels) is host code below, written as small functions over plain arrays.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import scipy.sparse
import torch

from . import _lib, ops

MIN_DIST = 0.1
SPREAD = 1.0


def default_seed() -> int:
    """RIBCA_UMAP_SEED overrides the default seed 0 (the reference's UMAP is unseeded; this build is reproducible)."""
    v = os.environ.get("RIBCA_UMAP_SEED")
    return int(v) if v not in (None, "") else 0


def find_ab_params(spread: float = SPREAD, min_dist: float = MIN_DIST) -> Tuple[float, float]:
    """umap.umap_.find_ab_params: least-squares fit of 1 / (1 + a x^(2b)) to the offset exponential of (spread, min_dist)."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def default_epochs(n: int) -> int:
    return 500 if n <= 10000 else 200


def fuzzy_union(idx: np.ndarray, w: np.ndarray, n: int) -> scipy.sparse.csr_matrix:
    """fuzzy_simplicial_set's union P + P^T - P o P^T (set_op_mix_ratio 1) of the directed membership table, as canonical CSR."""
    k = idx.shape[1]
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    p = scipy.sparse.coo_matrix((w.ravel().astype(np.float32), (rows, idx.ravel().astype(np.int64))), shape=(n, n))
    p.eliminate_zeros()
    pt = p.transpose()
    prod = p.multiply(pt)
    g = (p + pt - prod).tocsr()
    g.sum_duplicates()
    g.sort_indices()
    g.eliminate_zeros()
    return g


def prune_graph(g: scipy.sparse.csr_matrix, n_epochs: int) -> scipy.sparse.csr_matrix:
    """simplicial_set_embedding: weights below max / n_epochs are dropped."""
    g = g.copy()
    g.data[g.data < (g.data.max() / float(n_epochs))] = 0.0
    g.eliminate_zeros()
    g.sort_indices()
    return g


def epochs_per_sample(weights: np.ndarray, n_epochs: int) -> np.ndarray:
    """umap.umap_.make_epochs_per_sample (fp64): n_epochs / (n_epochs w / max w); -1 where that count is 0."""
    result = -1.0 * np.ones(weights.shape[0], dtype=np.float64)
    n_samples = n_epochs * (weights / weights.max())
    result[n_samples > 0] = float(n_epochs) / np.float64(n_samples[n_samples > 0])
    return result


def reverse_edges(g: scipy.sparse.csr_matrix) -> np.ndarray:
    """rev[e] = position of edge (k, j) for edge e = (j, k) of a symmetric canonical CSR matrix.  Sorting the edges by (column, row)
    lists them in the CSR order of the transpose, which is the matrix itself: the i-th edge of that order is the mirror of edge i."""
    rows = np.repeat(np.arange(g.shape[0], dtype=np.int64), np.diff(g.indptr))
    order = np.lexsort((rows, g.indices.astype(np.int64)))
    rev = np.empty(len(order), dtype=np.int64)
    rev[order] = np.arange(len(order), dtype=np.int64)
    return rev


def spectral_backend(default: str = "scipy") -> str:
    """RIBCA_SPECTRAL=gpu | scipy: who computes the spectral start (read per call).  ``scipy`` is umap's own host call (eigsh); ``gpu`` is
    spectral_component_gpu.  The caller names its default: the extra-cell-types step "scipy", the whole-batch plot "gpu"."""
    v = os.environ.get("RIBCA_SPECTRAL") or default
    if v not in ("gpu", "scipy"):
        raise ValueError(f"RIBCA_SPECTRAL must be 'gpu' or 'scipy', got {v!r}")
    return v


#: a connected component below this many vertices stays on eigsh whatever the backend: ARPACK needs a few milliseconds there, and the GPU
#: solver's fixed cost (a few dozen launches and small read-backs per iteration) is of the same size
SPECTRAL_GPU_MIN_ROWS = 256
SPECTRAL_MAX_DIM = 12      # block = wanted + guard columns <= 16, the widest ribca_spectral_spmm


class GpuSpectralPrims:
    """The three primitives of csrc/spectral.hip behind the interface spectral_component_gpu is written over (tests/spectral_numpy.py holds the
    numpy twin, bit-equal operation by operation).  A block is an (n, m) fp64 device tensor; small matrices cross as numpy arrays."""

    def __init__(self, device=None):
        self.dev = device or _lib.require_gpu()
        self._ws = None

    def graph(self, g: scipy.sparse.csr_matrix, dinv: np.ndarray):
        return (torch.from_numpy(g.indptr.astype(np.int64)).to(self.dev), torch.from_numpy(g.indices.astype(np.int32)).to(self.dev),
                torch.from_numpy(g.data.astype(np.float32)).to(self.dev), torch.from_numpy(np.ascontiguousarray(dinv, dtype=np.float64)).to(self.dev))

    def upload(self, a: np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def download(self, h) -> np.ndarray:
        return h.cpu().numpy()

    def empty(self, n: int, m: int):
        return torch.empty((n, m), dtype=torch.float64, device=self.dev)

    def spmm(self, graph, x, out, alpha=1.0, beta=0.0, gamma=0.0, z=None):
        return ops.spectral_spmm(graph[0], graph[1], graph[2], graph[3], x, out, alpha, beta, gamma, z)

    def gram(self, u, v) -> np.ndarray:
        need = ops.spectral_gram_ws_bytes(u.shape[0], u.shape[1], v.shape[1])
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 8), dtype=torch.uint8, device=self.dev)
        return ops.spectral_gram(u, v, self._ws).cpu().numpy()

    def combine(self, u, c: np.ndarray, out, add=False):
        return ops.spectral_combine(u, self.upload(c), out, add)


def _orthonormalise(prims, src, tmp, dst) -> bool:
    """dst = an orthonormal basis of the columns of src: two passes of src T with T = D^-1 V L^-1/2 from the eigendecomposition V L V^T of the
    diagonally scaled Gram matrix (a Cholesky factor would do on a well-conditioned block; this form also survives a filtered block whose
    columns lean on one another).  Gram + combine only.  False: a column vanished or is not finite."""
    for a, b in ((src, tmp), (tmp, dst)):
        gm = prims.gram(a, a)
        gm = (gm + gm.T) * 0.5
        d = np.sqrt(np.diag(gm))
        if not np.isfinite(d).all() or (d <= 0).any():
            return False
        lam, vec = np.linalg.eigh(gm / np.outer(d, d))
        lam = np.maximum(lam, lam.max() * 1e-15)
        prims.combine(a, (vec / np.sqrt(lam)) / d[:, None], b)
    return True


def spectral_component_gpu(g: scipy.sparse.csr_matrix, dim: int, tol: float = 1e-5, max_spmm: int = 20000, prims=None, seed: int = 0,
                           info: Optional[Dict] = None) -> Optional[np.ndarray]:
    """The eigenvectors 1..dim of L = I - S, S = D^-1/2 A D^-1/2, of one connected graph by the smallest non-trivial eigenvalues: (n, dim)
    fp64, unit columns, in each column the entry of largest magnitude (the first of them) positive -- or None where initial_embedding falls
    back to the seeded uniform start (fewer than dim + 2 vertices, a vertex without weight, ``max_spmm`` column products spent before every
    wanted pair has ||S x - theta x||_2 <= tol, a block that lost rank).

    Chebyshev-filtered subspace iteration on S with Rayleigh-Ritz.  The trivial eigenvector sqrt(deg) / ||sqrt(deg)||
    is known and projected out of every block, never computed.  The block holds dim wanted and a few guard columns (16 at most) and starts
    from RandomState(seed).  Every pass: Q = orthonormal basis of the block, H = Q^T S Q, (theta, W) = eigh(H), X = Q W, residuals; then the
    block becomes p(S) X with p the Chebyshev polynomial that is bounded by 1 / T_m(..) on [-1, cut] and 1 at 1, cut = the lowest Ritz value
    of the block, the degree m taken from the gap between the last wanted Ritz value and cut.  All work on n rows goes through ``prims``
    (spmm / gram / combine: GpuSpectralPrims, or the numpy twin of the tests); the host keeps the small eigh and the decisions, so two
    bit-equal sets of primitives give bit-equal results.  ``info`` receives iterations, spmm (column products), spmm_calls, block, degrees,
    eigenvalues (of L) and residuals."""
    n = g.shape[0]
    if dim < 1 or dim > SPECTRAL_MAX_DIM:
        raise ValueError(f"spectral_component_gpu needs 1 <= dim <= {SPECTRAL_MAX_DIM}, got {dim}")
    stats = {"iterations": 0, "spmm": 0, "spmm_calls": 0, "degrees": []}

    def give_up():
        if info is not None:
            info.update(stats)
        return None

    if n < dim + 2:
        return give_up()
    g = g.tocsr()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.indptr))
    deg = np.bincount(rows, weights=g.data.astype(np.float64), minlength=n)      # fp64 row sums in CSR order
    if not (deg > 0).all() or not np.isfinite(deg).all():
        return give_up()
    root = np.sqrt(deg)
    if prims is None:
        prims = GpuSpectralPrims()
    b = min(16, max(dim + 6, 2 * dim), n - 1)
    stats["block"] = b
    gr = prims.graph(g, 1.0 / root)
    v0 = prims.upload((root / np.sqrt(np.dot(root, root)))[:, None])
    q, sq, x, r, t = (prims.empty(n, b) for _ in range(5))
    cur = prims.upload(np.random.RandomState(seed).normal(size=(n, b)))

    def spend(cols):
        if stats["spmm"] + cols > max_spmm:
            return False
        stats["spmm"] += cols
        stats["spmm_calls"] += 1
        return True

    while True:
        prims.combine(v0, -prims.gram(v0, cur), cur, add=True)      # project the trivial eigenvector out
        if not _orthonormalise(prims, cur, t, q):
            return give_up()
        if not spend(b):
            return give_up()
        prims.spmm(gr, q, sq)
        h = prims.gram(q, sq)
        theta, w = np.linalg.eigh((h + h.T) * 0.5)
        theta, w = theta[::-1].copy(), np.ascontiguousarray(w[:, ::-1])      # descending in S = ascending in L
        prims.combine(q, w, x)
        prims.combine(sq, w, r)
        prims.combine(q, -(w * theta[None, :]), r, add=True)      # r = S x - x diag(theta)
        res = np.sqrt(np.maximum(np.diag(prims.gram(r, r)), 0.0))
        stats["eigenvalues"] = (1.0 - theta[:dim]).tolist()
        stats["residuals"] = res[:dim].tolist()
        if not np.isfinite(res).all():
            return give_up()
        if (res[:dim] <= tol).all():
            break
        stats["iterations"] += 1
        cut = float(min(max(theta[-1], -0.9), 1.0))
        if not cut < 1.0 - 1e-12:
            return give_up()
        gap = float(theta[dim - 1]) - cut
        m = 16      # the first pass sees the Ritz values of a random block: they say nothing yet
        if stats["iterations"] > 1 and gap > 0:
            want = min(max(10.0 * float(res[:dim].max()) / tol, 1e2), 1e5)      # damping wanted from this pass
            m = int(np.ceil(np.log(2.0 * want) / np.arccosh(1.0 + 2.0 * gap / (1.0 + cut))))
        m = min(max(m, 8), 64)
        stats["degrees"].append(m)
        if not spend(b * m):
            return give_up()
        # t -> (t - c) / e sends [-1, cut] to [-1, 1]; the three-term recurrence scaled so that the polynomial is 1 at t = 1
        e, c = (cut + 1.0) / 2.0, (cut - 1.0) / 2.0
        s1 = e / (1.0 - c)
        sig = s1
        stats["spmm_calls"] += m - 1
        prims.spmm(gr, x, r, alpha=s1 / e, beta=-c * s1 / e)
        prev, cur = x, r
        for _ in range(2, m + 1):
            nxt = 1.0 / (2.0 / s1 - sig)
            prims.spmm(gr, cur, prev, alpha=2.0 * nxt / e, beta=-2.0 * nxt * c / e, gamma=-sig * nxt, z=prev)
            prev, cur = cur, prev
            sig = nxt
    norms = np.sqrt(np.diag(prims.gram(x, x)))[:dim]
    out = prims.download(x)[:, :dim] / norms[None, :]
    for j in range(dim):
        if out[np.argmax(np.abs(out[:, j])), j] < 0:
            out[:, j] = -out[:, j]
    if info is not None:
        info.update(stats)
    return np.ascontiguousarray(out)


def _spectral_component(g: scipy.sparse.csr_matrix, dim: int, spectral: str = "scipy", seed: int = 0,
                        info: Optional[Dict] = None) -> Optional[np.ndarray]:
    """spectral_layout of one connected graph: the eigenvectors 1..dim of the normalised Laplacian by the smallest eigenvalues (eigsh,
    which="SM", v0 = ones, tol 1e-4), or None where umap falls back to a random start (eigsh fails, or too few vertices).
    ``spectral`` = "gpu": spectral_component_gpu instead, for a graph of SPECTRAL_GPU_MIN_ROWS vertices or more."""
    from scipy.sparse.linalg import eigsh
    n = g.shape[0]
    if n < dim + 2:
        return None
    if spectral == "gpu" and n >= SPECTRAL_GPU_MIN_ROWS:
        sub: Dict = {}
        out = spectral_component_gpu(g, dim, seed=seed, info=sub)
        if info is not None:
            for key in ("iterations", "spmm", "spmm_calls"):
                info[key] = info.get(key, 0) + sub.get(key, 0)
            info["gpu_components"] = info.get("gpu_components", 0) + 1
        return out
    deg = np.asarray(g.sum(axis=0)).ravel()
    d = scipy.sparse.spdiags(1.0 / np.sqrt(deg), 0, n, n)
    lap = scipy.sparse.identity(n, format="csr") - d @ g @ d
    k = dim + 1
    ncv = max(2 * k + 1, int(np.sqrt(n)))
    try:
        vals, vecs = eigsh(lap, k, which="SM", ncv=ncv, tol=1e-4, v0=np.ones(n), maxiter=n * 5)
    except Exception:      # ArpackNoConvergence, ArpackError, a singular factorisation: umap falls back to the random start
        return None
    order = np.argsort(vals)[1:k]
    return vecs[:, order]


def spectral_init(g: scipy.sparse.csr_matrix, dim: int, rng: np.random.RandomState, spectral: Optional[str] = None, seed: int = 0,
                  info: Optional[Dict] = None) -> np.ndarray:
    """umap's spectral start (``spectral``: None = spectral_backend("scipy"), or "gpu" / "scipy"; every component goes the same way).  A disconnected graph: every component is laid out on its own (spectral, or seeded uniform in [-1, 1) where
    umap would fall back), scaled to max |x| = 1 and centred on its own point of a grid of spacing 3 -- a simplification of umap's
    multi_component_layout, deterministic for a given seed.  Returns None for umap's global random fallback."""
    from scipy.sparse.csgraph import connected_components
    if spectral is None:
        spectral = spectral_backend("scipy")
    elif spectral not in ("gpu", "scipy"):
        raise ValueError(f"spectral must be 'gpu' or 'scipy', got {spectral!r}")
    if info is not None:
        info["spectral_backend"] = spectral
    n_comp, labels = connected_components(g, directed=False)
    if n_comp == 1:
        return _spectral_component(g, dim, spectral, seed, info)
    out = np.zeros((g.shape[0], dim), dtype=np.float64)
    side = int(np.ceil(n_comp ** (1.0 / dim) - 1e-9))
    for c in range(n_comp):      # component numbers follow the lowest vertex index (connected_components' labelling)
        members = np.flatnonzero(labels == c)
        sub = g[members][:, members]
        lay = _spectral_component(sub, dim, spectral, seed, info)
        if lay is None:
            lay = rng.uniform(low=-1.0, high=1.0, size=(len(members), dim)) if len(members) > 1 else np.zeros((1, dim))
        m = np.abs(lay).max()
        if m > 0:
            lay = lay / m
        centre = 3.0 * np.array(np.unravel_index(c, (side,) * dim), dtype=np.float64)
        out[members] = lay + centre
    return out


def initial_embedding(g: scipy.sparse.csr_matrix, dim: int, seed: int, spectral: Optional[str] = None, info: Optional[Dict] = None) -> np.ndarray:
    """simplicial_set_embedding's start: the spectral layout scaled to max |x| = 10 plus N(0, 1e-4) noise, or uniform [-10, 10) where
    the spectral layout is unavailable; then every column rescaled to [0, 10].  fp32.  ``spectral`` as in spectral_init; ``info`` receives
    spectral_backend and, from the GPU solver, its iterations and SpMM counts."""
    n = g.shape[0]
    rng = np.random.RandomState(seed)
    init = spectral_init(g, dim, rng, spectral, seed, info)
    if init is None:
        emb = rng.uniform(low=-10.0, high=10.0, size=(n, dim)).astype(np.float32)
    else:
        expansion = 10.0 / np.abs(init).max()
        emb = (init * expansion).astype(np.float32) + rng.normal(scale=0.0001, size=[n, dim]).astype(np.float32)
    lo, hi = emb.min(0), emb.max(0)
    span = np.where(hi - lo > 0, hi - lo, 1.0)
    return (10.0 * (emb - lo) / span).astype(np.float32, order="C")


def umap_embed(x: np.ndarray, n_components: int = 5, n_neighbors: int = 15, seed: Optional[int] = None,
               timings: Optional[Dict[str, float]] = None, spectral: Optional[str] = None) -> np.ndarray:
    """umap.UMAP(n_components, n_neighbors).fit_transform(x) with umap-learn 0.5's defaults (euclidean, min_dist 0.1, spread 1,
    5 negative samples, learning rate 1, spectral start) -> (n, n_components) float32.  ``timings`` (optional) receives the milliseconds
    of the stages: knn, fuzzy, graph, init, sgd, and spectral_backend (with spectral_iterations, spectral_spmm and spectral_gpu_components from the GPU solver).
    ``spectral``: who computes the spectral start -- None = spectral_backend("scipy"), or "gpu" / "scipy"."""
    import time
    seed = default_seed() if seed is None else int(seed)
    dev = _lib.require_gpu()
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    if n < 2:
        raise ValueError(f"umap_embed needs at least 2 rows, got {n}")
    k = min(n_neighbors, n - 1)
    t = {}
    t0 = time.perf_counter()
    xd = torch.from_numpy(x).to(dev)
    idx_d, dist_d = ops.knn_dense(xd, k)
    torch.cuda.synchronize(dev)
    t["knn"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    _, _, w_d = ops.umap_fuzzy_weights(idx_d, dist_d)
    idx, w = idx_d.cpu().numpy(), w_d.cpu().numpy()
    t["fuzzy"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    n_epochs = default_epochs(n)
    g = prune_graph(fuzzy_union(idx, w, n), n_epochs)
    eps = epochs_per_sample(g.data, n_epochs)
    rev = reverse_edges(g)
    a, b = find_ab_params()
    t["graph"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    sinfo: Dict = {}
    emb = initial_embedding(g, n_components, seed, spectral, sinfo)
    t["init"] = (time.perf_counter() - t0) * 1e3
    t["spectral_backend"] = sinfo["spectral_backend"]
    if "iterations" in sinfo:
        t["spectral_iterations"], t["spectral_spmm"], t["spectral_gpu_components"] = sinfo["iterations"], sinfo["spmm"], sinfo["gpu_components"]
    t0 = time.perf_counter()
    emb_d = torch.from_numpy(emb).to(dev)
    ops.umap_optimize(emb_d, torch.from_numpy(g.indptr.astype(np.int64)).to(dev), torch.from_numpy(g.indices.astype(np.int32)).to(dev),
                      torch.from_numpy(rev).to(dev), torch.from_numpy(eps).to(dev), a, b, n_epochs, seed)
    out = emb_d.cpu().numpy()
    t["sgd"] = (time.perf_counter() - t0) * 1e3
    if timings is not None:
        timings.update(t)
    return out


# ------------------------------------------------------------------------------------------------------------------------- HDBSCAN
def hdbscan_backend() -> str:
    """RIBCA_HDBSCAN=gpu (default) | sklearn: which clustering Annotator._find_extra_cell_types calls (read per call; sklearn is the
    reference's own host call, kept for A/B)."""
    v = os.environ.get("RIBCA_HDBSCAN") or "gpu"
    if v not in ("gpu", "sklearn"):
        raise ValueError(f"RIBCA_HDBSCAN must be 'gpu' or 'sklearn', got {v!r}")
    return v


def validate_hdbscan_params(min_cluster_size, min_samples=None, n: Optional[int] = None) -> int:
    """sklearn's rules for the two parameters (ValueError, as HDBSCAN.fit raises): min_cluster_size an int >= 2, min_samples None or an
    int >= 1 and at most the number of rows.  Returns the effective min_samples (min_cluster_size where None)."""
    import numbers

    def is_int(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if not is_int(min_cluster_size) or min_cluster_size < 2:
        raise ValueError(f"The 'min_cluster_size' parameter of HDBSCAN must be an int in the range [2, inf). Got {min_cluster_size!r} instead.")
    if min_samples is not None and (not is_int(min_samples) or min_samples < 1):
        raise ValueError(f"The 'min_samples' parameter of HDBSCAN must be an int in the range [1, inf) or None. Got {min_samples!r} instead.")
    ms = int(min_cluster_size if min_samples is None else min_samples)
    if n is not None and ms > n:
        raise ValueError(f"min_samples ({ms}) must be at most the number of samples in X ({n})")
    return ms


def sort_mst_edges(u: np.ndarray, v: np.ndarray, w: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """the spanning tree's edges (u < v) in the total order (weight, u, v): the order the single-linkage tree is built in"""
    u, v, w = np.asarray(u), np.asarray(v), np.asarray(w)
    order = np.lexsort((v, u, w))
    return u[order], v[order], w[order]


def single_linkage(u: np.ndarray, v: np.ndarray, w: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The dendrogram of sorted spanning-tree edges, in scipy's layout: merge i makes node n + i out of left[i] = the node that holds u[i]
    and right[i] = the node that holds v[i] (the side of the edge's first end is the left child, as in sklearn's make_single_linkage),
    at height value[i] = w[i], with size[i] points.  Union-find with path compression over the 2 n - 1 nodes."""
    m = len(u)
    n = m + 1
    top = list(range(2 * n - 1))
    count = [1] * n + [0] * m
    left, right = [0] * m, [0] * m
    for i, (a, b) in enumerate(zip(np.asarray(u).tolist(), np.asarray(v).tolist())):
        ra = a
        while top[ra] != ra:
            ra = top[ra]
        while a != ra:
            nxt = top[a]
            top[a] = ra
            a = nxt
        rb = b
        while top[rb] != rb:
            rb = top[rb]
        while b != rb:
            nxt = top[b]
            top[b] = rb
            b = nxt
        node = n + i
        top[ra] = top[rb] = node
        left[i], right[i] = ra, rb
        count[node] = count[ra] + count[rb]
    return (np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64), np.asarray(w, dtype=np.float64),
            np.asarray(count[n:], dtype=np.int64))


def condense_tree(left: np.ndarray, right: np.ndarray, value: np.ndarray, size: np.ndarray,
                  min_cluster_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The dendrogram with every side smaller than min_cluster_size dropped: rows (parent, child, lambda = 1 / height, size of the child).
    The root is cluster n.  The dendrogram is walked breadth first from the top (left child before right); a merge whose two sides both
    reach min_cluster_size is a true split -- its left side gets the next free cluster id, then its right side -- a side below the size
    falls out of the parent point by point (the points of its subtree breadth first, size 1 each) and the other side, if large enough,
    keeps the parent's id.  Cluster ids therefore grow from the root down, and the row order is the walk's order (both are what sklearn's
    _condense_tree produces; the stabilities are summed in row order)."""
    m = len(left)
    n = m + 1
    root = 2 * m
    lt, rt, ht, sz = left.tolist(), right.tolist(), value.tolist(), size.tolist()
    order = [root]
    i = 0
    while i < len(order):
        x = order[i]
        i += 1
        if x >= n:
            order.append(lt[x - n])
            order.append(rt[x - n])
    cluster_of = [0] * (root + 1)
    cluster_of[root] = n
    next_id = n + 1
    dropped = bytearray(root + 1)
    rows_p: List[int] = []
    rows_c: List[int] = []
    rows_l: List[float] = []
    rows_s: List[int] = []

    def fall_out(sub, par, lam):
        queue = [sub]
        j = 0
        while j < len(queue):
            y = queue[j]
            j += 1
            dropped[y] = 1
            if y < n:
                rows_p.append(par)
                rows_c.append(y)
                rows_l.append(lam)
                rows_s.append(1)
            else:
                queue.append(lt[y - n])
                queue.append(rt[y - n])

    for node in order:
        if node < n or dropped[node]:
            continue
        k = node - n
        a, b, d = lt[k], rt[k], ht[k]
        lam = 1.0 / d if d > 0.0 else np.inf
        na = sz[a - n] if a >= n else 1
        nb = sz[b - n] if b >= n else 1
        par = cluster_of[node]
        if na >= min_cluster_size and nb >= min_cluster_size:
            for side, cnt in ((a, na), (b, nb)):
                cluster_of[side] = next_id
                rows_p.append(par)
                rows_c.append(next_id)
                rows_l.append(lam)
                rows_s.append(cnt)
                next_id += 1
        elif na < min_cluster_size and nb < min_cluster_size:
            fall_out(a, par, lam)
            fall_out(b, par, lam)
        elif na < min_cluster_size:
            cluster_of[b] = par
            fall_out(a, par, lam)
        else:
            cluster_of[a] = par
            fall_out(b, par, lam)
    return (np.asarray(rows_p, dtype=np.int64), np.asarray(rows_c, dtype=np.int64), np.asarray(rows_l, dtype=np.float64),
            np.asarray(rows_s, dtype=np.int64))


def cluster_stabilities(parent: np.ndarray, child: np.ndarray, lam: np.ndarray, size: np.ndarray) -> np.ndarray:
    """stability[c - root] = sum over the rows with parent c of (lambda - birth(c)) * size, birth = the lambda of the row that made c (0 for
    the root), summed in row order (np.bincount adds in input order)."""
    root = int(parent.min())
    births = np.full(max(int(child.max()), root) + 1, np.nan)
    births[child] = lam
    births[root] = 0.0
    with np.errstate(invalid="ignore"):      # duplicated points: inf - inf, as in sklearn
        contrib = (lam - births[parent]) * size
    return np.bincount(parent - root, weights=contrib, minlength=int(parent.max()) - root + 1)


def select_clusters(parent: np.ndarray, child: np.ndarray, size: np.ndarray, stability: np.ndarray) -> List[int]:
    """Excess of mass with the root excluded (allow_single_cluster=False): from the highest cluster id down, a cluster whose children's
    summed (already propagated) stability exceeds its own passes that sum up and is not selected; otherwise it is selected and everything
    below it is not.  Returns the selected ids in ascending order."""
    root = int(parent.min())
    stab = stability.tolist()
    kids: Dict[int, List[int]] = {}
    inner = size > 1
    for p, c in zip(parent[inner].tolist(), child[inner].tolist()):
        kids.setdefault(p, []).append(c)
    chosen = [True] * len(stab)
    chosen[0] = False
    for node in range(root + len(stab) - 1, root, -1):
        sub = 0.0
        for c in kids.get(node, ()):
            sub += stab[c - root]
        if sub > stab[node - root]:
            chosen[node - root] = False
            stab[node - root] = sub
        else:
            stack = list(kids.get(node, ()))
            while stack:
                c = stack.pop()
                chosen[c - root] = False
                stack.extend(kids.get(c, ()))
    return [root + k for k, on in enumerate(chosen) if on]


def assign_labels(parent: np.ndarray, child: np.ndarray, size: np.ndarray, clusters: Sequence[int]) -> np.ndarray:
    """Every point gets the number of the nearest selected cluster on its way up the condensed tree, -1 where that way reaches the root.
    The selected clusters are numbered in ascending id (sklearn's tree_to_labels rule)."""
    root = int(parent.min())
    top = np.arange(int(parent.max()) + 1, dtype=np.int64)
    selected = set(int(c) for c in clusters)
    inner = size > 1
    for c, p in sorted(zip(child[inner].tolist(), parent[inner].tolist())):      # ascending id: a parent before its children
        if c not in selected:
            top[c] = top[p]
    number = np.full(len(top), -1, dtype=np.int64)
    for k, c in enumerate(sorted(selected)):
        number[c] = k
    labels = np.full(root, -1, dtype=np.int64)
    pts = ~inner
    labels[child[pts]] = number[top[parent[pts]]]
    return labels


def labels_from_mst(u: np.ndarray, v: np.ndarray, w: np.ndarray, min_cluster_size: int) -> np.ndarray:
    """the tree part of HDBSCAN: spanning-tree edges (any order, u < v) -> labels (n) int64, -1 = noise"""
    su, sv, sw = sort_mst_edges(u, v, w)
    tree = condense_tree(*single_linkage(su, sv, sw), int(min_cluster_size))
    parent, child, lam, size = tree
    clusters = select_clusters(parent, child, size, cluster_stabilities(parent, child, lam, size))
    return assign_labels(parent, child, size, clusters)


def hdbscan(x: np.ndarray, min_cluster_size: int, min_samples: Optional[int] = None, timings: Optional[Dict[str, float]] = None) -> np.ndarray:
    """sklearn.cluster.HDBSCAN(min_cluster_size, min_samples).fit(x).labels_ with sklearn's defaults (euclidean, alpha 1, excess of mass, no
    single cluster, epsilon 0) -> (n) int64, -1 = noise.  Ties between equal mutual-reachability weights are broken by point index, where
    sklearn's depend on the visiting order of its Prim loop: the clusters agree up to their numbering and a handful of border points
    (DESIGN.md section "Extra cell types").  ``timings`` (optional) receives the milliseconds of the stages: core, mst, tree."""
    import time
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"hdbscan expects a 2-D array, got {x.ndim} dimension(s)")
    n = x.shape[0]
    ms = validate_hdbscan_params(min_cluster_size, min_samples, n)
    if not np.isfinite(x).all():
        raise ValueError("Input X contains NaN or infinity.")
    dev = _lib.require_gpu()
    x = np.ascontiguousarray(x, dtype=np.float32)
    t = {}
    t0 = time.perf_counter()
    xd = torch.from_numpy(x).to(dev)
    core2 = ops.core_distance(xd, ms)      # synchronises (reads the non-finite flag)
    t["core"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    u, v, w = (a.cpu().numpy() for a in ops.mreach_mst(xd, core2))
    t["mst"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    labels = labels_from_mst(u, v, w, int(min_cluster_size))
    t["tree"] = (time.perf_counter() - t0) * 1e3
    if timings is not None:
        timings.update(t)
    return labels
