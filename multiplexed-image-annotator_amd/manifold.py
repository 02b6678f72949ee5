"""GPU UMAP embedding for the extra-cell-types step (reference Annotator._find_extra_cell_types, model.py:642-675, which calls
``umap.UMAP(n_components=5).fit_transform``).  umap-learn 0.5's ``fit_transform`` defaults restated: the k-NN search, the fuzzy
membership weights and the layout SGD run in the HIP library (csrc/umap.hip); the graph union, the pruning, the (a, b) fit and the
spectral start are small host steps in scipy, as in umap itself.  DESIGN.md section "Extra cell types" lists the two deliberate
deviations of the SGD (Jacobi epochs, hashed negative samples): same input and seed, same bits.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

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


def _spectral_component(g: scipy.sparse.csr_matrix, dim: int) -> Optional[np.ndarray]:
    """spectral_layout of one connected graph: the eigenvectors 1..dim of the normalised Laplacian by the smallest eigenvalues (eigsh,
    which="SM", v0 = ones, tol 1e-4), or None where umap falls back to a random start (eigsh fails, or too few vertices)."""
    from scipy.sparse.linalg import eigsh
    n = g.shape[0]
    if n < dim + 2:
        return None
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


def spectral_init(g: scipy.sparse.csr_matrix, dim: int, rng: np.random.RandomState) -> np.ndarray:
    """umap's spectral start.  A disconnected graph: every component is laid out on its own (spectral, or seeded uniform in [-1, 1) where
    umap would fall back), scaled to max |x| = 1 and centred on its own point of a grid of spacing 3 -- a simplification of umap's
    multi_component_layout, deterministic for a given seed.  Returns None for umap's global random fallback."""
    from scipy.sparse.csgraph import connected_components
    n_comp, labels = connected_components(g, directed=False)
    if n_comp == 1:
        return _spectral_component(g, dim)
    out = np.zeros((g.shape[0], dim), dtype=np.float64)
    side = int(np.ceil(n_comp ** (1.0 / dim) - 1e-9))
    for c in range(n_comp):      # component numbers follow the lowest vertex index (connected_components' labelling)
        members = np.flatnonzero(labels == c)
        sub = g[members][:, members]
        lay = _spectral_component(sub, dim)
        if lay is None:
            lay = rng.uniform(low=-1.0, high=1.0, size=(len(members), dim)) if len(members) > 1 else np.zeros((1, dim))
        m = np.abs(lay).max()
        if m > 0:
            lay = lay / m
        centre = 3.0 * np.array(np.unravel_index(c, (side,) * dim), dtype=np.float64)
        out[members] = lay + centre
    return out


def initial_embedding(g: scipy.sparse.csr_matrix, dim: int, seed: int) -> np.ndarray:
    """simplicial_set_embedding's start: the spectral layout scaled to max |x| = 10 plus N(0, 1e-4) noise, or uniform [-10, 10) where
    the spectral layout is unavailable; then every column rescaled to [0, 10].  fp32."""
    n = g.shape[0]
    rng = np.random.RandomState(seed)
    init = spectral_init(g, dim, rng)
    if init is None:
        emb = rng.uniform(low=-10.0, high=10.0, size=(n, dim)).astype(np.float32)
    else:
        expansion = 10.0 / np.abs(init).max()
        emb = (init * expansion).astype(np.float32) + rng.normal(scale=0.0001, size=[n, dim]).astype(np.float32)
    lo, hi = emb.min(0), emb.max(0)
    span = np.where(hi - lo > 0, hi - lo, 1.0)
    return (10.0 * (emb - lo) / span).astype(np.float32, order="C")


def umap_embed(x: np.ndarray, n_components: int = 5, n_neighbors: int = 15, seed: Optional[int] = None,
               timings: Optional[Dict[str, float]] = None) -> np.ndarray:
    """umap.UMAP(n_components, n_neighbors).fit_transform(x) with umap-learn 0.5's defaults (euclidean, min_dist 0.1, spread 1,
    5 negative samples, learning rate 1, spectral start) -> (n, n_components) float32.  ``timings`` (optional) receives the milliseconds
    of the stages: knn, fuzzy, graph, init, sgd."""
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
    emb = initial_embedding(g, n_components, seed)
    t["init"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    emb_d = torch.from_numpy(emb).to(dev)
    ops.umap_optimize(emb_d, torch.from_numpy(g.indptr.astype(np.int64)).to(dev), torch.from_numpy(g.indices.astype(np.int32)).to(dev),
                      torch.from_numpy(rev).to(dev), torch.from_numpy(eps).to(dev), a, b, n_epochs, seed)
    out = emb_d.cpu().numpy()
    t["sgd"] = (time.perf_counter() - t0) * 1e3
    if timings is not None:
        timings.update(t)
    return out
