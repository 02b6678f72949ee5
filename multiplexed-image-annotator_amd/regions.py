"""Tissue regions on the GPU (reference spatial_methods.tissue_region_partition, spatial_methods.py:133-198, which calls scikit-learn's
``PCA(n_components=0.99).fit_transform`` and ``KMeans(n_clusters=n).fit_predict`` on the host, unseeded).  scikit-learn 1.7's defaults
restated and seeded: everything that touches all n rows runs in the HIP library (csrc/regions.hip); the F x F eigen-decomposition, the
k-means++ draws and the stopping decisions are small host steps.  DESIGN.md section 11 states the arithmetic and what differs from
scikit-learn; tests/regions_numpy.py reproduces it bit for bit.  Same table and seed, same labels -- on every rank of a run.
"""
from __future__ import annotations

import math
import numbers
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

MAX_ITER = 300
TOL = 1e-4
MASK64 = 0xFFFFFFFFFFFFFFFF


def region_backend() -> str:
    """RIBCA_REGIONS=gpu (default) | sklearn: which PCA + k-means Annotator.tissue_region_analysis calls (read per call; sklearn is the
    reference's own pair of host calls, kept for A/B)."""
    v = os.environ.get("RIBCA_REGIONS") or "gpu"
    if v not in ("gpu", "sklearn"):
        raise ValueError(f"RIBCA_REGIONS must be 'gpu' or 'sklearn', got {v!r}")
    return v


def default_seed() -> int:
    """RIBCA_REGION_SEED overrides the default seed 0 (the reference's KMeans is unseeded; this build is reproducible)."""
    v = os.environ.get("RIBCA_REGION_SEED")
    return int(v) if v not in (None, "") else 0


def validate_n_clusters(k, n: Optional[int] = None) -> int:
    """scikit-learn's rules for ``n_clusters`` (ValueError, as KMeans.fit raises): an int >= 1, and at most the number of rows."""
    if not isinstance(k, numbers.Integral) or isinstance(k, bool) or k < 1:
        raise ValueError(f"The 'n_clusters' parameter of KMeans must be an int in the range [1, inf). Got {k!r} instead.")
    if n is not None and n < k:
        raise ValueError(f"n_samples={n} should be >= n_clusters={int(k)}.")
    return int(k)


# ------------------------------------------------------------------------------------------------------------------------------ PCA
def pca_from_gram(gram: np.ndarray, colsum: np.ndarray, n: int, size_col: np.ndarray, var: float = 0.99):
    """mean (F), components (d, F), eigenvalues (F) of the table count / size from the exact integer sums of the counts: the covariance in a
    fixed fp64 formula, numpy.linalg.eigh, then what scikit-learn's PCA does with its own (eigenvalues descending and clamped at 0, the
    entry of largest magnitude of every component positive, d = searchsorted(cumsum(ratio), var, side='right') + 1)."""
    size = np.asarray(size_col, dtype=np.float64)
    mean = colsum.astype(np.float64) / size / float(n)
    cov = (gram.astype(np.float64) / (size[:, None] * size[None, :]) - float(n) * (mean[:, None] * mean[None, :])) / float(n - 1)
    lam, vec = np.linalg.eigh(cov)
    lam = lam[::-1].copy()
    vt = np.ascontiguousarray(vec[:, ::-1].T)
    lam[lam < 0.0] = 0.0
    top = np.argmax(np.abs(vt), axis=1)
    sign = np.sign(vt[np.arange(vt.shape[0]), top])
    sign[sign == 0] = 1.0
    vt *= sign[:, None]
    ratio = lam / lam.sum()
    d = int(np.searchsorted(np.cumsum(ratio), var, side="right")) + 1
    d = min(d, vt.shape[0])
    return mean, np.ascontiguousarray(vt[:d]), lam, d


def pca_project(counts: torch.Tensor, sizes: Sequence[int], var: float = 0.99, info: Optional[dict] = None) -> torch.Tensor:
    """``PCA(n_components=var).fit_transform(counts / size)`` of the (n, n_sizes, n_types) int16 device count table of
    ops.knn_composition_counts -> (n, d) fp64 device tensor.  ``info`` (optional) receives mean, components, eigenvalues, d."""
    if counts.dim() != 3 or counts.shape[1] != len(sizes):
        raise ValueError("pca_project expects an (n, n_sizes, n_types) count table")
    n, _, t = counts.shape
    if n < 2:
        raise ValueError("pca_project needs at least 2 rows")
    flat = counts.reshape(n, len(sizes) * t)
    size_col = np.repeat(np.asarray(list(sizes), dtype=np.float64), t)
    colsum, gram = ops.region_gram(flat)
    mean, comps, lam, d = pca_from_gram(gram.cpu().numpy(), colsum.cpu().numpy(), n, size_col, var)
    dev = counts.device
    y = ops.region_project(flat, torch.from_numpy(size_col).to(dev), torch.from_numpy(mean).to(dev), torch.from_numpy(comps).to(dev))
    if info is not None:
        info.update(mean=mean, components=comps, eigenvalues=lam, d=d)
    return y


# -------------------------------------------------------------------------------------------------------------------------- k-means
def _splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed: int, step: int, trial: int) -> float:
    """uniform in [0, 1): the top 53 bits of splitmix64(splitmix64(splitmix64(seed) ^ step) ^ trial) -- counter-based, as the negative
    samples of the UMAP layout are"""
    h = _splitmix64(_splitmix64(_splitmix64(int(seed) & MASK64) ^ int(step)) ^ int(trial))
    return (h >> 11) * (1.0 / 9007199254740992.0)


def kmeans_plusplus(y: torch.Tensor, k: int, seed: int) -> Tuple[List[int], torch.Tensor]:
    """Greedy k-means++ with 2 + floor(ln k) trials per step (scikit-learn's default): the rows picked, and min d2 of every row to them.
    Step 0 takes row floor(u n).  In step c a draw u picks the first row whose sequential prefix sum of the current min d2 reaches
    u * total (host: n fp64 per step); the distance work and the potential of every trial run on the device; the trial of least
    (potential, trial index) wins."""
    n = y.shape[0]
    dev = y.device
    trials = 2 + int(math.log(k))
    first = min(int(draw(seed, 0, 0) * n), n - 1)
    picks = [first]
    d2, _ = ops.kmeans_trials(y, torch.tensor([first], dtype=torch.int32, device=dev), None)
    closest = d2[0].contiguous()
    for c in range(1, k):
        prefix = np.cumsum(closest.cpu().numpy())
        targets = np.array([draw(seed, c, t) for t in range(trials)], dtype=np.float64) * prefix[-1]
        cand = np.minimum(np.searchsorted(prefix, targets, side="left"), n - 1).astype(np.int32)
        d2, pot = ops.kmeans_trials(y, torch.from_numpy(cand).to(dev), closest)
        best = int(np.argmin(pot.cpu().numpy()))
        picks.append(int(cand[best]))
        closest = d2[best].contiguous()
    return picks, closest


def kmeans(y, k: int, seed: Optional[int] = None, timings: Optional[Dict[str, float]] = None, init: Optional[np.ndarray] = None,
           trace: Optional[list] = None) -> np.ndarray:
    """``KMeans(n_clusters=k).fit_predict(y)`` with scikit-learn's defaults (one k-means++ start, Lloyd, max_iter 300, tol 1e-4 x the mean
    column variance on the summed squared centre shift, stop also when no label changed, one more assignment after a stop by tol, empty
    clusters relocated to the rows farthest from their centres) on the (n, d) fp64 rows y (device tensor or array) -> (n) int64 labels;
    cluster j is the j-th k-means++ pick.  ``init`` (k, d) replaces the k-means++ start; ``timings`` receives iterations, picks, inertia,
    init_ms, lloyd_ms; ``trace`` (a list) receives (labels, centres) of every Lloyd iteration."""
    k = validate_n_clusters(k, None)
    dev = _lib.require_gpu()
    if not isinstance(y, torch.Tensor):
        y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev)
    if y.dim() != 2 or y.dtype != torch.float64:
        raise ValueError("kmeans expects an (n, d) float64 table")
    y = y.contiguous()
    n, d = y.shape
    validate_n_clusters(k, n)
    seed = default_seed() if seed is None else int(seed)
    yh = y.cpu().numpy()
    if not np.isfinite(yh).all():
        raise ValueError("Input X contains NaN or infinity.")
    tol = float(np.mean(np.var(yh, axis=0)) * TOL)
    t0 = time.perf_counter()
    if init is None:
        picks, _ = kmeans_plusplus(y, k, seed)
        centres = y[torch.tensor(picks, dtype=torch.int64, device=y.device)].contiguous()
    else:
        picks = []
        centres = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64)).to(y.device)
        if tuple(centres.shape) != (k, d):
            raise ValueError(f"The shape of the initial centers {tuple(centres.shape)} does not match (n_clusters, n_features) = ({k}, {d})")
    torch.cuda.synchronize()
    t_init = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    other = torch.empty_like(centres)
    labels = torch.full((n,), -1, dtype=torch.int32, device=y.device)
    mind2 = torch.empty(n, dtype=torch.float64, device=y.device)
    changed = torch.zeros(1, dtype=torch.int32, device=y.device)
    sums = torch.empty((k, d), dtype=torch.float64, device=y.device)
    counts = torch.empty(k, dtype=torch.int32, device=y.device)
    stat = torch.empty(1 + 2 * k, dtype=torch.float64, device=y.device)
    ws = torch.empty(max(ops.kmeans_update_ws_bytes(n, d, k), 256), dtype=torch.uint8, device=y.device)
    strict = False
    iterations = 0
    for it in range(MAX_ITER):
        ops.kmeans_assign(y, centres, labels, mind2, changed)
        ops.kmeans_update(y, labels, centres, other, sums, counts, changed, stat, ws)
        st = stat.cpu().numpy()
        empty = np.flatnonzero(st[1:1 + k] == 0.0)
        if len(empty):
            # scikit-learn's rule: the rows farthest from their centres, farthest first (ties to the lowest row index), one per empty cluster
            far = np.lexsort((np.arange(n), -mind2.cpu().numpy()))[:len(empty)]
            ops.kmeans_relocate(y, labels, torch.from_numpy(far.astype(np.int32)).to(y.device), torch.from_numpy(empty.astype(np.int32)).to(y.device),
                                sums, counts)
            ops.kmeans_finalize(sums, counts, centres, other, changed, stat)
            st = stat.cpu().numpy()
        centres, other = other, centres
        iterations = it + 1
        if trace is not None:
            trace.append((labels.cpu().numpy().astype(np.int64), centres.cpu().numpy().copy()))
        if st[0] == 0.0:
            strict = True
            break
        shift = 0.0
        for v in st[1 + k:1 + 2 * k].tolist():
            shift = shift + v
        if shift <= tol:
            break
    if not strict:
        ops.kmeans_assign(y, centres, labels, mind2, changed)
    out = labels.cpu().numpy().astype(np.int64)
    if timings is not None:
        timings.update(iterations=iterations, picks=picks, init_ms=t_init, lloyd_ms=(time.perf_counter() - t0) * 1e3, tol=tol,
                       inertia=float(np.cumsum(mind2.cpu().numpy())[-1]), centres=centres.cpu().numpy())
    return out
