"""The umap kernels of the extra-cell-types step (csrc/umap.hip) against the plain restatement in tests/umap_restatement.py, the
embedding's quality on planted data, and the cell-type kernels of knn.hip beyond 32 types."""
import numpy as np
import pytest
import torch

import umap_restatement as R
from kernel_harness import umap_graph
from multiplexed_image_annotator_amd import _lib, manifold, ops

pytestmark = pytest.mark.gpu


def _ulp_close(a, b, ulps=2):
    return abs(float(a) - float(b)) <= ulps * float(np.spacing(np.float32(max(abs(a), abs(b)))))


@pytest.mark.parametrize("dim", [15, 37, 100])
def test_knn_dense_matches_brute_force(dim):
    dev = _lib.require_gpu()
    n, k = 5000 if dim < 100 else 1500, 15
    rng = np.random.RandomState(dim)
    x = rng.randn(n, dim).astype(np.float32)
    x[100:110] = x[7]            # duplicated rows: distance 0 ties, broken towards the lower index
    x[2000 % n:2000 % n + 5] = x[11]
    idx, dist = ops.knn_dense(torch.from_numpy(x).to(dev), k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    # fp64 brute force
    x64 = x.astype(np.float64)
    sq = (x64 ** 2).sum(1)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2 * x64 @ x64.T, 0)
    for i in range(len(x)):
        d2[i, i] = 0
    d2[np.abs(x64[:, None, :5] - x64[None, :, :5]).sum(-1) == 0] = 0      # cheap exact-duplicate fix-up (rows equal -> 0)
    ref_idx = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), d2), axis=1)[:, :k]
    assert np.all(idx[:, 0] <= np.arange(n))                   # the row itself, or an earlier identical row
    assert np.array_equal(idx[7, :11], [7] + list(range(100, 110)))
    # distances: against fp64 on the kernel's own indices
    d_own = np.sqrt(((x64[:, None, :] - x64[idx]) ** 2).sum(-1))
    assert np.allclose(dist, d_own, rtol=1e-6, atol=1e-6)
    assert np.all(np.diff(dist, axis=1) >= 0)
    ref_d = np.sqrt(np.take_along_axis(d2, ref_idx, axis=1))
    bad = 0
    for i in np.flatnonzero((idx != ref_idx).any(1)):
        for p in np.flatnonzero(idx[i] != ref_idx[i]):
            # an index may differ only where two distances lie within 2 ulp of each other
            if not _ulp_close(dist[i, p], ref_d[i, p]) and not np.isclose(dist[i, p], ref_d[i, p], rtol=2.5e-7, atol=1e-6):
                bad += 1
    assert bad == 0


@pytest.mark.parametrize("dim,k", [(15, 15), (37, 40), (64, 64), (100, 20)])
def test_knn_dense_matches_fp32_restatement(dim, k):
    """the same fp32 sums in the same order: the same indices; distances within the rounding of one sqrt"""
    dev = _lib.require_gpu()
    x = np.random.RandomState(dim).randn(700, dim).astype(np.float32)
    x[50] = x[3]
    idx, dist = ops.knn_dense(torch.from_numpy(x).to(dev), k)
    ri, rd = R.knn(x, k)
    assert np.array_equal(idx.cpu().numpy(), ri)
    assert np.allclose(dist.cpu().numpy(), rd, rtol=2.5e-7, atol=0)


def test_knn_dense_refuses_unsupported_sizes():
    dev = _lib.require_gpu()
    x = torch.zeros((10, 300), device=dev)
    with pytest.raises(_lib.RibcaError, match="ribca_knn_dense"):
        ops.knn_dense(x[:, :4].contiguous(), 11)              # k > n
    with pytest.raises(_lib.RibcaError, match="ribca_knn_dense"):
        ops.knn_dense(torch.zeros((100, 4), device=dev), 65)   # k > 64
    with pytest.raises(_lib.RibcaError, match="ribca_knn_dense"):
        ops.knn_dense(torch.zeros((10, 257), device=dev), 5)   # dim > 256


def test_fuzzy_weights_match_restatement():
    dev = _lib.require_gpu()
    x = np.random.RandomState(9).randn(3000, 12).astype(np.float32)
    x[200:230] = x[17]           # a row whose 15 neighbours are all at distance 0: the global-mean floor
    idx_d, dist_d = ops.knn_dense(torch.from_numpy(x).to(dev), 15)
    sigma, rho, w = (t.cpu().numpy() for t in ops.umap_fuzzy_weights(idx_d, dist_d))
    idx, dist = idx_d.cpu().numpy(), dist_d.cpu().numpy()
    rs, rr = R.smooth_knn_dist(dist)
    assert (rr[200:230] == 0).all()
    assert np.allclose(rho, rr, rtol=1e-5, atol=0)
    assert np.allclose(sigma, rs, rtol=1e-5, atol=0)
    assert np.allclose(w, R.membership(idx, dist, rs, rr), rtol=1e-5, atol=1e-7)


def _gpu_optimize(emb, g, eps, rev, epochs, n_epochs, a, b, seed):
    dev = _lib.require_gpu()
    e = torch.from_numpy(emb.copy()).to(dev)
    ops.umap_optimize(e, torch.from_numpy(g.indptr.astype(np.int64)).to(dev), torch.from_numpy(g.indices.astype(np.int32)).to(dev),
                      torch.from_numpy(rev).to(dev), torch.from_numpy(eps).to(dev), a, b, epochs, seed)
    return e.cpu().numpy()


@pytest.mark.parametrize("dim", [2, 5])
def test_sgd_matches_restated_jacobi_epochs(dim):
    g, eps, rev = umap_graph(400, dim)
    a, b = manifold.find_ab_params()
    emb0 = manifold.initial_embedding(g, dim, 0)
    for epochs in (1, 3, 10):
        # the GPU run of `epochs` epochs uses the alpha schedule of an n_epochs = epochs run; so does the restatement
        got = _gpu_optimize(emb0, g, eps, rev, epochs, epochs, a, b, 7)
        ref = R.optimize(emb0.copy(), g.indptr, g.indices, rev, eps, epochs, epochs, a, b, 7)
        assert np.abs(got - ref).max() < 1e-4, (epochs, np.abs(got - ref).max())


def test_sgd_is_deterministic_and_seeded():
    g, eps, rev = umap_graph(1500, 1)
    a, b = manifold.find_ab_params()
    emb0 = manifold.initial_embedding(g, 5, 0)
    r1 = _gpu_optimize(emb0, g, eps, rev, 50, 500, a, b, 3)
    r2 = _gpu_optimize(emb0, g, eps, rev, 50, 500, a, b, 3)
    r3 = _gpu_optimize(emb0, g, eps, rev, 50, 500, a, b, 4)
    assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32))
    assert not np.array_equal(r1, r3)


def test_sgd_refuses_one_byte_less_than_its_query():
    """the workspace check of ribca_umap_optimize is its query; it needs indptr[n] from the device, so unlike the other four it cannot be
    asked without one.  Refused before any launch: emb keeps its bytes."""
    dev = _lib.require_gpu()
    n, dim, nnz = 400, 2, 1000
    indptr = torch.linspace(0, nnz, n + 1, device=dev).to(torch.int64)
    indices, rev = torch.zeros(nnz, dtype=torch.int32, device=dev), torch.zeros(nnz, dtype=torch.int64, device=dev)
    eps, emb = torch.ones(nnz, dtype=torch.float64, device=dev), torch.full((n, dim), 3.0, dtype=torch.float32, device=dev)
    need = ops.umap_optimize_ws_bytes(n, dim, nnz)
    assert need == 2 * 8192 + 3328 and int(indptr[n]) == nnz
    with pytest.raises(_lib.RibcaError, match="ribca_umap_optimize.*workspace"):
        ops.umap_optimize(emb, indptr, indices, rev, eps, 1.5, 0.9, 3, 7, ws=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    assert bool((emb == 3.0).all())


def test_umap_embed_quality_on_planted_blobs():
    from sklearn.cluster import HDBSCAN
    from sklearn.manifold import trustworthiness
    from sklearn.metrics import adjusted_rand_score
    x, y = R.planted_blobs(0)
    emb = manifold.umap_embed(x, n_components=5, seed=0)
    assert emb.shape == (len(x), 5) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert np.array_equal(emb, manifold.umap_embed(x, n_components=5, seed=0))
    lab = HDBSCAN(min_cluster_size=50).fit(emb).labels_
    blob = y >= 0
    ari = adjusted_rand_score(y[blob], lab[blob])
    sub = np.random.RandomState(1).choice(len(x), 3000, replace=False)
    tw = trustworthiness(x[sub], emb[sub], n_neighbors=5)
    print(f"[umap quality] n = {len(x)}: ARI {ari:.4f} on the blob points, trustworthiness {tw:.4f}")
    assert ari >= 0.95 and tw >= 0.9


@pytest.mark.parametrize("T", [100, 254])
def test_cooccurrence_and_compositions_beyond_32_types(T):
    from oracle import ref_spatial
    dev = _lib.require_gpu()
    rng = np.random.RandomState(T)
    n = 600
    x, y = rng.uniform(0, 500, n), rng.uniform(0, 500, n)
    x[10], y[10] = x[20], y[20]
    types = rng.randint(0, T, n)
    types[0] = T - 1
    m = ops.knn_cooccurrence(x, y, types, T, 25, device=dev).cpu().numpy()
    assert np.array_equal(m.astype(np.float64), ref_spatial.cooccurrence(x, y, types, T, 25))
    c = ops.knn_compositions(x, y, types, T, device=dev)
    assert np.array_equal(c, ref_spatial.compositions(x, y, types))
    with pytest.raises(_lib.RibcaError):
        ops.knn_cooccurrence(x, y, types, 255, 25, device=dev)
