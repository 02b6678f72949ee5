"""manifold.spectral_component_gpu run over the numpy primitives of tests/spectral_numpy.py (the solver's loop is shared with the GPU run and the
primitives are bit-equal, tests/test_gpu_spectral.py), checked against dense numpy.linalg.eigh with derived bounds; the backend switch; and
the host arithmetic of the scatter plot.

Fixture A: three blobs (150 / 200 / 250 points, centres of norm 4), 20.6 entries per row, L has eigenvalues 0, 0.0142, 0.0373, then 0.2927.
Fixture B: four blobs (100 / 150 / 200 / 250, norm 3), dim 3: 0, 0.0531, 0.0669, 0.1124, then 0.3048."""
import numpy as np
import pytest
import scipy.sparse

import scatter_numpy as SC
import spectral_numpy as SN
from multiplexed_image_annotator_amd import manifold, ops

TOL = 1e-5


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, fx in (("A", SN.fixture_a), ("B", SN.fixture_b)):
        g, dim = fx()
        info = {}
        vec = manifold.spectral_component_gpu(g, dim, tol=TOL, prims=SN.NumpyPrims(), info=info)
        out[name] = (g, dim, vec, info)
    return out


@pytest.mark.parametrize("name", ["A", "B"])
def test_solver_meets_the_derived_bounds(solved, name):
    g, dim, vec, info = solved[name]
    assert vec is not None
    from scipy.sparse.csgraph import connected_components
    assert connected_components(g, directed=False)[0] == 1
    rep = SN.check_against_dense(g, dim, vec, TOL)
    print(f"[spectral {name}] n = {g.shape[0]}, {g.nnz / g.shape[0]:.1f} entries per row, block {info['block']}, {info['iterations']} filter passes "
          f"(degrees {info['degrees']}), {info['spmm']} column products; residuals {rep['residuals']}, sine {rep['sine']:.2e} <= {rep['bound']:.2e}; "
          f"exact {rep['exact']}")
    # the solver's own report agrees with the recomputation (same vectors, another summation order)
    assert np.allclose(info["eigenvalues"], rep["eigenvalues"], rtol=0, atol=1e-12)
    assert np.allclose(info["residuals"], rep["residuals"], rtol=0, atol=1e-12)
    assert info["spmm"] == info["block"] * (info["iterations"] + 1 + sum(info["degrees"]))


def test_fixture_a_is_the_stated_graph(solved):
    g = solved["A"][0]
    _, lam, _ = SN.dense_normalised(g)
    assert g.shape == (600, 600) and abs(g.nnz / 600 - 20.6) < 0.05
    assert np.allclose(lam[:4], [0, 0.0142, 0.0373, 0.2927], rtol=0, atol=5e-5)


def test_solver_is_a_function_of_graph_and_seed(solved):
    g, dim, vec, info = solved["A"]
    again = manifold.spectral_component_gpu(g, dim, tol=TOL, prims=SN.NumpyPrims())
    assert np.array_equal(vec.view(np.uint64), again.view(np.uint64))
    other = manifold.spectral_component_gpu(g, dim, tol=TOL, prims=SN.NumpyPrims(), seed=1)
    assert not np.array_equal(vec, other)
    SN.check_against_dense(g, dim, other, TOL)      # another start, the same subspace and the same signs' rule


def test_ring_of_64_has_degenerate_pairs():
    g = SN.ring_graph(64)
    vec = manifold.spectral_component_gpu(g, 2, tol=TOL, prims=SN.NumpyPrims())
    rep = SN.check_against_dense(g, 2, vec, TOL, degenerate=True)
    assert np.allclose(rep["eigenvalues"], 1 - np.cos(2 * np.pi / 64), rtol=0, atol=TOL)


def test_solver_gives_up_with_none():
    g, dim = SN.fixture_a()
    info = {}
    assert manifold.spectral_component_gpu(g, dim, max_spmm=1, prims=SN.NumpyPrims(), info=info) is None
    assert info["spmm"] == 0 and info["iterations"] == 0
    info = {}
    assert manifold.spectral_component_gpu(g, dim, max_spmm=100, prims=SN.NumpyPrims(), info=info) is None      # the first filter does not fit
    assert info["spmm"] <= 100
    tiny = SN.ring_graph(3)
    assert manifold.spectral_component_gpu(tiny, 2, prims=SN.NumpyPrims()) is None      # n < dim + 2
    lone = scipy.sparse.csr_matrix(np.array([[0, 1, 0, 0, 0], [1, 0, 1, 0, 0], [0, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=np.float32))
    assert manifold.spectral_component_gpu(lone, 2, prims=SN.NumpyPrims()) is None      # a vertex without weight
    with pytest.raises(ValueError):
        manifold.spectral_component_gpu(g, 13, prims=SN.NumpyPrims())


def test_small_graph_spans_the_whole_complement():
    """n - 1 < dim + guard columns: the block is the whole complement of the trivial eigenvector, and one Rayleigh-Ritz pass is exact"""
    g = SN.ring_graph(7)
    g = g + scipy.sparse.csr_matrix(([0.5, 0.5], ([0, 3], [3, 0])), shape=(7, 7), dtype=np.float32)      # a chord: no degenerate pairs left to chance
    g = g.tocsr()
    g.sort_indices()
    info = {}
    vec = manifold.spectral_component_gpu(g, 2, tol=TOL, prims=SN.NumpyPrims(), info=info)
    assert info["block"] == 6 and info["iterations"] == 0
    SN.check_against_dense(g, 2, vec, TOL, degenerate=True)


def test_backend_switch(monkeypatch):
    monkeypatch.delenv("RIBCA_SPECTRAL", raising=False)
    assert manifold.spectral_backend("scipy") == "scipy" and manifold.spectral_backend("gpu") == "gpu"
    monkeypatch.setenv("RIBCA_SPECTRAL", "gpu")
    assert manifold.spectral_backend("scipy") == "gpu"
    monkeypatch.setenv("RIBCA_SPECTRAL", "scipy")
    assert manifold.spectral_backend("gpu") == "scipy"
    monkeypatch.setenv("RIBCA_SPECTRAL", "bogus")
    with pytest.raises(ValueError, match="RIBCA_SPECTRAL"):
        manifold.spectral_backend("gpu")
    g, dim = SN.fixture_a()
    with pytest.raises(ValueError, match="RIBCA_SPECTRAL"):
        manifold.initial_embedding(g, dim, 0)
    with pytest.raises(ValueError):
        manifold.initial_embedding(g, dim, 0, spectral="arpack")


# ---- a copy of the start as it stood before the switch existed: the arithmetic spectral="scipy" must keep, bit for bit
def _old_component(g, dim):
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
    except Exception:
        return None
    return vecs[:, np.argsort(vals)[1:k]]


def _old_initial_embedding(g, dim, seed):
    from scipy.sparse.csgraph import connected_components
    n = g.shape[0]
    rng = np.random.RandomState(seed)
    n_comp, labels = connected_components(g, directed=False)
    if n_comp == 1:
        init = _old_component(g, dim)
    else:
        init = np.zeros((n, dim), dtype=np.float64)
        side = int(np.ceil(n_comp ** (1.0 / dim) - 1e-9))
        for c in range(n_comp):
            members = np.flatnonzero(labels == c)
            lay = _old_component(g[members][:, members], dim)
            if lay is None:
                lay = rng.uniform(low=-1.0, high=1.0, size=(len(members), dim)) if len(members) > 1 else np.zeros((1, dim))
            m = np.abs(lay).max()
            if m > 0:
                lay = lay / m
            init[members] = lay + 3.0 * np.array(np.unravel_index(c, (side,) * dim), dtype=np.float64)
    if init is None:
        emb = rng.uniform(low=-10.0, high=10.0, size=(n, dim)).astype(np.float32)
    else:
        emb = (init * (10.0 / np.abs(init).max())).astype(np.float32) + rng.normal(scale=0.0001, size=[n, dim]).astype(np.float32)
    lo, hi = emb.min(0), emb.max(0)
    span = np.where(hi - lo > 0, hi - lo, 1.0)
    return (10.0 * (emb - lo) / span).astype(np.float32, order="C")


def test_scipy_backend_keeps_the_bits(monkeypatch):
    monkeypatch.delenv("RIBCA_SPECTRAL", raising=False)
    g, dim = SN.fixture_a()
    two = scipy.sparse.block_diag([g, SN.ring_graph(3), SN.fixture_b()[0]], format="csr").astype(np.float32)      # three components, one too small
    two.sort_indices()
    for graph, d in ((g, dim), (g, 5), (two, 2)):
        want = _old_initial_embedding(graph, d, 3)
        info = {}
        assert np.array_equal(manifold.initial_embedding(graph, d, 3, spectral="scipy", info=info).view(np.uint32), want.view(np.uint32))
        assert info == {"spectral_backend": "scipy"}
        assert np.array_equal(manifold.initial_embedding(graph, d, 3).view(np.uint32), want.view(np.uint32))      # the default is scipy


# ---- primitives: the vectorised numpy forms are the plain loops
def test_numpy_spmm_is_the_plain_loop():
    rng = np.random.RandomState(5)
    n = 40
    dense = np.triu((rng.rand(n, n) < 0.15) * rng.rand(n, n), 1)
    dense[0, 1:] = rng.rand(n - 1)      # a hub row
    dense[:, 7] = 0
    dense[7, :] = 0                     # an empty row
    g = scipy.sparse.csr_matrix((dense + dense.T).astype(np.float32))
    g.sort_indices()
    gr = SN.NumpyPrims().graph(g, rng.rand(n) + 0.5)
    x, z = rng.randn(n, 3), rng.randn(n, 3)
    assert np.array_equal(SN.spmm(*gr, x), SN.spmm_loop(*gr, x))
    y = SN.spmm(*gr, x, 0.3, -0.2, 1.7, z)
    assert np.array_equal(y, SN.spmm_loop(*gr, x, 0.3, -0.2, 1.7, z))
    assert np.array_equal(y[7], -0.2 * x[7] + 1.7 * z[7])
    u, v = rng.randn(2100, 3), rng.randn(2100, 2)
    want = np.zeros((3, 2))
    for ch in range(3):
        part = np.zeros((3, 2))
        for r in range(ch * 1024, min(2100, (ch + 1) * 1024)):
            part = part + u[r][:, None] * v[r][None, :]
        want = want + part
    assert np.array_equal(SN.gram(u, v), want)
    assert np.allclose(SN.combine(u, rng.randn(3, 4)).shape, (2100, 4))


# ---- the plot's host arithmetic
def test_disc_offsets():
    assert SC.disc_offsets(0) == [(0, 0)]
    assert len(SC.disc_offsets(1)) == 9      # dx^2 + dy^2 <= 2: the full 3 x 3
    two = SC.disc_offsets(2)
    assert len(two) == 21 and (2, 1) in two and (1, -2) in two and (2, 2) not in two      # <= 5: the 5 x 5 without its corners
    assert len(SC.disc_offsets(3)) == 37      # <= 10: (3, 1) in, (3, 2) out


def test_affine_map_has_five_percent_margins():
    pts = np.array([[-3.0, 10.0], [7.0, 30.0], [2.0, 12.0], [np.nan, 1e9]])
    h, w = 1200, 1600
    aff = ops.scatter_affine(pts, h, w)
    assert np.allclose(aff, SC.affine(pts, h, w), rtol=1e-15, atol=0)
    ax, bx, ay, by = aff
    assert np.isclose(ax * (-3.0 - 0.5) + bx, 0) and np.isclose(ax * (7.0 + 0.5) + bx, w - 1)
    assert np.isclose(ay * (30.0 + 1.0) + by, 0) and np.isclose(ay * (10.0 - 1.0) + by, h - 1)      # y grows upwards
    # the extreme points land 1 / 22 of the canvas inside its edge
    assert np.isclose(ax * -3.0 + bx, (w - 1) / 22) and np.isclose(ay * 30.0 + by, (h - 1) / 22)
    one = ops.scatter_affine(np.array([[4.0, 4.0]]), 64, 96)      # no spread: a span of 1
    assert np.isclose(one[0] * 4.0 + one[1], 95 / 2) and np.isclose(one[2] * 4.0 + one[3], 63 / 2)
    img, skipped, index = SC.raster(pts, np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 9, 9]], dtype=np.uint8), h, w, aff)
    assert skipped == 1 and (index > 0).sum() == 3 * 21 and set(np.unique(index)) == {0, 1, 2, 3}
    assert (img[index == 0] == 255).all() and (img[index == 2] == [0, 255, 0]).all()


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    """the argument checks run before any HIP call: NULL buffers, m = 17, a short workspace and aliasing come back as a status with a text"""
    import ctypes
    from multiplexed_image_annotator_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    skipped = ctypes.c_int64(0)
    for call, text in (
            (lambda: lib.ribca_spectral_spmm(None, None, None, 0, None, 257, 8, p, 1.0, 0.0, 0.0, None, p, None), b"ribca_spectral_spmm: NULL buffer"),
            (lambda: lib.ribca_spectral_spmm(p, p, p, 5, p, 257, 17, p, 1.0, 0.0, 0.0, None, p, None), b"ribca_spectral_spmm: needs 1 <= m <= 16"),
            (lambda: lib.ribca_spectral_spmm(p, p, p, 5, p, 0, 8, p, 1.0, 0.0, 0.0, None, p, None), b"ribca_spectral_spmm: needs n >= 1"),
            (lambda: lib.ribca_spectral_spmm(p, p, p, 5, p, 257, 8, p, 1.0, 0.0, 0.0, None, p, None), b"ribca_spectral_spmm: y must not be x"),
            (lambda: lib.ribca_spectral_gram(p, p, 257, 8, 8, p, p, 511, None), b"ribca_spectral_gram: workspace too small"),
            (lambda: lib.ribca_spectral_gram(p, p, 257, 49, 8, p, p, 1 << 20, None), b"ribca_spectral_gram: needs 1 <= p, q <= 48"),
            (lambda: lib.ribca_spectral_gram(p, None, 257, 8, 8, p, p, 1 << 20, None), b"ribca_spectral_gram: NULL buffer"),
            (lambda: lib.ribca_spectral_combine(p, 257, 8, None, 8, 0, p, None), b"ribca_spectral_combine: NULL buffer"),
            (lambda: lib.ribca_spectral_combine(p, 257, 8, p, 49, 0, p + 8, None), b"ribca_spectral_combine: needs 1 <= p, m <= 48"),
            (lambda: lib.ribca_scatter_raster(None, None, 5, 1.0, 0.0, 1.0, 0.0, 8, 8, 2, p, ctypes.byref(skipped), p, 1 << 20, None),
             b"ribca_scatter_raster: NULL buffer"),
            (lambda: lib.ribca_scatter_raster(p, p, 5, 1.0, 0.0, 1.0, 0.0, 8, 8, 17, p, ctypes.byref(skipped), p, 1 << 20, None),
             b"ribca_scatter_raster: needs 0 <= radius <= 16"),
            (lambda: lib.ribca_scatter_raster(p, p, 5, 1.0, 0.0, 1.0, 0.0, 8, 8, 2, p, ctypes.byref(skipped), p, 256, None),
             b"ribca_scatter_raster: workspace too small")):
        status = call()
        assert status != 0 and text in lib.ribca_last_error(), (text, lib.ribca_last_error())
    assert lib.ribca_spectral_gram_ws_bytes(1025, 3, 5) == 8 * 2 * 15 and lib.ribca_spectral_gram_ws_bytes(10, 49, 1) == 0
    assert lib.ribca_scatter_raster_ws_bytes(9, 12) == 256 + 512 and lib.ribca_scatter_raster_ws_bytes(0, 12) == 0
    # 2 al(8 nnz) + al(4 n dim); the refusal of one byte less needs indptr[n] from the device: tests/test_gpu_umap.py
    assert lib.ribca_umap_optimize_ws_bytes(400, 2, 1000) == 2 * 8192 + 3328 and lib.ribca_umap_optimize_ws_bytes(1025, 5, 0) == 20736
    assert lib.ribca_umap_optimize_ws_bytes(400, 9, 1000) == 0 and lib.ribca_umap_optimize_ws_bytes(0, 2, 1000) == 0
    assert lib.ribca_umap_optimize_ws_bytes(400, 2, -1) == 0
