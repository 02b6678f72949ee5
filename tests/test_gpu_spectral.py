"""csrc/spectral.hip against its numpy twin (tests/spectral_numpy.py), bit for bit, and manifold.spectral_component_gpu on the GPU against its own
run over the numpy primitives: the same iteration count and the same bytes."""
import ctypes

import numpy as np
import pytest
import scipy.sparse
import torch

import spectral_numpy as SN
from multiplexed_image_annotator_amd import _lib, manifold, ops

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _graph(n, seed):
    """a symmetric canonical CSR graph of about 12 entries per row with one 300-entry hub row (where n allows) and one empty row"""
    rng = np.random.RandomState(seed)
    if n == 1:
        return scipy.sparse.csr_matrix((1, 1), dtype=np.float32)
    m = 6 * n
    i, j = rng.randint(0, n, m), rng.randint(0, n, m)
    hub = rng.choice(n, min(300, n - 1), replace=False)
    i, j = np.concatenate([i, np.zeros(len(hub), dtype=np.int64)]), np.concatenate([j, hub])
    keep = i != j
    a = scipy.sparse.coo_matrix((rng.rand(keep.sum()).astype(np.float32), (i[keep], j[keep])), shape=(n, n)).tocsr()
    a = a.maximum(a.T).tolil()
    empty = n // 2
    a[empty, :] = 0
    a[:, empty] = 0
    g = a.tocsr().astype(np.float32)
    g.eliminate_zeros()
    g.sort_indices()
    return g


def _dev_graph(g, dinv, dev):
    return (torch.from_numpy(g.indptr.astype(np.int64)).to(dev), torch.from_numpy(g.indices.astype(np.int32)).to(dev),
            torch.from_numpy(g.data.astype(np.float32)).to(dev), torch.from_numpy(dinv).to(dev))


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_spmm_matches_numpy_bit_for_bit(n):
    dev = _lib.require_gpu()
    g = _graph(n, n)
    rng = np.random.RandomState(n + 1)
    dinv = 1.0 / np.sqrt(rng.rand(n) + 0.5)
    if n > 1:
        assert np.diff(g.indptr).max() >= min(300, n - 1) - 2 and np.diff(g.indptr)[n // 2] == 0
    gd = _dev_graph(g, dinv, dev)
    gn = (g.indptr, g.indices, g.data, dinv)
    for m in (1, 3, 8, 16):
        x, z = rng.randn(n, m), rng.randn(n, m)
        xd, zd = torch.from_numpy(x).to(dev), torch.from_numpy(z).to(dev)
        plain = ops.spectral_spmm(*gd, xd).cpu().numpy()
        assert np.array_equal(_bits(plain), _bits(SN.spmm(*gn, x))), (n, m)
        fused = ops.spectral_spmm(*gd, xd, alpha=0.37, beta=-1.25, gamma=0.61, z=zd).cpu().numpy()
        want = SN.spmm(*gn, x, 0.37, -1.25, 0.61, z)
        assert np.array_equal(_bits(fused), _bits(want)), (n, m)
        assert np.array_equal(fused[n // 2], (0.37 * 0.0 + -1.25 * x[n // 2]) + 0.61 * z[n // 2])      # the empty row: beta x + gamma z
        # in place over z, as the three-term recurrence of the solver calls it
        ops.spectral_spmm(*gd, xd, out=zd, alpha=0.37, beta=-1.25, gamma=0.61, z=zd)
        assert np.array_equal(_bits(zd.cpu().numpy()), _bits(want))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3 * 1024 + 17])
def test_gram_and_combine_match_numpy_bit_for_bit(n):
    dev = _lib.require_gpu()
    rng = np.random.RandomState(n)
    for p, q in ((1, 1), (9, 1), (9, 24), (24, 9), (48, 48), (1, 48)):
        u, v = rng.randn(n, p), rng.randn(n, q)
        ud, vd = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
        assert np.array_equal(_bits(ops.spectral_gram(ud, vd).cpu().numpy()), _bits(SN.gram(u, v))), (n, p, q)
        c = rng.randn(p, q)
        cd = torch.from_numpy(c).to(dev)
        got = ops.spectral_combine(ud, cd)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(SN.combine(u, c))), (n, p, q)
        ops.spectral_combine(ud, cd, out=vd, add=True)
        assert np.array_equal(_bits(vd.cpu().numpy()), _bits(SN.combine(u, c, v, add=True))), (n, p, q)


@pytest.fixture(scope="module")
def numpy_runs():
    out = {}
    for name, fx in (("A", SN.fixture_a), ("B", SN.fixture_b)):
        g, dim = fx()
        info = {}
        out[name] = (g, dim, manifold.spectral_component_gpu(g, dim, tol=TOL, prims=SN.NumpyPrims(), info=info), info)
    return out


@pytest.mark.parametrize("name", ["A", "B"])
def test_solver_is_bit_equal_to_its_numpy_run(numpy_runs, name):
    g, dim, want, winfo = numpy_runs[name]
    info = {}
    got = manifold.spectral_component_gpu(g, dim, tol=TOL, info=info)
    print(f"[spectral gpu {name}] {info}")
    assert info["iterations"] == winfo["iterations"] and info["spmm"] == winfo["spmm"] and info["degrees"] == winfo["degrees"]
    assert np.array_equal(_bits(got), _bits(want))
    assert info["residuals"] == winfo["residuals"] and info["eigenvalues"] == winfo["eigenvalues"]
    SN.check_against_dense(g, dim, got, TOL)
    again = manifold.spectral_component_gpu(g, dim, tol=TOL)
    assert np.array_equal(_bits(got), _bits(again))


def test_initial_embedding_takes_the_gpu_backend(numpy_runs):
    g, dim, want, _ = numpy_runs["A"]
    info = {}
    emb = manifold.initial_embedding(g, dim, 0, spectral="gpu", info=info)
    assert info["spectral_backend"] == "gpu" and info["gpu_components"] == 1 and info["iterations"] >= 1
    # the start is the solver's vectors scaled to max |x| = 10, plus the seeded noise, rescaled per column to [0, 10]
    rng = np.random.RandomState(0)
    ref = (want * (10.0 / np.abs(want).max())).astype(np.float32) + rng.normal(scale=0.0001, size=want.shape).astype(np.float32)
    lo, hi = ref.min(0), ref.max(0)
    assert np.array_equal(emb, (10.0 * (ref - lo) / (hi - lo)).astype(np.float32))


def test_entry_points_refuse_bad_requests():
    dev = _lib.require_gpu()
    lib = _lib.lib()
    g = _graph(257, 3)
    dinv = np.ones(257)
    gd = _dev_graph(g, dinv, dev)
    with pytest.raises(_lib.RibcaError, match="ribca_spectral_spmm.*m <= 16"):
        ops.spectral_spmm(*gd, torch.zeros((257, 17), dtype=torch.float64, device=dev))
    wide = torch.zeros((257, 8), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        ops.spectral_spmm(*gd, wide[:, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        ops.spectral_gram(wide[:, ::2], wide)
    with pytest.raises(ValueError):
        ops.spectral_spmm(*gd, wide.float())
    with pytest.raises(_lib.RibcaError, match="y must not be x"):
        ops.spectral_spmm(*gd, wide, out=wide)
    with pytest.raises(_lib.RibcaError, match="ribca_spectral_gram.*48"):
        ops.spectral_gram(torch.zeros((10, 49), dtype=torch.float64, device=dev), torch.zeros((10, 2), dtype=torch.float64, device=dev))
    with pytest.raises(_lib.RibcaError, match="workspace too small"):
        ops.spectral_gram(wide, wide, ws=torch.empty(8 * 64 - 1, dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.RibcaError, match="ribca_spectral_combine.*48"):
        ops.spectral_combine(wide, torch.zeros((8, 49), dtype=torch.float64, device=dev))

    def refused(status, name):
        assert status != 0 and name.encode() in lib.ribca_last_error()

    x = wide.data_ptr()
    refused(lib.ribca_spectral_spmm(None, None, None, 0, None, 257, 8, x, 1.0, 0.0, 0.0, None, x, None), "ribca_spectral_spmm")
    refused(lib.ribca_spectral_spmm(gd[0].data_ptr(), gd[1].data_ptr(), gd[2].data_ptr(), g.nnz, gd[3].data_ptr(), 0, 8, x, 1.0, 0.0, 0.0, None, x, None),
            "ribca_spectral_spmm")
    refused(lib.ribca_spectral_gram(x, None, 257, 8, 8, x, x, 1 << 20, None), "ribca_spectral_gram")
    refused(lib.ribca_spectral_gram(x, x, 257, 8, 8, x, None, 0, None), "ribca_spectral_gram")
    refused(lib.ribca_spectral_combine(x, 257, 8, None, 8, 0, x, None), "ribca_spectral_combine")
    assert lib.ribca_spectral_gram_ws_bytes(1025, 3, 5) == 8 * 2 * 15 and lib.ribca_spectral_gram_ws_bytes(10, 49, 1) == 0
    skipped = ctypes.c_int64(0)
    refused(lib.ribca_scatter_raster(None, None, 5, 1.0, 0.0, 1.0, 0.0, 8, 8, 2, x, ctypes.byref(skipped), x, 1 << 20, None), "ribca_scatter_raster")
    refused(lib.ribca_scatter_raster(x, x, 5, 1.0, 0.0, 1.0, 0.0, 8, 8, 17, x, ctypes.byref(skipped), x, 1 << 20, None), "ribca_scatter_raster")
    refused(lib.ribca_scatter_raster(x, x, 5, 1.0, 0.0, 1.0, 0.0, 8, 8, 2, x, ctypes.byref(skipped), x, 256, None), "ribca_scatter_raster")
    torch.cuda.synchronize()
