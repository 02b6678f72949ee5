"""Host side of the extra-cell-types step (min_cells > 0, reference model.py:642-675): the umap constants and graph steps of manifold.py
against the plain restatement (tests/umap_restatement.py), the relabelling of the Annotator, the sharding rule, and the compile checks of
the new kernels.  No GPU needed."""
import os

import numpy as np
import pytest

import umap_restatement as R
from multiplexed_image_annotator_amd import manifold, ops


def test_find_ab_params_matches_umap_constants():
    a, b = manifold.find_ab_params()
    assert abs(a - 1.5769) < 1e-3 and abs(b - 0.8951) < 1e-3, (a, b)


def _table(n=300, k=15, seed=3):
    x = np.random.RandomState(seed).randn(n, 7).astype(np.float32)
    x[5] = x[9]      # a duplicated row
    idx, dist = R.knn(x, k)
    sigma, rho = R.smooth_knn_dist(dist)
    return idx, R.membership(idx, dist, sigma, rho)


def test_union_pruning_and_epochs_per_sample_match_restatement():
    idx, w = _table()
    n = idx.shape[0]
    g = manifold.fuzzy_union(idx, w, n)
    ref = R.union(idx, w, n)
    assert np.array_equal(g.indptr, ref.indptr) and np.array_equal(g.indices, ref.indices)
    assert np.allclose(g.data, ref.data, rtol=1e-6, atol=0)
    assert abs(g - g.T).max() == 0      # symmetric to the bit
    for ep in (200, 500):
        gp, rp = manifold.prune_graph(g, ep), R.prune(ref, ep)
        assert np.array_equal(gp.indices, rp.indices) and np.array_equal(gp.indptr, rp.indptr)
        assert gp.data.min() >= gp.data.max() / ep
        e1, e2 = manifold.epochs_per_sample(gp.data, ep), R.epochs_per_sample(gp.data, ep)
        assert np.allclose(e1, e2, rtol=1e-12) and e1.min() == pytest.approx(1.0)
    assert np.array_equal(manifold.reverse_edges(gp), R.rev_index(gp))
    assert manifold.default_epochs(10000) == 500 and manifold.default_epochs(10001) == 200


def test_initial_embedding_is_seeded_and_scaled():
    idx, w = _table()
    g = manifold.prune_graph(manifold.fuzzy_union(idx, w, idx.shape[0]), 500)
    a = manifold.initial_embedding(g, 5, 0)
    assert a.dtype == np.float32 and a.shape == (idx.shape[0], 5)
    assert np.allclose(a.min(0), 0) and np.allclose(a.max(0), 10)
    assert np.array_equal(a, manifold.initial_embedding(g, 5, 0)) and not np.array_equal(a, manifold.initial_embedding(g, 5, 1))


def test_initial_embedding_of_a_disconnected_graph_separates_components():
    x = np.concatenate([np.random.RandomState(1).randn(60, 4), 100 + np.random.RandomState(2).randn(50, 4), [[500, 0, 0, 0]] * 3])
    idx, dist = R.knn(x, 10)
    sigma, rho = R.smooth_knn_dist(dist)
    g = manifold.prune_graph(manifold.fuzzy_union(idx, R.membership(idx, dist, sigma, rho), len(x)), 500)
    from scipy.sparse.csgraph import connected_components
    assert connected_components(g)[0] >= 2
    e = manifold.initial_embedding(g, 5, 0)
    assert np.array_equal(e, manifold.initial_embedding(g, 5, 0))
    # the two large components occupy disjoint intervals along at least one axis
    A, B = e[:60], e[60:110]
    assert ((A.max(0) < B.min(0)) | (B.max(0) < A.min(0))).any()


def test_seed_switch(monkeypatch):
    monkeypatch.delenv("RIBCA_UMAP_SEED", raising=False)
    assert manifold.default_seed() == 0
    monkeypatch.setenv("RIBCA_UMAP_SEED", "17")
    assert manifold.default_seed() == 17


class _Fake:
    """the state _apply_extra_labels / _get_unique_cell_types read and write, without images or a GPU"""

    def __init__(self, labels):
        from multiplexed_image_annotator_amd.annotator import Annotator
        self.__class__ = type("FakeAnnotator", (Annotator,), {})
        gid = {n: i for i, n in enumerate(ops.GLOBAL_NAMES)}
        self.annotations = [list(l) for l in labels]
        self.label_ids = [np.array([gid[n] for n in l], dtype=np.int64) for l in labels]
        self.confidence = [[0.9 if n != "Others" else 0.4 for n in l] for l in labels]
        self._conf_arrays = [np.array(c, dtype=np.float32) for c in self.confidence]
        self.tile_mode = False
        self.extra_names = []


def test_relabelling_names_order_and_confidences():
    labels = [["B cell", "Others", "Others", "CD4 T cell"], ["Others"] * 12]
    a = _Fake(labels)
    pooled = [(0, 1), (0, 2)] + [(1, j) for j in range(12)]
    cluster = np.array([0, 2, -1, 1, 1, 10, 10, 2, 2, 0, -1, 3, 4, 5])
    a._apply_extra_labels(pooled, cluster)
    assert a.annotations[0] == ["B cell", "Additional type 0", "Additional type 2", "CD4 T cell"]
    assert a.annotations[1][0] == "Others" and a.annotations[1][3] == "Additional type 10"
    for i, j in pooled:
        assert a.confidence[i][j] == -1 and a._conf_arrays[i][j] == -1.0
    assert a.confidence[0][0] == 0.9 and a.confidence[0][3] == 0.9
    names = a._label_names()
    for i in range(2):
        assert [names[g] for g in a.label_ids[i]] == a.annotations[i]
    types = a._get_unique_cell_types()
    types = np.append(np.delete(types, np.where(types == "Others")), "Others")
    # np.sort of the names, "Others" last: the reference's order ("Additional type 10" before "Additional type 2")
    assert list(types[:4]) == ["Additional type 0", "Additional type 1", "Additional type 10", "Additional type 2"]
    assert types[-1] == "Others"
    a.cell_types = types
    ints = a._cell_type_ints(0)
    assert [types[t] for t in ints] == a.annotations[0]


def test_few_others_stay_others_with_confidence_minus_one():
    a = _Fake([["Others", "B cell", "Others"]])
    a.min_cells = 5
    a.rank, a.world_size = 0, 1
    a._find_extra_cell_types(min_samples=5)      # 2 pooled cells <= 10: no embedding, no GPU
    assert a.annotations[0] == ["Others", "B cell", "Others"]
    assert a.confidence[0] == [-1, 0.9, -1] and a.extra_names == []


def test_tile_mode_refused_with_min_cells(monkeypatch):
    from multiplexed_image_annotator_amd.annotator import Annotator, tile_mode_env
    monkeypatch.setenv("RIBCA_TILE_MODE", "1")
    with pytest.raises(ValueError, match="RIBCA_TILE_MODE"):
        Annotator("no_markers.txt", "no_images.csv", "cuda", "./", "b", True, False, 20)
    assert tile_mode_env(-1) == "1"
    monkeypatch.delenv("RIBCA_TILE_MODE")
    assert tile_mode_env(20) == "0" and tile_mode_env(-1) is None
    from multiplexed_image_annotator_amd import dist
    assert dist.tile_mode(4, 2, tile_mode_env(20)) is False and dist.tile_mode(4, 2, tile_mode_env(-1)) is True


@pytest.mark.parametrize("src", ["umap.hip", "knn.hip"])
def test_new_kernels_compile_without_spills_or_scratch(src, tmp_path):
    import test_kernel_resources
    test_kernel_resources.test_no_spills_no_scratch(src, tmp_path)


def test_new_entry_points_refuse_bad_arguments_with_a_status():
    from multiplexed_image_annotator_amd import _lib
    lib = _lib.lib()
    calls = (("ribca_knn_dense", lambda: lib.ribca_knn_dense(None, 10, 3, 2, None, None, None)),
             ("ribca_umap_fuzzy_weights", lambda: lib.ribca_umap_fuzzy_weights(None, None, 10, 3, None, None, None, None)),
             ("ribca_umap_optimize", lambda: lib.ribca_umap_optimize(None, 10, 2, None, None, None, None, 1.0, 1.0, 1.0, 1.0, 5.0, 10, 0, None, 0,
                                                                    None)))
    for name, call in calls:
        assert call() != 0 and name.encode() in lib.ribca_last_error()
