"""The host part of manifold.hdbscan (no GPU): the tree code against sklearn's own routines on the same spanning tree, the numpy oracle of
the GPU part (tests/hdbscan_numpy.py) plus that tree code against sklearn.cluster.HDBSCAN, parameter validation, and the argument checks
of the two C entry points."""
import ctypes

import numpy as np
import pytest

import hdbscan_numpy as H


def _sklearn_tree_routines():
    """sklearn's private tree routines; another sklearn without them skips"""
    try:
        from sklearn.cluster._hdbscan._linkage import MST_edge_dtype, make_single_linkage
        from sklearn.cluster._hdbscan._tree import _condense_tree, tree_to_labels
    except ImportError as e:      # pragma: no cover
        pytest.skip(f"this sklearn has no _hdbscan tree routines: {e}")
    return MST_edge_dtype, make_single_linkage, _condense_tree, tree_to_labels


def _blob(seed, n):
    return (np.random.RandomState(seed).randn(n, 5) * 0.3).astype(np.float32)


TREE_CASES = {
    "planted-10": lambda: (H.planted(0, 1500)[0], 10),
    "planted-25": lambda: (H.planted(1, 1500)[0], 25),
    "planted-5": lambda: (H.planted(4, 2000)[0], 5),
    "planted-50": lambda: (H.planted(2, 2000)[0], 50),
    "lattice-duplicates": lambda: (H.lattice(7, 900), 8),
    "lattice-duplicates-2": lambda: (H.lattice(8, 600, side=2), 5),
    "all-noise": lambda: (np.random.RandomState(3).uniform(0, 10, size=(200, 5)).astype(np.float32), 150),
    "root-only": lambda: (_blob(5, 300), 120),
}


@pytest.mark.parametrize("case", sorted(TREE_CASES))
def test_tree_code_matches_sklearn_routines_on_the_same_tree(case):
    from multiplexed_image_annotator_amd import manifold
    MST_edge_dtype, make_single_linkage, _condense_tree, tree_to_labels = _sklearn_tree_routines()
    x, m = TREE_CASES[case]()
    u, v, w, _ = H.mst(x, m)
    rng = np.random.RandomState(1)
    perm = rng.permutation(len(u))      # the library returns the edges in no particular order
    su, sv, sw = manifold.sort_mst_edges(u[perm], v[perm], w[perm])
    assert np.array_equal(su, u) and np.array_equal(sv, v) and np.array_equal(sw, w)
    edges = np.zeros(len(su), dtype=MST_edge_dtype)
    edges["current_node"], edges["next_node"], edges["distance"] = su, sv, sw
    ref_tree = make_single_linkage(edges)
    left, right, value, size = manifold.single_linkage(su, sv, sw)
    assert np.array_equal(left, ref_tree["left_node"]) and np.array_equal(right, ref_tree["right_node"])
    assert np.array_equal(value, ref_tree["value"]) and np.array_equal(size, ref_tree["cluster_size"])
    ref_cond = _condense_tree(ref_tree, m)
    parent, child, lam, csize = manifold.condense_tree(left, right, value, size, m)
    assert np.array_equal(parent, ref_cond["parent"]) and np.array_equal(child, ref_cond["child"])
    assert np.array_equal(lam, ref_cond["value"]) and np.array_equal(csize, ref_cond["cluster_size"])
    ref_labels = np.asarray(tree_to_labels(ref_tree, m)[0])
    labels = manifold.labels_from_mst(u[perm], v[perm], w[perm], m)
    assert labels.dtype == np.int64 and np.array_equal(labels, ref_labels)
    if case in ("all-noise", "root-only"):
        assert (labels == -1).all()
    elif case.startswith("planted"):
        assert labels.max() + 1 >= 6


@pytest.mark.parametrize("seed,n,m", H.PLANTED)
def test_oracle_and_tree_code_match_sklearn_hdbscan(seed, n, m):
    from sklearn.cluster import HDBSCAN
    from multiplexed_image_annotator_amd import manifold
    x, _ = H.planted(seed, n)
    u, v, w, _ = H.mst(x, m)
    labels = manifold.labels_from_mst(u, v, w, m)
    ref = HDBSCAN(min_cluster_size=m).fit(x).labels_
    diff = H.best_renaming_mismatches(ref, labels)
    print(f"[hdbscan oracle vs sklearn] seed {seed} n {n} m {m}: {labels.max() + 1} / {ref.max() + 1} clusters, {diff} points differ")
    assert labels.max() == ref.max()
    assert diff <= H.CAP * n


def test_parameter_validation_raises_what_sklearn_raises():
    """min_cluster_size < 2 and min_samples > n raise ValueError here as in sklearn.  Non-finite input is refused with a ValueError as
    well: sklearn 1.7 does not raise for it (it labels such rows -3 / -2 as outliers); this build requires finite rows, which is what the
    embedding delivers.  All of it happens before any GPU call."""
    from sklearn.cluster import HDBSCAN
    from multiplexed_image_annotator_amd import manifold
    x = H.planted(0, 60)[0]
    for kwargs in ({"min_cluster_size": 1}, {"min_cluster_size": 5, "min_samples": 61}, {"min_cluster_size": 100}):
        with pytest.raises(ValueError):
            HDBSCAN(**kwargs).fit(x)
        with pytest.raises(ValueError):
            manifold.hdbscan(x, **kwargs)
    for bad_value in (np.nan, np.inf):
        bad = x.copy()
        bad[7, 2] = bad_value
        with pytest.raises(ValueError, match="NaN or infinity"):
            manifold.hdbscan(bad, 5)
    assert manifold.validate_hdbscan_params(7) == 7 and manifold.validate_hdbscan_params(7, 3, 10) == 3


def test_backend_switch_is_read_per_call(monkeypatch):
    from multiplexed_image_annotator_amd import manifold
    monkeypatch.delenv("RIBCA_HDBSCAN", raising=False)
    assert manifold.hdbscan_backend() == "gpu"
    monkeypatch.setenv("RIBCA_HDBSCAN", "sklearn")
    assert manifold.hdbscan_backend() == "sklearn"
    monkeypatch.setenv("RIBCA_HDBSCAN", "cpu")
    with pytest.raises(ValueError, match="RIBCA_HDBSCAN"):
        manifold.hdbscan_backend()


def test_hdbscan_kernels_compile_without_spills_or_scratch(tmp_path):
    import test_kernel_resources
    test_kernel_resources.test_no_spills_no_scratch("hdbscan.hip", tmp_path)


def test_hdbscan_entry_points_refuse_bad_arguments_with_a_status():
    """the argument checks run before any HIP call: no launch, no dereference (the buffers here are host memory the library never touches)"""
    from multiplexed_image_annotator_amd import _lib, ops
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def refused(status, name, word):
        msg = lib.ribca_last_error()
        assert status != 0 and name.encode() in msg and word.encode() in msg, msg

    refused(lib.ribca_core_distance(None, 10, 3, 2, None, None, 0, None), "ribca_core_distance", "NULL")
    refused(lib.ribca_core_distance(p, 1, 3, 1, p, p, 256, None), "ribca_core_distance", "n >= 2")
    refused(lib.ribca_core_distance(p, 10, 3, 0, p, p, 256, None), "ribca_core_distance", "min_samples")
    refused(lib.ribca_core_distance(p, 10, 3, 11, p, p, 256, None), "ribca_core_distance", "min_samples")
    refused(lib.ribca_core_distance(p, 10, 65, 2, p, p, 256, None), "ribca_core_distance", "dim")
    assert lib.ribca_core_distance_ws_bytes(10, 3, 2) == 256 and lib.ribca_core_distance_ws_bytes(1025, 15, 65) == 256
    assert lib.ribca_core_distance_ws_bytes(1, 3, 1) == 0 and lib.ribca_core_distance_ws_bytes(10, 65, 2) == 0 and lib.ribca_core_distance_ws_bytes(10, 3, 11) == 0
    refused(lib.ribca_core_distance(p, 10, 3, 2, p, p, lib.ribca_core_distance_ws_bytes(10, 3, 2) - 1, None), "ribca_core_distance", "workspace")
    refused(lib.ribca_mreach_mst(None, 10, 3, None, None, None, None, None, 0, None), "ribca_mreach_mst", "NULL")
    refused(lib.ribca_mreach_mst(p, 1, 3, p, p, p, p, p, 4096, None), "ribca_mreach_mst", "n >= 2")
    refused(lib.ribca_mreach_mst(p, 10, 65, p, p, p, p, p, 4096, None), "ribca_mreach_mst", "dim")
    # 256 + al(8 n) + 9 al(4 n)
    assert lib.ribca_mreach_mst_ws_bytes(10) == 256 + 256 + 9 * 256 and lib.ribca_mreach_mst_ws_bytes(1025) == 256 + 8448 + 9 * 4352
    assert lib.ribca_mreach_mst_ws_bytes(1) == 0 and ops.mreach_mst_ws_bytes(10) == lib.ribca_mreach_mst_ws_bytes(10)
    refused(lib.ribca_mreach_mst(p, 10, 3, p, p, p, p, p, lib.ribca_mreach_mst_ws_bytes(10) - 1, None), "ribca_mreach_mst", "workspace")
