"""GPU HDBSCAN (csrc/hdbscan.hip, manifold.hdbscan, Annotator(min_cells > 0)): the core distances and the mutual-reachability spanning tree
bit for bit / edge for edge against the numpy oracle (tests/hdbscan_numpy.py), determinism, the labels against the oracle path and against
sklearn.cluster.HDBSCAN, statuses for bad requests, and the Annotator's backend switch."""
import os

import numpy as np
import pytest
import torch

import hdbscan_numpy as H
from batch_harness import planted_case, run_annotator, threshold

pytestmark = pytest.mark.gpu


def _dev():
    from multiplexed_image_annotator_amd import _lib
    return _lib.require_gpu()


def _with_duplicates(seed, n, dim):
    """n rows (n is no multiple of any tile size), the last 37 of them copies of earlier rows"""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, dim).astype(np.float32) * 3
    x[n - 37:] = x[rng.randint(n - 37, size=37)]
    return x


@pytest.mark.parametrize("dim", [2, 5, 15, 64])
def test_core_distance_bit_equal_to_numpy_oracle(dim):
    from multiplexed_image_annotator_amd import ops
    n = 1237
    x = _with_duplicates(dim, n, dim)
    d2 = H.dist2(x)
    xd = torch.from_numpy(x).to(_dev())
    for ms in (1, 2, 5, 16, 17, 64, 65, 200, n):
        got = ops.core_distance(xd, ms).cpu().numpy()
        ref = H.core2(d2, ms)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (dim, ms, np.abs(got - ref).max())


def _mst_cases():
    two = H.two_groups(3, 1100)
    return {"n=2": (np.array([[0, 0, 0], [3, 4, 0]], dtype=np.float32), 2), "n=3-duplicates": (np.zeros((3, 2), dtype=np.float32), 2),
            "planted": (H.planted(2, 3000)[0], 50), "planted-small-k": (H.planted(4, 2000)[0], 5), "planted-k-100": (H.planted(5, 1500)[0], 100),
            "lattice": (H.lattice(7, 900), 8), "two-groups": (two, 10), "dim-15": (_with_duplicates(1, 777, 15), 12),
            "dim-64": (_with_duplicates(2, 515, 64), 6)}


def _check_spanning_tree(n, u, v):
    assert len(u) == n - 1 and (u < v).all() and u.min() >= 0 and v.max() < n
    parent = list(range(n))
    for a, b in zip(u.tolist(), v.tolist()):
        while parent[a] != a:
            a = parent[a]
        while parent[b] != b:
            b = parent[b]
        assert a != b, "cycle"
        parent[b] = a
    assert sum(1 for i, p in enumerate(parent) if i == p) == 1


@pytest.mark.parametrize("case", sorted(_mst_cases()))
def test_mreach_mst_is_the_oracles_kruskal_tree(case):
    from multiplexed_image_annotator_amd import manifold, ops
    x, ms = _mst_cases()[case]
    n = len(x)
    ru, rv, rw, rc = H.mst(x, ms)
    xd = torch.from_numpy(x).to(_dev())
    core2 = ops.core_distance(xd, ms)
    assert np.array_equal(core2.cpu().numpy().view(np.uint32), rc.view(np.uint32))
    u, v, w = (t.cpu().numpy() for t in ops.mreach_mst(xd, core2))
    _check_spanning_tree(n, u, v)
    su, sv, sw = manifold.sort_mst_edges(u, v, w)
    order = np.lexsort((rv, ru))
    mine = np.lexsort((v, u))
    assert np.array_equal(u[mine], ru[order]) and np.array_equal(v[mine], rv[order]), "edge set differs from the oracle's tree"
    assert np.array_equal(w[mine].view(np.uint32), rw[order].view(np.uint32)), "weights are not bit-equal"
    assert np.array_equal(sw, rw)      # sqrt is monotone: sorted by weight both ways
    if case == "two-groups":
        assert (w > 500).sum() == 1


def test_two_calls_and_a_second_stream_give_identical_bytes():
    from multiplexed_image_annotator_amd import ops
    x = H.planted(6, 2500)[0]
    xd = torch.from_numpy(x).to(_dev())

    def run(ms):
        c = ops.core_distance(xd, ms)
        return [t.cpu().numpy().tobytes() for t in (c,) + ops.mreach_mst(xd, c)]

    for ms in (15, 100):
        a = run(ms)
        b = run(ms)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = run(ms)
        side.synchronize()
        assert a == b and a == c


@pytest.mark.parametrize("seed,n,m", H.PLANTED)
def test_hdbscan_equals_the_oracle_path_label_for_label(seed, n, m):
    from multiplexed_image_annotator_amd import manifold
    x, _ = H.planted(seed, n)
    u, v, w, _ = H.mst(x, m)
    ref = manifold.labels_from_mst(u, v, w, m)
    t = {}
    got = manifold.hdbscan(x, m, timings=t)
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert set(t) == {"core", "mst", "tree"}
    # min_samples of its own
    u, v, w, _ = H.mst(x, 7)
    assert np.array_equal(manifold.hdbscan(x, m, min_samples=7), manifold.labels_from_mst(u, v, w, m))


def test_hdbscan_20k_points_against_sklearn():
    from sklearn.cluster import HDBSCAN
    from multiplexed_image_annotator_amd import manifold
    n, m = 20011, 50
    x, truth = H.planted(11, n)
    t = {}
    got = manifold.hdbscan(x, m, timings=t)
    ref = HDBSCAN(min_cluster_size=m).fit(x).labels_
    diff = H.best_renaming_mismatches(ref, got)
    print(f"[hdbscan 20k vs sklearn] {got.max() + 1} / {ref.max() + 1} clusters, {diff} of {n} points differ; ms {t}")
    assert got.max() == ref.max()
    assert diff <= H.CAP * n


def test_bad_requests_return_a_status_not_an_abort():
    from multiplexed_image_annotator_amd import _lib, ops
    dev = _dev()
    x = torch.from_numpy(H.planted(0, 300)[0]).to(dev)
    with pytest.raises(_lib.RibcaError, match="ribca_core_distance.*min_samples"):
        ops.core_distance(x, 0)
    with pytest.raises(_lib.RibcaError, match="ribca_core_distance.*min_samples"):
        ops.core_distance(x, 301)
    with pytest.raises(_lib.RibcaError, match="ribca_core_distance.*dim"):
        ops.core_distance(torch.zeros((300, 65), device=dev), 5)
    with pytest.raises(_lib.RibcaError, match="ribca_core_distance.*n >= 2"):
        ops.core_distance(x[:1], 1)
    core2 = ops.core_distance(x, 5)
    with pytest.raises(_lib.RibcaError, match="ribca_mreach_mst.*dim"):
        ops.mreach_mst(torch.zeros((300, 65), device=dev), core2)
    short = torch.empty(ops.mreach_mst_ws_bytes(300) - 1, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.RibcaError, match="ribca_mreach_mst.*workspace"):
        ops.mreach_mst(x, core2, ws=short)
    # a non-finite core distance is a status too (no launch faults on it: every comparison with a NaN is false)
    bad = core2.clone()
    bad[17] = float("nan")
    with pytest.raises(_lib.RibcaError, match="ribca_mreach_mst.*finite"):
        ops.mreach_mst(x, bad)
    xn = x.clone()
    xn[5, 1] = float("nan")
    with pytest.raises(_lib.RibcaError, match="ribca_core_distance.*finite"):
        ops.core_distance(xn, 5)
    with pytest.raises(_lib.RibcaError, match="ribca_core_distance.*finite"):
        ops.core_distance(xn, 100)
    # and the library still works afterwards
    u, v, w = ops.mreach_mst(x, core2)
    _check_spanning_tree(300, u.cpu().numpy(), v.cpu().numpy())


def test_annotator_backend_switch(tmp_path, monkeypatch):
    root = str(tmp_path / "case")
    planted_case(root)
    thr = threshold(root, str(tmp_path))
    monkeypatch.delenv("RIBCA_HDBSCAN", raising=False)
    a = run_annotator(root, str(tmp_path / "gpu"), 20, thr)
    b = run_annotator(root, str(tmp_path / "gpu2"), 20, thr)
    monkeypatch.setenv("RIBCA_HDBSCAN", "sklearn")
    s = run_annotator(root, str(tmp_path / "sk"), 20, thr)
    assert a.extra_stats["backend"] == "gpu" and s.extra_stats["backend"] == "sklearn"
    assert {"core_ms", "mst_ms", "tree_ms", "cluster_ms"} <= set(a.extra_stats)
    assert a.extra_stats["clusters"] == s.extra_stats["clusters"] >= 2

    def labels(run):
        return np.array([int(n.split()[-1]) if n.startswith("Additional type ") else -1 for n in run.annotations[0] if
                         n == "Others" or n.startswith("Additional type ")])
    la, ls = labels(a), labels(s)
    others_a = [j for j, n in enumerate(a.annotations[0]) if n == "Others" or n.startswith("Additional type ")]
    others_s = [j for j, n in enumerate(s.annotations[0]) if n == "Others" or n.startswith("Additional type ")]
    assert others_a == others_s
    diff = H.best_renaming_mismatches(ls, la)
    print(f"[annotator backends] {len(la)} pooled, {a.extra_stats['clusters']} clusters, {diff} points differ; gpu {a.extra_stats}; sklearn {s.extra_stats}")
    assert diff <= H.CAP * len(la)
    csv_a = open(os.path.join(str(tmp_path / "gpu"), "results", "x_annotation_0.csv")).read()
    csv_b = open(os.path.join(str(tmp_path / "gpu2"), "results", "x_annotation_0.csv")).read()
    assert "Additional type 0" in csv_a and csv_a == csv_b
