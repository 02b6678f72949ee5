"""The tissue-region restatement without a GPU: the numpy oracle (tests/regions_numpy.py: integer Gram, PCA rule, projection loop, k-means++
and Lloyd in the summation order of DESIGN.md section 11) against scikit-learn on planted inputs, the counter-based draws, the empty-cluster
rule, and the host-side switches / parameter checks of multiplexed_image_annotator_amd.regions."""
import numpy as np
import pytest

import regions_numpy as R

#: (n, cell types, planted bands, k): a jittered point field cut into bands, each with its own Dirichlet type mix; counts from a 201-NN query
PLANTED = [(3000, 6, 3, 3), (5000, 13, 5, 5), (4000, 9, 4, 7), (20000, 13, 6, 6)]

_cache = {}


def planted_case(n, t, bands, seed=None):
    key = (n, t, bands, seed)
    if key not in _cache:
        counts, band = R.planted_counts(n, t, bands, 1000 + n + t if seed is None else seed)
        c2 = counts.reshape(n, -1)
        size_col = R.size_columns(R.SIZES, t)
        colsum, g = R.gram(c2)
        mean, comps, lam, d = R.pca_from_gram(g, colsum, n, size_col)
        _cache[key] = dict(counts=counts, band=band, c2=c2, size_col=size_col, mean=mean, comps=comps, lam=lam, d=d,
                           y=R.project(c2, size_col, mean, comps))
    return _cache[key]


@pytest.mark.parametrize("n,t,bands,k", PLANTED)
def test_oracle_pca_matches_sklearn(n, t, bands, k):
    from sklearn.decomposition import PCA
    case = planted_case(n, t, bands)
    table = case["c2"].astype(np.float64) / case["size_col"]
    pca = PCA(n_components=0.99)
    ys = pca.fit_transform(table)
    err = np.abs(case["y"] - ys).max() if ys.shape == case["y"].shape else np.inf
    print(f"n={n} T={t}: d oracle {case['d']} sklearn {pca.n_components_}, max |dY| {err:.3e}")
    assert case["d"] == pca.n_components_
    assert err <= 1e-9


@pytest.mark.parametrize("n,t,bands,k", PLANTED)
def test_oracle_lloyd_matches_sklearn_from_the_same_centres(n, t, bands, k):
    from sklearn.cluster import KMeans
    y = planted_case(n, t, bands)["y"]
    labels, centres, iters, inertia, picks = R.kmeans(y, k, seed=0)
    km = KMeans(n_clusters=k, init=y[picks], n_init=1).fit(y)
    mism = int((km.labels_ != labels).sum())
    rel = abs(km.inertia_ - inertia) / km.inertia_
    print(f"n={n} k={k}: iterations oracle {iters} sklearn {km.n_iter_}, label mismatches {mism}, inertia rel. diff {rel:.3e}")
    assert len(set(picks)) == k
    assert mism == 0
    assert km.n_iter_ == iters
    assert rel <= 1e-12


def test_draws_are_counter_based_and_seeded():
    from multiplexed_image_annotator_amd import regions
    u = [R.draw(0, s, t) for s in range(4) for t in range(3)]
    assert all(0.0 <= v < 1.0 for v in u) and len(set(u)) == len(u)
    assert u == [R.draw(0, s, t) for s in range(4) for t in range(3)]
    assert u == [regions.draw(0, s, t) for s in range(4) for t in range(3)]      # the package's host draw is the oracle's
    assert R.draw(1, 0, 0) != R.draw(0, 0, 0)
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF      # the published first output of splitmix64 from state 0
    y = planted_case(3000, 6, 3)["y"]
    p0, _ = R.kmeans_plusplus(y, 5, 0)
    assert p0 == R.kmeans_plusplus(y, 5, 0)[0] and len(p0) == 5
    assert p0 != R.kmeans_plusplus(y, 5, 1)[0]


def test_empty_cluster_rule_on_fewer_distinct_rows_than_clusters():
    """3 distinct rows, k = 5: k-means++ has to pick duplicates, their clusters come out empty, and scikit-learn's rule hands each empty
    cluster the row farthest from its centre (ties to the lowest row index); the run ends, every label is valid, equal rows share one"""
    base = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 9.0]])
    y = np.repeat(base, 40, axis=0)[np.random.RandomState(0).permutation(120)]
    trace = []
    labels, centres, iters, inertia, picks = R.kmeans(y, 5, seed=0, trace=trace)
    assert iters < 300 and labels.min() >= 0 and labels.max() < 5 and inertia == 0.0
    for row in base:
        assert len(set(labels[(y == row).all(axis=1)].tolist())) == 1
    # the rule itself
    lab = np.array([0, 0, 0, 1, 1, 1], dtype=np.int64)
    pts = np.array([[0.0], [1.0], [5.0], [10.0], [11.0], [15.0]])
    sums, counts = R.centre_sums(pts, lab, 3)
    assert counts.tolist() == [3, 3, 0]
    far = R.relocate(pts, lab, np.array([4.0, 1.0, 9.0, 4.0, 1.0, 9.0]), sums, counts)
    assert far.tolist() == [2] and counts.tolist() == [2, 3, 1] and sums[:, 0].tolist() == [1.0, 36.0, 5.0]


def test_summation_order_is_the_documented_one():
    """rows of a 1024-chunk in ascending order, then the chunks in ascending order -- not numpy's pairwise sum"""
    rng = np.random.RandomState(3)
    v = rng.uniform(size=2500) * 10.0 ** rng.randint(-8, 8, size=2500)
    parts = []
    for r in range(0, 2500, 1024):
        s = 0.0
        for x in v[r:r + 1024].tolist():
            s = s + x
        parts.append(s)
    total = 0.0
    for p in parts:
        total = total + p
    assert R.chunked_sum(v) == total
    y = np.stack([v, -v], axis=1)
    sums, counts = R.centre_sums(y, np.zeros(2500, dtype=np.int64), 1)
    assert sums[0, 0] == total and sums[0, 1] == -total and counts[0] == 2500


def test_backend_switch_and_parameter_validation(monkeypatch):
    from multiplexed_image_annotator_amd import regions
    monkeypatch.delenv("RIBCA_REGIONS", raising=False)
    monkeypatch.delenv("RIBCA_REGION_SEED", raising=False)
    assert regions.region_backend() == "gpu" and regions.default_seed() == 0
    monkeypatch.setenv("RIBCA_REGIONS", "sklearn")
    monkeypatch.setenv("RIBCA_REGION_SEED", "7")
    assert regions.region_backend() == "sklearn" and regions.default_seed() == 7
    monkeypatch.setenv("RIBCA_REGIONS", "cpu")
    with pytest.raises(ValueError, match="RIBCA_REGIONS"):
        regions.region_backend()
    for bad in (0, -1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="n_clusters"):
            regions.validate_n_clusters(bad)
    with pytest.raises(ValueError, match="n_samples=4 should be >= n_clusters=5"):
        regions.validate_n_clusters(5, 4)
    assert regions.validate_n_clusters(np.int64(3), 3) == 3


def test_package_pca_rule_is_the_oracles():
    from multiplexed_image_annotator_amd import regions
    case = planted_case(3000, 6, 3)
    colsum, g = R.gram(case["c2"])
    mean, comps, lam, d = regions.pca_from_gram(g, colsum, 3000, case["size_col"])
    assert d == case["d"] and np.array_equal(mean, case["mean"]) and np.array_equal(comps, case["comps"]) and np.array_equal(lam, case["lam"])


def test_entry_points_refuse_out_of_range_requests_with_a_status():
    """argument checks run before any HIP call: no GPU needed, no abort"""
    from multiplexed_image_annotator_amd import _lib
    lib = _lib.lib()

    def refused(status, name):
        assert status != 0
        msg = lib.ribca_last_error()
        assert msg and name.encode() in msg, (name, msg)

    refused(lib.ribca_region_gram(None, 10, 8, None, None, None, 0, None), "ribca_region_gram")
    refused(lib.ribca_region_gram(1, 10, 2033, 1, 1, 1, 256, None), "ribca_region_gram")
    refused(lib.ribca_region_gram(1, 0, 8, 1, 1, 1, 256, None), "ribca_region_gram")
    refused(lib.ribca_region_project(1, 10, 8, 1, 1, 1, 9, 1, None), "ribca_region_project")
    refused(lib.ribca_kmeans_trials(1, 10, 4, 1, 9, None, 1, 1, 1, 1 << 20, None), "ribca_kmeans_trials")
    refused(lib.ribca_kmeans_assign(1, 10, 4, 1, 257, 1, None, 1, None), "ribca_kmeans_assign")
    refused(lib.ribca_kmeans_assign(1, 10, 2033, 1, 3, 1, None, 1, None), "ribca_kmeans_assign")
    refused(lib.ribca_kmeans_assign(1, 4, 4, 1, 5, 1, None, 1, None), "ribca_kmeans_assign")      # n < k
    refused(lib.ribca_kmeans_update(1, 10, 4, 1, 3, 1, 1, 1, 1, None, 1, 1, 0, None), "ribca_kmeans_update")      # workspace too small
    refused(lib.ribca_kmeans_relocate(1, 10, 4, 3, 1, 1, 1, 3, 1, 1, None), "ribca_kmeans_relocate")
    refused(lib.ribca_kmeans_finalize(None, None, 3, 4, None, None, None, None, None), "ribca_kmeans_finalize")
    assert lib.ribca_kmeans_update_ws_bytes(10, 4, 300) == 0 and lib.ribca_kmeans_update_ws_bytes(100000, 43, 5) > 0
    # the sizes the library asks for, pinned: a layout or a chunk that moves shows here, without a GPU
    assert lib.ribca_kmeans_update_ws_bytes(1025, 5, 7) == 768 + 256 and lib.ribca_kmeans_update_ws_bytes(10, 4, 3) == 256 + 256      # al(8 c k d) + al(4 c k)
    assert lib.ribca_region_gram_ws_bytes(10, 8) == 256 and lib.ribca_region_gram_ws_bytes(10, 2033) == 0 and lib.ribca_region_gram_ws_bytes(0, 8) == 0
    assert lib.ribca_kmeans_trials_ws_bytes(1025, 3) == 48 and lib.ribca_kmeans_trials_ws_bytes(1024, 8) == 64      # 8 n_cand ceil(n / 1024), not rounded
    assert lib.ribca_kmeans_trials_ws_bytes(10, 9) == 0 and lib.ribca_kmeans_trials_ws_bytes(0, 3) == 0


def test_one_byte_less_than_the_query_is_refused():
    """every entry point's own check is its query: query - 1 bytes come back as "workspace too small" before any launch"""
    from multiplexed_image_annotator_amd import _lib
    lib = _lib.lib()

    def short(status, name):
        msg = lib.ribca_last_error()
        assert status != 0 and name.encode() in msg and b"workspace" in msg, (name, msg)

    short(lib.ribca_region_gram(1, 10, 8, 1, 1, 1, lib.ribca_region_gram_ws_bytes(10, 8) - 1, None), "ribca_region_gram")
    short(lib.ribca_kmeans_trials(1, 1025, 4, 1, 3, None, 1, 1, 1, lib.ribca_kmeans_trials_ws_bytes(1025, 3) - 1, None), "ribca_kmeans_trials")
    short(lib.ribca_kmeans_update(1, 1025, 5, 1, 7, 1, 1, 1, 1, None, 1, 1, lib.ribca_kmeans_update_ws_bytes(1025, 5, 7) - 1, None), "ribca_kmeans_update")
