"""Host side of the neighbourhood enrichment (multiplexed_image_annotator_amd/enrichment.py, tests/enrichment_numpy.py): the keyed bijection
sigma_p is a permutation and depends on every part of its key, its null of the co-occurrence counts has the closed-form mean, a planted pattern
scores positive, zero variance is NaN, the z-scores are exact beyond int64, and the argument checks of the new entry points (they run before
any HIP call: no GPU needed)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import enrichment_numpy as EN
from multiplexed_image_annotator_amd import _lib, enrichment, ops

SIZES = [1, 2, 3, 4, 5, 7, 16, 17, 100, 257, 1000, 4097, 100000]


@pytest.mark.parametrize("n", SIZES)
def test_sigma_is_a_permutation(n):
    longest = 0
    for seed, image, p in ((0, 0, 0), (0, 0, 1), (7, 3, 999), (2 ** 64 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        s, passes = EN.sigma(n, seed, image, p, want_passes=True)
        assert np.array_equal(np.sort(s), np.arange(n)), (n, seed, image, p)
        longest = max(longest, passes)
        assert passes <= 4 ** EN.half_bits(n) - n + 1      # the walk stays on the cycle of its start
        for i in sorted({0, n // 2, n - 1}):      # the array form is the definition on Python integers
            assert EN.sigma_scalar(n, seed, image, p, i) == s[i]
    assert 4 ** EN.half_bits(n) >= n and (n <= 2 or 4 ** EN.half_bits(n) < 4 * n)
    print(f"[sigma n = {n}] longest walk {longest} passes")


def test_every_part_of_the_key_changes_the_permutation():
    n = 1000
    base = EN.sigma(n, 0, 0, 0)
    for other in (EN.sigma(n, 0, 0, 1), EN.sigma(n, 1, 0, 0), EN.sigma(n, 0, 1, 0), EN.sigma(n, 0, 1, 1)):
        assert (other != base).mean() > 0.9
    assert np.array_equal(base, EN.sigma(n, 0, 0, 0)) and np.array_equal(base, EN.sigma(n, 2 ** 64, 0, 0))      # the seed is taken modulo 2^64
    assert (base != np.arange(n)).mean() > 0.9


def _graph(n, m, seed):
    rng = np.random.RandomState(seed)
    x, y = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    return x, y, EN.knn_list(x, y, m + 1)


def test_null_mean_against_the_closed_form():
    """n 200, m 7, T 4, P 4000, seed 0: with M = n m pairs, E[count_ab] = M n_a n_b / (n (n - 1)) for a != b and M n_a (n_a - 1) / (n (n - 1)) for
    a == b under a uniform permutation; every entry of the sample mean within 4.5 standard errors of it."""
    n, m, t, p = 200, 7, 4, 4000
    _, _, idx = _graph(n, m, 1)
    labels = np.random.RandomState(2).randint(0, t, n)
    counts = EN.perm_counts(idx, labels, t, 0, 0, 0, p)
    assert (counts.sum(axis=(1, 2)) == n * m).all()
    na = np.bincount(labels, minlength=t).astype(np.float64)
    expect = n * m * np.outer(na, na) / (n * (n - 1.0))
    expect[np.diag_indices(t)] = n * m * na * (na - 1.0) / (n * (n - 1.0))
    mean, std = counts.mean(axis=0), counts.std(axis=0)
    dev = np.abs(mean - expect) / (std / np.sqrt(p))
    print("[null mean] deviations in standard errors:\n", np.round(dev, 2))
    assert (dev <= 4.5).all(), dev.max()
    stats = enrichment.z_scores(np.zeros((t, t), dtype=np.int64), counts)
    assert np.allclose(stats["mean"], mean, rtol=1e-14, atol=0) and np.allclose(stats["std"], std, rtol=1e-12, atol=0)


def test_a_planted_pattern_scores_positive_on_the_diagonal():
    n, m, t, p = 400, 7, 4, 200
    x, _, idx = _graph(n, m, 3)
    labels = np.minimum((x * t).astype(np.int64), t - 1)      # four vertical bands: neighbours mostly share the band
    observed = EN.pair_counts(idx, labels, t)
    stats = enrichment.z_scores(observed, EN.perm_counts(idx, labels, t, 0, 0, 0, p))
    assert (np.diag(stats["z"]) > 5.0).all(), np.diag(stats["z"])
    assert (np.diag(stats["n_ge"]) == 0).all() and (np.diag(stats["n_le"]) == p).all()
    assert stats["z"][0, t - 1] < 0.0      # the two outer bands never touch
    want = EN.z_scores(observed, EN.perm_counts(idx, labels, t, 0, 0, 0, p))
    for k in ("mean", "std", "z", "n_ge", "n_le"):
        assert stats[k].tobytes() == want[k].tobytes(), k


def test_zero_variance_is_nan_and_the_csv_says_so():
    n, m = 30, 3
    _, _, idx = _graph(n, m, 4)
    labels = np.zeros(n, dtype=np.int64)
    perm = EN.perm_counts(idx, labels, 2, 0, 0, 0, 5)      # one type present: every permutation counts n m pairs of (0, 0)
    observed = EN.pair_counts(idx, labels, 2)
    stats = enrichment.z_scores(observed, perm)
    assert np.isnan(stats["z"]).all() and not stats["std"].any() and stats["mean"][0, 0] == n * m
    assert (stats["n_ge"] == 5).all() and (stats["n_le"] == 5).all()
    assert enrichment.colour_limit(stats["z"]) == 1.0
    text = enrichment.matrix_csv(["a", "b"], stats["z"])
    assert text == "cell_type,a,b,\na,nan,nan,\nb,nan,nan,\n"
    long = enrichment.table_csv(["a", "b"], observed, stats).split("\n")
    assert long[0] == "cell_type,neighbour,observed,null_mean,null_std,z,n_ge,n_le" and long[1] == f"a,a,{n * m},{n * m},0,nan,5,5" and len(long) == 6
    # a mixed table: the limit is the largest finite |z|
    z = np.array([[np.nan, -2.5], [1.0, np.inf]])
    assert enrichment.colour_limit(z) == 2.5
    assert enrichment.matrix_csv(["a", "b"], z) == "cell_type,a,b,\na,nan,-2.500,\nb,1.000,inf,\n"


def test_z_scores_are_exact_where_int64_overflows():
    big = 2 ** 33
    perm = np.array([big, big + 2, big + 4], dtype=np.int64).reshape(3, 1, 1)
    assert 3 * int((perm.astype(object) ** 2).sum()) > 2 ** 63      # P S2 does not fit int64
    stats = enrichment.z_scores(np.array([[big + 5]], dtype=np.int64), perm)
    # mean = big + 2, variance = 8 / 3 exactly: std = sqrt(3 * S2 - S1^2) / 3 = sqrt(24) / 3
    assert stats["mean"][0, 0] == float(big + 2) and stats["std"][0, 0] == np.sqrt(24.0) / 3.0
    assert stats["z"][0, 0] == 3.0 / (np.sqrt(24.0) / 3.0)
    assert Fraction(3 * sum(int(v) ** 2 for v in perm.ravel()) - sum(int(v) for v in perm.ravel()) ** 2) == 24
    assert stats["n_ge"][0, 0] == 0 and stats["n_le"][0, 0] == 3
    want = EN.z_scores(np.array([[big + 5]]), perm)
    assert all(stats[k].tobytes() == want[k].tobytes() for k in want)
    # uint64 counts, as the device tensor holds them
    assert enrichment.z_scores(np.array([[5]], dtype=np.uint64), np.array([[[2 ** 63 + 1]], [[2 ** 63 + 3]]], dtype=np.uint64))["std"][0, 0] == 1.0
    with pytest.raises(ValueError):
        enrichment.z_scores(np.zeros((2, 2), dtype=np.int64), np.zeros((0, 2, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        enrichment.z_scores(np.zeros((2, 2)), np.zeros((3, 2, 2)))


def test_the_seed_is_read_at_every_call(monkeypatch):
    monkeypatch.delenv("RIBCA_ENRICH_SEED", raising=False)
    assert enrichment.default_seed() == 0
    monkeypatch.setenv("RIBCA_ENRICH_SEED", "41")
    assert enrichment.default_seed() == 41
    monkeypatch.setenv("RIBCA_ENRICH_SEED", "")
    assert enrichment.default_seed() == 0


def test_table_raster_oracle_rules():
    lut = np.arange(768, dtype=np.uint8).reshape(256, 3)
    v = np.array([[-1.0, 0.0, 0.5], [1.0, 2.0, np.nan]])
    img = EN.table_raster(v, lut, 1, 0, 0.0, 1.0)
    assert (img[0, 0] == lut[0]).all() and (img[0, 1] == lut[0]).all() and (img[0, 2] == lut[128]).all()
    assert (img[1, 0] == lut[255]).all() and (img[1, 1] == lut[255]).all() and (img[1, 2] == 192).all()
    flat = EN.table_raster(v, lut, 1, 0, 0.5, 0.5)
    assert (flat[0] == lut[128]).all() and (flat[1, 2] == 192).all()
    assert (EN.table_raster(v, lut, 4, 1, 0.0, 1.0)[0] == 255).all()


def test_labels_out_of_range_raise_before_any_launch():
    idx = torch.zeros((4, 2), dtype=torch.int32)
    for bad in ([0, 1, 2, 3], [0, -1, 1, 1]):
        with pytest.raises(ValueError, match=r"labels must lie in \[0, 3\)"):
            ops.nhood_perm_counts(idx, np.array(bad), 3, 0, 0, 0, 1)
    with pytest.raises(ValueError):
        ops.nhood_perm_counts(idx.to(torch.int64), np.zeros(4), 3, 0, 0, 0, 1)
    with pytest.raises(ValueError):
        ops.nhood_perm_counts(idx, np.zeros(5), 3, 0, 0, 0, 1)


def test_new_entry_points_refuse_bad_arguments_with_a_status():
    lib = _lib.lib()
    p = ctypes.c_void_p(4096)      # never dereferenced: the checks come first
    need = lib.ribca_nhood_perm_counts_ws_bytes(100, 7)
    assert need == 768 and lib.ribca_nhood_perm_counts_ws_bytes(100, 1000) == 128 * 100 and lib.ribca_nhood_perm_counts_ws_bytes(100, 1) == 256
    assert lib.ribca_nhood_perm_counts_ws_bytes(0, 7) == 0 and lib.ribca_nhood_perm_counts_ws_bytes(100, 0) == 0

    def perm(idx=p, types=p, n=100, m=24, t=12, image=0, p0=0, n_perms=7, counts=p, ws=p, ws_bytes=need):
        return lib.ribca_nhood_perm_counts(idx, types, n, m, t, 0, image, p0, n_perms, counts, ws, ws_bytes, None)

    for call, text in ((lambda: perm(t=65), b"ribca_nhood_perm_counts: needs 1 <= T <= 64"),
                       (lambda: perm(t=0), b"ribca_nhood_perm_counts: needs 1 <= T <= 64"),
                       (lambda: perm(m=32), b"ribca_nhood_perm_counts: needs 1 <= m <= 31"),
                       (lambda: perm(m=0), b"ribca_nhood_perm_counts: needs 1 <= m <= 31"),
                       (lambda: perm(n=0), b"ribca_nhood_perm_counts: needs 1 <= n"),
                       (lambda: perm(idx=None), b"ribca_nhood_perm_counts: NULL buffer"),
                       (lambda: perm(counts=None), b"ribca_nhood_perm_counts: NULL buffer"),
                       (lambda: perm(ws=None), b"ribca_nhood_perm_counts: NULL buffer"),
                       (lambda: perm(image=-1), b"ribca_nhood_perm_counts: needs image >= 0"),
                       (lambda: perm(p0=2 ** 31 - 6), b"ribca_nhood_perm_counts: needs image >= 0"),
                       (lambda: perm(ws_bytes=need - 1), b"ribca_nhood_perm_counts: workspace too small"),
                       (lambda: lib.ribca_knn_neighbours(p, p, 100, 33, p, None), b"ribca_knn_neighbours: k must be in [2, 32]"),
                       (lambda: lib.ribca_knn_neighbours(p, p, 100, 1, p, None), b"ribca_knn_neighbours: k must be in [2, 32]"),
                       (lambda: lib.ribca_knn_neighbours(p, p, 5, 6, p, None), b"ribca_knn_neighbours: k exceeds the number of cells"),
                       (lambda: lib.ribca_knn_neighbours(p, None, 100, 25, p, None), b"ribca_knn_neighbours: NULL buffer"),
                       (lambda: lib.ribca_table_raster(None, 2, 2, p, 8, 1, 0.0, 1.0, p, None), b"ribca_table_raster: NULL buffer"),
                       (lambda: lib.ribca_table_raster(p, 257, 2, p, 8, 1, 0.0, 1.0, p, None), b"ribca_table_raster: needs 1 <= rows"),
                       (lambda: lib.ribca_table_raster(p, 2, 2, p, 8, 4, 0.0, 1.0, p, None), b"ribca_table_raster: needs 1 <= cell"),
                       (lambda: lib.ribca_table_raster(p, 2, 2, p, 8, 1, 1.0, 0.0, p, None), b"ribca_table_raster: needs finite vmin <= vmax"),
                       (lambda: lib.ribca_table_raster(p, 2, 2, p, 8, 1, 0.0, float("nan"), p, None), b"ribca_table_raster: needs finite vmin <= vmax")):
        assert call() == 1
        assert lib.ribca_last_error().startswith(text), (lib.ribca_last_error(), text)
    assert ops.NHOOD_MAX_TYPES == 64 and ops.NHOOD_MAX_NEIGHBOURS == 31
