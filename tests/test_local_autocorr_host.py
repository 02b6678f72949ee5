"""Host side of the local indicators of spatial association (multiplexed_image_annotator_amd/local_autocorr.py, tests/local_autocorr_numpy.py):
the argument checks of the three entry points (they run before any HIP call: no GPU needed), the statistics, the class rule and the CSVs on
hand-made counts, and the properties of the restated conditional permutation: the two-cell case, additivity, ties, the null's mean and variance
against their closed forms, a planted gradient and a planted disc, and the mean of the local values against the global Moran's I."""
import ctypes

import numpy as np
import pytest

import autocorr_numpy as AN
import enrichment_numpy as EN
import local_autocorr_numpy as LN
from multiplexed_image_annotator_amd import _lib, colors, local_autocorr


def _align(v):
    return (v + 255) // 256 * 256


def test_entry_points_refuse_bad_arguments_with_a_status():
    lib = _lib.lib()
    assert lib.ribca_version() >= 104
    p = ctypes.c_void_p(4096)      # never dereferenced: the checks come first
    # the workspace: the rows (batch, n, L) fp64 of a batch of permutations -- the batch and L of ribca_autocorr_perm -- then the inverse of
    # sigma (batch, n) int32
    assert lib.ribca_local_perm_counts_ws_bytes(100, 3, 7) == _align(7 * 100 * 4 * 8) + _align(7 * 100 * 4)
    assert lib.ribca_local_perm_counts_ws_bytes(100, 15, 7) == _align(7 * 100 * 16 * 8) + _align(7 * 100 * 4)
    assert lib.ribca_local_perm_counts_ws_bytes(100, 17, 7) == _align(7 * 100 * 32 * 8) + _align(7 * 100 * 4)
    assert lib.ribca_local_perm_counts_ws_bytes(100, 1, 2) == _align(2 * 100 * 8) + _align(2 * 100 * 4)
    assert lib.ribca_local_perm_counts_ws_bytes(100, 3, 1000) == _align(32 * 100 * 4 * 8) + _align(32 * 100 * 4)      # a batch holds at most 32
    assert lib.ribca_local_perm_counts_ws_bytes(9000, 64, 15) == _align(14 * 9000 * 64 * 8) + _align(14 * 9000 * 4)      # ... and at most 64 MiB of rows
    assert lib.ribca_local_perm_counts_ws_bytes(99972, 15, 999) == _align(5 * 99972 * 16 * 8) + _align(5 * 99972 * 4)
    assert lib.ribca_local_perm_counts_ws_bytes(2 ** 30, 64, 5) == 2 ** 30 * 64 * 8 + 2 ** 30 * 4      # one permutation when a single one is larger
    for n, c, perms in ((0, 3, 7), (2 ** 30 + 1, 3, 7), (100, 0, 7), (100, 65, 7), (100, 3, 0), (-1, 3, 7)):
        assert lib.ribca_local_perm_counts_ws_bytes(n, c, perms) == 0
    need = lib.ribca_local_perm_counts_ws_bytes(100, 3, 7)

    def lag(z=p, idx=p, n=100, c=3, m=24, out=p):
        return lib.ribca_local_lag(z, idx, n, c, m, out, None)

    def counts(z=p, idx=p, lag=p, n=100, c=3, m=24, image=0, p0=0, n_perms=7, ge=p, le=p, ws=p, ws_bytes=need):
        return lib.ribca_local_perm_counts(z, idx, lag, n, c, m, 0, image, p0, n_perms, ge, le, ws, ws_bytes, None)

    sizes = [({"n": 0}, "needs 1 <= n <= 2^30"), ({"n": 2 ** 30 + 1}, "needs 1 <= n <= 2^30"), ({"c": 0}, "needs 1 <= C <= 64"),
             ({"c": 65}, "needs 1 <= C <= 64"), ({"m": 0}, "needs 1 <= m <= 31"), ({"m": 32}, "needs 1 <= m <= 31")]
    null = lambda *names: [({k: None}, "NULL buffer") for k in names]
    for name, fn, cases in (("ribca_local_lag", lag, null("z", "idx", "out") + sizes),
                            ("ribca_local_perm_counts", counts, null("z", "idx", "lag", "ge", "le", "ws") + sizes
                             + [({"ws_bytes": need - 1}, "workspace too small")])):
        for kwargs, text in cases:
            assert fn(**kwargs) == 1
            assert lib.ribca_last_error() == f"{name}: {text}".encode(), (lib.ribca_last_error(), name, text)
    for kwargs in ({"image": -1}, {"p0": -1}, {"n_perms": 0}, {"p0": 2 ** 31 - 6}):
        assert counts(**kwargs) == 1
        assert lib.ribca_last_error() == b"ribca_local_perm_counts: needs image >= 0, p0 >= 0, 1 <= P, p0 + P <= 2^31"


def test_statistics_classes_and_csv_on_hand_made_counts():
    # n = 4, m = 2, P = 39, alpha = 1/20: significant iff 2 (min + 1) 20 <= 40, i.e. min(ge, le) == 0 -- the boundary itself
    z = np.array([[1.0, 0.0], [-1.0, 0.0], [2.0, 0.0], [0.0, 0.0]])
    lag = np.array([[2.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [3.0, 0.0]])
    ge = np.array([[0, 39], [39, 39], [5, 39], [0, 39]])
    le = np.array([[39, 39], [0, 39], [39, 39], [39, 39]])
    s = local_autocorr.statistics(z, lag, ge, le, np.array([4.0, 0.0]), m=2, n_perms=39)
    # I_i = 4 z lag / (2 * 4); Gi* = (lag + z) / (sqrt(4 / 4) sqrt((4 * 3 - 9) / 3)) = lag + z
    assert np.array_equal(s["local_i"][:, 0], [1.0, -0.5, -1.0, 0.0]) and np.array_equal(s["gi_star"][:, 0], [3.0, 0.0, 1.0, 3.0])
    assert np.isnan(s["local_i"][:, 1]).all() and np.isnan(s["gi_star"][:, 1]).all()      # D == 0
    assert np.array_equal(s["p"][:, 0], [2.0 / 40.0, 2.0 / 40.0, 12.0 / 40.0, 2.0 / 40.0]) and np.array_equal(s["p"][:, 1], [1.0] * 4)
    assert s["class"].dtype == np.uint8
    assert s["class"][:, 0].tolist() == [1, 2, 0, 0]      # HH; LH; not significant; z == 0
    assert s["class"][:, 1].tolist() == [0, 0, 0, 0]
    text = local_autocorr.table_csv([7, 8, 9, 12], ["CD3", "DAPI"], s)
    lines = text.split("\n")
    assert text.endswith("\n") and len(lines) == 6
    assert lines[0] == ("cell_id,CD3_z,CD3_lag,CD3_local_i,CD3_gi_star,CD3_n_ge,CD3_n_le,CD3_p,CD3_class,"
                        "DAPI_z,DAPI_lag,DAPI_local_i,DAPI_gi_star,DAPI_n_ge,DAPI_n_le,DAPI_p,DAPI_class")
    assert lines[1] == f"7,1,2,1,3,0,39,{0.05:.17g},1,0,0,nan,nan,39,39,1,0"
    assert lines[3] == f"9,2,-1,-1,1,5,39,{0.3:.17g},0,0,0,nan,nan,39,39,1,0"
    assert float(lines[1].split(",")[7]) == 0.05
    assert local_autocorr.summary_csv(["CD3", "DAPI"], s["class"]) == "marker,cells,not_significant,HH,LH,LL,HL\nCD3,4,2,1,1,0,0\nDAPI,4,4,0,0,0,0\n"
    # one step past the boundary: min = 1 -> 80 > 40
    t = local_autocorr.statistics(z, lag, np.maximum(ge, 1), np.maximum(le, 1), np.array([4.0, 0.0]), 2, 39)
    assert not t["class"].any()
    # the other two quadrants, a lag of exactly 0, and alpha as a decimal text: 0.1 = 1/10 -> 2 (min + 1) 10 <= 40: min <= 1
    z2, lag2 = np.array([[-1.0], [3.0], [1.0], [-3.0]]), np.array([[-2.0], [-0.5], [0.0], [-1.0]])
    u = local_autocorr.statistics(z2, lag2, np.array([[39], [38], [39], [37]]), np.array([[1], [1], [0], [2]]), np.array([20.0]), 2, 39, alpha=0.1)
    assert u["class"][:, 0].tolist() == [3, 4, 0, 0]
    assert local_autocorr.alpha_fraction(0.05) == (1, 20) and local_autocorr.alpha_fraction("0.001") == (1, 1000) and local_autocorr.alpha_fraction(1) == (1, 1)
    # n <= m + 1: no Gi*
    v = local_autocorr.statistics(z[:3], lag[:3], ge[:3], le[:3], np.array([6.0, 0.0]), 2, 39)
    assert np.isnan(v["gi_star"]).all() and np.isfinite(v["local_i"][:, 0]).all()
    for bad in (lambda: local_autocorr.statistics(z, lag[:3], ge, le, np.zeros(2), 2, 39), lambda: local_autocorr.statistics(z, lag, ge, le, np.zeros(3), 2, 39),
                lambda: local_autocorr.statistics(z, lag, ge, le, np.zeros(2), 0, 39), lambda: local_autocorr.statistics(z, lag, ge, le, np.zeros(2), 2, 0),
                lambda: local_autocorr.statistics(z, lag, ge, le, np.zeros(2), 2, 39, alpha=0), lambda: local_autocorr.alpha_fraction(1.5)):
        with pytest.raises(ValueError):
            bad()
    assert colors.LISA_COLORS.tolist() == [[211, 211, 211], [215, 25, 28], [171, 217, 233], [44, 123, 182], [253, 174, 97]]
    assert local_autocorr.CLASSES == ("not_significant", "HH", "LH", "LL", "HL")


def test_seed_from_the_environment(monkeypatch):
    monkeypatch.delenv("RIBCA_LOCAL_SEED", raising=False)
    assert local_autocorr.default_seed() == 0
    monkeypatch.setenv("RIBCA_LOCAL_SEED", "41")
    assert local_autocorr.default_seed() == 41
    monkeypatch.setenv("RIBCA_LOCAL_SEED", "")
    assert local_autocorr.default_seed() == 0


def test_two_cells_always_draw_each_other():
    z = np.array([[0.25], [-0.25]])
    idx = np.array([[1], [0]])
    ge, le = LN.perm_counts(z, idx, LN.lag(z, idx), 0, 0, 0, 11)
    assert (ge == 11).all() and (le == 11).all()


def test_additivity_skipped_entries_self_entries_and_ties():
    n, c, m = 300, 3, 6
    rng = np.random.RandomState(7)
    z = rng.randn(n, c)
    z[:, 2] = 0.5      # a constant channel: every permuted sum ties with the observed one
    idx = rng.randint(-2, n + 2, (n, m))
    idx[5, 1] = 5      # a list that holds its own cell
    idx[9, 0] = idx[9, 3] = 17      # ... and one that holds a duplicate
    assert (idx < 0).any() and (idx >= n).any()
    lag = LN.lag(z, idx)
    by_hand = np.array([sum((z[j] for j in idx[i] if 0 <= j < n), np.zeros(c)) for i in (5, 9, 40)])
    assert np.array_equal(lag[[5, 9, 40]], by_hand)
    # the sources: the cell itself stays, the others are other cells, distinct for distinct entries
    for p in range(3):
        sg = EN.sigma(n, 3, 1, p)
        src = LN.sources(idx, sg)
        ok = (idx >= 0) & (idx < n)
        own = np.arange(n)[:, None]
        assert ((src == own) == (idx == own))[ok].all()
        for i in range(n):
            entries, drawn = idx[i][ok[i]], src[i][ok[i]]
            assert len(set(drawn.tolist())) == len(set(entries.tolist()))
    ge7, le7 = LN.perm_counts(z, idx, lag, 3, 1, 0, 7)
    ge5, le5 = LN.perm_counts(z, idx, lag, 3, 1, 0, 5)
    ge2, le2 = LN.perm_counts(z, idx, lag, 3, 1, 5, 2)
    assert np.array_equal(ge7, ge5 + ge2) and np.array_equal(le7, le5 + le2)
    ties = ge7 + le7 - 7
    assert (ties[:, 2] == 7).all()
    has = ((idx >= 0) & (idx < n) & (idx != np.arange(n)[:, None])).any(axis=1)      # a cell with a neighbour other than itself
    assert (ties[has][:, :2] == 0).all() and has.sum() >= n - 1


def planted_case():
    """RandomState(400): 400 uniform points in 1000^2, k = 9; channels: two kinds of noise, a gradient along x with noise, a disc of radius 150
    at (300, 300) raised by 3 with noise, a constant"""
    rng = np.random.RandomState(400)
    n = 400
    x, y = rng.uniform(0, 1000, n), rng.uniform(0, 1000, n)
    disc = (x - 300.0) ** 2 + (y - 300.0) ** 2 <= 150.0 ** 2
    table = np.stack([rng.randn(n), rng.rand(n), x / 1000 + 0.1 * rng.randn(n), 3.0 * disc + rng.randn(n), np.full(n, 0.5)], axis=1)
    return EN.knn_list(x, y, 9), table, disc


@pytest.fixture(scope="module")
def planted():
    idx, table, disc = planted_case()
    z, m2 = AN.centred(table)
    return {"idx": idx, "z": z, "m2": m2, "disc": disc, "lag": LN.lag(z, idx)}


def test_null_mean_and_variance_against_their_closed_forms(planted):
    """the m sources of a cell are a sample without replacement of the other n - 1 rows: mean -m z_i / (n - 1), variance
    m (n - 1 - m) / (n - 2) ((D - z_i^2) / (n - 1) - (z_i / (n - 1))^2)"""
    z, idx, d = planted["z"][:, :4], planted["idx"], planted["m2"][:4]
    n, m, p = len(z), idx.shape[1], 200
    sums = np.stack([LN.perm_sums(z, idx, 0, 0, j) for j in range(p)])
    mean = -m * z / (n - 1)
    var = m * (n - 1 - m) / (n - 2) * ((d - z * z) / (n - 1) - (z / (n - 1)) ** 2)
    dev = np.abs(sums.mean(axis=0) - mean) / np.sqrt(var / p)
    ratio = (sums.var(axis=0, ddof=1) / var).mean(axis=0)
    print("[null of the lag] largest deviation in standard errors per channel", np.round(dev.max(axis=0), 2), "mean variance ratio", np.round(ratio, 3))
    assert (dev <= 4.5).all()
    assert ((ratio >= 0.9) & (ratio <= 1.1)).all()


def test_planted_structure_is_found_where_it_is(planted):
    z, idx, disc = planted["z"], planted["idx"], planted["disc"]
    p = 999
    ge, le = LN.perm_counts(z, idx, planted["lag"], 0, 0, 0, p)
    s = local_autocorr.statistics(z, planted["lag"], ge, le, planted["m2"], idx.shape[1], p, alpha=0.05)
    flagged = (s["class"] > 0).sum(axis=0)
    hh = s["class"][:, 3] == 1
    print("[planted] flagged per channel", flagged, "disc cells", int(disc.sum()), "HH", int(hh.sum()), "HH in the disc", int((hh & disc).sum()))
    # noise: alpha n = 20 expected, sd about 4.4 (more with the overlap of neighbouring lists): at most 40
    assert (flagged[:2] <= 40).all()
    # the gradient: the cells of the outer halves (|x - 500| > 250, half of them) have an expected lag of magnitude 8 * 0.25 against a null
    # standard deviation of about sqrt(8) * 0.3: well over 2 sigma.  More than a third of all cells, all of them HH or LL
    assert flagged[2] > 400 // 3 and np.isin(s["class"][:, 2], (0, 1, 3)).mean() > 0.98
    # the disc: its cells are HH
    assert (hh & disc).sum() >= 25 and disc.sum() <= 40
    # the constant: nothing, exactly
    assert flagged[4] == 0 and (z[:, 4] == 0.0).all() and (planted["lag"][:, 4] == 0.0).all() and np.isnan(s["local_i"][:, 4]).all()
    assert (ge[:, 4] == p).all() and (le[:, 4] == p).all() and (s["p"][:, 4] == 1.0).all()


def test_mean_of_the_local_values_is_the_global_moran(planted):
    z, idx, d = planted["z"][:, :4], planted["idx"], planted["m2"][:4]
    n, m = len(z), idx.shape[1]
    s = local_autocorr.statistics(z, planted["lag"][:, :4], np.zeros(z.shape, int), np.zeros(z.shape, int), d, m, 1)
    want = AN.observed(z, idx)[0] / (m * d)
    t = np.array([np.abs(z[:, c][:, None] * z[idx, c]).sum() for c in range(z.shape[1])])
    bound = 4.0 * (n * m) * 2.0 ** -53 * t / (m * d)
    got = s["local_i"].mean(axis=0)
    print(f"[mean of local_i] |difference| {np.abs(got - want)} allowed {bound}")
    assert (np.abs(got - want) <= bound).all()
