"""Host side of the spatial autocorrelation (multiplexed_image_annotator_amd/autocorr.py, tests/autocorr_numpy.py): THE tree against a dense
formulation of Moran's I, the permutation null's mean against its closed form, a planted gradient, the statistics on hand-made numbers, the CSV,
the seed, and the argument checks of the four entry points (they run before any HIP call: no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

import autocorr_numpy as AN
import enrichment_numpy as EN
from multiplexed_image_annotator_amd import _lib, autocorr, ops


def _case(n, k, channels, seed):
    rng = np.random.RandomState(seed)
    x, y = rng.uniform(0, 1000, n), rng.uniform(0, 1000, n)
    z, m2 = AN.centred(rng.randn(n, channels) * rng.uniform(0.5, 50.0, channels) + rng.uniform(-5, 5, channels))
    return EN.knn_list(x, y, k), z, m2


@pytest.mark.parametrize("n,k", [(5, 5), (257, 9), (600, 25)])
def test_tree_against_a_dense_formulation(n, k):
    """I from the tree against I = (n / S0) z'Wz / z'z with a dense W.  Allowed per channel: 4 N u T / (m D), N = n m terms, u = 2^-53, T = the
    sum of |z_i z_j| over the edges -- twice the first-order bound N u T of any summation order of the numerator, divided by m D."""
    idx, z, m2 = _case(n, k, 3, n)
    m = k - 1
    got = AN.observed(z, idx)[0] / (m * m2)
    want = AN.dense_moran(z, idx)
    t = np.array([np.abs(z[:, c][:, None] * z[idx, c]).sum() for c in range(z.shape[1])])
    bound = 4.0 * (n * m) * 2.0 ** -53 * t / (m * m2)
    print(f"[dense n = {n}] |difference| {np.abs(got - want)} allowed {bound}")
    assert (np.abs(got - want) <= bound).all()
    stats = autocorr.statistics(AN.observed(z, idx), AN.perm(z, idx, 0, 0, 0, 2), m2, n, m)
    assert np.array_equal(stats["i"], got)
    # Geary's C against its definition, same graph: (n - 1) sum w (z_i - z_j)^2 / (2 S0 sum z^2)
    geary = np.array([(n - 1) * ((z[:, c][:, None] - z[idx, c]) ** 2).sum() / (2.0 * n * m * (z[:, c] ** 2).sum()) for c in range(z.shape[1])])
    assert np.allclose(stats["c"], geary, rtol=1e-12, atol=0)


def planted_case():
    """RandomState(400): 400 uniform points in 1000^2, k = 9; channels: a gradient along x with noise, two kinds of noise, a constant"""
    rng = np.random.RandomState(400)
    n = 400
    x, y = rng.uniform(0, 1000, n), rng.uniform(0, 1000, n)
    table = np.stack([x / 1000 + 0.1 * rng.randn(n), rng.randn(n), rng.rand(n), np.full(n, 0.5)], axis=1)
    return EN.knn_list(x, y, 9), table


@pytest.fixture(scope="module")
def planted():
    idx, table = planted_case()
    z, m2 = AN.centred(table)
    p = 200
    stats = autocorr.statistics(AN.observed(z, idx), AN.perm(z, idx, 0, 0, 0, p), m2, len(z), idx.shape[1])
    return {"idx": idx, "z": z, "m2": m2, "P": p, "stats": stats}


def test_null_mean_against_the_closed_form(planted):
    """under a uniform permutation E[I] = -1 / (n - 1) for any centred channel; the sample mean of the null within 4.5 standard errors of it"""
    s, n, p = planted["stats"], len(planted["z"]), planted["P"]
    dev = np.abs(s["i_null_mean"][:3] + 1.0 / (n - 1)) / (s["i_null_std"][:3] / np.sqrt(p))
    print("[null mean of I] deviations in standard errors:", np.round(dev, 2))
    assert (dev <= 4.5).all(), dev


def test_a_planted_gradient_scores_and_noise_does_not(planted):
    s = planted["stats"]
    print("[planted] i_z", s["i_z"], "c_z", s["c_z"])
    assert s["i_z"][0] > 10.0 and s["c_z"][0] < -10.0
    assert (np.abs(s["i_z"][1:3]) < 4.5).all() and (np.abs(s["c_z"][1:3]) < 4.5).all()
    assert s["i_n_ge"][0] == 0 and s["i_n_le"][0] == planted["P"] and s["c_n_le"][0] == 0 and s["c_n_ge"][0] == planted["P"]
    # the constant channel: D == 0 exactly, every float NaN
    assert planted["m2"][3] == 0.0
    for key in ("i", "i_null_mean", "i_null_std", "i_z", "c", "c_null_mean", "c_null_std", "c_z"):
        assert np.isnan(s[key][3]) and np.isfinite(s[key][:3]).all(), key
    assert s["i_n_ge"][3] == 0 and s["i_n_le"][3] == 0
    # another seed, another null; the observed values stay
    other = autocorr.statistics(AN.observed(planted["z"], planted["idx"]), AN.perm(planted["z"], planted["idx"], 1, 0, 0, 5), planted["m2"], 400, 8)
    assert np.array_equal(other["i"][:3], s["i"][:3]) and not np.array_equal(other["i_null_mean"][:3], s["i_null_mean"][:3])


def test_statistics_on_hand_made_numbers():
    obs = np.array([[6.0, 1.0, 0.0], [40.0, 3.0, 0.0]])
    null = np.array([[[2.0, 1.0, 0.0], [10.0, 3.0, 0.0]], [[4.0, 1.0, 0.0], [20.0, 3.0, 0.0]], [[6.0, 1.0, 0.0], [30.0, 3.0, 0.0]]])
    s = autocorr.statistics(obs, null, np.array([2.0, 4.0, 0.0]), cells=5, m=2)
    # I = N / (m D) = N / 4; C = (n - 1) G / (2 n m D) = G / 10: every value below but the std is exact in binary
    std = np.sqrt((0.25 + 0.0 + 0.25) / 3.0)
    assert s["i"][0] == 1.5 and s["c"][0] == 4.0 and s["i"][1] == 0.125
    assert np.array_equal(s["i_null_mean"][:2], [1.0, 0.125]) and s["i_null_std"][0] == std
    assert s["i_z"][0] == 0.5 / std and (s["i_n_ge"][0], s["i_n_le"][0]) == (1, 3)
    std_c = np.sqrt((1.0 + 0.0 + 1.0) / 3.0)
    assert s["c_null_mean"][0] == 2.0 and s["c_null_std"][0] == std_c and s["c_z"][0] == 2.0 / std_c and (s["c_n_ge"][0], s["c_n_le"][0]) == (0, 3)
    # a null without spread: std 0, z NaN, every permutation on both sides
    assert s["i_null_std"][1] == 0.0 and np.isnan(s["i_z"][1]) and (s["i_n_ge"][1], s["i_n_le"][1]) == (3, 3)
    # D == 0: NaN
    assert all(np.isnan(s[k][2]) for k in ("i", "c", "i_z", "c_z", "i_null_mean", "c_null_std"))
    assert np.array_equal(autocorr.figure_values(s)[:2], np.stack([s["i"], 1.0 - s["c"]], axis=1)[:2])
    # the null's moments do not depend on the order of the permutations
    t = autocorr.statistics(obs, null[::-1], np.array([2.0, 4.0, 0.0]), cells=5, m=2)
    assert all(s[k].tobytes() == t[k].tobytes() for k in s)
    for bad in (lambda: autocorr.statistics(obs, null[:0], np.zeros(3), 5, 2), lambda: autocorr.statistics(obs[0], null, np.zeros(3), 5, 2),
                lambda: autocorr.statistics(obs, null, np.zeros(2), 5, 2), lambda: autocorr.statistics(obs, null, np.zeros(3), 0, 2)):
        with pytest.raises(ValueError):
            bad()


def test_csv_bytes():
    obs = np.array([[6.0, 0.0], [12.0, 0.0]])
    null = np.array([[[2.0, 0.0], [10.0, 0.0]], [[6.0, 0.0], [30.0, 0.0]]])
    s = autocorr.statistics(obs, null, np.array([2.0, 0.0]), cells=5, m=2)      # I = N / 4: 1.5 against 0.5, 1.5; C = G / 10: 1.2 against 1, 3
    text = autocorr.table_csv(["CD3", "DAPI"], 5, s)
    assert text == ("marker,cells,morans_i,i_null_mean,i_null_std,i_z,i_n_ge,i_n_le,gearys_c,c_null_mean,c_null_std,c_z,c_n_ge,c_n_le\n"
                    "CD3,5,1.5,1,0.5,1,1,2,1.2,2,1,-0.80000000000000004,1,1\n"
                    "DAPI,5,nan,nan,nan,nan,0,0,nan,nan,nan,nan,0,0\n")
    row = text.split("\n")[1].split(",")
    assert np.array([float(row[8]), float(row[11])]).tobytes() == np.array([s["c"][0], s["c_z"][0]]).tobytes()      # 17 digits parse back to the same double


def test_the_seed_is_read_at_every_call(monkeypatch):
    monkeypatch.delenv("RIBCA_AUTOCORR_SEED", raising=False)
    assert autocorr.default_seed() == 0
    monkeypatch.setenv("RIBCA_AUTOCORR_SEED", "41")
    assert autocorr.default_seed() == 41
    monkeypatch.setenv("RIBCA_AUTOCORR_SEED", "")
    assert autocorr.default_seed() == 0
    monkeypatch.setenv("RIBCA_ENRICH_SEED", "7")      # the enrichment's seed is another switch
    assert autocorr.default_seed() == 0


def test_wrappers_refuse_before_any_launch():
    z, idx = torch.zeros((4, 2), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.int32)
    for bad in (float("nan"), float("inf")):
        zz = z.clone()
        zz[2, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            ops.autocorr_observed(zz, idx)
        with pytest.raises(ValueError, match="not finite"):
            ops.autocorr_perm(zz, idx, 0, 0, 0, 1)
    for call in (lambda: ops.autocorr_observed(z.float(), idx), lambda: ops.autocorr_observed(z, idx.long()), lambda: ops.autocorr_observed(z, idx[:3]),
                 lambda: ops.autocorr_perm(z[0], idx, 0, 0, 0, 1), lambda: ops.autocorr_perm(z, idx, 0, 0, 0, 1, ws=torch.zeros(8, dtype=torch.float32))):
        with pytest.raises(ValueError, match="autocorr_"):
            call()
    assert ops.AUTOCORR_MAX_CHANNELS == 64


def _align(v):
    return (v + 255) // 256 * 256


def test_entry_points_refuse_bad_arguments_with_a_status():
    lib = _lib.lib()
    assert lib.ribca_version() >= 103
    p = ctypes.c_void_p(4096)      # never dereferenced: the checks come first
    # the workspace: the partials (chunks, batch, 2, C) fp64, and before them the rows (batch, n, L) fp64 of a batch of permutations, L = C padded
    # to a power of two up to 16 and to a multiple of 16 above
    assert lib.ribca_autocorr_observed_ws_bytes(100, 3) == 256 and lib.ribca_autocorr_observed_ws_bytes(4097, 15) == _align(17 * 2 * 15 * 8)
    assert lib.ribca_autocorr_perm_ws_bytes(100, 3, 7) == _align(7 * 100 * 4 * 8) + _align(7 * 2 * 3 * 8)
    assert lib.ribca_autocorr_perm_ws_bytes(100, 15, 7) == _align(7 * 100 * 16 * 8) + _align(7 * 2 * 15 * 8)
    assert lib.ribca_autocorr_perm_ws_bytes(100, 17, 7) == _align(7 * 100 * 32 * 8) + _align(7 * 2 * 17 * 8)
    assert lib.ribca_autocorr_perm_ws_bytes(100, 1, 2) == _align(2 * 100 * 8) + 256
    assert lib.ribca_autocorr_perm_ws_bytes(100, 3, 1000) == _align(32 * 100 * 4 * 8) + _align(32 * 2 * 3 * 8)      # a batch holds at most 32
    assert lib.ribca_autocorr_perm_ws_bytes(9000, 64, 15) == _align(14 * 9000 * 64 * 8) + _align(36 * 14 * 2 * 64 * 8)      # ... and at most 64 MiB of rows
    assert lib.ribca_autocorr_perm_ws_bytes(99972, 15, 1000) == _align(5 * 99972 * 16 * 8) + _align(391 * 5 * 2 * 15 * 8)
    assert lib.ribca_autocorr_perm_ws_bytes(2 ** 30, 64, 5) == 2 ** 30 * 64 * 8 + _align(2 ** 22 * 2 * 64 * 8)      # one permutation when a single one is larger
    for n, c, perms in ((0, 3, 7), (2 ** 30 + 1, 3, 7), (100, 0, 7), (100, 65, 7), (100, 3, 0), (-1, 3, 7)):
        assert lib.ribca_autocorr_perm_ws_bytes(n, c, perms) == 0
        assert perms == 0 or lib.ribca_autocorr_observed_ws_bytes(n, c) == 0
    need_o, need_p = lib.ribca_autocorr_observed_ws_bytes(100, 3), lib.ribca_autocorr_perm_ws_bytes(100, 3, 7)

    def observed(z=p, idx=p, n=100, c=3, m=24, out=p, ws=p, ws_bytes=need_o):
        return lib.ribca_autocorr_observed(z, idx, n, c, m, out, ws, ws_bytes, None)

    def perm(z=p, idx=p, n=100, c=3, m=24, image=0, p0=0, n_perms=7, out=p, ws=p, ws_bytes=need_p):
        return lib.ribca_autocorr_perm(z, idx, n, c, m, 0, image, p0, n_perms, out, ws, ws_bytes, None)

    for name, fn in (("ribca_autocorr_observed", observed), ("ribca_autocorr_perm", perm)):
        for kwargs, text in (({"z": None}, "NULL buffer"), ({"idx": None}, "NULL buffer"), ({"out": None}, "NULL buffer"), ({"ws": None}, "NULL buffer"),
                             ({"n": 0}, "needs 1 <= n <= 2^30"), ({"n": 2 ** 30 + 1}, "needs 1 <= n <= 2^30"), ({"c": 0}, "needs 1 <= C <= 64"),
                             ({"c": 65}, "needs 1 <= C <= 64"), ({"m": 0}, "needs 1 <= m <= 31"), ({"m": 32}, "needs 1 <= m <= 31"),
                             ({"ws_bytes": (need_o if fn is observed else need_p) - 1}, "workspace too small")):
            assert fn(**kwargs) == 1
            assert lib.ribca_last_error() == f"{name}: {text}".encode(), (lib.ribca_last_error(), name, text)
    for kwargs in ({"image": -1}, {"p0": -1}, {"n_perms": 0}, {"p0": 2 ** 31 - 6}):
        assert perm(**kwargs) == 1
        assert lib.ribca_last_error() == b"ribca_autocorr_perm: needs image >= 0, p0 >= 0, 1 <= P, p0 + P <= 2^31"
