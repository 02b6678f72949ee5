"""The nearest cell of every type without a GPU: the version, every refusal of the two entry points and their workspace queries (a status whose
text names the entry point, before any HIP call), the host module on a hand-made case of six cells whose every number is written out here, and
the statistic on a planted attraction, restatement only (tests/nearest_numpy.py)."""
import ctypes

import numpy as np
import pytest

import nearest_numpy as NN
from multiplexed_image_annotator_amd import _lib, nearest

CAP = 1 << 21


def _edges(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def test_version():
    assert _lib.lib().ribca_version() >= 105


def test_refusals_are_a_status_naming_the_entry_point():
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)      # never dereferenced: every case below is refused by its sizes, before any HIP call
    big = 1 << 40

    def refused(status, text):
        assert status == 1
        msg = lib.ribca_last_error()
        assert msg and msg.startswith(text.encode()), (text, msg)

    name = "ribca_nearest_by_type"
    for hole in range(6):
        args = [p, p, p, p, p, p]
        args[hole] = None
        x, y, t, near2, arg, ws = args
        refused(lib.ribca_nearest_by_type(x, y, t, 8, 3, near2, arg, ws, big, None), f"{name}: NULL buffer")
    refused(lib.ribca_nearest_by_type(p, p, p, 0, 3, p, p, p, big, None), f"{name}: needs 1 <= n <= 2^21")
    refused(lib.ribca_nearest_by_type(p, p, p, CAP + 1, 3, p, p, p, big, None), f"{name}: needs 1 <= n <= 2^21")
    refused(lib.ribca_nearest_by_type(p, p, p, 8, 0, p, p, p, big, None), f"{name}: needs 1 <= T <= 254")
    refused(lib.ribca_nearest_by_type(p, p, p, 8, 255, p, p, p, big, None), f"{name}: needs 1 <= T <= 254")
    need = lib.ribca_nearest_by_type_ws_bytes(8, 3)
    assert need > 0 and need % 256 == 0
    refused(lib.ribca_nearest_by_type(p, p, p, 8, 3, p, p, p, need - 1, None), f"{name}: workspace too small")
    for n, t in ((0, 3), (CAP + 1, 3), (-1, 3), (8, 0), (8, 255)):
        assert lib.ribca_nearest_by_type_ws_bytes(n, t) == 0
    assert lib.ribca_nearest_by_type_ws_bytes(CAP, 254) > lib.ribca_nearest_by_type_ws_bytes(CAP - 4096, 254) > 0

    name = "ribca_nearest_perm_counts"
    good = _edges([1.0, 4.0])

    def call(x=p, y=p, t=p, n=8, T=3, r2=good, B=2, image=0, p0=0, P=4, counts=p, ws=p, ws_bytes=big):
        return lib.ribca_nearest_perm_counts(x, y, t, n, T, r2, B, 0, image, p0, P, counts, ws, ws_bytes, None)

    for hole in ("x", "y", "t", "r2", "counts", "ws"):
        refused(call(**{hole: None}), f"{name}: NULL buffer")
    refused(call(n=0), f"{name}: needs 1 <= n <= 2^21")
    refused(call(n=CAP + 1), f"{name}: needs 1 <= n <= 2^21")
    refused(call(T=0), f"{name}: needs 1 <= T <= 64")
    refused(call(T=65), f"{name}: needs 1 <= T <= 64")
    refused(call(T=255), f"{name}: needs 1 <= T <= 64")
    refused(call(B=0), f"{name}: needs 1 <= B <= 32")
    refused(call(r2=_edges(np.arange(1.0, 34.0)), B=33), f"{name}: needs 1 <= B <= 32")
    for bad in ([4.0, 1.0], [2.0, 2.0], [-1.0, 4.0], [1.0, float("nan")], [1.0, float("inf")]):
        refused(call(r2=_edges(bad)), f"{name}: the squared radii must be finite, non-negative and strictly increasing")
    window = f"{name}: needs image >= 0, p0 >= 0, 1 <= P, p0 + P <= 2^31"
    refused(call(p0=(1 << 31) - 3, P=4), window)
    refused(call(P=0), window)
    refused(call(p0=-1), window)
    refused(call(image=-1), window)
    need = lib.ribca_nearest_perm_counts_ws_bytes(8, 3, 4)
    assert need > 0 and need % 256 == 0
    refused(call(ws_bytes=need - 1), f"{name}: workspace too small")
    for n, t, pp in ((0, 3, 4), (CAP + 1, 3, 4), (8, 0, 4), (8, 65, 4), (8, 3, 0)):
        assert lib.ribca_nearest_perm_counts_ws_bytes(n, t, pp) == 0
    # the copies of a batch: min(P, 32, max(1, 64 MiB / (16 n))) of them, 16 n bytes each
    assert lib.ribca_nearest_perm_counts_ws_bytes(1024, 3, 33) == lib.ribca_nearest_perm_counts_ws_bytes(1024, 3, 32)
    assert lib.ribca_nearest_perm_counts_ws_bytes(1024, 3, 32) - lib.ribca_nearest_perm_counts_ws_bytes(1024, 3, 31) == 16 * 1024
    assert lib.ribca_nearest_perm_counts_ws_bytes(CAP, 3, 9) == lib.ribca_nearest_perm_counts_ws_bytes(CAP, 3, 2) > 2 * 16 * CAP


# ---- six cells on a line: A A B B B A at x = 0, 3, 4, 10, 10, 20; the type C has no cell --------------------------------------------------------
X = np.array([0.0, 3.0, 4.0, 10.0, 10.0, 20.0])
LABELS = np.array([0, 0, 1, 1, 1, 0])
IDS = np.array([3, 5, 6, 9, 10, 12])
NAMES = ["A", "B c", "C"]
INF = float("inf")
NEAR2 = np.array([[9.0, 16.0, INF], [9.0, 1.0, INF], [1.0, 36.0, INF], [49.0, 0.0, INF], [49.0, 0.0, INF], [289.0, 100.0, INF]])
ARG = np.array([[1, 2, -1], [0, 2, -1], [1, 3, -1], [1, 4, -1], [1, 3, -1], [1, 3, -1]])
RADII = [1.0, 5.0, 10.0]
#: [band][anchor][target]
OBSERVED = np.array([[[0, 1, 0], [1, 2, 0], [0, 0, 0]],
                     [[2, 1, 0], [0, 0, 0], [0, 0, 0]],
                     [[0, 1, 0], [2, 1, 0], [0, 0, 0]]])
PRESENT = np.array([3, 3, 0])


def test_the_restatement_on_the_hand_made_case():
    near2, arg = NN.nearest_by_type(X, np.zeros(6), LABELS, 3)
    assert np.array_equal(near2, NEAR2) and np.array_equal(arg, ARG)
    assert np.array_equal(NN.band_counts(near2, LABELS, 3, np.array(RADII) ** 2), OBSERVED)


def test_observed_counts_on_the_hand_made_case():
    got = nearest.observed_counts(NEAR2, LABELS, 3, np.array(RADII) ** 2)
    assert got.dtype == np.int64 and np.array_equal(got, OBSERVED)
    # 100 = 10^2 sits in the band that ends at it; one ulp above it the cell is beyond the last radius
    edge = np.array([1.0, 25.0, np.nextafter(100.0, 0.0)])
    want = OBSERVED.copy()
    want[2, 0, 1] = 0
    assert np.array_equal(nearest.observed_counts(NEAR2, LABELS, 3, edge), want)
    # a label outside [0, T) is no anchor
    odd = LABELS.copy()
    odd[5] = 7
    want = OBSERVED.copy()
    want[2, 0, 1] = 0
    assert np.array_equal(nearest.observed_counts(NEAR2, odd, 3, np.array(RADII) ** 2), want)
    with pytest.raises(ValueError):
        nearest.observed_counts(NEAR2[:, :2], LABELS, 3, [1.0])


def test_statistics_on_the_hand_made_case():
    s = nearest.statistics(OBSERVED, None, PRESENT)
    assert sorted(s) == ["G", "cumulative"]
    cum = s["cumulative"]
    assert cum[:, 0, 0].tolist() == [0, 2, 2] and cum[:, 0, 1].tolist() == [1, 2, 3]
    assert cum[:, 1, 0].tolist() == [1, 1, 3] and cum[:, 1, 1].tolist() == [2, 2, 3] and not cum[:, :, 2].any() and not cum[:, 2, :].any()
    g = s["G"]
    assert g[:, 0, 0].tolist() == [0.0, 2 / 3, 2 / 3] and g[:, 0, 1].tolist() == [1 / 3, 2 / 3, 1.0]
    assert g[:, 1, 0].tolist() == [1 / 3, 1 / 3, 1.0] and g[:, 1, 1].tolist() == [2 / 3, 2 / 3, 1.0]
    assert g[:, 0, 2].tolist() == [0.0, 0.0, 0.0] and np.isnan(g[:, 2, :]).all()
    null = np.zeros((2, 3, 3, 3), dtype=np.int64)
    null[0, :, 0, 1] = [0, 1, 0]      # cumulative 0 1 1
    null[1, :, 0, 1] = [2, 0, 1]      # cumulative 2 2 3   against the observed 1 2 3
    s = nearest.statistics(OBSERVED, null, PRESENT)
    assert s["mean"][:, 0, 1].tolist() == [1.0, 1.5, 2.0] and s["std"][:, 0, 1].tolist() == [1.0, 0.5, 1.0]
    assert s["z"][:, 0, 1].tolist() == [0.0, 1.0, 1.0]
    assert s["n_ge"][:, 0, 1].tolist() == [1, 1, 1] and s["n_le"][:, 0, 1].tolist() == [1, 2, 2]
    # a null that never counts: mean 0, std 0, no z; it is at or below everything and at or above only a zero
    assert s["mean"][:, 1, 1].tolist() == [0.0, 0.0, 0.0] and np.isnan(s["z"][:, 1, 1]).all()
    assert s["n_ge"][:, 1, 1].tolist() == [0, 0, 0] and s["n_le"][:, 1, 1].tolist() == [2, 2, 2] and s["n_ge"][:, 0, 0].tolist() == [2, 0, 0]
    want = NN.statistics(OBSERVED, null, PRESENT)
    for key in want:
        assert np.array_equal(s[key], want[key], equal_nan=True), key
    with pytest.raises(ValueError):
        nearest.statistics(OBSERVED, null[:, :2], PRESENT)
    with pytest.raises(ValueError):
        nearest.statistics(OBSERVED.astype(np.float64), None, PRESENT)


def test_cells_csv_on_the_hand_made_case():
    text = nearest.cells_csv(IDS, LABELS, NAMES, NEAR2, ARG)
    assert text == ("cell_id,cell_type,d_A,id_A,d_B_c,id_B_c,d_C,id_C\n"
                    "3,A,3,5,4,6,inf,\n"
                    "5,A,3,3,1,6,inf,\n"
                    "6,B c,1,5,6,9,inf,\n"
                    "9,B c,7,5,0,10,inf,\n"
                    "10,B c,7,5,0,9,inf,\n"
                    "12,A,17,5,10,9,inf,\n")
    # distances that are no integers parse back to the very doubles
    rng = np.random.RandomState(3)
    near2 = rng.uniform(0.0, 1e6, (6, 3))
    rows = nearest.cells_csv(IDS, LABELS, NAMES, near2, ARG).strip().split("\n")[1:]
    back = np.array([[float(r.split(",")[2 + 2 * b]) for b in range(3)] for r in rows])
    assert np.array_equal(back, np.sqrt(near2))
    with pytest.raises(ValueError):
        nearest.cells_csv(IDS, LABELS, NAMES[:2], NEAR2, ARG)


def test_table_csv_on_the_hand_made_case():
    rows = nearest.table_csv(NAMES, RADII, OBSERVED, PRESENT).split("\n")
    assert rows[0] == "anchor,target,anchor_cells,r,count,cum_count,G" and rows[-1] == "" and len(rows) == 1 + 27 + 1
    assert rows[1:4] == ["A,A,3,1,0,0,0", "A,A,3,5,2,2,0.66666666666666663", "A,A,3,10,0,2,0.66666666666666663"]
    assert rows[4:7] == ["A,B c,3,1,1,1,0.33333333333333331", "A,B c,3,5,1,2,0.66666666666666663", "A,B c,3,10,1,3,1"]
    assert rows[10] == "B c,A,3,1,1,1,0.33333333333333331" and rows[15] == "B c,B c,3,10,1,3,1"
    assert rows[19] == "C,A,0,1,0,0,nan"
    null = np.zeros((2, 3, 3, 3), dtype=np.int64)
    null[0, :, 0, 1] = [0, 1, 0]
    null[1, :, 0, 1] = [2, 0, 1]
    stats = nearest.statistics(OBSERVED, null, PRESENT)
    rows = nearest.table_csv(NAMES, RADII, OBSERVED, PRESENT, stats).split("\n")
    assert rows[0] == "anchor,target,anchor_cells,r,count,cum_count,G,null_mean,null_std,z,n_ge,n_le"
    assert rows[4:7] == ["A,B c,3,1,1,1,0.33333333333333331,1,1,0,1,1", "A,B c,3,5,1,2,0.66666666666666663,1.5,0.5,1,1,2",
                         "A,B c,3,10,1,3,1,2,1,1,1,2"]
    assert rows[1] == "A,A,3,1,0,0,0,0,0,nan,2,2"
    for r in rows[1:-1]:      # every float parses back to the double it was written from
        a, b, k = NAMES.index(r.split(",")[0]), NAMES.index(r.split(",")[1]), RADII.index(float(r.split(",")[3]))
        for col, key in ((6, "G"), (7, "mean"), (8, "std"), (9, "z")):
            assert np.array_equal(float(r.split(",")[col]), stats[key][k, a, b], equal_nan=True)
    with pytest.raises(ValueError):
        nearest.table_csv(NAMES, RADII[:2], OBSERVED, PRESENT)


def test_the_seed_and_the_colour_index(monkeypatch):
    monkeypatch.delenv("RIBCA_NEAREST_SEED", raising=False)
    assert nearest.default_seed() == 0
    monkeypatch.setenv("RIBCA_NEAREST_SEED", "41")
    assert nearest.default_seed() == 41
    monkeypatch.setenv("RIBCA_NEAREST_SEED", "")
    assert nearest.default_seed() == 0
    # int(min(d / r_max, 1) * 255): 0 at distance 0, 127 at half the last radius, 255 at and beyond it, and where there is no such cell
    assert nearest.distance_colour_index(np.array([0.0, 25.0, 100.0, 99.0 ** 2, 1e9, INF]), 10.0).tolist() == [0, 127, 255, 255, 255, 255]
    assert nearest.distance_colour_index(np.array([0.0, 4.0]), 0.0).tolist() == [0, 255]


def test_the_command_line_switches():
    """both flags default to 0; the pipeline calls the method only with --nearest-bands > 0, with N radii of one cell size and the permutations"""
    import types
    import main as cli
    common = ["--marker-list-path", "m.txt", "--image-path", "i.npy", "--mask-path", "k.npy", "--batch-id", "c"]
    args = cli.parse_args(common)
    assert args.nearest_bands == 0 and args.nearest_perms == 0
    args = cli.parse_args(common + ["--nearest-bands", "4", "--nearest-perms", "9"])
    assert args.nearest_bands == 4 and args.nearest_perms == 9

    class Recorder:
        cell_size = 30
        channel_parser = types.SimpleNamespace(immune_base=True, immune_extended=False, immune_full=False, struct=False, nerve=False)

        def __init__(self):
            self.calls = []

        def min_cells_per_image(self):
            return 0

        def __getattr__(self, name):
            return lambda *a, **kw: self.calls.append((name, a, kw))

    off = Recorder()
    cli._pipeline(off, 16, 0)
    cli._pipeline(off, 16, 0, nearest_perms=9)      # read only with --nearest-bands > 0
    assert "nearest_type_distances" not in [c[0] for c in off.calls]
    on = Recorder()
    cli._pipeline(on, 16, 0, nearest_bands=3, nearest_perms=9)
    got = [c for c in on.calls if c[0] == "nearest_type_distances"]
    assert len(got) == 1 and got[0][2]["radii"].tolist() == [30.0, 60.0, 90.0] and got[0][2]["n_perms"] == 9 and got[0][2]["integrate"] is True
    assert [c[0] for c in on.calls if c[0] != "nearest_type_distances"] == [c[0] for c in off.calls][:len(off.calls) // 2]


def test_planted_attraction_restatement_only():
    """RandomState(400): 120 A cells uniform on 1000 x 1000, one B cell 12 px from each in a random direction, 160 C cells uniform; 8 bands of
    30 px, 200 permutations of the keyed bijection, seed 0.  A throw-away probe of this layout with numpy's own permutations gave
    z[band 0][A][B] = 13.7, z[band 0][B][A] = 13.6, G_AB(30) = 1.0 against a null mean of 0.40, and 2.0 for the largest |z| of a shuffled labelling
    against the same null; the bounds leave about 40 % under the probe for the change of generator.  With the bijection (printed below, DESIGN.md
    section 18): 12.74 and 12.26, G_AB(30) = 1.0 against a null mean of 0.431, 58 finite entries, largest |z| of permutation 200: 2.42."""
    rng = np.random.RandomState(400)
    ax, ay = rng.uniform(0, 1000, 120), rng.uniform(0, 1000, 120)
    theta = rng.uniform(0, 2 * np.pi, 120)
    cx, cy = rng.uniform(0, 1000, 160), rng.uniform(0, 1000, 160)
    x = np.concatenate([ax, ax + 12.0 * np.cos(theta), cx])
    y = np.concatenate([ay, ay + 12.0 * np.sin(theta), cy])
    labels = np.repeat([0, 1, 2], [120, 120, 160])
    r2 = (30.0 * np.arange(1, 9)) ** 2
    present = np.bincount(labels, minlength=3)
    observed = NN.band_counts(NN.nearest_by_type(x, y, labels, 3)[0], labels, 3, r2)
    assert np.array_equal(observed, nearest.observed_counts(NN.nearest_by_type(x, y, labels, 3)[0], labels, 3, r2))
    null = NN.perm_counts(x, y, labels, 3, r2, 0, 0, 0, 200)
    s = nearest.statistics(observed, null, present)
    finite = np.isfinite(s["z"])
    print("z[0][A][B]", s["z"][0, 0, 1], "z[0][B][A]", s["z"][0, 1, 0], "G_AB(30)", s["G"][0, 0, 1], "null mean of G_AB(30)", s["mean"][0, 0, 1] / 120,
          "finite z", int(finite.sum()))
    assert s["G"][0, 0, 1] == 1.0
    assert s["z"][0, 0, 1] > 8.0 and s["z"][0, 1, 0] > 8.0
    # one labelling of the null's own kind, outside the 200: nothing stands out
    other = NN.perm_counts(x, y, labels, 3, r2, 0, 0, 200, 1)[0]
    zo = nearest.statistics(other, null, present)["z"]
    fo = np.isfinite(zo)
    print("permuted labelling: largest |z|", np.abs(zo[fo]).max(), "over", int(fo.sum()), "finite entries")
    assert fo.any() and (np.abs(zo[fo]) < 4.5).all()
