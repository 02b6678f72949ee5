"""Host side of the co-occurrence by distance (multiplexed_image_annotator_amd/cooccurrence.py, tests/cooccurrence_numpy.py): the lift on a
hand-made count tensor, NaN for zero marginals, exactness beyond int64 against fractions.Fraction, the cumulative form, the CSV text, the file-name
slug, the default radii, the numpy oracle on a case counted by hand, and the argument checks of the two new entry points (they run before any HIP
call: no GPU needed)."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import cooccurrence_numpy as CO
from multiplexed_image_annotator_amd import _lib, cooccurrence, ops


def test_lift_on_a_hand_made_tensor():
    # band 0: rows R = (6, 4), S = 10; band 1: independent types (an outer product), every lift 1
    n = np.array([[[4, 2], [2, 2]], [[9, 6], [6, 4]]], dtype=np.int64)
    got = cooccurrence.lift(n)
    assert got[0].tolist() == [[4 * 10 / 36, 2 * 10 / 24], [2 * 10 / 24, 2 * 10 / 16]]
    assert (got[1] == 1.0).all()
    tot = cooccurrence.band_totals(n)
    assert tot["rows"].tolist() == [[6, 4], [15, 10]] and tot["total"].tolist() == [10, 25]
    assert got.tobytes() == CO.lift(n).tobytes()
    values = cooccurrence.figure_values(n, got)
    assert values[1].tolist() == [[0.0, 0.0], [0.0, 0.0]] and abs(values[0, 0, 0] - math.log2(40 / 36)) < 1e-15
    for bad in (np.zeros((2, 2), dtype=np.int64), np.zeros((1, 2, 3), dtype=np.int64), np.zeros((1, 2, 2))):
        with pytest.raises(ValueError):
            cooccurrence.lift(bad)


def test_zero_marginals_are_nan_and_zero_counts_have_no_figure_value():
    n = np.array([[[0, 3, 0], [3, 2, 0], [0, 0, 0]], [[0, 0, 0], [0, 0, 0], [0, 0, 0]]], dtype=np.int64)
    got = cooccurrence.lift(n)
    assert np.isnan(got[0, 2]).all() and np.isnan(got[0, :, 2]).all() and np.isnan(got[1]).all()
    assert got[0, 0, 0] == 0.0 and got[0, 0, 1] == 3 * 8 / (3 * 5) and got[0, 1, 1] == 2 * 8 / 25
    values = cooccurrence.figure_values(n, got)
    assert np.isnan(values[0, 0, 0]) and np.isnan(values[1]).all() and abs(values[0, 0, 1] - math.log2(got[0, 0, 1])) < 1e-15      # no log2(0) = -inf
    assert np.isfinite(values[n > 0]).all() and np.isnan(values[n == 0]).all()
    assert got.tobytes() == CO.lift(n).tobytes()


def test_counts_near_2_to_the_40_stay_exact():
    big = 2 ** 40
    n = np.array([[[big + 1, big - 3], [big - 3, big + 7]]], dtype=np.int64)
    rows = [2 * big - 2, 2 * big + 4]
    assert (big + 1) * sum(rows) > 2 ** 63      # the numerator does not fit int64
    got = cooccurrence.lift(n)
    for a in range(2):
        for c in range(2):
            assert got[0, a, c] == float(Fraction(int(n[0, a, c]) * sum(rows), rows[a] * rows[c])), (a, c)
    assert got[0, 0, 0] != got[0, 0, 1] and got.tobytes() == CO.lift(n).tobytes()
    # uint64 counts, as the device tensor holds them
    assert cooccurrence.lift(n.astype(np.uint64)).tobytes() == got.tobytes()


def test_cumulative_form_is_the_band_form_of_the_merged_bands():
    rng = np.random.RandomState(3)
    half = rng.randint(0, 50, (4, 3, 3))
    n = half + half.transpose(0, 2, 1)      # symmetric band matrices
    cum = cooccurrence.cumulative_counts(n)
    assert [[int(v) for v in cum[b].ravel()] for b in range(4)] == [n[:b + 1].sum(axis=0).ravel().tolist() for b in range(4)]
    got = cooccurrence.cumulative_lift(n)
    for b in range(4):
        merged = n[:b + 1].sum(axis=0)[None]
        assert got[b].tobytes() == cooccurrence.lift(merged)[0].tobytes(), b
    assert got[0].tobytes() == cooccurrence.lift(n)[0].tobytes()


def test_csv_text_of_a_tiny_case():
    n = np.array([[[0, 1], [1, 2]], [[2, 0], [0, 0]]], dtype=np.int64)
    text = cooccurrence.table_csv(["a", "b c"], [1.5, 4.0], n)
    assert text == ("band,r_lo,r_hi,cell_type,neighbor_type,count,lift,cum_count,cum_lift\n"
                    "0,0.0,1.5,a,a,0,0.0,0,0.0\n"
                    "0,0.0,1.5,a,b c,1,1.3333333333333333,1,1.3333333333333333\n"
                    "0,0.0,1.5,b c,a,1,1.3333333333333333,1,1.3333333333333333\n"
                    "0,0.0,1.5,b c,b c,2,0.8888888888888888,2,0.8888888888888888\n"
                    "1,1.5,4.0,a,a,2,1.0,2,1.3333333333333333\n"
                    "1,1.5,4.0,a,b c,0,nan,1,0.6666666666666666\n"
                    "1,1.5,4.0,b c,a,0,nan,1,0.6666666666666666\n"
                    "1,1.5,4.0,b c,b c,0,nan,2,1.3333333333333333\n")
    assert text == CO.table_csv(["a", "b c"], [1.5, 4.0], n)
    with pytest.raises(ValueError):
        cooccurrence.table_csv(["a"], [1.5, 4.0], n)


def test_slug_and_default_radii_and_radius_checks():
    assert cooccurrence.slug("Proliferating/tumor cell") == "Proliferating_tumor_cell"
    assert cooccurrence.slug("CD4 T cell") == "CD4_T_cell" and cooccurrence.slug("a-b.c/é") == "a_b_c__"
    r = cooccurrence.default_radii(30)
    assert r.dtype == np.float64 and r.tolist() == [30.0 * k for k in range(1, 17)]
    assert cooccurrence.default_radii(7.5, 3).tolist() == [7.5, 15.0, 22.5]
    assert cooccurrence.check_radii([0.0, 1.0], 32).tolist() == [0.0, 1.0]
    for bad in ([], list(range(1, 34)), [1.0, 1.0], [2.0, 1.0], [-1.0, 1.0], [1.0, float("nan")], [1.0, float("inf")], [1e200, 1e201]):
        with pytest.raises(ValueError):
            cooccurrence.check_radii(bad, 32)
    assert ops.RADIAL_MAX_BANDS == 32 and ops.RADIAL_MAX_CELLS == 2 ** 21


def test_the_oracle_counts_a_case_done_by_hand():
    """four cells on a line at 0, 1, 3 and 3 (a duplicate), labels 0, 1, 0 and one outside: r2 = (0, 1, 4): band 0 holds d2 = 0 only, the edge d2 = 1
    belongs to band 1, d2 = 4 to band 2, d2 = 9 to none"""
    x, y = np.array([0.0, 1.0, 3.0, 3.0]), np.zeros(4)
    got = CO.pair_counts(x, y, [0, 1, 0, 0], 2, [0.0, 1.0, 4.0])
    want = np.zeros((3, 2, 2), dtype=np.int64)
    want[0, 0, 0] = 2      # the duplicate pair, both orders
    want[1, 0, 1] = want[1, 1, 0] = 1      # 0 - 1
    want[2, 1, 0] = want[2, 0, 1] = 2      # 1 - 3, twice
    assert np.array_equal(got, want)
    got = CO.pair_counts(x, y, [0, 1, 0, 2], 2, [0.0, 1.0, 4.0], chunk=3)      # the fourth cell now carries no label
    want[0, 0, 0] = 0
    want[2, 1, 0] = want[2, 0, 1] = 1
    assert np.array_equal(got, want)
    assert CO.pair_counts(x[:1], y[:1], [0], 2, [1.0]).sum() == 0


def test_new_entry_points_refuse_bad_arguments_with_a_status():
    lib = _lib.lib()
    p = ctypes.c_void_p(4096)      # never dereferenced: the checks come first
    assert lib.ribca_radial_pair_counts_ws_bytes(100, 12, 16) == 0 and lib.ribca_radial_pair_counts_ws_bytes(0, 0, 0) == 0

    def edges(values):
        return (ctypes.c_double * len(values))(*values)

    good = edges([1.0, 4.0, 9.0])

    def call(x=p, y=p, types=p, n=100, t=12, r2=good, b=3, counts=p, ws=None, ws_bytes=0):
        return lib.ribca_radial_pair_counts(x, y, types, n, t, r2, b, counts, ws, ws_bytes, None)

    nan, inf = float("nan"), float("inf")
    radii = b"ribca_radial_pair_counts: the squared radii must be finite, non-negative and strictly increasing"
    for bad, text in ((lambda: call(x=None), b"ribca_radial_pair_counts: NULL buffer"),
                      (lambda: call(y=None), b"ribca_radial_pair_counts: NULL buffer"),
                      (lambda: call(types=None), b"ribca_radial_pair_counts: NULL buffer"),
                      (lambda: call(r2=None), b"ribca_radial_pair_counts: NULL buffer"),
                      (lambda: call(counts=None), b"ribca_radial_pair_counts: NULL buffer"),
                      (lambda: call(n=0), b"ribca_radial_pair_counts: needs 1 <= n <= 2^21"),
                      (lambda: call(n=-5), b"ribca_radial_pair_counts: needs 1 <= n <= 2^21"),
                      (lambda: call(n=2 ** 21 + 1), b"ribca_radial_pair_counts: needs 1 <= n <= 2^21"),
                      (lambda: call(t=0), b"ribca_radial_pair_counts: needs 1 <= T <= 254"),
                      (lambda: call(t=255), b"ribca_radial_pair_counts: needs 1 <= T <= 254"),
                      (lambda: call(b=0), b"ribca_radial_pair_counts: needs 1 <= B <= 32"),
                      (lambda: call(r2=edges([float(k) for k in range(33)]), b=33), b"ribca_radial_pair_counts: needs 1 <= B <= 32"),
                      (lambda: call(r2=edges([1.0, nan, 9.0])), radii),
                      (lambda: call(r2=edges([nan]), b=1), radii),
                      (lambda: call(r2=edges([1.0, 4.0, inf])), radii),
                      (lambda: call(r2=edges([-1.0, 4.0, 9.0])), radii),
                      (lambda: call(r2=edges([-0.5]), b=1), radii),
                      (lambda: call(r2=edges([1.0, 1.0, 9.0])), radii),
                      (lambda: call(r2=edges([4.0, 1.0, 9.0])), radii),
                      (lambda: call(ws_bytes=-1), b"ribca_radial_pair_counts: workspace too small")):
        assert bad() == 1
        assert lib.ribca_last_error() == text, (lib.ribca_last_error(), text)
