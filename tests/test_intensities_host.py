"""Cell intensities without a GPU: the version, every refusal of ribca_cell_intensities (a status whose text names the entry point, before any HIP
call), the two forms of the restatement against each other (tests/intensities_numpy.py), the restatement and the host module against numpy's own
mean / std / quantile / min / max within bounds derived below, the CSV writers, the colour indices, the comparison with the window table and the
command-line switch."""
import ctypes
import math
import types
from fractions import Fraction

import numpy as np
import pytest

import intensities_numpy as IN
from multiplexed_image_annotator_amd import _lib, intensities, ops

CAP = 1 << 21
U = 2.0 ** -53      # the unit roundoff of fp64


def test_version():
    assert _lib.lib().ribca_version() >= 108
    assert ops.INTENSITY_RESIDENT == 4096 and ops.INTENSITY_SMALL_BOX == 1024


def test_refusals_are_a_status_naming_the_entry_point():
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)      # never dereferenced: every case below is refused by its sizes, before any HIP call
    name = "ribca_cell_intensities"
    quartiles = (ctypes.c_int32 * 8)(0, 1, 2, 3, 4, 0, 0, 0)      # q_num is a host array: the entry point reads it

    def refused(status, text):
        assert status == 1
        msg = lib.ribca_last_error()
        assert msg and msg.startswith(text.encode()), (text, msg)

    def call(image=p, C=3, H=64, W=64, mask=p, ids=p, bbox=p, n=9, q_num=quartiles, Q=5, q_den=4, area=p, sums=p, order=p):
        q = ctypes.addressof(q_num) if q_num is not None else None
        return lib.ribca_cell_intensities(image, C, H, W, mask, ids, bbox, n, q, Q, q_den, area, sums, order, None)

    for hole in ("image", "mask", "ids", "bbox", "q_num", "area", "sums", "order"):
        refused(call(**{hole: None}), f"{name}: NULL buffer")
    refused(call(C=0), f"{name}: needs 1 <= C <= 64")
    refused(call(C=65), f"{name}: needs 1 <= C <= 64")
    sizes = f"{name}: needs 1 <= H, W <= 65535 and H W < 2^31"
    refused(call(H=0), sizes)
    refused(call(W=0), sizes)
    refused(call(H=65536, W=1), sizes)
    refused(call(H=1, W=65536), sizes)
    refused(call(H=65535, W=32769), sizes)      # H W = 2^31 + 32767
    refused(call(H=1 << 15, W=1 << 16), sizes)
    refused(call(n=-1), f"{name}: needs 1 <= n <= 2^21")
    refused(call(n=CAP + 1), f"{name}: needs 1 <= n <= 2^21")
    refused(call(Q=0), f"{name}: needs 1 <= Q <= 8")
    refused(call(Q=9), f"{name}: needs 1 <= Q <= 8")
    refused(call(q_den=0), f"{name}: needs 1 <= q_den")
    refused(call(q_den=3), f"{name}: needs 0 <= q_num[k] <= q_den")      # 4 / 3
    refused(call(q_num=(ctypes.c_int32 * 8)(0, -1, 2, 3, 4, 0, 0, 0)), f"{name}: needs 0 <= q_num[k] <= q_den")
    assert call(n=0) == 0      # nothing to do, nothing touched
    assert call(n=0, image=None, q_num=None) == 0


def _case():
    mask = IN.generated_mask()
    ids = np.array([1, 2, 3, 4, 5, 6, 7, 20, 39, 40, 0, -3], dtype=np.int32)
    bbox = IN.boxes_of(mask, ids)
    return mask, ids, bbox


def test_the_generated_mask_has_the_sizes_the_cases_name():
    mask, ids, bbox = _case()
    assert mask.shape == (100, 130)
    assert int((mask == 1).sum()) == ops.INTENSITY_RESIDENT and int((mask == 2).sum()) == ops.INTENSITY_RESIDENT + 1
    assert int((mask == 3).sum()) == 1 and int((mask == 40).sum()) == 0 and int((mask == 39).sum()) == 15 and mask[99, 129] == 39
    r0, r1, c0, c1 = bbox[3]      # label 4: two blobs, and other cells inside its box
    inside = mask[r0:r1 + 1, c0:c1 + 1]
    assert {5, 6, 0} <= set(np.unique(inside).tolist()) and int((inside == 4).sum()) == 25 + 28


def test_the_two_forms_of_the_restatement_agree():
    mask, ids, bbox = _case()
    image = IN.generated_image(3, 100, 130)
    bbox = bbox.copy()
    bbox[4] = (bbox[4][0] - 50, bbox[4][1] + 200, bbox[4][2] - 7, bbox[4][3] + 500)      # a box that reaches past the image: clipped
    for q_num, q_den in (((0, 1, 2, 3, 4), 4), ((0, 7, 3, 3, 1, 0, 7, 5), 7), ((1,), 2)):
        a0, s0, o0 = IN.direct(image, mask, ids, bbox, q_num, q_den)
        a1, s1, o1 = IN.arrays(image, mask, ids, bbox, q_num, q_den)
        assert np.array_equal(a0, a1) and np.array_equal(s0.view(np.int64), s1.view(np.int64)) and np.array_equal(o0.view(np.int32), o1.view(np.int32))
        assert a0.tolist()[:6] == [4096, 4097, 1, 53, 55, 60] and a0.tolist()[-3:] == [0, 0, 0]
        assert (o0.view(np.uint32)[-3:] == IN.NAN_BITS).all() and not s0[-3:].any()
    # the key orders -0.0 below +0.0 and keeps every bit pattern
    v = np.array([0.0, -0.0, 1e-45, -1e-45, -np.inf, np.inf, 1.0, -1.0], dtype=np.float32)
    back = IN.from_key(np.sort(IN.to_key(v)))
    assert back.view(np.uint32).tolist() == np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], dtype=np.float32).view(np.uint32).tolist()
    assert IN.ranks(5, (0, 1, 2, 3, 4), 4) == [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)]
    assert IN.ranks(4, (0, 1, 2, 3, 4), 4) == [(0, 0), (0, 1), (1, 2), (2, 3), (3, 3)] and IN.ranks(1, (0, 3, 7), 7) == [(0, 0)] * 3


def test_the_restatement_against_numpy_within_derived_bounds():
    """Bounds, with u = 2^-53 and v the a values of a cell in fp64 (exact: they are fp32 values):

    * sum: any order of a - 1 additions differs from the exact sum by at most (a - 1) u S, S = sum |v| (first order); the tree and numpy's
      own sum are two such orders, so they differ by at most 2 (a - 1) u S; the means add one rounded division each: + 2 u |mean|.
    * ssd, against exact rational arithmetic on the restatement's own mean m: d = v - m and d * d are three roundings relative to d^2 (two of
      them through the square), the tree a - 1 more: (a + 2) u sum d^2, to first order; 1.01 covers the second-order terms at these sizes.
      np.std is compared through that exact value: its own mean differs from m by delta, which moves sum d^2 by at most 2 delta sum |d| + a
      delta^2, and its own roundings are bounded like the tree's; the division and the root add two roundings each side: 4 u std.
    * a quantile: features' formula lo + (hi - lo) * rest / q_den has four roundings, numpy's lerp three (its weight is exact at q_den = 4 and
      a - 1 below 2^51), every intermediate is at most max(|lo|, |hi|) in size up to the weight: 7 u max(|lo|, |hi|).  At q_den = 7 numpy's own
      weight q (a - 1) is rounded, an error that grows with a, so that case is held against exact rational arithmetic of the formula instead:
      4 u max(|lo|, |hi|)."""
    mask, ids, bbox = _case()
    image = IN.generated_image(2, 100, 130, seed=11)
    ids, bbox = ids[[0, 3, 5, 6, 8]], bbox[[0, 3, 5, 6, 8]]
    area, sums, order = IN.arrays(image, mask, ids, bbox)
    feat = intensities.features(area, sums, order)
    assert intensities.statistic_names() == ["mean", "std", "min", "q25", "median", "q75", "max"]
    q7 = (0, 1, 2, 3, 5, 7)
    area7, sums7, order7 = IN.arrays(image, mask, ids, bbox, q7, 7)
    feat7 = intensities.features(area7, sums7, order7, q7, 7)
    for i, label in enumerate(ids):
        for c in range(image.shape[0]):
            v = image[c][mask == label].astype(np.float64)
            a = len(v)
            assert a == area[i]
            s_abs = float(np.abs(v).sum())
            total, ssd = sums[i, c]
            assert abs(total - math.fsum(v)) <= (a - 1) * U * s_abs
            mean = total / a
            mean_tol = 2 * (a - 1) * U * s_abs / a + 2 * U * abs(mean)
            assert abs(mean - np.mean(v)) <= mean_tol
            exact = sum((Fraction(x) - Fraction(mean)) ** 2 for x in v.tolist())
            ssd_tol = 1.01 * (a + 2) * U * float(exact)
            assert abs(Fraction(ssd) - exact) <= Fraction(ssd_tol)
            delta = abs(mean - float(np.mean(v)))
            moved = 2 * delta * float(np.abs(v - mean).sum()) + a * delta * delta
            std, std_np = math.sqrt(ssd / a), float(np.std(v))
            std_tol = (2 * ssd_tol + moved) / a / (std + std_np) + 4 * U * std if std + std_np > 0 else 0.0
            assert abs(std - std_np) <= std_tol
            # the reported scale: (x + 1) / 2 and std / 2, two more roundings of values of about that size
            assert abs(feat[i, c, 0] - (np.mean(v) + 1) / 2) <= mean_tol / 2 + 2 * U * abs(feat[i, c, 0])
            assert abs(feat[i, c, 1] - np.std(v) / 2) <= std_tol / 2      # halving is exact
            assert feat[i, c, 2] == (v.min() + 1) / 2 and feat[i, c, 6] == (v.max() + 1) / 2
            for k, q in enumerate((0.0, 0.25, 0.5, 0.75, 1.0)):
                lo, hi = (float(x) for x in order[i, c, k])
                want = float(np.quantile(v, q))
                tol = 7 * U * max(abs(lo), abs(hi))
                assert abs(feat[i, c, 2 + k] - (want + 1) / 2) <= tol / 2 + 2 * U * abs(feat[i, c, 2 + k]), (label, c, q, want)
            for k, num in enumerate(q7):
                lo, hi = (Fraction(float(x)) for x in order7[i, c, k])
                rest = ((a - 1) * num) % 7
                exact_q = lo + (hi - lo) * rest / 7
                tol = 4 * U * max(abs(float(lo)), abs(float(hi)))
                assert abs(Fraction(float(feat7[i, c, 2 + k])) - (exact_q + 1) / 2) <= Fraction(tol / 2 + 2 * U * abs(float(feat7[i, c, 2 + k])))


def test_features_of_hand_written_cases():
    area = np.array([4, 0, 1], dtype=np.int32)
    sums = np.array([[[2.0, 5.0]], [[0.0, 0.0]], [[-1.0, 0.0]]])
    order = np.zeros((3, 1, 5, 2), dtype=np.float32)
    order[0, 0] = [(-1, -1), (-1, 0), (0, 1), (1, 2), (2, 2)]      # values -1, 0, 1, 2: ranks 0, 0.75, 1.5, 2.25, 3
    order[1] = np.nan
    order[2] = -1.0
    f = intensities.features(area, sums, order)
    assert f.shape == (3, 1, 7)
    assert f[0, 0].tolist() == [(0.5 + 1) / 2, math.sqrt(5.0 / 4) / 2, 0.0, (-0.25 + 1) / 2, (0.5 + 1) / 2, (1.25 + 1) / 2, 1.5]
    assert np.isnan(f[1]).all()
    assert f[2, 0].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    inf = np.full((1, 1, 5, 2), np.inf, dtype=np.float32)
    assert intensities.features([5], np.zeros((1, 1, 2)), inf)[0, 0, 2:].tolist() == [np.inf] * 5      # a whole rank: lo itself, no inf - inf
    assert intensities.statistic_names((0, 1, 3, 7), 7) == ["mean", "std", "min", "q1of7", "q3of7", "max"]
    assert intensities.features(np.zeros(0, np.int32), np.zeros((0, 2, 2)), np.zeros((0, 2, 5, 2), np.float32)).shape == (0, 2, 7)
    with pytest.raises(ValueError, match="features takes"):
        intensities.features(area, sums, order[:, :, :4])


def test_the_csv_writers():
    names = ["B cell", "T cell"]
    markers = ["CD3", "HLA-DR"]
    stats = ["mean", "max"]
    feat = np.array([[[0.5, 1.0], [0.25, 0.75]], [[np.nan, np.nan], [np.nan, np.nan]], [[0.125, 0.5], [1.0, 1.0]]])
    text = intensities.cells_csv([3, 5, 9], [1, 0, 7], names, [12, 0, 2], markers, stats, feat)
    assert text == ("id,cell type,area,CD3_mean,CD3_max,HLA-DR_mean,HLA-DR_max\n"
                    "3,T cell,12,0.5,1,0.25,0.75\n"
                    "5,B cell,0,nan,nan,nan,nan\n"
                    "9,,2,0.125,0.5,1,1\n")
    with pytest.raises(ValueError, match="cells_csv takes"):
        intensities.cells_csv([3, 5], [1, 0, 7], names, [12, 0, 2], markers, stats, feat)
    types_ = np.array([0, 0, 0, 1, 1, 0])
    means = np.array([[0.1, 1.0], [0.3, 1.0], [0.8, 1.0], [0.5, 0.0], [0.7, 0.5], [np.nan, np.nan]])
    medians = means * 0.5
    s = intensities.type_summary(types_, 3, means, medians)
    assert s.shape == (3, 2, 4)
    assert s[0, 0].tolist() == [3.0, (0.1 + 0.3 + 0.8) / 3, 0.3, 0.15] and s[1, 1].tolist() == [2.0, 0.25, 0.25, 0.125]
    assert s[2, 0, 0] == 0 and np.isnan(s[2, :, 1:]).all()
    text = intensities.summary_csv(["A", "B"], markers, s[:2])
    assert text.splitlines()[0] == "cell_type,marker,n,mean_of_means,median_of_means,median_of_medians"
    assert text.splitlines()[1] == f"A,CD3,3,{(0.1 + 0.3 + 0.8) / 3:.17g},{0.3:.17g},{0.15:.17g}" and len(text.splitlines()) == 5
    # CD3 over all cells: median 0.5, |x - 0.5| = .4 .2 .3 0 .2 -> MAD 0.2; HLA-DR: median 1.0, MAD 0 -> 0
    z = intensities.standardised_medians(types_, 3, means)
    assert z[0, 0] == (0.3 - 0.5) / (1.4826 * np.median(np.abs(means[:5, 0] - 0.5))) and z[1, 0] == (0.6 - 0.5) / (1.4826 * np.median(np.abs(means[:5, 0] - 0.5)))
    assert z[:2, 1].tolist() == [0.0, 0.0] and np.isnan(z[2]).all()
    assert intensities.matrix_csv(["A", "B"], markers, np.array([[1.0, -0.5], [np.nan, 0.0]])) == "cell_type,CD3,HLA-DR\nA,1,-0.5\nB,nan,0\n"
    assert intensities.file_slug("HLA-DR (1)") == "HLA_DR__1_" and intensities.file_slug("CD3") == "CD3"
    assert intensities.Z_LIMIT == 3.0


def test_the_colour_indices_of_the_maps():
    assert intensities.colour_index(np.array([0.0, 0.25, 0.5, 0.999, 1.0, 7.0, -2.0, np.nan])).tolist() == [0, 63, 127, 254, 255, 255, 0, 0]
    assert intensities.colour_index(np.zeros(0)).shape == (0,)


def test_vs_window_on_planted_columns():
    rng = np.random.default_rng(3)
    exact = rng.random((50, 4))
    window = exact.copy()
    window[:, 1] = exact[:, 1] + 0.25             # shifted: r = 1, difference 0.25
    window[:, 2] = 1.0 - exact[:, 2]              # mirrored: r = -1
    exact[:, 3] = 0.5                             # constant on one side: no r
    exact[7] = np.nan                             # a cell without a pixel drops out
    t = intensities.vs_window(exact, window)
    assert t.shape == (4, 3)
    assert t[0, 0] == pytest.approx(1.0, abs=1e-15) and t[0, 1] == 0.0 and t[0, 2] == 0.0
    assert t[1, 0] == pytest.approx(1.0, abs=1e-12) and t[1, 1] == pytest.approx(0.25, abs=1e-15) and t[1, 2] == pytest.approx(0.25, abs=1e-15)
    assert t[2, 0] == pytest.approx(-1.0, abs=1e-12)
    keep = np.arange(50) != 7
    assert np.isnan(t[3, 0]) and t[3, 2] == np.abs(0.5 - window[keep, 3]).max()
    assert np.isnan(intensities.vs_window(np.full((3, 1), np.nan), np.zeros((3, 1)))).all()
    text = intensities.vs_window_csv(["a", "b"], np.array([[1.0, 0.0, 0.0], [np.nan, 0.5, 0.75]]))
    assert text == "marker,pearson_r,mean_abs_difference,max_abs_difference\na,1,0,0\nb,nan,0.5,0.75\n"
    with pytest.raises(ValueError, match="vs_window takes"):
        intensities.vs_window(exact, window[:, :3])


def test_the_command_line_switch():
    """--intensities is off by default; the pipeline calls the method only with it, after cell_morphology and before colorize; the parameter stands
    directly after ``morphology``"""
    import inspect
    import main as cli
    common = ["--marker-list-path", "m.txt", "--image-path", "i.npy", "--mask-path", "k.npy", "--batch-id", "c"]
    assert cli.parse_args(common).intensities is False
    assert cli.parse_args(common + ["--intensities"]).intensities is True

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
    assert "cell_intensities" not in [c[0] for c in off.calls]
    on = Recorder()
    cli._pipeline(on, 16, 0, intensities=True)
    got = [c for c in on.calls if c[0] == "cell_intensities"]
    assert len(got) == 1 and got[0][2] == {"integrate": True}
    assert [c[0] for c in on.calls if c[0] != "cell_intensities"] == [c[0] for c in off.calls]      # with the flag off the sequence is unchanged
    both = Recorder()
    cli._pipeline(both, 16, 0, contact_distance=1, morphology=True, intensities=True)
    order = [c[0] for c in both.calls]
    assert order.index("contact_analysis") < order.index("cell_morphology") < order.index("cell_intensities") < order.index("colorize")
    for fn in (cli._pipeline, cli.run, cli.batch_run):
        params = list(inspect.signature(fn).parameters)
        assert inspect.signature(fn).parameters["intensities"].default is False
        at = params.index("intensities")
        assert params[at - 1] == "morphology" and params[at + 1] == "contact_distance"


def test_cell_intensities_needs_annotations():
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = object.__new__(Annotator)
    a.tile_mode = False
    a.annotations = []
    a.cell_types = ["A", "B"]
    with pytest.raises(ValueError, match="No annotations"):
        a.cell_intensities()
    assert not hasattr(a, "intensity_stats")
