"""The host side of the marker localisation (no GPU): the restated depth against scipy's exact Euclidean distance transform per label, every
formula of localization.features against plain loops -- empty compartments, deepest == -1, cells without a pixel, edge + inner == 0 --, the CSV
texts against hand-written expectations, and the refusal of a band that is no shell edge."""
import math

import numpy as np
import pytest

import expand_numpy as EN
import localization_numpy as LN
from multiplexed_image_annotator_amd import localization as L


@pytest.mark.parametrize("seed, shape, d", [(0, (37, 45), 1), (0, (37, 45), 5), (1, (20, 70), 8), (2, (33, 33), 32), (3, (40, 40), 3)])
def test_the_restated_depth_is_scipy_s_distance_transform_per_label(seed, shape, d):
    from scipy import ndimage
    mask = EN.random_discs(shape[0], shape[1], 14, seed, rmax=9.0)
    mask[3:9, 5:30] = -4      # negative pixels are background
    got = LN.depth(mask, d)
    assert got.dtype == np.int32 and not got[mask <= 0].any() and (got[mask > 0] != 0).all()
    seen_far = False
    for label in np.unique(mask[mask > 0]):
        own = mask == label
        if own.all():
            continue
        exact = np.rint(ndimage.distance_transform_edt(own) ** 2).astype(np.int64)      # nothing outside the image is a feature for scipy either
        near = own & (got != -1)
        assert np.array_equal(got[near], exact[near]) and (got[near] <= d * d).all()
        far = own & (got == -1)
        assert (exact[far] > d * d).all()
        seen_far |= bool(far.any())
    assert seen_far or d > 3      # discs of radius up to 9: some pixel lies deeper than 3
    assert not seen_far or d < 32


def test_the_restated_depth_on_cases_written_by_hand():
    mask = np.full((5, 7), 3, dtype=np.int32)
    assert (LN.depth(mask, 32) == -1).all()      # one label over the image: nothing differs, the border is no edge
    mask[2, 3] = 0      # a hole of one pixel
    want = np.array([[(r - 2) ** 2 + (c - 3) ** 2 for c in range(7)] for r in range(5)])
    assert np.array_equal(LN.depth(mask, 32), want)
    assert np.array_equal(LN.depth(mask, 2), np.where(want <= 4, want, -1))
    seam = np.array([[1, 1, 1, 2, 2, 2, 2]], dtype=np.int32)      # two labels, no background between them: the neighbour is the edge
    assert LN.depth(seam, 3).tolist() == [[9, 4, 1, 1, 4, 9, -1]]


def _case():
    """five cells over two markers: both compartments; edge only; inner only (deepest == -1); no pixel; means that cancel"""
    count = np.array([[4, 3, 2, 1, 0, 0, 0], [5, 2, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 9], [0, 0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 2, 0, 0]], dtype=np.int32)
    deepest = np.array([16, 4, -1, 0, 25], dtype=np.int32)
    rng = np.random.default_rng(3)
    sums = rng.normal(0.0, 3.0, size=(5, 2, 7)) * (count[:, None, :] > 0)
    sums[4, 0] = (-2.0, 0, 0, 0, -2.0, 0, 0)      # raw means -1 and -1: reported 0 and 0, edge + inner == 0
    sums[4, 1] = (-3.0, 0, 0, 0, 1.0, 0, 0)       # raw means -1.5 and 0.5: reported -0.25 and 0.75
    return count, deepest, sums


@pytest.mark.parametrize("band", L.EDGES)
def test_features_are_the_plain_loops(band):
    count, deepest, sums = _case()
    got, want = L.features(count, deepest, sums, band), LN.features(count, deepest, sums, band, L.EDGES)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].astype(got[key].dtype).tobytes(), (band, key)


def test_features_on_the_special_cells():
    count, deepest, sums = _case()
    f = L.features(count, deepest, sums, 2)
    assert f["edge_area"].tolist() == [7, 7, 0, 0, 2] and f["inner_area"].tolist() == [3, 0, 9, 0, 2] and f["area"].tolist() == [10, 7, 9, 0, 4]
    assert f["inradius"][0] == 4.0 and f["inradius"][1] == 2.0 and math.isinf(f["inradius"][2]) and math.isnan(f["inradius"][3]) and f["inradius"][4] == 5.0
    assert f["edge"][0, 0] == ((sums[0, 0, 0] + sums[0, 0, 1]) / 7.0 + 1.0) / 2.0
    assert f["inner"][0, 1] == ((sums[0, 1, 2] + sums[0, 1, 3]) / 3.0 + 1.0) / 2.0      # the empty shells add 0.0
    assert np.isfinite(f["contrast"][0]).all()
    assert np.isfinite(f["edge"][1]).all() and np.isnan(f["inner"][1]).all() and np.isnan(f["contrast"][1]).all()      # no inner compartment
    assert np.isnan(f["edge"][2]).all() and np.isfinite(f["inner"][2]).all() and np.isnan(f["contrast"][2]).all()      # no edge compartment
    assert np.isnan(f["edge"][3]).all() and np.isnan(f["inner"][3]).all() and np.isnan(f["contrast"][3]).all()
    assert f["edge"][4, 0] == 0.0 and f["inner"][4, 0] == 0.0 and math.isnan(f["contrast"][4, 0])      # edge + inner == 0
    assert f["edge"][4, 1] == -0.25 and f["inner"][4, 1] == 0.75 and f["contrast"][4, 1] == -2.0
    wide = L.features(count, deepest, sums, 8)      # every shell but the last is edge: cell 0 has no inner compartment left
    assert wide["edge_area"].tolist() == [10, 7, 0, 0, 4] and np.isnan(wide["contrast"][[0, 1, 3, 4]]).all()


@pytest.mark.parametrize("band", [0, 5, 7, 9, -1, 2.0, "2", True, None])
def test_a_band_that_is_no_shell_edge_is_refused(band):
    count, deepest, sums = _case()
    with pytest.raises(ValueError, match="band"):
        L.features(count, deepest, sums, band)
    with pytest.raises(ValueError, match="band"):
        L.check_band(band)


def test_constants_and_shapes():
    from multiplexed_image_annotator_amd import _lib
    assert _lib.lib().ribca_version() >= 113 and "ribca_mask_depth" in _lib.SIGNATURES and "ribca_cell_shell_sums" in _lib.SIGNATURES
    assert L.EDGES == (1, 2, 3, 4, 6, 8) and L.DEPTH == 8 and L.edges2().tolist() == [1, 4, 9, 16, 36, 64] and L.edges2().dtype == np.int32
    assert L.shell_names() == ["<=1", "<=2", "<=3", "<=4", "<=6", "<=8", ">8"]
    count, deepest, sums = _case()
    with pytest.raises(ValueError):
        L.features(count[:, :6], deepest, sums, 2)
    with pytest.raises(ValueError):
        L.features(count, deepest, sums[:4], 2)
    idx = L.colour_index(np.array([-1.0, 0.0, 1.0, np.nan, -3.0, 2.0, 0.5]))
    assert idx.dtype == np.uint8 and idx.tolist() == [0, 127, 255, 0, 0, 255, 191]


def test_csv_texts():
    count = np.array([[2, 0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0]], dtype=np.int32)
    deepest = np.array([-1, 0, 4], dtype=np.int32)
    sums = np.zeros((3, 1, 7))
    sums[0, 0, 0], sums[0, 0, 6] = 2.0, -1.0      # raw means 1 and -0.5: reported 1 and 0.25
    sums[2, 0, 0], sums[2, 0, 1] = 0.0, 1.0       # raw mean 0.5 over the two edge pixels: reported 0.75
    f = L.features(count, deepest, sums, 2)
    text = L.cells_csv([5, 9, 12], [1, 0, 7], ["T", "B"], ["CD3"], f)
    assert text == ("id,cell type,area,inradius,edge_area,inner_area,CD3_edge,CD3_inner,CD3_contrast\n"
                    "5,B,4,>8,2,2,1,0.25,0.59999999999999998\n"
                    "9,T,0,,0,0,nan,nan,nan\n"
                    "12,,2,2,2,0,0.75,nan,nan\n")
    assert L.cells_csv([], [], ["T"], ["CD3"], L.features(count[:0], deepest[:0], sums[:0], 2)).count("\n") == 1
    pixels, mean = L.profile([1, 0, 1], 2, count, sums)
    assert pixels.tolist() == [[0] * 7, [3, 1, 0, 0, 0, 0, 2]]
    assert mean[1, 0, 0] == (2.0 / 3.0 + 1.0) / 2.0 and mean[1, 0, 1] == 1.0 and mean[1, 0, 6] == 0.25 and np.isnan(mean[0]).all() and np.isnan(mean[1, 0, 2:6]).all()
    text = L.profile_csv(["T", "B"], ["CD3"], pixels, mean)
    rows = text.split("\n")
    assert rows[0] == "cell_type,marker,shell,pixels,mean" and len(rows) == 1 + 2 * 7 + 1
    assert rows[1] == "T,CD3,<=1,0,nan" and rows[8] == f"B,CD3,<=1,3,{(2.0 / 3.0 + 1.0) / 2.0:.17g}" and rows[9] == "B,CD3,<=2,1,1" and rows[14] == "B,CD3,>8,2,0.25"
    contrast = np.array([[0.5], [np.nan], [-0.25], [0.25]])
    s = L.summary([0, 0, 0, 1], 3, contrast)
    assert s[0, 0].tolist() == [3.0, 1.0, 0.125, 0.125] and s[1, 0].tolist() == [1.0, 0.0, 0.25, 0.25] and s[2, 0, :2].tolist() == [0.0, 0.0] and np.isnan(s[2, 0, 2:]).all()
    assert L.summary_csv(["a", "b", "c"], ["m"], s) == ("cell_type,marker,n,n_nan,mean_contrast,median_contrast\n"
                                                       "a,m,3,1,0.125,0.125\nb,m,1,0,0.25,0.25\nc,m,0,0,nan,nan\n")
    assert L.matrix_csv(["a", "b", "c"], ["m"], s[:, :, 3]) == "cell_type,m\na,0.125\nb,0.25\nc,nan\n"
