"""Host side of the cell-type heat map and composition pie (multiplexed_image_annotator_amd/plots.py, tests/celltype_numpy.py): the summation tree
against np.sum, the wedge order against arctan2, the dropped wedges, the legend and CSV texts, the look-up table, the index rule, and the argument
checks of the three entry points (they run before any HIP call: no GPU needed)."""
import ctypes

import numpy as np
import pytest

import celltype_numpy as CN
from multiplexed_image_annotator_amd import _lib, colors, ops, plots


def test_tree_oracle_agrees_with_np_sum_within_the_derived_bound():
    rng = np.random.RandomState(5)
    n, c, groups = 3 * CN.R + 7, 15, 5
    x = rng.randn(n, c) * 10.0 ** rng.uniform(-8, 8, (n, c))
    g = rng.randint(-1, groups + 1, n)
    sums, counts, skipped = CN.group_sums(x, g, groups)
    assert skipped == int(((g < 0) | (g >= groups)).sum()) and counts.sum() + skipped == n
    assert ops.GROUP_SUM_ROWS == CN.R
    for k in range(groups):
        rows = x[g == k]
        assert counts[k] == len(rows) > 0
        # both are fp64 sums of n_g terms in some order: each is within (n_g - 1) 2^-53 sum|x| of the exact sum
        bound = 2.0 * (len(rows) - 1) * 2.0 ** -53 * np.abs(rows).sum(axis=0)
        assert (np.abs(sums[k] - rows.sum(axis=0)) <= bound).all()
    # n = 0 and an empty group give +0.0
    s0, c0, k0 = CN.group_sums(np.zeros((0, 3)), np.zeros(0, dtype=np.int32), 4)
    assert s0.shape == (4, 3) and not s0.any() and not c0.any() and k0 == 0


def test_wedge_comparator_equals_arctan2_classification():
    counts = (5, 3, 0, 9)      # N = 17: no boundary passes through a pixel centre of the canvas, so the two must agree on every pixel
    kept, rays = plots.pie_wedges(counts)
    assert kept.tolist() == [0, 1, 3] and rays.shape == (2, 2)
    got = CN.pie_wedge_index(rays, 65, 30)
    want = CN.pie_wedge_index_by_angle(counts, 65, 30)
    centre = np.zeros((65, 65), dtype=bool)
    centre[32, 32] = True      # wedge 0 by rule
    assert np.array_equal(got[~centre], want[~centre]) and got[32, 32] == 0
    assert (got >= 0).sum() == (want >= 0).sum() > 2500 and set(np.unique(got)) == {-1, 0, 1, 2}
    # matplotlib's convention: the first wedge starts at 3 o'clock and runs counter-clockwise ON SCREEN (upwards first)
    assert got[32, 32 + 20] == 0 and got[32 - 10, 32 + 20] == 0 and got[32 + 10, 32 + 20] == 2


@pytest.mark.parametrize("counts,kept,m", [((0, 4, 4), [1, 2], 1), ((4, 0, 4), [0, 2], 1), ((4, 4, 0), [0, 1], 1), ((0, 7, 0), [1], 0),
                                           ((0, 0, 0), [], 0)])
def test_empty_wedges_are_dropped(counts, kept, m):
    k, rays = plots.pie_wedges(counts)
    assert k.tolist() == kept and rays.shape == (m, 2) and rays.dtype == np.float64
    if m == 1:      # two equal halves: the boundary at 9 o'clock, whichever wedge was empty
        assert rays[0, 0] == np.cos(np.pi) and rays[0, 1] == np.sin(np.pi)
        w = CN.pie_wedge_index(rays, 65, 30)
        assert (w[:32][w[:32] >= 0] == 0).all() and (w[33:][w[33:] >= 0] == 1).all()
    if kept == [1]:
        assert (CN.pie_wedge_index(rays, 65, 30).max() == 0)


def test_legend_texts():
    names, counts = ["B cell", "CD4 T cell", "Others"], [1, 0, 2]
    assert plots.legend_texts(names, counts, True) == ["B cell (33.33 %)", "CD4 T cell (0.00 %)", "Others (66.67 %)"]
    # the reference multiplies the raw count by 100 when reduction is off (model.py:876)
    assert plots.legend_texts(names, counts, False) == ["B cell (100.00 %)", "CD4 T cell (0.00 %)", "Others (200.00 %)"]
    for name, c, text in zip(names, counts, plots.legend_texts(names, counts, True)):
        v = c / 3
        assert text == f"{name} ({v * 100:.2f} %)"


def test_csv_formats():
    means = np.array([[0.1, 1.0 / 3.0], [2.0, 5e-324]])
    text = plots.heatmap_csv(["B cell", "Others"], ["CD20", "DAPI"], means, [3, 1])
    lines = text.split("\n")
    assert lines[0] == "cell_type,CD20,DAPI,cells" and lines[-1] == "" and len(lines) == 4
    assert lines[1] == "B cell,0.10000000000000001,0.33333333333333331,3"
    back = np.array([[float(v) for v in l.split(",")[1:-1]] for l in lines[1:3]])
    assert np.array_equal(back, means)      # 17 significant digits: the text is the doubles
    comp = plots.composition_csv(["B cell", "CD4 T cell", "Others"], [1, 0, 2])
    assert comp == "cell_type,cells,fraction\nB cell,1,0.33333333333333331\nCD4 T cell,0,0\nOthers,2,0.66666666666666663\n"
    assert plots.composition_csv(["Others"], [0]) == "cell_type,cells,fraction\nOthers,0,0\n"


def test_diverging_table():
    lut = colors.diverging_table()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert lut[0, 2] > lut[0, 0] and lut[255, 0] > lut[255, 2]      # blue end, red end
    assert lut[127].min() > 230      # near-white middle
    assert len({tuple(r) for r in lut.tolist()}) > 200


def test_index_rule_edges():
    means = np.array([[0.25, 0.5], [0.75, 1.0]])
    idx = CN.colour_index(means, 0.25, 1.0)
    assert idx.tolist() == [[0, 85], [170, 255]]      # the value equal to vmax: floor(256) clamps to 255
    assert CN.colour_index(np.full((2, 3), 0.7), 0.7, 0.7).tolist() == [[0, 0, 0], [0, 0, 0]]      # a constant table
    lut = colors.diverging_table()
    m = np.array([[1.0, 2.0], [np.nan, np.nan], [3.0, 1.5]])
    img, vmin, vmax = CN.heatmap_raster(m, lut, 4, 1)
    assert (vmin, vmax) == (1.0, 3.0) and img.shape == (12, 8, 3)
    assert (img[5, 1] == 192).all() and (img[4, 1] == 255).all() and (img[1, 1] == lut[0]).all() and (img[9, 2] == lut[255]).all()
    assert (img[9, 5] == lut[64]).all()
    img, vmin, vmax = CN.heatmap_raster(np.full((1, 1), np.nan), lut, 3, 0)
    assert np.isnan(vmin) and np.isnan(vmax) and (img == 192).all()


def test_figures_keep_the_rectangles_where_the_layout_says():
    lut = colors.diverging_table()
    rect = np.random.RandomState(0).randint(0, 255, (2 * 24, 3 * 24, 3)).astype(np.uint8)
    fig, lay = plots.heatmap_figure(rect, lut, 0.125, 0.875, ["B cell", "Proliferating/tumor cell"], ["CD20", "DAPI", "HLA-DR"], 24)
    arr = np.array(fig)
    assert arr.shape == (lay["height"], lay["width"], 3)
    assert np.array_equal(arr[lay["top"]:lay["top"] + 48, lay["left"]:lay["left"] + 72], rect)
    assert (arr[lay["top"]:lay["top"] + 48, :lay["left"]] != 255).any() and (arr[lay["top"] + 48:] != 255).any()      # labels were drawn
    bar = arr[lay["top"]:lay["top"] + 48, lay["left"] + 72 + plots.BAR_GAP]
    assert (bar[0] == lut[255]).all() and (bar[-1] == lut[255 - (47 * 256) // 48]).all()
    disc = np.full((65, 65, 3), 7, dtype=np.uint8)
    fig, lay = plots.pie_figure(disc, ["B cell (50.00 %)", "Others (50.00 %)"], [(255, 0, 0), (192, 192, 192)])
    arr = np.array(fig)
    assert np.array_equal(arr[lay["top"]:lay["top"] + 65, :65], disc) and arr.shape[1] > 65
    assert (arr[:, 65:] == (255, 0, 0)).all(axis=2).sum() >= 100 and (arr[:, 65:] == (192, 192, 192)).all(axis=2).sum() >= 100


def test_entry_points_refuse_bad_arguments_with_a_status():
    lib = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    sk, lo, hi = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0)
    for call, text in (
            (lambda: lib.ribca_group_sums(None, None, 5, 3, 4, p, p, ctypes.byref(sk), p, 1 << 20, None), b"ribca_group_sums: NULL buffer"),
            (lambda: lib.ribca_group_sums(p, p, -1, 3, 4, p, p, ctypes.byref(sk), p, 1 << 20, None), b"ribca_group_sums: needs 0 <= n < 2^31 - 1"),
            (lambda: lib.ribca_group_sums(p, p, 5, ops.GROUP_SUM_MAX_COLUMNS + 1, 4, p, p, ctypes.byref(sk), p, 1 << 20, None), b"ribca_group_sums: needs 1 <= c"),
            (lambda: lib.ribca_group_sums(p, p, 5, 3, ops.GROUP_SUM_MAX_GROUPS + 1, p, p, ctypes.byref(sk), p, 1 << 20, None), b"ribca_group_sums: needs 1 <= groups"),
            (lambda: lib.ribca_group_sums(p, p, 5, 3, 0, p, p, ctypes.byref(sk), p, 1 << 20, None), b"ribca_group_sums: needs 1 <= groups"),
            (lambda: lib.ribca_group_sums(p, p, 5, 3, 4, p, p, ctypes.byref(sk), p, lib.ribca_group_sums_ws_bytes(5, 3, 4) - 1, None),
             b"ribca_group_sums: workspace too small"),
            (lambda: lib.ribca_heatmap_raster(None, p, 2, 2, p, 8, 1, p, ctypes.byref(lo), ctypes.byref(hi), p, 256, None), b"ribca_heatmap_raster: NULL buffer"),
            (lambda: lib.ribca_heatmap_raster(p, p, 257, 2, p, 8, 1, p, ctypes.byref(lo), ctypes.byref(hi), p, 256, None), b"ribca_heatmap_raster: needs 1 <= rows"),
            (lambda: lib.ribca_heatmap_raster(p, p, 2, 2, p, 8, 4, p, ctypes.byref(lo), ctypes.byref(hi), p, 256, None), b"ribca_heatmap_raster: needs 1 <= cell"),
            (lambda: lib.ribca_heatmap_raster(p, p, 2, 2, p, 8, 1, p, ctypes.byref(lo), ctypes.byref(hi), p, 255, None), b"ribca_heatmap_raster: workspace too small"),
            (lambda: lib.ribca_pie_raster(None, 2, p, 65, 30, p, None), b"ribca_pie_raster: NULL buffer"),
            (lambda: lib.ribca_pie_raster(p, 257, p, 65, 30, p, None), b"ribca_pie_raster: needs 0 <= m <= 256"),
            (lambda: lib.ribca_pie_raster(p, 2, p, 0, 0, p, None), b"ribca_pie_raster: needs 1 <= size"),
            (lambda: lib.ribca_pie_raster(p, 2, p, 65, 66, p, None), b"ribca_pie_raster: needs 0 <= radius")):
        assert call() != 0
        assert lib.ribca_last_error().startswith(text), (text, lib.ribca_last_error())
    # the queries: every piece starts at a multiple of 256 bytes; 0 for what the entry point refuses
    assert lib.ribca_group_sums_ws_bytes(0, 3, 4) == 256
    assert lib.ribca_group_sums_ws_bytes(3 * CN.R + 7, 15, 5) == 2560 + 256 + 256
    assert lib.ribca_group_sums_ws_bytes(5, 0, 4) == 0 and lib.ribca_group_sums_ws_bytes(5, 3, 257) == 0 and lib.ribca_group_sums_ws_bytes(2 ** 31 - 1, 3, 4) == 0
    assert lib.ribca_heatmap_raster_ws_bytes(2, 2, 8, 1) == 256 and lib.ribca_heatmap_raster_ws_bytes(2, 2, 8, 4) == 0
