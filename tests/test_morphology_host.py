"""Cell morphology without a GPU: the version, every refusal of ribca_mask_morphology and its workspace query (a status whose text names the
entry point, before any HIP call), the two forms of the restatement against each other (tests/morphology_numpy.py), the Euler number and the
perimeter of every cell of the generated mask against scipy.ndimage, closed forms of the host module, the crop window, the CSV writers and the
command-line switch."""
import ctypes
import math
import types

import numpy as np
import pytest
from scipy import ndimage

import contact_numpy as CN
import morphology_numpy as MN
from multiplexed_image_annotator_amd import _lib, morphology

CAP = 1 << 21


def test_version():
    assert _lib.lib().ribca_version() >= 107


def test_refusals_are_a_status_naming_the_entry_point():
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)      # never dereferenced: every case below is refused by its sizes, before any HIP call
    big = 1 << 40
    name = "ribca_mask_morphology"

    def refused(status, text):
        assert status == 1
        msg = lib.ribca_last_error()
        assert msg and msg.startswith(text.encode()), (text, msg)

    def call(mask=p, H=64, W=64, l2c=p, L=10, n=9, rect=p, sums=p, bbox=p, ws=p, ws_bytes=big):
        return lib.ribca_mask_morphology(mask, H, W, l2c, L, n, rect, sums, bbox, ws, ws_bytes, None)

    for hole in ("mask", "l2c", "sums", "bbox", "ws"):      # rect may be NULL
        refused(call(**{hole: None}), f"{name}: NULL buffer")
    sizes = f"{name}: needs 1 <= H, W <= 65535 and H W < 2^31"
    refused(call(H=0), sizes)
    refused(call(W=0), sizes)
    refused(call(H=65536, W=1), sizes)
    refused(call(H=1, W=65536), sizes)
    refused(call(H=65535, W=32769), sizes)      # H W = 2^31 + 32767
    refused(call(H=1 << 15, W=1 << 16), sizes)
    refused(call(L=0), f"{name}: needs 1 <= L")
    refused(call(n=0), f"{name}: needs 1 <= n <= 2^21")
    refused(call(n=CAP + 1), f"{name}: needs 1 <= n <= 2^21")
    need = lib.ribca_mask_morphology_ws_bytes(64, 64, 9)
    assert need > 0 and need % 256 == 0
    refused(call(ws_bytes=need - 1), f"{name}: workspace too small")
    for h, w, n in ((0, 64, 9), (64, 0, 9), (65536, 1, 9), (1, 65536, 9), (65535, 32769, 9), (64, 64, 0), (64, 64, CAP + 1), (-1, 64, 9)):
        assert lib.ribca_mask_morphology_ws_bytes(h, w, n) == 0
    assert lib.ribca_mask_morphology_ws_bytes(65535, 32768, CAP) > 0      # H W = 2^31 - 32768


def _generated():
    mask = MN.generated_mask()
    table, n = CN.identity_table(mask)
    return mask, table, n


def test_the_two_forms_of_the_restatement_agree():
    mask, table, n = _generated()
    assert mask.shape == (96, 80) and n == 60
    odd = mask.copy()
    odd[odd == 7] = 90            # a label past the table
    odd[0:2, 0:3] = -4            # negative labels
    odd_table = table.copy()
    odd_table[5] = -1             # an unmapped label
    odd_table[9] = n + 3          # mapped past the cells
    for m, t in ((mask, table), (odd, odd_table)):
        plain = MN.sums_loop(m, t, n)
        rect = MN.windows_and_others(plain[1], 96, 80, 12, 3)
        loop, fast = MN.sums_loop(m, t, n, rect), MN.sums_arrays(m, t, n, rect)
        assert np.array_equal(loop[0], fast[0]) and np.array_equal(loop[1], fast[1]) and loop[1].dtype == np.int32
        assert np.array_equal(loop[0][:, :15], plain[0][:, :15]) and not plain[0][:, 15].any() and loop[0][:, 15].any()
        assert (loop[0][:, 15] <= loop[0][:, 0]).all()
    sums, bbox = MN.sums_arrays(odd, odd_table, n)
    assert not sums[[4, 6, 8]].any() and (bbox[[4, 6, 8]] == [MN.INT32_MAX, -1, MN.INT32_MAX, -1]).all()
    # column 6 is the row sum of the contact weights at reach 1
    w = CN.pair_weights(mask, table, n, 1)
    per_cell = np.zeros(n, dtype=np.int64)
    for (i, _), v in w.items():
        per_cell[i] += v
    assert np.array_equal(MN.sums_arrays(mask, table, n)[0][:, 6], per_cell) and per_cell.any()
    # thin images: every neighbour of a row leaves the image above and below
    line = np.array([[1, 1, 0, 2, 1]], dtype=np.int32)
    for m in (line, line.T.copy(), np.array([[1]], dtype=np.int32)):
        a, b = MN.sums_loop(m, np.array([-1, 0, 1], dtype=np.int32), 2), MN.sums_arrays(m, np.array([-1, 0, 1], dtype=np.int32), 2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert MN.sums_loop(line, np.array([-1, 0, 1], dtype=np.int32), 2)[0][:, 6:9].tolist() == [[1, 1, 8], [1, 1, 2]]


def test_euler_and_perimeter_are_scipy_s_on_the_generated_mask():
    """per cell: components at 8-connectivity minus holes at 4-connectivity from scipy.ndimage.label, and scikit-image's perimeter(neighbourhood=4)
    restated with binary_erosion, convolve and bincount"""
    mask, table, n = _generated()
    sums, bbox = MN.sums_arrays(mask, table, n)
    feat = morphology.features(sums, bbox)
    weights = np.zeros(50)
    weights[[5, 7, 15, 17, 25, 27]] = 1.0
    weights[[21, 33]] = math.sqrt(2.0)
    weights[[13, 23]] = (1.0 + math.sqrt(2.0)) / 2.0
    cross = ndimage.generate_binary_structure(2, 1)
    odd = 0
    for i in range(n):
        own = mask == i + 1
        assert own.any()
        parts = ndimage.label(own, structure=np.ones((3, 3)))[1]
        holes = ndimage.label(~np.pad(own, 1), structure=cross)[1] - 1
        assert feat["euler"][i] == parts - holes, i
        odd += parts - holes != 1
        image = own.astype(np.uint8)
        border = image - ndimage.binary_erosion(image, cross, border_value=0)
        classes = ndimage.convolve(border, np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]), mode="constant", cval=0)
        hist = np.bincount(classes.ravel(), minlength=50)
        assert np.array_equal(sums[i, 9:12], [hist[[5, 7, 15, 17, 25, 27]].sum(), hist[[21, 33]].sum(), hist[[13, 23]].sum()]), i
        assert feat["perimeter"][i] == sums[i, 9] + sums[i, 10] * math.sqrt(2.0) + sums[i, 11] * (1.0 + math.sqrt(2.0)) / 2.0
        assert abs(feat["perimeter"][i] - float(hist @ weights)) <= 1e-12 * feat["perimeter"][i]      # another order of the same three products
    assert odd > n // 2      # most cells have a hole or a fragment


def _one(mask):
    sums, bbox = MN.sums_arrays(mask, np.array([-1, 0], dtype=np.int32), 1)
    return sums, bbox, {k: v[0] for k, v in morphology.features(sums, bbox).items()}


def test_closed_forms():
    """the moments of an h x w rectangle are (h^2 - 1) / 12 and (w^2 - 1) / 12: 4 and 2 / 3 for 7 x 3.  Every float below comes from at most six
    correctly rounded operations on numbers of magnitude one: 1e-14 relative is two orders above that, and far below any wrong formula."""
    tall = np.zeros((12, 9), dtype=np.int32)
    tall[2:9, 4:7] = 1
    sums, bbox, f = _one(tall)
    assert sums[0, :6].tolist() == [21, 105, 105, 609, 539, 525] and bbox.tolist() == [[2, 8, 4, 6]]
    assert f["major_axis"] == 8.0
    assert f["minor_axis"] == pytest.approx(4.0 * math.sqrt(2.0 / 3.0), rel=1e-14)
    assert f["eccentricity"] == pytest.approx(math.sqrt(5.0 / 6.0), rel=1e-14)
    assert f["orientation"] == 0.0 and f["extent"] == 1.0 and f["euler"] == 1 and f["area"] == 21 and (f["bbox_h"], f["bbox_w"]) == (7, 3)
    assert f["centroid_r"] == 5.0 and f["centroid_c"] == 5.0 and f["equivalent_diameter"] == math.sqrt(84.0 / math.pi)
    assert f["contact_fraction"] == 0.0 and f["on_image_edge"] == 0 and math.isnan(f["patch_coverage"]) is False and f["patch_coverage"] == 0.0
    # its border ring of 16 pixels: four corners at v = 1 + 2 * 2 = 5 ... every border pixel has two border 4-neighbours
    assert sums[0, 6:9].tolist() == [0, 20, 0] and f["perimeter"] == 16.0 and f["circularity"] == 4.0 * math.pi * 21 / 256.0
    wide = np.ascontiguousarray(tall.T)
    f = _one(wide)[2]
    assert f["orientation"] == math.pi / 2 and f["major_axis"] == 8.0 and (f["bbox_h"], f["bbox_w"]) == (3, 7)
    # a diagonal: the major axis at +45 degrees from the row axis towards the columns
    f = _one(np.eye(6, dtype=np.int32))[2]
    assert f["orientation"] == pytest.approx(math.pi / 4, rel=1e-14) and f["minor_axis"] == 0.0 and f["eccentricity"] == 1.0 and f["euler"] == 1
    f = _one(np.eye(6, dtype=np.int32)[::-1].copy())[2]
    assert f["orientation"] == pytest.approx(-math.pi / 4, rel=1e-14)
    # one pixel in the image corner
    dot = np.zeros((5, 5), dtype=np.int32)
    dot[0, 0] = 1
    sums, _, f = _one(dot)
    assert f["perimeter"] == 0.0 and math.isnan(f["circularity"]) and f["euler"] == 1 and f["major_axis"] == 0.0 and f["eccentricity"] == 0.0
    assert sums[0, 6:9].tolist() == [0, 2, 2] and f["on_image_edge"] == 1 and sums[0, 12:15].tolist() == [4, 0, 0]
    # a ring, and one label in two blobs
    ring = np.zeros((9, 9), dtype=np.int32)
    ring[2:7, 2:7] = 1
    ring[4, 4] = 0
    assert _one(ring)[2]["euler"] == 0
    ring[3:6, 3:6] = 0
    assert _one(ring)[2]["euler"] == 0
    two = np.zeros((9, 9), dtype=np.int32)
    two[1:3, 1:3], two[6:8, 5:8] = 1, 1
    assert _one(two)[2]["euler"] == 2
    two[3, 3] = 1      # touches the first blob on a diagonal: one component at 8-connectivity
    assert _one(two)[2]["euler"] == 2 and _one(two)[0][0, 14] == 1
    two[6, 6] = 0      # a pixel missing on the blob's edge is no hole
    assert _one(two)[2]["euler"] == 2
    # two cells side by side: half of the 3-pixel border of a 3 x 3 square's twelve leaving edges
    pair = np.zeros((5, 8), dtype=np.int32)
    pair[1:4, 1:4], pair[1:4, 4:7] = 1, 2
    sums, bbox = MN.sums_arrays(pair, np.array([-1, 0, 1], dtype=np.int32), 2)
    assert morphology.features(sums, bbox)["contact_fraction"].tolist() == [0.25, 0.25]
    # a cell without a pixel
    none = morphology.features(np.zeros((1, 16), dtype=np.int64), np.array([[MN.INT32_MAX, -1, MN.INT32_MAX, -1]], dtype=np.int32))
    assert none["area"][0] == 0 and none["euler"][0] == 0 and none["bbox_h"][0] == 0 and math.isnan(none["perimeter"][0])
    # sums past 2^53 and products past 2^64 stay exact: a 3 x 3 square at (60000, 30000)
    far = np.zeros((9, 16), dtype=np.int64)
    rr, cc = np.mgrid[60000:60003, 30000:30003]
    far = np.array([[9, rr.sum(), cc.sum(), (rr * rr).sum(), (cc * cc).sum(), (rr * cc).sum()] + [0] * 10], dtype=np.int64)
    f = morphology.features(far, np.array([[60000, 60002, 30000, 30002]], dtype=np.int32))
    assert f["major_axis"][0] == f["minor_axis"][0] == 4.0 * math.sqrt(2.0 / 3.0) and f["eccentricity"][0] == 0.0 and f["centroid_r"][0] == 60001.0


def test_patch_rect():
    """P = 40: half 20; P = 41: half 21 (the kernel truncates rmid - 20.5); the image corner clamps r0 at 0, the far border clamps r1 at H"""
    bbox = np.array([[0, 9, 0, 5], [100, 121, 200, 260], [490, 499, 590, 599], [30, 31, 7, 60]], dtype=np.int32)
    assert morphology.patch_rect(bbox, 500, 600, 40).tolist() == [[0, 40, 0, 40], [90, 130, 210, 250], [474, 500, 574, 600], [10, 50, 13, 53]]
    assert morphology.patch_rect(bbox, 500, 600, 41).tolist() == [[0, 41, 0, 41], [89, 130, 209, 250], [473, 500, 573, 600], [9, 50, 12, 53]]
    assert morphology.patch_rect(bbox, 500, 600, 40).dtype == np.int32 and morphology.patch_rect(bbox[:0], 5, 6, 40).shape == (0, 4)
    # the same numbers as the kernels' own arithmetic: int(rmid - P / 2.0) where positive, else 0
    for p in (40, 41, 53):
        for lo, hi in ((0, 9), (100, 121), (3, 70), (20, 21)):
            mid = (lo + hi) >> 1
            want = int(mid - p / 2.0) if mid - p / 2.0 > 0.0 else 0
            assert morphology.patch_rect(np.array([[lo, hi, lo, hi]]), 500, 500, p)[0, 0] == want


IDS = np.array([2, 3, 5])
LABELS = np.array([0, 1, 0])
NAMES = ["A", "B c", "C"]


def _three_cells():
    mask = np.zeros((8, 12), dtype=np.int32)
    mask[1:4, 1:4], mask[1:4, 4:7], mask[5:8, 8:12] = 2, 3, 5
    table = np.full(6, -1, dtype=np.int32)
    table[IDS] = np.arange(3)
    bbox = MN.sums_arrays(mask, table, 3)[1]
    rect = np.array([[0, 3, 0, 3], [0, 8, 0, 12], [0, 0, 0, 0]], dtype=np.int32)
    return morphology.features(*MN.sums_arrays(mask, table, 3, rect)), bbox


def test_the_csv_writers():
    feat, bbox = _three_cells()
    rows = morphology.cells_csv(IDS, LABELS, NAMES, feat).split("\n")
    assert rows[0] == "cell_id,cell_type," + ",".join(morphology.FEATURES) and len(rows) == 5 and rows[4] == ""
    assert len(morphology.FEATURES) == 17 and rows[0].split(",")[2:9] == ["area", "centroid_r", "centroid_c", "bbox_h", "bbox_w", "extent", "equivalent_diameter"]
    first = rows[1].split(",")
    assert first[:7] == ["2", "A", "9", "2", "2", "3", "3"] and first[7] == "1" and first[15] == "1" and first[16] == "0.25" and first[17] == "0"
    assert first[18] == f"{4 / 9:.17g}" and len(first[18]) >= 18 and float(first[8]) == math.sqrt(36.0 / math.pi)
    assert rows[2].split(",")[:3] == ["3", "B c", "9"] and rows[2].split(",")[18] == "1"
    last = rows[3].split(",")
    assert last[:3] == ["5", "A", "12"] and last[17] == "1" and last[18] == "0"      # on the image edge; an empty rectangle
    for line in rows[1:4]:      # every float parses back to the double it was written from
        cols = line.split(",")
        i = rows.index(line) - 1
        assert [float(c) for c in cols[2:]] == [float(feat[name][i]) for name in morphology.FEATURES]
    with pytest.raises(ValueError):
        morphology.cells_csv(IDS, LABELS[:2], NAMES, feat)
    assert morphology.cells_csv(IDS[:0], LABELS[:0], NAMES, morphology.features(np.zeros((0, 16)), np.zeros((0, 4)))) == rows[0] + "\n"
    # the summary: type A has the cells 2 and 5, type B c one cell, type C none
    table = morphology.summary(LABELS, 3, feat)
    assert table.shape == (3, 17, 8)
    k = morphology.FEATURES.index("area")
    assert table[0, k].tolist() == [2.0, 10.5, 1.5, 9.0, 9.75, 10.5, 11.25, 12.0] and table[1, k].tolist() == [1.0, 9.0, 0.0, 9.0, 9.0, 9.0, 9.0, 9.0]
    assert table[2, k, 0] == 0 and np.isnan(table[2, k, 1:]).all()
    lines = morphology.summary_csv(NAMES, table).split("\n")
    assert lines[0] == "cell_type,feature,n,mean,std,min,q25,median,q75,max" and len(lines) == 2 + 3 * 17
    assert lines[1] == "A,area,2,10.5,1.5,9,9.75,10.5,11.25,12" and lines[1 + 2 * 17] == "C,area,0,nan,nan,nan,nan,nan,nan,nan"
    z = morphology.standardised_means(LABELS, 3, feat)
    assert z.shape == (3, 17) and np.isnan(z[2]).all()
    assert z[0, k] == (10.5 - 10.0) / math.sqrt(2.0) and z[1, k] == (9.0 - 10.0) / math.sqrt(2.0)
    assert np.isnan(z[:, morphology.FEATURES.index("euler")]).all()      # no spread
    text = morphology.matrix_csv(NAMES, z).split("\n")
    assert text[0] == "cell_type," + ",".join(morphology.FEATURES) and text[3].startswith("C,nan,nan") and len(text) == 5
    assert text[1].split(",")[1] == f"{z[0, k]:.17g}"
    with pytest.raises(ValueError):
        morphology.matrix_csv(NAMES[:2], z)
    with pytest.raises(ValueError):
        morphology.summary_csv(NAMES[:2], table)
    # what a tile-per-rank run sends and rebuilds
    back = morphology.from_matrix(morphology.feature_matrix(feat))
    assert morphology.cells_csv(IDS, LABELS, NAMES, back) == "\n".join(rows)


def test_the_colour_indices_of_the_maps():
    """FIXED scales: equivalent_diameter / (2 cell_size) saturating at 1, and patch_coverage itself"""
    assert morphology.diameter_colour_index(np.array([0.0, 15.0, 30.0, 59.9, 60.0, 200.0, np.nan]), 30).tolist() == [0, 63, 127, 254, 255, 255, 0]
    assert morphology.coverage_colour_index(np.array([0.0, 0.5, 0.999, 1.0, np.nan])).tolist() == [0, 127, 254, 255, 0]
    assert morphology.coverage_colour_index(np.zeros(0)).shape == (0,) and morphology.Z_LIMIT == 3.0


def test_the_command_line_switch():
    """--morphology is off by default; the pipeline calls the method only with it, beside the contact step and without a cell-count guard"""
    import main as cli
    common = ["--marker-list-path", "m.txt", "--image-path", "i.npy", "--mask-path", "k.npy", "--batch-id", "c"]
    assert cli.parse_args(common).morphology is False
    assert cli.parse_args(common + ["--morphology"]).morphology is True

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
    assert "cell_morphology" not in [c[0] for c in off.calls]
    on = Recorder()
    cli._pipeline(on, 16, 0, morphology=True)
    got = [c for c in on.calls if c[0] == "cell_morphology"]
    assert len(got) == 1 and got[0][2] == {"integrate": True}
    assert [c[0] for c in on.calls if c[0] != "cell_morphology"] == [c[0] for c in off.calls]
    both = Recorder()
    cli._pipeline(both, 16, 0, contact_distance=1, morphology=True)
    order = [c[0] for c in both.calls]
    assert order.index("contact_analysis") < order.index("cell_morphology") < order.index("colorize")
    import inspect
    for fn in (cli._pipeline, cli.run, cli.batch_run):
        assert inspect.signature(fn).parameters["morphology"].default is False


def test_cell_morphology_needs_annotations():
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = object.__new__(Annotator)
    a.tile_mode = False
    a.annotations = []
    a.cell_types = ["A", "B"]
    with pytest.raises(ValueError, match="No annotations"):
        a.cell_morphology()
    assert not hasattr(a, "morphology_stats")
