"""The host side of the marker colocalisation (no GPU): every formula of colocalization.features against plain loops; on the restatement's
outputs r against np.corrcoef and m1 / m2 against a direct numpy evaluation on the u scale; a constant channel; a planted pair and anti-pair;
the CSV texts against hand-written expectations; the refusals of the entry point, which come before any HIP call; and that the GPU test's own
images can tell the stated summation order from np.sum's and from 64 partials.

THE 1e-10 BAR on r, m1 and m2 (cells of at most 4096 pixels, markers with a standard deviation of at least 1e-3): by Cauchy-Schwarz
sum |d_k d_l| <= sqrt(X_kk X_ll), so the rounding of the tree moves r by about (a / 256 + 10) 2^-53, roughly 3e-15; the bar leaves a wide
margin for the divisions and for np.corrcoef's own rounding."""
import ctypes
import math

import numpy as np
import pytest

import coloc_numpy as CN
from multiplexed_image_annotator_amd import colocalization as CO

INTENSITY_SMALL_BOX, COLOC_RESIDENT = 1024, 4096      # ops constants, restated: ops imports torch, this file needs none


def _hand():
    """four cells over K = 2: a clean one; a constant first marker; one pixel; no pixel"""
    area = np.array([4, 3, 1, 0], dtype=np.int32)
    both = np.array([[2, 1, 2], [3, 2, 2], [0, 0, 1], [0, 0, 0]], dtype=np.int32)      # (0,0), (0,1), (1,1)
    sums = np.array([[0.0, 0.0], [1.5, -1.0], [-1.0, 0.5], [0.0, 0.0]])
    cross = np.array([[4.0, 2.0, 4.0], [0.0, 0.0, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    gated = np.array([[[0.5, 1.0], [-1.0, 1.5]], [[1.5, 1.0], [-1.0, 0.25]], [[0.0, -1.0], [0.0, 0.5]], [[0.0, 0.0], [0.0, 0.0]]])
    return area, both, sums, cross, gated


def _same_dict(got, want):
    assert sorted(got) == sorted(want) == sorted(CO.STATS)
    for key in want:
        assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].astype(got[key].dtype).tobytes(), key


def test_features_are_the_plain_loops_on_a_hand_case():
    f = CO.features(*_hand())
    _same_dict(f, CN.features(*_hand()))
    assert f["r"][0, 0] == 0.5 and f["overlap"][0, 0] == 0.75 and f["m1"][0, 0] == 0.75 and f["m2"][0, 0] == 0.25
    assert f["both"][:, 0].tolist() == [1, 2, 0, 0] and f["both_fraction"][0, 0] == 0.25 and f["jaccard"][0, 0] == 1.0 / 3.0
    assert math.isnan(f["r"][1, 0]) and np.isfinite(f["overlap"][1, 0]) and f["jaccard"][1, 0] == 2.0 / 3.0      # a constant marker: no r
    assert math.isnan(f["r"][2, 0])                                                                     # one pixel: no r
    assert math.isnan(f["overlap"][2, 0]) and math.isnan(f["m1"][2, 0]) and f["m2"][2, 0] == 0.0        # u_0 = 0 there: R_00 = 0, S_0 + a = 0
    assert all(math.isnan(f[s][3, 0]) for s in CO.STATS if s != "both") and f["both"][3, 0] == 0        # no pixel
    with pytest.raises(ValueError):
        CO.features(_hand()[0], _hand()[1][:, :2], *_hand()[2:])


@pytest.fixture(scope="module")
def restated():
    """the restatement on the GPU test's small image at K = 6, and the inputs"""
    mask, ids, bbox = CN.small_cells(INTENSITY_SMALL_BOX)
    image = CN.generated_image(6, 96, 128, 41)
    chan = CN.SELECTIONS[2]
    thr = np.array([CN.GATES[c] for c in chan], dtype=np.float32)
    return image, mask, ids, bbox, chan, thr, CN.coloc(image, mask, ids, bbox, chan, thr)


def test_features_are_the_plain_loops_on_the_restatement_s_outputs(restated):
    out = restated[6]
    _same_dict(CO.features(*out), CN.features(*out))


def test_r_is_corrcoef_and_m1_m2_are_the_direct_sums_within_1e_10(restated):
    image, mask, ids, bbox, chan, thr, out = restated
    f = CO.features(*out)
    off = CO.off_pairs(len(chan))
    checked = 0
    for i in range(len(ids)):
        a = int(out[0][i])
        if a < 2 or a > 4096:
            continue
        r0, r1, c0, c1 = CN.clipped_box(bbox[i], *mask.shape)
        inside = mask[r0:r1 + 1, c0:c1 + 1] == ids[i]
        v32 = image[list(chan)][:, r0:r1 + 1, c0:c1 + 1][:, inside]
        u = (v32.astype(np.float64) + 1.0) / 2.0
        if (v32.astype(np.float64).std(axis=1) < 1e-3).any():
            continue
        g = v32 > thr[:, None]
        cc = np.corrcoef(u)
        for j, (k, l) in enumerate(off):
            assert abs(f["r"][i, j] - cc[k, l]) <= 1e-10, (i, k, l)
            assert abs(f["overlap"][i, j] - (u[k] * u[l]).sum() / math.sqrt((u[k] * u[k]).sum() * (u[l] * u[l]).sum())) <= 1e-10
            assert abs(f["m1"][i, j] - u[k][g[l]].sum() / u[k].sum()) <= 1e-10, (i, k, l)
            assert abs(f["m2"][i, j] - u[l][g[k]].sum() / u[l].sum()) <= 1e-10, (i, k, l)
            assert f["both"][i, j] == int((g[k] & g[l]).sum())
            checked += 1
    assert checked >= 9 * len(off)


def _planted():
    """three markers over a grid of 6 x 8 cells: A bright on the left half of every cell and exactly -1 (u = 0) on the right; B on A's
    pixels with noise of its own; C on the complementary half.  Channel 3 is constant."""
    rng = np.random.default_rng(12)
    mask = np.zeros((40, 60), dtype=np.int32)
    ids, bbox = [], []
    for r in range(0, 40, 8):
        for c in range(0, 60, 10):
            ids.append(len(ids) + 1)
            mask[r:r + 6, c:c + 8] = ids[-1]
            bbox.append((r, r + 5, c, c + 7))
    left = (np.arange(60) % 10 < 4)[None, :] & (mask > 0)
    right = (mask > 0) & ~left
    image = np.full((4, 40, 60), -1.0, dtype=np.float32)
    image[0][left] = (0.5 + 0.2 * rng.random(left.sum())).astype(np.float32)
    image[1][left] = (0.4 + 0.2 * rng.random(left.sum())).astype(np.float32)
    image[2][right] = (0.5 + 0.2 * rng.random(right.sum())).astype(np.float32)
    image[3] = np.float32(0.3)
    return image, mask, np.array(ids, dtype=np.int32), np.array(bbox, dtype=np.int32)


def test_a_planted_pair_an_anti_pair_and_a_constant_channel():
    image, mask, ids, bbox = _planted()
    out = CN.coloc(image, mask, ids, bbox, (0, 1, 2, 3), CO.gates(0.15, 4))
    f = CO.features(*out)
    col = {q: j for j, q in enumerate(CO.off_pairs(4))}
    assert (f["r"][:, col[0, 1]] > 0.9).all() and (np.abs(f["m1"][:, col[0, 1]] - 1.0) < 1e-12).all() and (f["jaccard"][:, col[0, 1]] == 1.0).all()
    anti = col[0, 2]
    assert (f["r"][:, anti] < -0.9).all() and not f["m1"][:, anti].any() and not f["m2"][:, anti].any() and not f["jaccard"][:, anti].any()
    assert not f["both"][:, anti].any() and not f["both_fraction"][:, anti].any()
    for pair in ((0, 3), (1, 3), (2, 3)):
        assert np.isnan(f["r"][:, col[pair]]).all() and np.isfinite(f["overlap"][:, col[pair]]).all()      # a constant channel: NaN r
    cross_with_3 = [j for j, q in enumerate(CO.all_pairs(4)) if 3 in q]
    assert not out[3][:, cross_with_3].any()      # exactly 0.0 in its row and column


def test_gates_thresholds_and_pairs():
    assert CO.THRESHOLD == 0.15 and CO.MAX_MARKERS == 32
    g = CO.gates(0.15, 3)
    assert g.dtype == np.float32 and g.tolist() == [float(np.float32(2.0 * 0.15 - 1.0))] * 3 and CO.gates(0, 2).tolist() == [-1.0, -1.0]
    for bad in (-0.1, 1.0, 2, "0.2", None, True, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            CO.check_threshold(bad)
    assert CO.all_pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)] == CN.pairs(3) and CO.off_pairs(3) == [(0, 1), (0, 2), (1, 2)]
    markers = ["CD3", "CD20", "Ki-67"]
    assert CO.pair_names(markers) == ["CD3~CD20", "CD3~Ki-67", "CD20~Ki-67"]
    assert CO.parse_pairs(["CD3:Ki-67", "CD20:CD3"], markers) == [1, 0] and CO.parse_pairs(None, markers) == []
    for bad in (["CD3"], ["CD3:CD4"], ["CD3:CD3"], ["CD3:CD20:Ki-67"], [":CD3"], ["CD3:CD20", "CD20:CD3"]):
        with pytest.raises(ValueError, match="pair"):
            CO.parse_pairs(bad, markers)
    idx = CO.colour_index(np.array([-1.0, 0.0, 1.0, np.nan, -3.0, 2.0, 0.5]))
    assert idx.dtype == np.uint8 and idx.tolist() == [0, 127, 255, 0, 0, 255, 191]


def test_csv_texts():
    area, both, sums, cross, gated = _hand()
    f = CO.features(area, both, sums, cross, gated)
    third = f"{1.0 / 3.0:.17g}"
    assert CO.cells_csv([5, 9, 12, 13], [1, 0, 7, 0], ["T", "B"], ["CD3", "CD20"], area, f["r"]) == (
        "id,cell type,area,CD3~CD20_r\n5,B,4,0.5\n9,T,3,nan\n12,,1,nan\n13,T,0,nan\n")
    assert CO.cells_csv([], [], ["T"], ["CD3", "CD20"], [], f["r"][:0]).count("\n") == 1
    text = CO.pairs_csv([5, 9, 12, 13], [1, 0, 7, 0], ["T", "B"], ["CD3", "CD20"], [0], area, f)
    rows = text.split("\n")
    assert rows[0] == ("id,cell type,area,CD3~CD20_r,CD3~CD20_overlap,CD3~CD20_m1,CD3~CD20_m2,CD3~CD20_both,CD3~CD20_both_fraction,"
                       "CD3~CD20_jaccard")
    assert rows[1] == f"5,B,4,0.5,0.75,0.75,0.25,1,0.25,{third}" and rows[4] == "13,T,0,nan,nan,nan,nan,0,nan,nan" and rows[5] == ""
    s = CO.summary([1, 0, 7, 0], 3, f)
    assert s.shape == (3, 1, 8) and s[1, 0, :4].tolist() == [1.0, 1.0, 0.5, 0.5] and s[1, 0, 4:].tolist() == [0.75, 0.75, 0.25, 0.25]
    assert s[0, 0, :2].tolist() == [2.0, 0.0] and np.isnan(s[0, 0, 2:4]).all() and s[0, 0, 4] == f["overlap"][1, 0] and s[0, 0, 7] == 2.0 / 3.0
    assert s[2, 0, :2].tolist() == [0.0, 0.0] and np.isnan(s[2, 0, 2:]).all()
    text = CO.summary_csv(["T", "B", "NK"], ["CD3", "CD20"], s)
    rows = text.split("\n")
    assert rows[0] == "cell_type,marker_a,marker_b,n,n_valid,mean_r,median_r,median_overlap,median_m1,median_m2,mean_both_fraction"
    assert rows[2] == "B,CD3,CD20,1,1,0.5,0.5,0.75,0.75,0.25,0.25" and rows[3] == "NK,CD3,CD20,0,0,nan,nan,nan,nan,nan,nan" and len(rows) == 5
    r = np.array([[0.5, np.nan, -1.0], [0.25, np.nan, 0.0], [np.nan, np.nan, 1.0]])
    m = CO.median_matrix(r, 3)
    assert m.tolist()[0][:2] == [1.0, 0.375] and math.isnan(m[0, 2]) and m[1, 2] == m[2, 1] == 0.0 and m[1, 0] == 0.375
    assert CO.median_matrix(r, 3, rows=[True, False, False])[0, 1] == 0.5 and math.isnan(CO.median_matrix(r[:0], 3)[0, 1])
    assert CO.matrix_csv(["a", "b", "c"], m) == "marker,a,b,c\na,1,0.375,nan\nb,0.375,1,0\nc,nan,0,1\n"


def test_the_entry_point_refuses_before_any_hip_call():
    """no GPU here: a call that got past its checks would fail in the launch, with another text"""
    from multiplexed_image_annotator_amd import _lib
    lib = _lib.lib()
    assert lib.ribca_version() >= 114 and "ribca_cell_coloc" in _lib.SIGNATURES
    keep = [ctypes.create_string_buffer(4096) for _ in range(9)]
    image, mask, ids, bbox, area, both, sums, cross, gated = (ctypes.addressof(b) for b in keep)

    def call(channels, gates, c=6, h=8, w=8, n=1, **null):
        ch = (ctypes.c_int32 * max(len(channels), 1))(*channels)
        th = (ctypes.c_float * max(len(gates), 1))(*gates)
        args = dict(image=image, mask=mask, ids=ids, bbox=bbox, chan=ctypes.addressof(ch), thr=ctypes.addressof(th), area=area, both=both,
                    sums=sums, cross=cross, gated=gated)
        args.update(null)
        status = lib.ribca_cell_coloc(args["image"], c, h, w, args["mask"], args["ids"], args["bbox"], n, args["chan"], args["thr"], len(channels),
                                      args["area"], args["both"], args["sums"], args["cross"], args["gated"], None)
        return status, (lib.ribca_last_error() or b"").decode()

    assert call((0, 1), (0.0, 0.0), n=0, image=None)[0] == 0      # n == 0 returns 0 and touches nothing
    for name in ("image", "mask", "ids", "bbox", "chan", "thr", "area", "both", "sums", "cross", "gated"):
        status, text = call((0, 1), (0.0, 0.0), **{name: None})
        assert status != 0 and text == "ribca_cell_coloc: NULL buffer", (name, text)
    for chan, thr, kw, want in (((0,), (0.0,), {}, "needs 2 <= K <= 32"), (tuple(range(33)), (0.0,) * 33, {"c": 64}, "needs 2 <= K <= 32"),
                                ((2, 4, 2), (0.0,) * 3, {}, "chan holds a channel twice"), ((0, 6), (0.0, 0.0), {}, "needs 0 <= chan[k] < C"),
                                ((0, -1), (0.0, 0.0), {}, "needs 0 <= chan[k] < C"), ((0, 1), (0.0, float("nan")), {}, "needs a finite thr[k]"),
                                ((0, 1), (float("inf"), 0.0), {}, "needs a finite thr[k]"), ((0, 1), (0.0, 0.0), {"c": 65}, "needs 1 <= C <= 64"),
                                ((0, 1), (0.0, 0.0), {"h": 65536}, "H W < 2^31"), ((0, 1), (0.0, 0.0), {"n": (1 << 21) + 1}, "n <= 2^21")):
        status, text = call(chan, thr, **kw)
        assert status != 0 and text.startswith("ribca_cell_coloc: ") and want in text, (chan, thr, kw, text)


def test_the_gpu_test_s_images_can_tell_the_summation_orders_apart():
    """np.sum's order and 64 partials instead of 256 each change bytes of sums, cross and gated in at least one cell of every size class in
    which they can: 65 .. 256 pixels (one element per partial), 257 .. 4096 (several, resident) and above (streaming)"""
    cases = []
    mask, ids, bbox = CN.small_cells(INTENSITY_SMALL_BOX)
    cases.append((CN.generated_image(6, 96, 128, 41), mask, ids, bbox))
    mask, ids, bbox = CN.large_cells(COLOC_RESIDENT)
    cases.append((CN.generated_image(6, 128, 160, 42), mask, ids, bbox))
    chan = CN.SELECTIONS[1]
    thr = np.array([CN.GATES[c] for c in chan], dtype=np.float32)
    differs = {(v, cls, out): False for v in ("plain", "mod64") for cls in range(3) for out in (2, 3, 4)}
    for image, mask, ids, bbox in cases:
        want = CN.coloc(image, mask, ids, bbox, chan, thr)
        for variant in ("plain", "mod64"):
            got = CN.coloc(image, mask, ids, bbox, chan, thr, variant=variant)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()      # the integers do not care
            assert np.allclose(got[2], want[2], rtol=0, atol=1e-9) and np.allclose(got[3], want[3], rtol=0, atol=1e-9)
            for i, a in enumerate(want[0]):
                if a < 65:
                    continue
                cls = 0 if a <= 256 else 1 if a <= COLOC_RESIDENT else 2
                for out in (2, 3, 4):
                    differs[variant, cls, out] |= got[out][i].tobytes() != want[out][i].tobytes()
    assert all(differs.values()), [key for key, hit in differs.items() if not hit]
