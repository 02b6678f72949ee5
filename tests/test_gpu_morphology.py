"""Cell morphology on the GPU: ribca_mask_morphology (csrc/morphology.hip) against tests/morphology_numpy.py for EQUALITY of every column and of
the bounding boxes, outputs and workspace junk-filled to exactly the queried size before every call: every kind of label that is no cell, masks
that are no multiple of the pixel tile and thinner than the halo, more cells in a tile than a workgroup's table holds, one cell over many tiles,
cells far from the origin, the contact graph's border lengths; and Annotator.cell_morphology() end to end: files against the restatement run on
the same masks, the maps' scales, the pipeline switch, two ranks."""
import io
import os

import numpy as np
import pytest
import torch

import contact_numpy as CN
import morphology_numpy as MN
from batch_harness import annotated_batch, cli_runs, result_files, run_annotator, two_ranks
from multiplexed_image_annotator_amd import _lib, colors, morphology, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _gpu(mask, table, n, rect=None, junk=0xA5):
    """the entry point itself on junk-filled outputs and a junk-filled workspace of exactly the size the query asks for"""
    dev = _lib.require_gpu()
    md = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.int32)).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(dev)
    rd = None if rect is None else torch.from_numpy(np.ascontiguousarray(rect, dtype=np.int32)).to(dev)
    h, w = mask.shape
    sums = torch.full((n, 16), junk, dtype=torch.int64, device=dev)
    bbox = torch.full((n, 4), junk, dtype=torch.int32, device=dev)
    ws = torch.full((ops.mask_morphology_ws_bytes(h, w, n),), junk, dtype=torch.uint8, device=dev)
    status = lib().ribca_mask_morphology(ptr(md), h, w, ptr(td), len(table), n, ptr(rd), ptr(sums), ptr(bbox), ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    return sums.cpu().numpy(), bbox.cpu().numpy()


def _rects(mask, table, n, patch=12, seed=3):
    """the crop windows for half of the cells, arbitrary and partly empty rows for the rest"""
    return MN.windows_and_others(MN.sums_arrays(mask, table, n)[1], mask.shape[0], mask.shape[1], patch, seed)


def _equal_to_the_restatement(mask, table, n, rect, junk=0xA5):
    want = MN.sums_arrays(mask, table, n, rect)
    got = _gpu(mask, table, n, rect, junk)
    for col in range(16):
        assert np.array_equal(got[0][:, col], want[0][:, col]), (mask.shape, "column", col)
    assert np.array_equal(got[1], want[1]) and got[1].dtype == np.int32, mask.shape
    return want


def _generated_case():
    """(a): the generated 96 x 80 mask with labels doubled, through a table that maps odd labels and one even label to -1 and one past n; negative
    labels and labels past the table in the mask; one label in a second blob by construction of the generator"""
    base = MN.generated_mask()
    m = base * 2
    top = int(m.max())
    table = np.full(top + 1, -1, dtype=np.int32)
    table[2::2] = np.arange(top // 2)
    n = top // 2
    m[m == 14] = top + 40
    m[0:2, 0:3] = -6
    m[1, 5:8] = 7
    table[10] = -1
    table[18] = n + 5
    rect = _rects(m, table, n)
    return m, table, n, rect


@pytest.fixture(scope="module")
def generated():
    return _generated_case()


def test_the_generated_mask_with_every_kind_of_label_that_is_no_cell(generated):
    m, table, n, rect = generated
    want = _equal_to_the_restatement(m, table, n, rect)
    assert n == 60 and not want[0][[4, 6, 8]].any() and (want[0][:, 0] > 0).sum() == 57
    assert want[0][:, 15].any() and (want[0][1::2, 15] == 0).any() and want[0][:, 9:15].any(axis=0).all()
    feat = morphology.features(*want)
    assert (feat["euler"][want[0][:, 0] > 0] != 1).sum() > 28      # holes and fragments went through


@pytest.mark.parametrize("shape, cells", [((70, 45), 25), ((1, 50), 6), ((50, 1), 6), ((1, 1), 1)])
def test_masks_that_are_no_multiple_of_the_tile(shape, cells):
    """(b): 70 x 45 is 3 x 2 tiles with ragged last ones and cells across every seam; one row, one column and one pixel are thinner than the halo"""
    if min(shape) > 1:
        mask = CN.random_mask(shape[0], shape[1], cells, 31, radius=8.0)
        mask[30:34, 10:40] = 3          # across the seams at row 32 and column 32
        mask[5:60, 31:33] = 5
    else:
        mask = (1 + (np.arange(shape[0] * shape[1]) // 7) % cells).astype(np.int32).reshape(shape)
        mask[mask == 2] = 0
    table, n = CN.identity_table(mask)
    want = _equal_to_the_restatement(mask, table, n, _rects(mask, table, n, patch=9))
    assert want[0][:, 8].any()      # somebody touches the image border


def test_more_cells_in_a_tile_than_the_workgroup_s_table_holds():
    """(c): 64 x 64 cells of one pixel: 1024 distinct cells per tile and up to 1156 with the ring, the table has 256 entries, so most events
    go straight to the global rows"""
    mask = np.arange(1, 64 * 64 + 1, dtype=np.int32).reshape(64, 64)
    table, n = CN.identity_table(mask)
    rect = np.tile(np.array([[0, 64, 0, 64]], dtype=np.int32), (n, 1))
    rect[::3] = (10, 20, 10, 20)
    want = _equal_to_the_restatement(mask, table, n, rect)
    assert (want[0][:, 0] == 1).all() and (want[0][:, 12] == 4).all() and not want[0][:, 9:12].any()
    assert (want[0][:, 6:9].sum(axis=1) == 4).all() and want[0][:, 15].sum() == n - len(rect[::3]) + len([i for i in range(0, n, 3) if 10 <= i // 64 < 20 and 10 <= i % 64 < 20])


def test_one_cell_over_many_tiles():
    """(d): one cell fills 600 x 600: every tile adds to one row, and sum r^2 = 600 * (599 * 600 * 1199 / 6) passes 2^32"""
    mask = np.ones((600, 600), dtype=np.int32)
    sums, bbox = _gpu(mask, np.array([-1, 0], dtype=np.int32), 1, np.array([[100, 140, 0, 600]], dtype=np.int32))
    s1, s2 = 599 * 600 // 2, 599 * 600 * 1199 // 6
    assert sums[0].tolist() == [360000, 600 * s1, 600 * s1, 600 * s2, 600 * s2, s1 * s1, 0, 0, 2400, 2396, 0, 0, 4, 0, 0, 40 * 600]
    assert 600 * s2 > 1 << 32 and bbox.tolist() == [[0, 599, 0, 599]]
    want = MN.sums_arrays(mask, np.array([-1, 0], dtype=np.int32), 1, np.array([[100, 140, 0, 600]], dtype=np.int32))
    assert np.array_equal(sums, want[0]) and np.array_equal(bbox, want[1])


def test_cells_far_from_the_origin():
    """(e): 2100 x 40 with cells only below row 2040: the moments are moved from tile-local to image coordinates at r0 = 2016 .. 2080"""
    mask = np.zeros((2100, 40), dtype=np.int32)
    mask[2040:, :] = CN.random_mask(60, 40, 12, 5, radius=7.0)
    table, n = CN.identity_table(mask)
    want = _equal_to_the_restatement(mask, table, n, _rects(mask, table, n, patch=10))
    assert want[1][want[0][:, 0] > 0, 0].min() >= 2040 and want[0][:, 3].max() > 2040 * 2040


def test_the_border_lengths_of_the_contact_graph():
    """(f): on the planted mask column 6 is the per-cell sum of the pixel pairs of ops.contact_graph at reach 1"""
    mask, _ = CN.planted_mask()
    ids = np.arange(1, 521)
    md = torch.from_numpy(mask).to(_lib.require_gpu())
    g = ops.contact_graph(md, ids, 1)
    per_cell = np.zeros(520, dtype=np.int64)
    np.add.at(per_cell, g["src"], g["pairs"])
    got = ops.mask_morphology(md, ids)
    assert np.array_equal(got["sums"][:, 6], per_cell) and per_cell.sum() >= 2 * 5 * 120      # the 120 dominoes share five pixel edges each
    want = MN.sums_arrays(mask, CN.identity_table(mask)[0], 520)
    assert np.array_equal(got["sums"], want[0]) and np.array_equal(got["bbox"], want[1]) and got["sums"].dtype == np.int64
    empty = ops.mask_morphology(md, np.zeros(0, dtype=np.int64))
    assert empty["sums"].shape == (0, 16) and empty["bbox"].shape == (0, 4)
    with pytest.raises(ValueError, match="one rectangle"):
        ops.mask_morphology(md, ids, np.zeros((3, 4), dtype=np.int32))


def test_two_calls_give_the_same_bytes_and_no_rectangle_means_column_15_is_zero(generated):
    """(g)"""
    m, table, n, rect = generated
    one, two = _gpu(m, table, n, rect, junk=0x11), _gpu(m, table, n, rect, junk=0xEE)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    bare = _gpu(m, table, n, None, junk=0x3C)
    assert not bare[0][:, 15].any() and np.array_equal(bare[0][:, :15], one[0][:, :15]) and np.array_equal(bare[1], one[1]) and one[0][:, 15].any()


@pytest.mark.parametrize("patch", [40, 41])
def test_the_rectangle_is_the_window_the_patch_kernels_crop(patch):
    """morphology.patch_rect against what ribca_extract_patches (40) and ribca_extract_patches_scaled (41) read: the image holds 1 + the pixel's
    index, so the corner of a patch whose window starts deep inside its own cell (soft mask 1 up to 1e-6, an error of 0.02 at most here) names
    the pixel the window starts at.  A 30 x 50 cell in the image corner (the row start clamps at 0, the window's last ten rows leave the cell)
    and a 50 x 60 cell larger than the window: column 15 is the own pixels inside that window, 30 P and P P."""
    dev = _lib.require_gpu()
    h, w = 120, 130
    mask = np.zeros((h, w), dtype=np.int32)
    mask[0:30, 0:50], mask[60:110, 65:125] = 1, 2
    md = torch.from_numpy(mask).to(dev)
    image = torch.from_numpy((1.0 + np.arange(h * w, dtype=np.float32)).reshape(1, h, w)).to(dev)
    ids, table, ids_d, bbox_d = ops.label_table(md, with_device=True)
    patches = ops.extract_patches(image, md, ops.channel_min(image), ids_d, bbox_d, patch_size=patch)[0].cpu().numpy()
    rect = morphology.patch_rect(table[:, :4], h, w, patch)
    starts = np.rint(patches[:, 0, 0, 0]).astype(np.int64) - 1
    assert [(int(v) // w, int(v) % w) for v in starts] == [(int(r[0]), int(r[2])) for r in rect]
    assert rect[:, 0].tolist() == [0, 84 - (patch + 1) // 2] and rect[:, 1].tolist() == [patch, 84 - (patch + 1) // 2 + patch]
    got = ops.mask_morphology(md, ids, rect)
    assert got["sums"][:, 15].tolist() == [30 * patch, patch * patch] and got["sums"][:, 0].tolist() == [1500, 3000]
    assert morphology.features(got["sums"], got["bbox"])["patch_coverage"].tolist() == [30 * patch / 1500, patch * patch / 3000]


# ---- end to end: (h) -----------------------------------------------------------------------------------------------------------------------------
def _analyse(a):
    assert a.cell_morphology(integrate=True) is None
    integrated = list(a.morphology_stats)
    assert a.cell_morphology(integrate=False) is None
    return integrated


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two-image batch of the cell-type plots, annotated once with "Others" among the cell types, and analysed"""
    return annotated_batch(tmp_path_factory, "morphology", _analyse, "_morphology")


def _restated(a, i):
    """morphology.py on the restatement's tables of image i: (ids, types, features)"""
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    ids = np.asarray(a.preprocessor.cell_ids[i], dtype=np.int64)
    table = np.full(int(ids.max()) + 1, -1, dtype=np.int32)
    table[ids] = np.arange(len(ids))
    boxes = MN.sums_arrays(mask, table, len(ids))[1]
    rect = morphology.patch_rect(boxes, mask.shape[0], mask.shape[1], a.preprocessor.patch_size)
    return ids, a._cell_type_ints(i), morphology.features(*MN.sums_arrays(mask, table, len(ids), rect))


def _check_group(a, files, stem, tail, images, stats):
    from PIL import Image
    mid = "_means" if tail else ""      # x_morphology_{k}.csv is the cell table of image k
    t = len(a.cell_types)
    names = [str(c) for c in a.cell_types]
    parts = [_restated(a, i) for i in images]
    types = np.concatenate([p[1] for p in parts])
    feat = {k: np.concatenate([p[2][k] for p in parts]) for k in morphology.FEATURES}
    z = morphology.standardised_means(types, t, feat)
    assert np.isfinite(z).any()
    assert files[f"{stem}_summary{tail}.csv"].decode() == morphology.summary_csv(names, morphology.summary(types, t, feat))
    assert files[f"{stem}{mid}{tail}.csv"].decode() == morphology.matrix_csv(names, z)
    expected = [f"{stem}_summary{tail}.csv", f"{stem}{mid}{tail}.csv", f"{stem}{mid}{tail}.png"]
    assert stats["files"] == expected and stats["file"] == expected[0]
    assert stats["n"] == len(types) and stats["T"] == t and stats["euler_not_one"] == int((feat["euler"] != 1).sum())
    assert stats["patch_truncated"] == int((feat["patch_coverage"] < 1.0).sum()) and stats["on_image_edge"] == int(feat["on_image_edge"].sum())
    assert min(stats["kernel_ms"], stats["draw_ms"]) >= 0.0
    dev = _lib.require_gpu()
    img = np.array(Image.open(io.BytesIO(files[stats["figure"]["file"]])))
    top, left = stats["figure"]["rect"]
    cell = a.HEATMAP_CELL
    rect = ops.table_raster(torch.from_numpy(np.ascontiguousarray(z)).to(dev), torch.from_numpy(colors.diverging_table()).to(dev), cell, a.HEATMAP_GAP,
                            -3.0, 3.0).cpu().numpy()
    assert stats["figure"]["limit"] == 3.0 and np.array_equal(img[top:top + t * cell, left:left + len(morphology.FEATURES) * cell], rect)
    return expected


def _check_image(a, files, i):
    from PIL import Image
    names = [str(c) for c in a.cell_types]
    ids, types, feat = _restated(a, i)
    number = a._image_number(i)
    assert files[f"x_morphology_{number}.csv"].decode() == morphology.cells_csv(ids, types, names, feat)
    rows = files[f"x_morphology_{number}.csv"].decode().strip().split("\n")
    assert len(rows) == 1 + len(ids) and [int(r.split(",")[0]) for r in rows[1:]] == ids.tolist()
    assert np.array_equal(feat["area"], a.preprocessor.cell_tables[i][:, 6])      # the label table's pixel counts
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    lut = colors.viridis_table()
    for name, value in ((f"x_morphology_diameter_{number}.png", np.minimum(feat["equivalent_diameter"] / (2.0 * a.cell_size), 1.0)),
                        (f"x_morphology_coverage_{number}.png", feat["patch_coverage"])):
        img = np.array(Image.open(io.BytesIO(files[name])))
        assert img.shape == mask.shape + (3,) and (img[mask == 0] == 0).all()
        for j in (0, len(ids) // 2, len(ids) - 1, int(np.argmax(feat["area"]))):      # a pixel of a known cell
            r, c = np.argwhere(mask == ids[j])[0]
            assert img[r, c].tolist() == lut[int(value[j] * 255)].tolist(), (name, j)
    return [f"x_morphology_{number}.csv", f"x_morphology_diameter_{number}.png", f"x_morphology_coverage_{number}.png"]


def test_files_and_maps_are_the_restatement_s(batch):
    a, files = batch["a"], batch["files"]
    assert len(a.cell_types) >= 3 and len(batch["integrated"]) == 1 and len(a.morphology_stats) == 2
    expected = _check_group(a, files, "x_integrated_morphology", "", [0, 1], batch["integrated"][0])
    for i in (0, 1):
        expected += _check_group(a, files, "x_morphology", f"_{i}", [i], a.morphology_stats[i])
        per_image = _check_image(a, files, i)
        assert a.morphology_stats[i]["image_files"] == per_image
        expected += per_image
    assert sorted(files) == sorted(expected)
    log = open(a.logger.log_file_path).read()
    assert log.count("Cell morphology x_integrated_morphology_summary.csv: ") == 1 and log.count("Cell morphology x_morphology_summary_1.csv: ") == 1
    from multiplexed_image_annotator_amd.annotator import Annotator
    root = batch["root"]
    fresh = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", os.path.join(batch["tmp"], "fresh"), "x", False, False,
                      -1, True, 0.3, 99.8, 0.3, 30, None)
    with pytest.raises(ValueError, match="No annotations"):
        fresh.cell_morphology()


def test_pipeline_switch(tmp_path):
    """without --morphology no morphology file is written and no other file changes; with it the per-image and the integrated ones appear"""
    listing, _ = cli_runs(tmp_path, {"off": [], "on": ["--morphology"]}, "morphology")
    off, on = listing["off"], listing["on"]
    assert [f for f in on if "morphology" in f] == sorted(["c_morphology_0.csv", "c_morphology_diameter_0.png", "c_morphology_coverage_0.png",
                                                          "c_integrated_morphology_summary.csv", "c_integrated_morphology.csv", "c_integrated_morphology.png"])
    for f in off:
        if f.endswith(".csv") or f.endswith(".png"):
            assert open(tmp_path / "off" / "results" / f, "rb").read() == open(tmp_path / "on" / "results" / f, "rb").read(), f
    rows = open(tmp_path / "on" / "results" / "c_morphology_0.csv").read().split("\n")
    assert rows[0] == "cell_id,cell_type," + ",".join(morphology.FEATURES) and len(rows) > 100


def _rank_body(rank, root, thr):
    a = run_annotator(root, os.path.join(root, "tiles"), -1, thr)
    assert a.tile_mode
    integrated = _analyse(a)
    return [[s["file"] for s in integrated], [s["file"] for s in a.morphology_stats]]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], batch["thr"])
    assert result_files(os.path.join(batch["root"], "tiles"), "_morphology") == batch["files"]
    assert wrote == [[["x_integrated_morphology_summary.csv"], ["x_morphology_summary_0.csv"]], [[], ["x_morphology_summary_1.csv"]]]
