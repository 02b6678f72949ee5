"""Cell intensities on the GPU: ribca_cell_intensities (csrc/intensities.hip) against tests/intensities_numpy.py BYTE FOR BYTE -- the areas, the
fp64 sums and the fp32 order statistics -- on junk-filled outputs: images full of exact ties, negatives, both zeros and denormals; cells of one
pixel, of exactly ops.INTENSITY_RESIDENT pixels and of one more (the streaming form), one label over the whole image, a label in two blobs, boxes
that hold other cells or reach past the image, ids that are no cell; and Annotator.cell_intensities() end to end: files against the restatement
run on the same images, the maps, the pipeline switch, two ranks, the comparison with the window table on a constant marker."""
import io
import os

import numpy as np
import pytest
import torch

import intensities_numpy as IN
from batch_harness import annotated_batch, cli_runs, planted_case, result_files, run_annotator, two_ranks, weights
from multiplexed_image_annotator_amd import _lib, colors, intensities, ops

pytestmark = pytest.mark.gpu

QUARTILES = ((0, 1, 2, 3, 4), 4)
SEVENTHS = ((0, 7, 3, 3, 1, 0, 7, 5), 7)      # Q = 8, repeated numerators, 0 and q_den among them


def _gpu(image, mask, ids, bbox, q_num=QUARTILES[0], q_den=QUARTILES[1], junk=0xA5):
    """the entry point through ops on junk-filled outputs"""
    dev = _lib.require_gpu()
    c, n, q = image.shape[0], len(ids), len(q_num)
    out = (torch.full((n,), junk, dtype=torch.int32, device=dev), torch.full((n, c, 2), float(junk), dtype=torch.float64, device=dev),
           torch.full((n, c, q, 2), float(junk), dtype=torch.float32, device=dev))
    ops.cell_intensities(torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(dev),
                         torch.from_numpy(np.ascontiguousarray(mask, dtype=np.int32)).to(dev), np.asarray(ids, dtype=np.int32),
                         np.asarray(bbox, dtype=np.int32), q_num, q_den, out=out)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same_bytes(got, want, what, sums=True):
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), (what, "area")
    if sums:
        assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64)), (what, "sums", np.argwhere(got[1] != want[1])[:4])
    assert np.array_equal(got[2].view(np.int32), want[2].view(np.int32)), (what, "order", np.argwhere(got[2].view(np.int32) != want[2].view(np.int32))[:4])


def _generated_case():
    """the generated 100 x 130 mask and a 64-channel image; every label, one id the mask does not hold, ids <= 0; the box of label 5 reaches past
    the image on every side, the box of label 7 is cut so that it leaves out a part of the cell, the box of label 8 is grown by six pixels, so
    that a box one wave takes also holds other cells"""
    mask = IN.generated_mask(ops.INTENSITY_RESIDENT)
    image = IN.generated_image(64, 100, 130)
    ids = np.array(list(range(1, 41)) + [0, -3], dtype=np.int32)
    bbox = IN.boxes_of(mask, ids)
    bbox[4] = (bbox[4][0] - 50, bbox[4][1] + 200, bbox[4][2] - 7, bbox[4][3] + 500)
    bbox[6][1] -= 1
    bbox[7] += np.array([-6, 6, -6, 6], dtype=np.int32)
    assert len(np.unique(mask[bbox[7][0]:bbox[7][1] + 1, bbox[7][2]:bbox[7][3] + 1])) >= 3
    assert (bbox[7][1] - bbox[7][0] + 1) * (bbox[7][3] - bbox[7][2] + 1) <= ops.INTENSITY_SMALL_BOX
    return image, mask, ids, bbox


@pytest.fixture(scope="module")
def generated():
    image, mask, ids, bbox = _generated_case()
    return {"image": image, "mask": mask, "ids": ids, "bbox": bbox, "want15": IN.arrays(image[:15], mask, ids, bbox)}


def test_the_generated_case_at_15_channels(generated):
    g = generated
    want = g["want15"]
    assert want[0][:4].tolist() == [ops.INTENSITY_RESIDENT, ops.INTENSITY_RESIDENT + 1, 1, 53] and want[0][-3:].tolist() == [0, 0, 0]
    assert int((g["mask"] == 7).sum()) == 10 and want[0][6] == 8 and (want[0][:39] > 0).all()      # the cut box leaves out the last row of label 7
    got = _gpu(g["image"][:15], g["mask"], g["ids"], g["bbox"])
    _same_bytes(got, want, "C = 15")
    assert (got[2].view(np.uint32)[-3:] == IN.NAN_BITS).all() and not got[1][-3:].any()
    again = _gpu(g["image"][:15], g["mask"], g["ids"], g["bbox"], junk=0x3C)      # two calls, other junk: the same bytes
    _same_bytes(again, got, "second call")


@pytest.mark.parametrize("c", [1, 17, 64])
def test_other_channel_counts(generated, c):
    g = generated
    keep = np.array([0, 1, 2, 3, 7, 8, 38, 39, 40])      # both large cells, the pixel, the two blobs, small cells, no cell
    ids, bbox = g["ids"][keep], g["bbox"][keep]
    _same_bytes(_gpu(g["image"][:c], g["mask"], ids, bbox), IN.arrays(g["image"][:c], g["mask"], ids, bbox), f"C = {c}")


@pytest.mark.parametrize("q_num, q_den", [((1,), 2), SEVENTHS, ((4,), 4), ((0, 0, 4, 4, 2, 2, 1, 3), 4)])
def test_other_quantiles(generated, q_num, q_den):
    g = generated
    image = g["image"][20:23]
    _same_bytes(_gpu(image, g["mask"], g["ids"], g["bbox"], q_num, q_den), IN.arrays(image, g["mask"], g["ids"], g["bbox"], q_num, q_den), (q_num, q_den))


def test_subsets_and_other_orders_give_the_same_rows(generated):
    g = generated
    want = g["want15"]
    pick = np.array([39, 1, 3, 0, 41, 12, 2])
    got = _gpu(g["image"][:15], g["mask"], g["ids"][pick], g["bbox"][pick])
    _same_bytes(got, tuple(w[pick] for w in want), "subset")
    one = _gpu(g["image"][:15], g["mask"], g["ids"][3:4], g["bbox"][3:4])      # n = 1
    _same_bytes(one, tuple(w[3:4] for w in want), "n = 1")


@pytest.mark.parametrize("shape", [(100, 130), (1, 50), (50, 1), (1, 1), (8, 8), (5, 13), (16, 16), (1, 257), (32, 32), (32, 33)])
def test_one_label_over_the_whole_image(shape):
    """from the streaming form down to one pixel; 64 and 65 pixels (one wave's lanes), 256 and 257 (the partials), and a box of exactly
    ops.INTENSITY_SMALL_BOX pixels and the first above it, where the kernel changes"""
    h, w = shape
    image = IN.generated_image(3, h, w, seed=h + w)
    mask = np.full(shape, 9, dtype=np.int32)
    ids = np.array([9], dtype=np.int32)
    bbox = np.array([[0, h - 1, 0, w - 1]], dtype=np.int32)
    want = IN.arrays(image, mask, ids, bbox)
    assert want[0][0] == h * w and ops.INTENSITY_SMALL_BOX == 1024
    _same_bytes(_gpu(image, mask, ids, bbox), want, shape)
    _same_bytes(_gpu(image, mask, ids, bbox, *SEVENTHS), IN.arrays(image, mask, ids, bbox, *SEVENTHS), shape)


def test_a_streamed_cell_with_holes_and_a_scattered_cell_in_the_same_box():
    """label 1 is everything but a lattice of single pixels of label 2: the streamed cell's pixels are not contiguous in any chunk, so the
    compaction rank carried across chunks decides which partial an element reaches"""
    image = IN.generated_image(4, 100, 130, seed=2)
    mask = np.ones((100, 130), dtype=np.int32)
    mask[::7, ::5] = 2
    mask[50:, 129] = 0
    ids = np.array([2, 1], dtype=np.int32)
    bbox = IN.boxes_of(mask, ids)
    want = IN.arrays(image, mask, ids, bbox)
    assert want[0][1] > ops.INTENSITY_RESIDENT > want[0][0] > 256
    _same_bytes(_gpu(image, mask, ids, bbox), want, "lattice")


def test_infinite_pixels_order_statistics_only():
    image = IN.generated_image(2, 100, 130, seed=4)
    rng = np.random.default_rng(8)
    image[rng.random(image.shape) < 0.02] = np.inf
    image[rng.random(image.shape) < 0.02] = -np.inf
    mask = IN.generated_mask(ops.INTENSITY_RESIDENT)
    ids = np.arange(1, 40, dtype=np.int32)
    bbox = IN.boxes_of(mask, ids)
    want = IN.arrays(image, mask, ids, bbox)
    assert np.isinf(want[2]).any()
    _same_bytes(_gpu(image, mask, ids, bbox), want, "inf", sums=False)


# ------------------------------------------------------------------------------------------------------------------- Annotator.cell_intensities
def _analyse(a):
    assert a.cell_intensities(integrate=True) is None
    integrated = list(a.intensity_stats)
    assert a.cell_intensities(integrate=False) is None
    return integrated


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two-image batch of the cell-type plots, annotated once with "Others" among the cell types, and analysed"""
    return annotated_batch(tmp_path_factory, "intensities", _analyse, "_intensit")


def _markers(a):
    return [str(m) for m in a.channel_parser.markers]


def _restated(a, i):
    """intensities.py on the restatement's outputs for image i: (ids, types, area, features)"""
    image = a.preprocessor.images_dev[i].cpu().numpy()
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    ids = np.asarray(a.preprocessor.cell_ids[i], dtype=np.int64)
    area, sums, order = IN.arrays(image, mask, ids, np.asarray(a.preprocessor.cell_tables[i])[:, :4])
    return ids, a._cell_type_ints(i), area, intensities.features(area, sums, order)


def _check_group(a, files, stem, tail, images, stats):
    from PIL import Image
    mid = "_medians" if tail else ""      # x_intensities_{k}.csv is the cell table of image k
    t = len(a.cell_types)
    names = [str(c) for c in a.cell_types]
    markers = _markers(a)
    parts = [_restated(a, i) for i in images]
    types = np.concatenate([p[1] for p in parts])
    feat = np.concatenate([p[3] for p in parts])
    window = np.concatenate([a.preprocessor.intensity_full[i] for i in images])
    means, medians = feat[:, :, 0], feat[:, :, 4]
    z = intensities.standardised_medians(types, t, means)
    assert np.isfinite(z).any()
    assert files[f"{stem}_summary{tail}.csv"].decode() == intensities.summary_csv(names, markers, intensities.type_summary(types, t, means, medians))
    assert files[f"{stem}{mid}{tail}.csv"].decode() == intensities.matrix_csv(names, markers, z)
    assert files[f"{stem}_vs_window{tail}.csv"].decode() == intensities.vs_window_csv(markers, intensities.vs_window(means, window))
    expected = [f"{stem}_summary{tail}.csv", f"{stem}{mid}{tail}.csv", f"{stem}{mid}{tail}.png", f"{stem}_vs_window{tail}.csv"]
    assert stats["files"] == expected and stats["file"] == expected[0]
    assert stats["n"] == len(types) and stats["T"] == t and stats["C"] == len(markers) and stats["area_zero"] == 0 and stats["streamed"] == 0
    assert min(stats["kernel_ms"], stats["draw_ms"]) >= 0.0
    dev = _lib.require_gpu()
    img = np.array(Image.open(io.BytesIO(files[stats["figure"]["file"]])))
    top, left = stats["figure"]["rect"]
    cell = a.HEATMAP_CELL
    rect = ops.table_raster(torch.from_numpy(np.ascontiguousarray(z)).to(dev), torch.from_numpy(colors.diverging_table()).to(dev), cell, a.HEATMAP_GAP,
                            -3.0, 3.0).cpu().numpy()
    assert stats["figure"]["limit"] == 3.0 and np.array_equal(img[top:top + t * cell, left:left + len(markers) * cell], rect)
    return expected


def _check_image(a, files, i):
    from PIL import Image
    names = [str(c) for c in a.cell_types]
    markers = _markers(a)
    ids, types, area, feat = _restated(a, i)
    number = a._image_number(i)
    text = files[f"x_intensities_{number}.csv"].decode()
    assert text == intensities.cells_csv(ids, types, names, area, markers, intensities.statistic_names(), feat)
    rows = text.strip().split("\n")
    assert len(rows) == 1 + len(ids) and [int(r.split(",")[0]) for r in rows[1:]] == ids.tolist()
    assert np.array_equal(area, a.preprocessor.cell_tables[i][:, 6])      # the label table's pixel counts
    assert np.array_equal(a.intensity_mask[i], feat[:, :, 0])
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    lut = colors.viridis_table()
    cell_of = np.full(int(ids.max()) + 1, -1)
    cell_of[ids] = np.arange(len(ids))
    out = [f"x_intensities_{number}.csv"]
    for c, marker in enumerate(markers):
        name = f"x_intensity_{intensities.file_slug(marker)}_{number}.png"
        out.append(name)
        img = np.array(Image.open(io.BytesIO(files[name])))
        assert img.shape == mask.shape + (3,) and (img[mask == 0] == 0).all()
        colour = lut[(np.clip(feat[:, c, 0], 0.0, 1.0) * 255).astype(np.int64)]      # every painted pixel has its cell's colour
        assert np.array_equal(img[mask > 0], colour[cell_of[mask[mask > 0]]]), name
    return out


def test_files_and_maps_are_the_restatement_s(batch):
    a, files = batch["a"], batch["files"]
    assert len(a.cell_types) >= 3 and len(batch["integrated"]) == 1 and len(a.intensity_stats) == 2 and len(a.intensity_mask) == 2
    expected = _check_group(a, files, "x_integrated_intensities", "", [0, 1], batch["integrated"][0])
    for i in (0, 1):
        expected += _check_group(a, files, "x_intensities", f"_{i}", [i], a.intensity_stats[i])
        per_image = _check_image(a, files, i)
        assert a.intensity_stats[i]["image_files"] == per_image
        expected += per_image
    assert sorted(files) == sorted(expected)
    log = open(a.logger.log_file_path).read()
    assert log.count("Cell intensities x_integrated_intensities_summary.csv: ") == 1 and log.count("Cell intensities x_intensities_summary_1.csv: ") == 1
    before = sorted(os.listdir(os.path.join(batch["out"], "results")))
    a.cell_intensities(integrate=False, maps=False)      # no maps: the tables only, the same bytes
    assert sorted(os.listdir(os.path.join(batch["out"], "results"))) == before and result_files(batch["out"], "_intensit") == files
    assert not [f for f in a.intensity_stats[0]["image_files"] if f.endswith(".png")]
    from multiplexed_image_annotator_amd.annotator import Annotator
    root = batch["root"]
    fresh = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", os.path.join(batch["tmp"], "fresh"), "x", False, False,
                      -1, True, 0.3, 99.8, 0.3, 30, None)
    with pytest.raises(ValueError, match="No annotations"):
        fresh.cell_intensities()


def test_pipeline_switch(tmp_path):
    """without --intensities no intensity file is written and no other file changes; with it the per-image and the integrated ones appear"""
    listing, _ = cli_runs(tmp_path, {"off": [], "on": ["--intensities"]}, "_intensit")
    off, on = listing["off"], listing["on"]
    markers = [m for m in open(tmp_path / "case" / "markers.txt").read().split("\n") if m]
    assert [f for f in on if "_intensit" in f] == sorted(
        ["c_intensities_0.csv", "c_integrated_intensities_summary.csv", "c_integrated_intensities.csv", "c_integrated_intensities.png",
         "c_integrated_intensities_vs_window.csv"] + [f"c_intensity_{intensities.file_slug(m)}_0.png" for m in markers])
    for f in off:
        if f.endswith(".csv") or f.endswith(".png"):
            assert open(tmp_path / "off" / "results" / f, "rb").read() == open(tmp_path / "on" / "results" / f, "rb").read(), f
    rows = open(tmp_path / "on" / "results" / "c_intensities_0.csv").read().split("\n")
    assert rows[0].startswith(f"id,cell type,area,{markers[0]}_mean,{markers[0]}_std,{markers[0]}_min,") and len(rows) > 100


def test_a_constant_marker_is_the_same_in_both_tables(tmp_path):
    """a channel that holds one value everywhere: the exact mask mean and the window table's soft-mask-weighted mean are both that value, so the
    comparison reports difference 0 (and no correlation: neither column varies); a marker that varies inside the cells differs"""
    root = str(tmp_path / "case")
    planted_case(root, n_cells=60, h=160, w=200)
    raw = np.load(os.path.join(root, "img.npy"))
    raw[2] = 700
    np.save(os.path.join(root, "img.npy"), raw)
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", str(tmp_path / "out"), "k", False, False, -1, False, 0.3,
                  99.8, 0.0, 30, None)      # no normalisation: the image on the device is the file's
    a.set_weights(weights())
    a.preprocess()
    a.predict(16)
    a.export_annotations()
    a.cell_intensities(integrate=True, maps=False)
    rows = open(os.path.join(str(tmp_path / "out"), "results", "k_integrated_intensities_vs_window.csv")).read().strip().split("\n")
    assert rows[0] == "marker,pearson_r,mean_abs_difference,max_abs_difference" and len(rows) == 1 + raw.shape[0]
    constant = rows[3].split(",")
    assert constant[1:] == ["nan", "0", "0"]
    assert (a.intensity_mask[0][:, 2] == (700.0 + 1) / 2).all()
    other = [float(v) for v in rows[1].split(",")[1:]]
    assert other[1] > 0.0 and other[2] >= other[1]


def _rank_body(rank, root, thr):
    a = run_annotator(root, os.path.join(root, "tiles"), -1, thr)
    assert a.tile_mode
    integrated = _analyse(a)
    return [[s["file"] for s in integrated], [s["file"] for s in a.intensity_stats]]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], batch["thr"])
    assert result_files(os.path.join(batch["root"], "tiles"), "_intensit") == batch["files"]
    assert wrote == [[["x_integrated_intensities_summary.csv"], ["x_intensities_summary_0.csv"]], [[], ["x_intensities_summary_1.csv"]]]
