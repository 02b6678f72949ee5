"""Annotator.marker_localization() end to end: a planted image whose cells carry one marker on their rim only and another in their interior
only, every file against the writers of localization.py run over the RESTATED depth and shell sums of the same device images, the maps, the two
groupings of the two-image batch, the pipeline switch, two tile-per-rank ranks, and a run with expand_mask, where the analysis reads the grown
mask."""
import io
import os

import numpy as np
import pytest
import torch

import localization_numpy as LN
from batch_harness import MARKERS, annotated_batch, cli_runs, planted_case, result_files, run_annotator, two_ranks, weights, write_case
from multiplexed_image_annotator_amd import _lib, colors, intensities, localization, ops

pytestmark = pytest.mark.gpu

BAND = 2
RIM, CORE = MARKERS.index("CD3"), MARKERS.index("Ki67")


def _markers(a):
    return [str(m) for m in a.channel_parser.markers]


def _restated(a, i):
    """the restatement on the device images of local image i: (ids, types, count, deepest, sums)"""
    image = a.preprocessor.images_dev[i].cpu().numpy()
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    ids = np.asarray(a.preprocessor.cell_ids[i], dtype=np.int64)
    depth2 = LN.depth(mask, localization.DEPTH)
    count, deepest, sums = LN.shell_sums(image, mask, depth2, ids, np.asarray(a.preprocessor.cell_tables[i])[:, :4], localization.edges2())
    return ids, a._cell_type_ints(i), count, deepest, sums


def _check_image(a, files, i, batch_id="x", maps=True):
    from PIL import Image
    names = [str(c) for c in a.cell_types]
    markers = _markers(a)
    ids, types, count, deepest, sums = _restated(a, i)
    feat = localization.features(count, deepest, sums, BAND)
    number = a._image_number(i)
    text = files[f"{batch_id}_localization_{number}.csv"].decode()
    assert text == localization.cells_csv(ids, types, names, markers, feat)
    rows = text.strip().split("\n")
    assert len(rows) == 1 + len(ids) and [int(r.split(",")[0]) for r in rows[1:]] == ids.tolist()
    assert rows[0].startswith(f"id,cell type,area,inradius,edge_area,inner_area,{markers[0]}_edge,{markers[0]}_inner,{markers[0]}_contrast,")
    assert np.array_equal(feat["area"], a.preprocessor.cell_tables[i][:, 6])      # the label table's pixel counts
    assert np.array_equal(a.localization_contrast[i], feat["contrast"], equal_nan=True)
    out = [f"{batch_id}_localization_{number}.csv"]
    if not maps:
        return out
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    lut = colors.diverging_table()
    cell_of = np.full(int(ids.max()) + 1, -1)
    cell_of[ids] = np.arange(len(ids))
    for c, marker in enumerate(markers):
        name = f"{batch_id}_localization_{intensities.file_slug(marker)}_{number}.png"
        out.append(name)
        img = np.array(Image.open(io.BytesIO(files[name])))
        assert img.shape == mask.shape + (3,) and (img[mask == 0] == 0).all()
        colour = lut[localization.colour_index(feat["contrast"][:, c])]      # every painted pixel has its cell's colour; a NaN cell entry 0
        assert np.array_equal(img[mask > 0], colour[cell_of[mask[mask > 0]]]), name
    return out


def _check_group(a, files, stem, tail, images, stats):
    from PIL import Image
    mid = "_medians" if tail else ""      # x_localization_{k}.csv is the cell table of image k
    t = len(a.cell_types)
    names = [str(c) for c in a.cell_types]
    markers = _markers(a)
    parts = [_restated(a, i) for i in images]
    types, count, deepest, sums = (np.concatenate([p[k] for p in parts]) for k in (1, 2, 3, 4))
    feat = localization.features(count, deepest, sums, BAND)
    summary = localization.summary(types, t, feat["contrast"])
    assert np.isfinite(summary[:, :, 3]).any()
    assert files[f"{stem}_profile{tail}.csv"].decode() == localization.profile_csv(names, markers, *localization.profile(types, t, count, sums))
    assert files[f"{stem}_summary{tail}.csv"].decode() == localization.summary_csv(names, markers, summary)
    assert files[f"{stem}{mid}{tail}.csv"].decode() == localization.matrix_csv(names, markers, summary[:, :, 3])
    expected = [f"{stem}_profile{tail}.csv", f"{stem}_summary{tail}.csv", f"{stem}{mid}{tail}.csv", f"{stem}{mid}{tail}.png"]
    assert stats["files"] == expected and stats["file"] == expected[0]
    assert stats["n"] == len(types) and stats["T"] == t and stats["C"] == len(markers) and stats["band"] == BAND
    assert stats["deeper"] == int((deepest == -1).sum()) and stats["undefined"] == int(np.isnan(feat["contrast"]).all(axis=1).sum())
    assert min(stats["kernel_ms"], stats["draw_ms"]) >= 0.0
    dev = _lib.require_gpu()
    img = np.array(Image.open(io.BytesIO(files[stats["figure"]["file"]])))
    top, left = stats["figure"]["rect"]
    cell = a.HEATMAP_CELL
    rect = ops.table_raster(torch.from_numpy(np.ascontiguousarray(summary[:, :, 3])).to(dev), torch.from_numpy(colors.diverging_table()).to(dev), cell,
                            a.HEATMAP_GAP, -1.0, 1.0).cpu().numpy()
    assert stats["figure"]["limit"] == 1.0 and np.array_equal(img[top:top + t * cell, left:left + len(markers) * cell], rect)
    return expected


# ------------------------------------------------------------------------------------------------------------------------------ the planted image
def test_a_rim_marker_and_an_interior_marker(tmp_path):
    """CD3 is painted on the pixels at most BAND pixels below their cell's edge (restated depth2 <= 4) and nowhere else, Ki67 on the deeper pixels
    and nowhere else.  After background subtraction a pixel painted 0 is 0, and the sigma = 0.3 blur moves under 2 % of a painted neighbourhood
    into it (exp(-1 / 0.18) = 0.4 % per 4-neighbour), so the unpainted compartment's mean stays below 1 / 19 of the painted one's: contrast > 0.9
    and < -0.9 for every cell with both compartments"""
    root = str(tmp_path / "planted")
    planted_case(root, n_cells=150, h=256, w=300)
    raw, mask = np.load(os.path.join(root, "img.npy")), np.load(os.path.join(root, "mask.npy")).astype(np.int32)
    depth2 = LN.depth(mask, localization.DEPTH)
    rim = (mask > 0) & (depth2 != -1) & (depth2 <= BAND * BAND)
    raw[RIM] = np.where(rim, 6000, 0)
    raw[CORE] = np.where((mask > 0) & ~rim, 6000, 0)
    case = tmp_path / "case"
    case.mkdir()
    marker_file, csv = write_case(case, raw, mask, MARKERS)
    from multiplexed_image_annotator_amd.annotator import Annotator
    out = str(tmp_path / "out")
    a = Annotator(marker_file, csv, "cuda", out, "x", False, False, -1, True, 0.3, 99.8, 0.0, 30, None)
    a.set_weights(weights())
    a.preprocess()
    a.predict(16)
    a.export_annotations()
    for bad in (0, 5, "2", 2.0, True):
        with pytest.raises(ValueError, match="band"):      # before anything is written or set
            a.marker_localization(band=bad)
    assert not hasattr(a, "localization_stats") and not hasattr(a, "localization_contrast") and not result_files(out, "_localization")
    assert a.marker_localization(band=BAND, integrate=True) is None
    assert np.array_equal(a.preprocessor.masks_dev[0].cpu().numpy(), mask)
    files = result_files(out, "_localization")
    expected = _check_group(a, files, "x_integrated_localization", "", [0], a.localization_stats[0]) + _check_image(a, files, 0)
    assert sorted(files) == sorted(expected) and a.localization_stats[0]["image_files"] == expected[4:]
    _, _, count, deepest, sums = _restated(a, 0)
    feat = localization.features(count, deepest, sums, BAND)
    both = (feat["edge_area"] > 0) & (feat["inner_area"] > 0)
    assert both.sum() > 100 and (~both).sum() == int(np.isnan(feat["contrast"][:, RIM]).sum())
    contrast = a.localization_contrast[0]
    assert (contrast[both, RIM] > 0.9).all(), contrast[both, RIM].min()
    assert (contrast[both, CORE] < -0.9).all(), contrast[both, CORE].max()
    assert np.array_equal(feat["edge_area"], [int((rim & (mask == v)).sum()) for v in a.preprocessor.cell_ids[0]])
    log = open(a.logger.log_file_path).read()
    assert log.count("Marker localization x_integrated_localization_profile.csv: ") == 1
    from multiplexed_image_annotator_amd.annotator import Annotator as Fresh
    fresh = Fresh(marker_file, csv, "cuda", str(tmp_path / "fresh"), "x", False, False, -1, True, 0.3, 99.8, 0.3, 30, None)
    with pytest.raises(ValueError, match="No annotations"):
        fresh.marker_localization()


# -------------------------------------------------------------------------------------------------------------------------- the two-image batch
def _analyse(a):
    assert a.marker_localization(band=BAND, integrate=True) is None
    integrated = list(a.localization_stats)
    assert a.marker_localization(band=BAND, integrate=False) is None
    return integrated


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two-image batch of the cell-type plots, annotated once with "Others" among the cell types, and analysed"""
    return annotated_batch(tmp_path_factory, "localization", _analyse, "_localization")


def test_files_and_maps_are_the_restatement_s(batch):
    a, files = batch["a"], batch["files"]
    assert len(a.cell_types) >= 3 and len(batch["integrated"]) == 1 and len(a.localization_stats) == 2 and len(a.localization_contrast) == 2
    expected = _check_group(a, files, "x_integrated_localization", "", [0, 1], batch["integrated"][0])
    for i in (0, 1):
        expected += _check_group(a, files, "x_localization", f"_{i}", [i], a.localization_stats[i])
        per_image = _check_image(a, files, i)
        assert a.localization_stats[i]["image_files"] == per_image
        expected += per_image
    assert sorted(files) == sorted(expected)
    log = open(a.logger.log_file_path).read()
    assert log.count("Marker localization x_integrated_localization_profile.csv: ") == 1 and log.count("Marker localization x_localization_profile_1.csv: ") == 1
    before = sorted(os.listdir(os.path.join(batch["out"], "results")))
    a.marker_localization(band=BAND, integrate=False, maps=False)      # no maps: the tables only, the same bytes
    assert sorted(os.listdir(os.path.join(batch["out"], "results"))) == before and result_files(batch["out"], "_localization") == files
    assert not [f for f in a.localization_stats[0]["image_files"] if f.endswith(".png")]


def test_pipeline_switch(tmp_path):
    """without --localization no localization file is written and no other file changes; with it the per-image and the integrated ones appear"""
    listing, _ = cli_runs(tmp_path, {"off": [], "on": ["--localization", str(BAND)]}, "_localization")
    off, on = listing["off"], listing["on"]
    markers = [m for m in open(tmp_path / "case" / "markers.txt").read().split("\n") if m]
    assert [f for f in on if "_localization" in f] == sorted(
        ["c_localization_0.csv", "c_integrated_localization_profile.csv", "c_integrated_localization_summary.csv", "c_integrated_localization.csv",
         "c_integrated_localization.png"] + [f"c_localization_{intensities.file_slug(m)}_0.png" for m in markers])
    for f in off:
        if f.endswith(".csv") or f.endswith(".png") or f.endswith(".npy"):
            assert open(tmp_path / "off" / "results" / f, "rb").read() == open(tmp_path / "on" / "results" / f, "rb").read(), f
    rows = open(tmp_path / "on" / "results" / "c_localization_0.csv").read().split("\n")
    assert rows[0].startswith("id,cell type,area,inradius,edge_area,inner_area,") and len(rows) > 100
    import main as cli
    with pytest.raises(SystemExit):
        cli.parse_args(["--marker-list-path", "m", "--batch-id", "b", "--image-path", "i", "--mask-path", "k", "--localization", "5"])


def _rank_body(rank, root, thr):
    a = run_annotator(root, os.path.join(root, "tiles"), -1, thr)
    assert a.tile_mode
    integrated = _analyse(a)
    return [[s["file"] for s in integrated], [s["file"] for s in a.localization_stats]]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], batch["thr"], tile=True)
    assert result_files(os.path.join(batch["root"], "tiles"), "_localization") == batch["files"]
    assert wrote == [[["x_integrated_localization_profile.csv"], ["x_localization_profile_0.csv"]], [[], ["x_localization_profile_1.csv"]]]


def test_with_expand_mask_the_analysis_reads_the_grown_mask(tmp_path):
    root = str(tmp_path / "case")
    planted_case(root, n_cells=150, h=256, w=300)
    from multiplexed_image_annotator_amd.annotator import Annotator
    out = str(tmp_path / "out")
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", out, "x", False, False, -1, True, 0.3, 99.8, 0.0, 30, None,
                  expand_mask=4)
    a.set_weights(weights())
    a.preprocess()
    a.predict(16)
    a.export_annotations()
    a.marker_localization(band=BAND, integrate=False, maps=False)
    core = np.load(os.path.join(root, "mask.npy")).astype(np.int32)
    grown = a.preprocessor.masks_dev[0].cpu().numpy()
    assert (grown != core).any() and np.array_equal(grown > 0, grown != 0)
    files = result_files(out, "_localization")
    _check_image(a, files, 0, maps=False)      # the restatement over masks_dev: the grown mask
    table = open(os.path.join(out, "results", "x_expansion_0.csv")).read().strip().split("\n")
    assert table[0].split(",")[:3] == ["id", "area_core", "area_cell"]
    rows = files["x_localization_0.csv"].decode().strip().split("\n")
    assert [r.split(",")[0] for r in rows[1:]] == [r.split(",")[0] for r in table[1:]]
    assert [int(r.split(",")[2]) for r in rows[1:]] == [int(r.split(",")[2]) for r in table[1:]]      # area == area_cell
    assert sum(int(r.split(",")[2]) for r in rows[1:]) == int((grown > 0).sum()) > int((core > 0).sum())
