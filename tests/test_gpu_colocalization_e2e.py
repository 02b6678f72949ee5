"""Annotator.marker_colocalization() end to end: a planted image whose cells carry two markers on the same half of every cell and a third on
the complementary half, every file against the writers of colocalization.py run over the RESTATED sums of the same device images, the maps, the
two groupings of the two-image batch, a selection of markers and named pairs, the pipeline switches, two tile-per-rank ranks, and the refusals
of more than 32 channels and of an unknown marker."""
import io
import os

import numpy as np
import pytest
import torch

import coloc_numpy as CN
from batch_harness import MARKERS, annotated_batch, cli_runs, planted_case, result_files, run_annotator, two_ranks, weights, write_case
from multiplexed_image_annotator_amd import _lib, colocalization, colors, intensities, ops

pytestmark = pytest.mark.gpu

SELECTED = ["CD3", "CD20", "Ki67", "CD4"]      # not in the order of the marker list
PAIRS = ["CD3:CD20", "CD4:CD3"]
A, B, C = MARKERS.index("CD3"), MARKERS.index("CD20"), MARKERS.index("Ki67")


def _restated(a, i, sel):
    """the restatement on the device images of local image i: (ids, types, area, both, sums, cross, gated)"""
    listed = [str(m) for m in a.channel_parser.markers]
    image = a.preprocessor.images_dev[i].cpu().numpy()
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    ids = np.asarray(a.preprocessor.cell_ids[i], dtype=np.int64)
    chan = [listed.index(m) for m in sel]
    out = CN.coloc(image, mask, ids, np.asarray(a.preprocessor.cell_tables[i])[:, :4], chan, colocalization.gates(0.15, len(chan)))
    return (ids, a._cell_type_ints(i)) + out


def _check_image(a, files, i, sel, pairs, batch_id="x", maps=True):
    from PIL import Image
    names = [str(c) for c in a.cell_types]
    ids, types, area, both, sums, cross, gated = _restated(a, i, sel)
    feat = colocalization.features(area, both, sums, cross, gated)
    number = a._image_number(i)
    text = files[f"{batch_id}_colocalization_{number}.csv"].decode()
    assert text == colocalization.cells_csv(ids, types, names, sel, area, feat["r"])
    rows = text.strip().split("\n")
    assert len(rows) == 1 + len(ids) and [int(r.split(",")[0]) for r in rows[1:]] == ids.tolist()
    assert rows[0].startswith(f"id,cell type,area,{sel[0]}~{sel[1]}_r,") and rows[0].count(",") == 2 + len(sel) * (len(sel) - 1) // 2
    assert np.array_equal(area, a.preprocessor.cell_tables[i][:, 6])      # the label table's pixel counts
    assert np.array_equal(a.colocalization_r[i], feat["r"], equal_nan=True)
    out = [f"{batch_id}_colocalization_{number}.csv"]
    columns = colocalization.parse_pairs(pairs, sel)
    if not columns:
        return out
    out.append(f"{batch_id}_colocalization_pairs_{number}.csv")
    assert files[out[-1]].decode() == colocalization.pairs_csv(ids, types, names, sel, columns, area, feat)
    if not maps:
        return out
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    lut = colors.diverging_table()
    cell_of = np.full(int(ids.max()) + 1, -1)
    cell_of[ids] = np.arange(len(ids))
    off = colocalization.off_pairs(len(sel))
    for col in columns:
        name = f"{batch_id}_colocalization_{intensities.file_slug(sel[off[col][0]])}_{intensities.file_slug(sel[off[col][1]])}_{number}.png"
        out.append(name)
        img = np.array(Image.open(io.BytesIO(files[name])))
        assert img.shape == mask.shape + (3,) and (img[mask == 0] == 0).all()
        colour = lut[colocalization.colour_index(feat["r"][:, col])]      # every painted pixel has its cell's colour; a NaN cell entry 0
        assert np.array_equal(img[mask > 0], colour[cell_of[mask[mask > 0]]]), name
    return out


def _check_group(a, files, stem, tail, images, stats, sel, pairs):
    from PIL import Image
    mid = "_medians" if tail else ""      # x_colocalization_{k}.csv is the cell table of image k
    t, k = len(a.cell_types), len(sel)
    names = [str(c) for c in a.cell_types]
    parts = [_restated(a, i, sel) for i in images]
    types, area, both, sums, cross, gated = (np.concatenate([p[j] for p in parts]) for j in (1, 2, 3, 4, 5, 6))
    feat = colocalization.features(area, both, sums, cross, gated)
    assert files[f"{stem}_summary{tail}.csv"].decode() == colocalization.summary_csv(names, sel, colocalization.summary(types, t, feat))
    expected = [f"{stem}_summary{tail}.csv"]
    present = [("", None)] + [("_" + intensities.file_slug(names[x]), types == x) for x in range(t) if (types == x).any()]
    assert len(present) >= 2
    dev = _lib.require_gpu()
    for n_fig, (suffix, rows) in enumerate(present):
        matrix = colocalization.median_matrix(feat["r"], k, rows)
        assert np.isfinite(matrix).all() or suffix
        assert files[f"{stem}{mid}{suffix}{tail}.csv"].decode() == colocalization.matrix_csv(sel, matrix)
        expected += [f"{stem}{mid}{suffix}{tail}.csv", f"{stem}{mid}{suffix}{tail}.png"]
        fig = stats["figures"][n_fig]
        img = np.array(Image.open(io.BytesIO(files[fig["file"]])))
        top, left = fig["rect"]
        cell = a.HEATMAP_CELL
        rect = ops.table_raster(torch.from_numpy(np.ascontiguousarray(matrix)).to(dev), torch.from_numpy(colors.diverging_table()).to(dev), cell,
                                a.HEATMAP_GAP, -1.0, 1.0).cpu().numpy()
        assert fig["file"] == expected[-1] and fig["limit"] == 1.0 and np.array_equal(img[top:top + k * cell, left:left + k * cell], rect)
    assert stats["files"] == expected and stats["file"] == expected[0] and stats["figure"] == stats["figures"][0]
    assert stats["n"] == len(types) and stats["T"] == t and stats["K"] == k and stats["markers"] == list(sel) and stats["threshold"] == 0.15
    assert stats["pairs"] == [colocalization.pair_names(sel)[c] for c in colocalization.parse_pairs(pairs, sel)]
    assert stats["valid"] == int((~np.isnan(feat["r"])).any(axis=1).sum()) and min(stats["kernel_ms"], stats["draw_ms"]) >= 0.0
    return expected


# ------------------------------------------------------------------------------------------------------------------------------ the planted image
def test_a_planted_pair_and_an_anti_pair_through_the_pipeline(tmp_path):
    """CD3 and CD20 are painted on the left half of every cell's box (CD20 at 0.8 of CD3's level, each with pixel noise of its own) and are 0
    elsewhere, Ki67 on the other half.  After background subtraction an unpainted pixel is 0, and the sigma = 0.3 blur moves under 2 % of a
    painted neighbour into it, so over a cell with both halves r(CD3, CD20) > 0.9, r(CD3, Ki67) < -0.9, and no pixel is above both gates of
    the anti-pair: jaccard = 0 and both Manders fractions under 5 %"""
    root = str(tmp_path / "planted")
    planted_case(root, n_cells=150, h=256, w=300)
    raw, mask = np.load(os.path.join(root, "img.npy")), np.load(os.path.join(root, "mask.npy")).astype(np.int32)
    rng = np.random.default_rng(3)
    cols = np.broadcast_to(np.arange(mask.shape[1])[None, :], mask.shape)
    mid = np.zeros(int(mask.max()) + 1)
    for v in np.unique(mask[mask > 0]):
        cc = cols[mask == v]
        mid[v] = (cc.min() + cc.max() + 1) / 2.0
    left = (mask > 0) & (cols < mid[mask])
    right = (mask > 0) & ~left
    raw[A] = np.where(left, 6000 * (1.0 + 0.05 * rng.standard_normal(mask.shape)), 0)
    raw[B] = np.where(left, 4800 * (1.0 + 0.05 * rng.standard_normal(mask.shape)), 0)
    raw[C] = np.where(right, 6000 * (1.0 + 0.05 * rng.standard_normal(mask.shape)), 0)
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
    for bad in (dict(markers=["CD3", "CD99"]), dict(markers=["CD3", "CD3"]), dict(markers=["CD3"]), dict(pairs=["CD3"]), dict(pairs=["CD3:CD99"]),
                dict(markers=["CD3", "CD20"], pairs=["CD3:Ki67"]), dict(threshold=1.0), dict(threshold=-0.1), dict(threshold="0.15")):
        with pytest.raises(ValueError):      # before anything is written or set
            a.marker_colocalization(**bad)
    assert not hasattr(a, "colocalization_stats") and not hasattr(a, "colocalization_r") and not result_files(out, "_colocalization")
    sel, pairs = ["CD3", "CD20", "Ki67"], ["CD3:CD20", "CD3:Ki67"]
    assert a.marker_colocalization(markers=sel, pairs=pairs, integrate=True) is None
    assert np.array_equal(a.preprocessor.masks_dev[0].cpu().numpy(), mask)
    files = result_files(out, "_colocalization")
    expected = _check_group(a, files, "x_integrated_colocalization", "", [0], a.colocalization_stats[0], sel, pairs)
    per_image = _check_image(a, files, 0, sel, pairs)
    assert sorted(files) == sorted(expected + per_image) and a.colocalization_stats[0]["image_files"] == per_image
    ids, _, area, both, sums, cross, gated = _restated(a, 0, sel)
    feat = colocalization.features(area, both, sums, cross, gated)
    halves = np.array([(left & (mask == v)).sum() >= 8 and (right & (mask == v)).sum() >= 8 for v in ids])
    assert halves.sum() > 100
    r = a.colocalization_r[0]
    assert (r[halves, 0] > 0.9).all(), r[halves, 0].min()
    assert (r[halves, 1] < -0.9).all(), r[halves, 1].max()
    assert not feat["jaccard"][halves, 1].any() and not feat["both"][halves, 1].any()
    assert (feat["m1"][halves, 1] < 0.05).all() and (feat["m2"][halves, 1] < 0.05).all()
    assert (feat["m1"][halves, 0] > 0.95).all() and (feat["jaccard"][halves, 0] > 0.9).all()
    log = open(a.logger.log_file_path).read()
    assert log.count("Marker colocalization x_integrated_colocalization_summary.csv: ") == 1
    from multiplexed_image_annotator_amd.annotator import Annotator as Fresh
    fresh = Fresh(marker_file, csv, "cuda", str(tmp_path / "fresh"), "x", False, False, -1, True, 0.3, 99.8, 0.3, 30, None)
    with pytest.raises(ValueError, match="No annotations"):
        fresh.marker_colocalization()


def test_more_than_32_channels_need_a_selection(tmp_path):
    rng = np.random.default_rng(5)
    mask = np.zeros((64, 64), dtype=np.int32)
    for j in range(30):
        r, c = 2 + 10 * (j // 6), 2 + 10 * (j % 6)
        mask[r:r + 7, c:c + 8] = j + 1
    markers = list(MARKERS) + [f"M{j}" for j in range(33 - len(MARKERS))]
    raw = rng.integers(100, 5000, size=(33, 64, 64)).astype(np.uint16)
    marker_file, csv = write_case(tmp_path, raw, mask, markers)
    from multiplexed_image_annotator_amd.annotator import Annotator
    out = str(tmp_path / "out")
    a = Annotator(marker_file, csv, "cuda", out, "x", False, False, -1, True, 0.3, 99.8, 0.0, 30, None)
    a.set_weights(weights())
    a.preprocess()
    a.predict(16)
    a.export_annotations()
    with pytest.raises(ValueError, match="select"):
        a.marker_colocalization()
    assert not hasattr(a, "colocalization_stats") and not result_files(out, "_colocalization")
    sel = markers[1:]      # 32 of the 33
    a.marker_colocalization(markers=sel, integrate=False, maps=False)
    _check_image(a, result_files(out, "_colocalization"), 0, sel, None)


# -------------------------------------------------------------------------------------------------------------------------- the two-image batch
def _analyse(a):
    assert a.marker_colocalization(markers=SELECTED, pairs=PAIRS, integrate=True) is None
    integrated = list(a.colocalization_stats)
    assert a.marker_colocalization(markers=SELECTED, pairs=PAIRS, integrate=False) is None
    return integrated


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two-image batch of the cell-type plots, annotated once with "Others" among the cell types, and analysed"""
    return annotated_batch(tmp_path_factory, "colocalization", _analyse, "_colocalization")


def test_files_and_maps_are_the_restatement_s(batch):
    a, files = batch["a"], batch["files"]
    assert len(a.cell_types) >= 3 and len(batch["integrated"]) == 1 and len(a.colocalization_stats) == 2 and len(a.colocalization_r) == 2
    expected = _check_group(a, files, "x_integrated_colocalization", "", [0, 1], batch["integrated"][0], SELECTED, PAIRS)
    for i in (0, 1):
        expected += _check_group(a, files, "x_colocalization", f"_{i}", [i], a.colocalization_stats[i], SELECTED, PAIRS)
        per_image = _check_image(a, files, i, SELECTED, PAIRS)
        assert a.colocalization_stats[i]["image_files"] == per_image
        expected += per_image
    assert sorted(files) == sorted(expected)
    assert "x_colocalization_CD3_CD20_0.png" in files and "x_colocalization_CD3_CD4_1.png" in files      # CD4:CD3 names the column CD3~CD4
    before = sorted(os.listdir(os.path.join(batch["out"], "results")))
    a.marker_colocalization(markers=SELECTED, pairs=PAIRS, integrate=False, maps=False)      # no maps: the tables only, the same bytes
    assert sorted(os.listdir(os.path.join(batch["out"], "results"))) == before and result_files(batch["out"], "_colocalization") == files
    assert not [f for f in a.colocalization_stats[0]["image_files"] if f.endswith(".png")]


def test_pipeline_switches(tmp_path):
    """without --colocalization no colocalisation file is written and no other file changes; with it the per-image table and the integrated
    files appear, with --coloc-markers / --coloc-pairs over the selection and with the pair table and maps"""
    listing, _ = cli_runs(tmp_path, {"off": [], "on": ["--colocalization"],
                                     "sel": ["--colocalization", "--coloc-markers", "CD3,CD20,Ki67", "--coloc-pairs", "CD20:CD3", "--coloc-threshold", "0.2"]},
                          "_colocalization")
    off, on, sel = listing["off"], listing["on"], listing["sel"]
    assert not [f for f in off if "_colocalization" in f]
    group = [f for f in on if "_integrated_colocalization" in f]
    assert [f for f in on if "_colocalization" in f] == sorted(["c_colocalization_0.csv"] + group)
    assert {"c_integrated_colocalization_summary.csv", "c_integrated_colocalization.csv", "c_integrated_colocalization.png"} <= set(group) and len(group) >= 5
    assert {"c_colocalization_0.csv", "c_colocalization_pairs_0.csv", "c_colocalization_CD3_CD20_0.png"} <= set(sel)
    for f in off:
        if f.endswith(".csv") or f.endswith(".png") or f.endswith(".npy"):
            for run in ("on", "sel"):
                assert open(tmp_path / "off" / "results" / f, "rb").read() == open(tmp_path / run / "results" / f, "rb").read(), (run, f)
    rows = open(tmp_path / "on" / "results" / "c_colocalization_0.csv").read().split("\n")
    assert rows[0].startswith(f"id,cell type,area,{MARKERS[0]}~{MARKERS[1]}_r,") and rows[0].count(",") == 2 + 66 and len(rows) > 100
    rows = open(tmp_path / "sel" / "results" / "c_colocalization_0.csv").read().split("\n")
    assert rows[0] == "id,cell type,area,CD3~CD20_r,CD3~Ki67_r,CD20~Ki67_r"
    rows = open(tmp_path / "sel" / "results" / "c_colocalization_pairs_0.csv").read().split("\n")
    assert rows[0] == "id,cell type,area," + ",".join(f"CD3~CD20_{s}" for s in colocalization.STATS)
    import main as cli
    base = ["--marker-list-path", str(tmp_path / "case" / "markers.txt"), "--batch-id", "b", "--image-path", "i", "--mask-path", "k"]
    assert cli.parse_args(base).coloc is None and cli.parse_args(base + ["--coloc-markers", "nonsense"]).coloc is None      # inert without the switch
    assert cli.parse_args(base + ["--colocalization"]).coloc == dict(markers=None, pairs=None, threshold=0.15)
    for bad in (["--coloc-markers", "CD3,CD99"], ["--coloc-markers", "CD3"], ["--coloc-markers", "CD3,CD3"], ["--coloc-pairs", "CD3"],
                ["--coloc-pairs", "CD3:CD99"], ["--coloc-pairs", "CD3:CD3"], ["--coloc-threshold", "1"], ["--coloc-threshold", "-0.5"],
                ["--coloc-markers", "CD3,CD20", "--coloc-pairs", "CD3:Ki67"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + ["--colocalization"] + bad)


def _rank_body(rank, root, thr):
    a = run_annotator(root, os.path.join(root, "tiles"), -1, thr)
    assert a.tile_mode
    integrated = _analyse(a)
    return [[s["file"] for s in integrated], [s["file"] for s in a.colocalization_stats]]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], batch["thr"], tile=True)
    assert result_files(os.path.join(batch["root"], "tiles"), "_colocalization") == batch["files"]
    assert wrote == [[["x_integrated_colocalization_summary.csv"], ["x_colocalization_summary_0.csv"]], [[], ["x_colocalization_summary_1.csv"]]]
