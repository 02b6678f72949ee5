"""Annotator(expand_mask=D) end to end on the two-image batch of the cell-type plots: with 0 a run is byte for byte the run that does not pass the
argument; with 3 every stage reads the mask tests/expand_numpy.py grows from the file's -- the device and host masks, the label table, the
lazy pixel lists, the .npy and the expansion CSV, the morphology areas, the contact graph -- the core and ring intensity tables add up to the
cell's, and two tile-per-rank ranks write the single-rank bytes."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import expand_numpy as EN
from batch_harness import run_annotator, two_image_case, two_ranks, weights
from multiplexed_image_annotator_amd import _lib, ops

pytestmark = pytest.mark.gpu

D = 3
U = 2.0 ** -53      # the unit roundoff of fp64, as tests/test_intensities_host.py names it


def _run_expanded(root, out, expand_mask):
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", out, "x", False, False, -1, True, 0.3, 99.8, 0.0, 30, None,
                  expand_mask=expand_mask)
    a.set_weights(weights())
    a.preprocess()
    a.predict(16)
    a.export_annotations()
    return a


def _analyse(a):
    a.cell_morphology(integrate=False)
    a.contact_analysis(distance=1, n_perms=0, integrate=True)
    a.cell_intensities(integrate=False, maps=False)
    a.colorize(from_script=True)


def _files(out):
    res = os.path.join(out, "results")
    return {f: open(os.path.join(res, f), "rb").read() for f in sorted(os.listdir(res)) if f != "log.txt"}      # the log carries the clock


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """three runs of one batch: without the argument, with expand_mask = 0 and with expand_mask = D; each analysed the same way"""
    tmp = tmp_path_factory.mktemp("expand")
    root = str(tmp / "case")
    os.makedirs(root)
    two_image_case(root)
    plain = run_annotator(root, str(tmp / "plain"), -1, 0.0)
    zero = _run_expanded(root, str(tmp / "zero"), 0)
    grown = _run_expanded(root, str(tmp / "grown"), D)
    for a in (plain, zero, grown):
        _analyse(a)
    cores = [np.load(os.path.join(root, d, "mask.npy")).astype(np.int32) for d in ("a", "b")]
    return {"root": root, "tmp": str(tmp), "plain": plain, "zero": zero, "grown": grown, "cores": cores, "want": [EN.expand(m, D) for m in cores]}


def test_expand_mask_zero_is_the_run_without_the_argument(runs):
    plain, zero = runs["plain"], runs["zero"]
    a, b = _files(os.path.join(runs["tmp"], "plain")), _files(os.path.join(runs["tmp"], "zero"))
    assert sorted(a) == sorted(b) and len(a) > 10 and not [f for f in a if "expan" in f]
    for f in a:
        assert a[f] == b[f], f
    assert zero.expand_mask == 0 and zero.expansion_stats == [] and plain.expansion_stats == []
    for i in range(2):
        assert torch.equal(zero.preprocessor.masks_dev[i], plain.preprocessor.masks_dev[i])
        assert np.array_equal(zero.preprocessor.masks[i], runs["cores"][i])
        for a_ in (zero, plain):
            assert a_.preprocessor.masks_core_dev[i] is a_.preprocessor.masks_dev[i]
            assert a_.preprocessor.core_tables[i] is a_.preprocessor.cell_tables[i]
            assert a_.preprocessor.core_bbox_dev[i] is a_.preprocessor.cell_bbox_dev[i]


def test_every_stage_reads_the_grown_mask(runs):
    grown, plain = runs["grown"], runs["plain"]
    pre = grown.preprocessor
    dev = _lib.require_gpu()
    res = os.path.join(runs["tmp"], "grown", "results")
    assert grown.expand_mask == D and pre.expand_mask == D and len(grown.expansion_stats) == 2
    for i in range(2):
        core, (want, _, _) = runs["cores"][i], runs["want"][i]
        assert (want != core).any()
        assert np.array_equal(pre.masks_dev[i].cpu().numpy(), want) and pre.masks_dev[i].dtype == torch.int32
        assert np.array_equal(pre.masks[i], want) and pre.masks[i].dtype == np.int32
        assert np.array_equal(pre.masks_core_dev[i].cpu().numpy(), core) and pre.masks_core_dev[i] is not pre.masks_dev[i]
        assert np.array_equal(pre.cell_ids[i], plain.preprocessor.cell_ids[i])      # no label made, none lost
        ids, table = ops.label_table(torch.from_numpy(want).to(dev))
        assert np.array_equal(pre.cell_ids[i], ids) and np.array_equal(pre.cell_tables[i], table)
        assert np.array_equal(pre.core_tables[i], plain.preprocessor.cell_tables[i])
        assert torch.equal(pre.cell_bbox_dev[i].cpu(), torch.from_numpy(np.ascontiguousarray(table[:, :4].astype(np.int32))))
        label = int(ids[len(ids) // 2])
        rows, cols = pre.cell_pos_dict[i][label]
        rr, cc = np.nonzero(want == label)
        assert rows == rr.tolist() and cols == cc.tolist()      # the lazy pixel lists are the grown cell's
        saved = np.load(os.path.join(res, f"x_expanded_mask_{i}.npy"))
        assert saved.dtype == np.int32 and np.array_equal(saved, want)
        text = open(os.path.join(res, f"x_expansion_{i}.csv")).read()
        assert text == EN.expansion_csv(core, want)
        _, area_core, _ = EN.label_rows(core)
        _, area_cell, _ = EN.label_rows(want)
        rec = grown.expansion_stats[i]
        assert rec["n"] == len(ids) and rec["D"] == D and rec["pixels_grown"] == int((want != core).sum()) == int((area_cell - area_core).sum())
        assert rec["cells_unchanged"] == int((area_cell == area_core).sum()) and rec["expand_ms"] > 0.0
        assert rec["files"] == [f"x_expanded_mask_{i}.npy", f"x_expansion_{i}.csv"]
        morph = open(os.path.join(res, f"x_morphology_{i}.csv")).read().strip().split("\n")
        assert morph[0].split(",")[:3] == ["cell_id", "cell_type", "area"]
        assert [int(r.split(",")[2]) for r in morph[1:]] == area_cell.tolist()
    log = open(grown.logger.log_file_path).read()
    assert log.count("Mask expansion x_expansion_0.csv: ") == 1 and log.count("Mask expansion x_expansion_1.csv: ") == 1
    assert grown.contact_stats[0]["E"] >= plain.contact_stats[0]["E"] > 0      # grown cells touch at least where the cores touched


def _csv_areas(path):
    rows = open(path).read().strip().split("\n")
    assert rows[0].split(",")[:3] == ["id", "cell type", "area"]
    return np.array([int(r.split(",")[2]) for r in rows[1:]], dtype=np.int64)


def test_core_and_ring_intensities_add_up_to_the_cell(runs):
    grown, plain = runs["grown"], runs["plain"]
    res = os.path.join(runs["tmp"], "grown", "results")
    cell_means = [m.copy() for m in grown.intensity_mask]
    before = {f for f in os.listdir(res)}
    kept = grown.intensity_mask
    grown.cell_intensities(integrate=False, maps=False, compartment="core")
    assert [s["compartment"] for s in grown.intensity_stats] == ["core", "core"]
    assert grown.intensity_stats[0]["files"] == ["x_intensities_core_summary_0.csv", "x_intensities_core_medians_0.csv", "x_intensities_core_medians_0.png"]
    assert grown.intensity_stats[1]["image_files"] == ["x_intensities_core_1.csv"]
    grown.cell_intensities(integrate=True, maps=True, compartment="ring")
    assert [s["compartment"] for s in grown.intensity_stats] == ["ring"] and grown.intensity_mask is kept
    new = sorted(set(os.listdir(res)) - before)
    assert not [f for f in new if "vs_window" in f] and all("_intensities_core" in f or "_intensities_ring" in f or "_intensity_ring_" in f for f in new)
    markers = len(grown.channel_parser.markers)
    assert len([f for f in new if f.startswith("x_intensity_ring_") and f.endswith(".png")]) == 2 * markers
    assert {"x_integrated_intensities_ring_summary.csv", "x_integrated_intensities_ring.csv", "x_integrated_intensities_ring.png", "x_intensities_ring_0.csv",
            "x_intensities_core_summary_1.csv"} <= set(new)
    assert plain.intensity_stats[0]["compartment"] == "cell"
    checked = 0
    for i in range(2):
        core, (want, _, _) = runs["cores"][i], runs["want"][i]
        _, area_core, _ = EN.label_rows(core)
        _, area_cell, _ = EN.label_rows(want)
        # the core of the grown run is the cell of the plain run: the same image, mask and boxes, so the same bytes
        assert np.array_equal(grown.intensity_core[i], plain.intensity_mask[i]) and np.array_equal(grown.intensity_mask[i], cell_means[i])
        assert np.array_equal(_csv_areas(os.path.join(res, f"x_intensities_core_{i}.csv")), area_core)
        assert np.array_equal(_csv_areas(os.path.join(res, f"x_intensities_{i}.csv")), area_cell)
        area_ring = _csv_areas(os.path.join(res, f"x_intensities_ring_{i}.csv"))
        assert np.array_equal(area_ring, area_cell - area_core) and (area_ring > 0).any()
        # a_core f_core + a_ring f_ring = a_cell f_cell for the reported means f = (sum / a + 1) / 2: exact in exact arithmetic.  The bound is the
        # one tests/test_intensities_host.py states for a reported mean: an fp64 sum of a terms in any order is off by at most (a - 1) U S,
        # S = sum |v| <= a M with M = the largest |pixel| of the image, so the mean m by (a - 1) U M plus U |m| <= U M for the division, and f by
        # no more than that plus 2 U |f| for the addition of 1 (halving is exact).  The identity is evaluated in rationals: nothing else rounds
        image = grown.preprocessor.images_dev[i].cpu().numpy().astype(np.float64)
        big = float(np.abs(image).max())

        def tol(a, f):
            return (a - 1) * U * big + U * big + 2 * U * abs(f)

        fc, fr, fl = grown.intensity_core[i], grown.intensity_ring[i], cell_means[i]
        for k in np.flatnonzero((area_core > 0) & (area_ring > 0)):
            ac, ar, al = int(area_core[k]), int(area_ring[k]), int(area_cell[k])
            for c in range(fc.shape[1]):
                gap = abs(ac * Fraction(float(fc[k, c])) + ar * Fraction(float(fr[k, c])) - al * Fraction(float(fl[k, c])))
                bound = ac * tol(ac, fc[k, c]) + ar * tol(ar, fr[k, c]) + al * tol(al, fl[k, c])
                assert gap <= Fraction(bound), (i, k, c, float(gap), bound)
                checked += 1
    assert checked > 100


def test_a_compartment_needs_an_expansion(runs):
    for a in (runs["plain"], runs["zero"]):
        kept = a.intensity_stats
        for compartment in ("ring", "core"):
            with pytest.raises(ValueError, match="expand_mask > 0"):
                a.cell_intensities(compartment=compartment)
        assert a.intensity_stats is kept and not hasattr(a, "intensity_ring")
    with pytest.raises(ValueError, match="compartment must be"):
        runs["grown"].cell_intensities(compartment="membrane")


def _rank_body(rank, root):
    a = _run_expanded(root, os.path.join(root, "tiles"), D)
    assert a.tile_mode and len(a.expansion_stats) == 1
    return a.expansion_stats[0]["files"]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(runs):
    wrote = two_ranks(_rank_body, runs["root"])
    single = {f: b for f, b in _files(os.path.join(runs["tmp"], "grown")).items() if "_expan" in f}
    tiles = {f: b for f, b in _files(os.path.join(runs["root"], "tiles")).items() if "_expan" in f}
    assert sorted(single) == ["x_expanded_mask_0.npy", "x_expanded_mask_1.npy", "x_expansion_0.csv", "x_expansion_1.csv"] and tiles == single
    assert wrote == [["x_expanded_mask_0.npy", "x_expansion_0.csv"], ["x_expanded_mask_1.npy", "x_expansion_1.csv"]]
