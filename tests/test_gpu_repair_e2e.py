"""Annotator(repair_mask=A) end to end on the two-image batch of the cell-type plots with faults painted into the mask files -- a label used
for two distant cells, a speck of two pixels, a hole, and a hole with a speck of another label inside: with 0 a run is byte for byte the run
that does not pass the argument; with 3 every stage reads the mask tests/components_numpy.py repairs from the file's -- the device and host
masks, the label table, the lazy pixel lists, the .npy and the repair CSV, the morphology areas --, cell_morphology reports an Euler number
of 1 for every cell but the one around the foreign speck, repair_mask=3 with expand_mask=2 is the restated expansion of the repaired mask,
and two tile-per-rank ranks write the single-rank bytes."""
import os

import numpy as np
import pytest
import torch

import components_numpy as CN
import expand_numpy as EN
from batch_harness import paint_faults, run_annotator, two_image_case, two_ranks, weights
from multiplexed_image_annotator_amd import _lib, ops

pytestmark = pytest.mark.gpu

A = 3
D = 2


def _run_repaired(root, out, **kw):
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", out, "x", False, False, -1, True, 0.3, 99.8, 0.0, 30, None,
                  **kw)
    a.set_weights(weights())
    a.preprocess()
    a.predict(16)
    a.export_annotations()
    return a


def _analyse(a):
    a.cell_morphology(integrate=False)
    a.colorize(from_script=True)


def _files(out):
    res = os.path.join(out, "results")
    return {f: open(os.path.join(res, f), "rb").read() for f in sorted(os.listdir(res)) if f != "log.txt"}      # the log carries the clock


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """four runs of one damaged batch: without the argument, with repair_mask = 0, with repair_mask = A, and with expand_mask = D on top"""
    tmp = tmp_path_factory.mktemp("repair")
    root = str(tmp / "case")
    os.makedirs(root)
    two_image_case(root)
    read, outer = [], []
    for d in ("a", "b"):
        path = os.path.join(root, d, "mask.npy")
        mask, enclosing = paint_faults(np.load(path).astype(np.int32))
        np.save(path, mask)
        read.append(mask)
        outer.append(enclosing)
    plain = run_annotator(root, str(tmp / "plain"), -1, 0.0)
    zero = _run_repaired(root, str(tmp / "zero"), repair_mask=0)
    fixed = _run_repaired(root, str(tmp / "fixed"), repair_mask=A)
    both = _run_repaired(root, str(tmp / "both"), repair_mask=A, expand_mask=D)
    for a in (plain, zero, fixed):
        _analyse(a)
    return {"root": root, "tmp": str(tmp), "plain": plain, "zero": zero, "fixed": fixed, "both": both, "read": read, "outer": outer,
            "want": [CN.repair(m, A) for m in read]}


def test_repair_mask_zero_is_the_run_without_the_argument(runs):
    plain, zero = runs["plain"], runs["zero"]
    a, b = _files(os.path.join(runs["tmp"], "plain")), _files(os.path.join(runs["tmp"], "zero"))
    assert sorted(a) == sorted(b) and len(a) > 8 and not [f for f in a if "repair" in f]
    for f in a:
        assert a[f] == b[f], f
    assert zero.repair_mask == 0 and zero.repair_stats == [] and plain.repair_stats == [] and zero.preprocessor.repair_rows == []
    for i in range(2):
        assert torch.equal(zero.preprocessor.masks_dev[i], plain.preprocessor.masks_dev[i])
        assert np.array_equal(zero.preprocessor.masks[i], runs["read"][i])
        for a_ in (zero, plain):
            assert a_.preprocessor.masks_core_dev[i] is a_.preprocessor.masks_dev[i]
            assert a_.preprocessor.core_tables[i] is a_.preprocessor.cell_tables[i]
            assert a_.preprocessor.core_bbox_dev[i] is a_.preprocessor.cell_bbox_dev[i]


def test_every_stage_reads_the_repaired_mask(runs):
    fixed = runs["fixed"]
    pre = fixed.preprocessor
    dev = _lib.require_gpu()
    res = os.path.join(runs["tmp"], "fixed", "results")
    assert fixed.repair_mask == A and pre.repair_mask == A and len(fixed.repair_stats) == 2
    for i in range(2):
        read, (want, text, counts) = runs["read"][i], runs["want"][i]
        assert (want != read).any()
        assert counts["components_split"] >= 2 and counts["components_dropped"] >= 1 and counts["holes_filled"] >= 1 and counts["holes_left"] >= 1
        assert np.array_equal(pre.masks_dev[i].cpu().numpy(), want) and pre.masks_dev[i].dtype == torch.int32
        assert np.array_equal(pre.masks[i], want) and pre.masks[i].dtype == np.int32
        assert pre.masks_core_dev[i] is pre.masks_dev[i] and pre.core_tables[i] is pre.cell_tables[i]      # the identities at expand_mask = 0
        ids, table = ops.label_table(torch.from_numpy(want).to(dev))
        assert np.array_equal(pre.cell_ids[i], ids) and np.array_equal(pre.cell_tables[i], table)
        assert np.array_equal(ids, np.unique(want[want > 0]))
        assert torch.equal(pre.cell_bbox_dev[i].cpu(), torch.from_numpy(np.ascontiguousarray(table[:, :4].astype(np.int32))))
        label = int(ids[-1])      # a label the repair made
        assert label > read.max()
        rows, cols = pre.cell_pos_dict[i][label]
        rr, cc = np.nonzero(want == label)
        assert rows == rr.tolist() and cols == cc.tolist()      # the lazy pixel lists are the repaired mask's
        saved = np.load(os.path.join(res, f"x_repaired_mask_{i}.npy"))
        assert saved.dtype == np.int32 and np.array_equal(saved, want)
        assert open(os.path.join(res, f"x_repair_{i}.csv")).read() == text
        rec = dict(fixed.repair_stats[i])
        assert rec.pop("files") == [f"x_repaired_mask_{i}.npy", f"x_repair_{i}.csv"] and rec.pop("repair_ms") > 0.0 and rec == counts
        _, area, _ = EN.label_rows(want)
        morph = open(os.path.join(res, f"x_morphology_{i}.csv")).read().strip().split("\n")
        assert morph[0].split(",")[:3] == ["cell_id", "cell_type", "area"]
        assert [int(r.split(",")[2]) for r in morph[1:]] == area.tolist()
    log = open(fixed.logger.log_file_path).read()
    assert log.count("Mask repair x_repair_0.csv: ") == 1 and log.count("Mask repair x_repair_1.csv: ") == 1


def _euler_column(path):
    rows = [r.split(",") for r in open(path).read().strip().split("\n")]
    k = rows[0].index("euler")
    return {int(r[0]): int(r[k]) for r in rows[1:]}


def test_after_the_repair_only_the_cell_around_the_foreign_speck_has_an_euler_number_other_than_one(runs):
    for i in range(2):
        before = _euler_column(os.path.join(runs["tmp"], "plain", "results", f"x_morphology_{i}.csv"))
        after = _euler_column(os.path.join(runs["tmp"], "fixed", "results", f"x_morphology_{i}.csv"))
        assert len([v for v in before.values() if v != 1]) >= 3      # the torn label, the two holes
        assert {c: v for c, v in after.items() if v != 1} == {runs["outer"][i]: 0}
    assert runs["fixed"].morphology_stats[0]["euler_not_one"] == 1


def test_repair_then_expand_is_the_restated_expansion_of_the_repaired_mask(runs):
    both = runs["both"]
    pre = both.preprocessor
    res = os.path.join(runs["tmp"], "both", "results")
    for i in range(2):
        repaired = runs["want"][i][0]
        grown = EN.expand(repaired, D)[0]
        assert (grown != repaired).any()
        assert np.array_equal(pre.masks_core_dev[i].cpu().numpy(), repaired) and np.array_equal(pre.masks_dev[i].cpu().numpy(), grown)
        assert np.array_equal(pre.masks[i], grown)
        assert np.array_equal(np.load(os.path.join(res, f"x_repaired_mask_{i}.npy")), repaired)
        assert np.array_equal(np.load(os.path.join(res, f"x_expanded_mask_{i}.npy")), grown)
        assert open(os.path.join(res, f"x_repair_{i}.csv")).read() == runs["want"][i][1]
        assert open(os.path.join(res, f"x_expansion_{i}.csv")).read() == EN.expansion_csv(repaired, grown)
    assert len(both.repair_stats) == 2 and len(both.expansion_stats) == 2


def _rank_body(rank, root):
    a = _run_repaired(root, os.path.join(root, "tiles"), repair_mask=A)
    assert a.tile_mode and len(a.repair_stats) == 1
    return a.repair_stats[0]["files"]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(runs):
    wrote = two_ranks(_rank_body, runs["root"])
    single = {f: b for f, b in _files(os.path.join(runs["tmp"], "fixed")).items() if "_repair" in f}
    tiles = {f: b for f, b in _files(os.path.join(runs["root"], "tiles")).items() if "_repair" in f}
    assert sorted(single) == ["x_repair_0.csv", "x_repair_1.csv", "x_repaired_mask_0.npy", "x_repaired_mask_1.npy"] and tiles == single
    assert wrote == [["x_repaired_mask_0.npy", "x_repair_0.csv"], ["x_repaired_mask_1.npy", "x_repair_1.csv"]]
