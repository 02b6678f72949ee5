"""The mask repair without a GPU: repair.py's decisions, fed with the component rows of the restatement in place of the kernel's the way
ops.repair_labels feeds them, give the mask and the CSV text of the restated repair (tests/components_numpy.py, plain loops over labels);
the properties of the result -- idempotent, every label one component, a hole is left only around another label, min_area = 1 drops nothing
--, the tie rule, the INT32_MAX refusal, and the ValueErrors of the constructors and the command line."""
import inspect
import os
import types

import numpy as np
import pytest

import components_numpy as CN
from multiplexed_image_annotator_amd import repair

INT32_MAX = 2 ** 31 - 1
SEEDS = (1, 2, 3, 4, 5, 6)
AREAS = (1, 3, 10)


def _rows(mask):
    """what ops._component_rows reads off the kernel's outputs, from the restatement's"""
    root, stats = CN.components(mask)
    roots = np.flatnonzero(stats[:, 0] > 0)
    return root, roots, mask.reshape(-1)[roots].astype(np.int64), stats[roots].astype(np.int64)


def host_repair(mask, min_area):
    """ops.repair_labels with numpy indexing in place of the two kernels"""
    mask = np.asarray(mask, dtype=np.int32)
    h, w = mask.shape
    root, roots, labels, rows = _rows(mask)
    fg = labels > 0
    action, new_id = repair.decide(roots[fg], labels[fg], rows[fg, 0], min_area)
    table = np.zeros(h * w, dtype=np.int32)
    table[roots[fg]] = new_id
    mid = table[root]
    root2, roots2, labels2, rows2 = _rows(mid)
    new2, hole, left = repair.fill(labels2, rows2[:, 1], rows2[:, 2], rows2[:, 3])
    table[:] = 0
    table[roots2] = new2
    out = table[root2]
    comps = repair.rows(roots[fg], labels[fg], rows[fg, 0], action, new_id, w, new2[hole], rows2[hole, 0])
    return out, comps, repair.stats(comps, min_area, int(hole.sum()), int(rows2[hole, 0].sum()), int(left.sum()), 0.5)


@pytest.fixture(scope="module")
def repaired():
    """(seed, min_area) -> (mask, repaired mask, rows, record), once"""
    out = {}
    for seed in SEEDS:
        mask = CN.damaged_discs(67, 131, 40, seed)
        for a in AREAS:
            out[seed, a] = (mask,) + host_repair(mask, a)
    return out


def test_the_decisions_give_the_restated_mask_and_text(repaired):
    faults = np.zeros(4, dtype=np.int64)
    for (seed, a), (mask, out, comps, record) in repaired.items():
        want, text, counts = CN.repair(mask, a)
        assert out.dtype == np.int32 and np.array_equal(out, want), (seed, a)
        assert repair.cells_csv(comps) == text
        assert record.pop("repair_ms") == 0.5 and record == counts
        assert text.split("\n")[0] == ",".join(repair.COLUMNS)
        faults += (counts["components_split"], counts["components_dropped"], counts["holes_filled"], counts["holes_left"])
    assert (faults > 0).all()      # the masks exercise every rule


def test_the_repair_is_idempotent(repaired):
    for (seed, a), (mask, out, comps, record) in repaired.items():
        again, comps2, record2 = host_repair(out, a)
        assert np.array_equal(again, out), (seed, a)
        assert record2["components_split"] == record2["components_dropped"] == record2["holes_filled"] == 0
        assert record2["labels_in"] == record2["labels_out"] == record["labels_out"] and record2["holes_left"] == record["holes_left"]
        assert (comps2[:, 4] == repair.KEPT).all() and np.array_equal(comps2[:, 0], comps2[:, 5]) and not comps2[:, 6].any()


def test_every_output_label_is_one_component_and_a_hole_is_left_only_around_another_label(repaired):
    from scipy import ndimage
    for (seed, a), (mask, out, comps, record) in repaired.items():
        for v in np.unique(out[out > 0]):
            own = out == v
            assert ndimage.label(own, structure=np.ones((3, 3), dtype=int))[1] == 1, (seed, a, v)
            assert own.sum() >= a
            outside, n = ndimage.label(~own)      # 4-connected: what the 8-connected label closes in
            for k in range(1, n + 1):
                region = outside == k
                rr, cc = np.nonzero(region)
                if rr.min() == 0 or cc.min() == 0 or rr.max() == out.shape[0] - 1 or cc.max() == out.shape[1] - 1:
                    continue
                assert (out[region] > 0).any(), (seed, a, v)      # enclosed by v: another cell sits inside
        assert (out >= 0).all()      # rule 5's enclosed background lies between SEVERAL labels: no single one closes it in


def test_min_area_one_drops_nothing(repaired):
    for seed in SEEDS:
        mask, out, comps, record = repaired[seed, 1]
        assert record["components_dropped"] == record["dropped_pixels"] == record["labels_removed"] == 0
        assert np.array_equal(out[mask > 0] > 0, np.ones(int((mask > 0).sum()), dtype=bool))      # every labelled pixel stays labelled
        assert len(comps) == record["labels_in"] + record["components_split"] == record["labels_out"]
        kept = comps[comps[:, 4] == repair.KEPT]
        assert np.array_equal(kept[:, 0], kept[:, 5]) and len(kept) == record["labels_in"]
        assert np.array_equal(np.sort(comps[comps[:, 4] == repair.SPLIT, 5]), int(mask.max()) + 1 + np.arange(record["components_split"]))
        assert comps[:, 6].sum() == record["hole_pixels"] == int((out > 0).sum() - (mask > 0).sum())


def test_equal_areas_go_to_the_smallest_root_and_new_ids_follow_the_roots():
    mask = np.zeros((9, 20), dtype=np.int32)
    mask[1:3, 12:14], mask[5:7, 2:4], mask[5:7, 16:18] = 7, 7, 7      # three pieces of four pixels: the first in raster order is the main one
    mask[1:4, 2:5] = 3
    mask[2, 3] = 0                                                    # a hole
    mask[7, 9:12] = 3                                                 # a smaller piece of 3
    out, comps, record = host_repair(mask, 1)
    assert out[1, 12] == 7 and out[5, 2] == 8 and out[5, 16] == 9 and out[7, 9] == 10 and out[2, 3] == 3
    assert repair.cells_csv(comps) == ("source_id,row,col,area,action,id,filled\n3,1,2,8,kept,3,1\n3,7,9,3,split,10,0\n"
                                       "7,1,12,4,kept,7,0\n7,5,2,4,split,8,0\n7,5,16,4,split,9,0\n")
    assert record == {"min_area": 1, "labels_in": 2, "labels_out": 5, "components_split": 3, "components_dropped": 0, "dropped_pixels": 0,
                      "labels_removed": 0, "holes_filled": 1, "hole_pixels": 1, "holes_left": 0, "repair_ms": 0.5}
    out, comps, record = host_repair(mask, 4)      # the piece of three pixels goes; a main piece goes too when it is small
    assert out[7, 9] == 0 and record["components_dropped"] == 1 and record["dropped_pixels"] == 3 and record["labels_removed"] == 0
    out, comps, record = host_repair(mask, 5)
    assert not (out == 7).any() and record["labels_removed"] == 1 and record["labels_out"] == 1 and set(np.unique(out)) == {0, 3}
    action, new_id = repair.decide([5, 9, 40], [2, 2, 2], [6, 6, 6], 1)
    assert action.tolist() == [0, 1, 1] and new_id.tolist() == [2, 3, 4]
    action, new_id = repair.decide([5, 9, 40], [2, 2, 2], [6, 7, 7], 7)
    assert action.tolist() == [2, 0, 1] and new_id.tolist() == [0, 2, 3]


def test_a_hole_with_a_foreign_speck_is_left_and_one_with_a_dropped_speck_is_filled():
    mask = np.zeros((12, 12), dtype=np.int32)
    mask[1:10, 1:10] = 5
    mask[3:7, 3:7] = 0
    mask[4:6, 4:6] = 8      # four pixels of another label inside the hole
    out, comps, record = host_repair(mask, 3)
    assert np.array_equal(out, mask) and record["holes_left"] == 1 and record["holes_filled"] == 0
    out, comps, record = host_repair(mask, 5)      # the speck is dropped first, then the hole is one label's
    assert (out[1:10, 1:10] == 5).all() and record["holes_filled"] == 1 and record["hole_pixels"] == 16 and record["labels_removed"] == 1
    assert comps[comps[:, 0] == 5, 6].tolist() == [16]


def test_new_ids_beyond_int32_max_are_refused():
    mask = np.zeros((3, 9), dtype=np.int32)
    mask[1, 1], mask[1, 4], mask[1, 7] = INT32_MAX - 1, INT32_MAX - 1, INT32_MAX - 1
    with pytest.raises(ValueError, match="INT32_MAX"):
        host_repair(mask, 1)
    with pytest.raises(ValueError, match="INT32_MAX"):
        CN.repair(mask, 1)
    mask[1, 7] = 0
    assert host_repair(mask, 1)[0][1, 4] == INT32_MAX      # one new id: the last one there is
    mask[1, 1], mask[1, 4] = INT32_MAX, INT32_MAX - 1      # nothing is split: nothing to refuse
    assert np.array_equal(host_repair(mask, 1)[0], mask)


def test_what_decide_refuses():
    for bad in (0, -1, True, 2.0, "3", None, 2 ** 31):
        with pytest.raises(ValueError, match="min_area must be an integer from 1 pixels up"):
            repair.check_min_area(bad)
    assert repair.check_min_area(np.int64(4)) == 4 and type(repair.check_min_area(np.int64(4))) is int
    assert repair.check_min_area(0, "repair_mask", allow_zero=True) == 0
    with pytest.raises(ValueError, match="ascending"):
        repair.decide([9, 5], [2, 2], [6, 6], 1)
    with pytest.raises(ValueError, match="foreground"):
        repair.decide([5, 9], [2, 0], [6, 6], 1)
    with pytest.raises(ValueError, match="one label and one area"):
        repair.decide([5, 9], [2], [6, 6], 1)
    action, new_id = repair.decide([], [], [], 3)
    assert len(action) == 0 and repair.cells_csv(repair.rows([], [], [], action, new_id, 7, [], [])) == ",".join(repair.COLUMNS) + "\n"


BAD = (-1, True, False, 2.0, "3", None)


def test_the_constructors_refuse_a_bad_repair_mask(tmp_path):
    from multiplexed_image_annotator_amd.annotator import Annotator
    from multiplexed_image_annotator_amd.preprocess import ImageProcessor
    markers, batch = str(tmp_path / "markers.txt"), str(tmp_path / "images.csv")
    with open(markers, "w") as f:
        f.write("DAPI\nCD45\nCD20\nCD4\nCD8\nCD3\n")
    with open(batch, "w") as f:
        f.write("image_path,mask_path\nnone.npy,none.npy\n")
    assert inspect.signature(ImageProcessor.__init__).parameters["repair_mask"].default == 0
    assert inspect.signature(Annotator.__init__).parameters["repair_mask"].default == 0
    for bad in BAD:
        with pytest.raises(ValueError, match="repair_mask must be an integer from 0 pixels up"):
            ImageProcessor(batch, None, str(tmp_path / "p"), "cuda", repair_mask=bad)
        with pytest.raises(ValueError, match="repair_mask must be an integer from 0 pixels up"):
            Annotator(markers, batch, "cuda", str(tmp_path / "a"), "x", False, repair_mask=bad)
    pre = ImageProcessor(batch, types.SimpleNamespace(), str(tmp_path / "p"), "cuda", repair_mask=np.int64(4))
    assert pre.repair_mask == 4 and type(pre.repair_mask) is int and pre.repair_rows == [] and pre.repair_records == [] and pre.expand_mask == 0
    a = Annotator(markers, batch, "cuda", str(tmp_path / "a"), "x", False, repair_mask=3, expand_mask=2)
    assert a.repair_mask == 3 and a.preprocessor.repair_mask == 3 and a.repair_stats == [] and a.expand_mask == 2
    assert Annotator(markers, batch, "cuda", str(tmp_path / "b"), "x", False).repair_mask == 0


def test_the_command_line():
    import main as cli
    common = ["--marker-list-path", "m.txt", "--image-path", "i.npy", "--mask-path", "k.npy", "--batch-id", "c"]
    assert cli.parse_args(common).repair_mask == 0
    assert cli.parse_args(common + ["--repair-mask", "12"]).repair_mask == 12
    for bad in ("-1", "2.5", "x", str(2 ** 31)):
        with pytest.raises(SystemExit):
            cli.parse_args(common + ["--repair-mask", bad])
    for fn in (cli.run, cli.batch_run):
        assert inspect.signature(fn).parameters["repair_mask"].default == 0
    for bad in (-1, True, 1.5):
        with pytest.raises(ValueError, match="repair_mask must be an integer from 0 pixels up"):
            cli.run("m.txt", "i.npy", "k.npy", "cuda", "unused", "c", 16, False, False, -1, 0, True, 0.3, 99.8, 0.3, 30, None, 0, repair_mask=bad)
        with pytest.raises(ValueError, match="repair_mask must be an integer from 0 pixels up"):
            cli.batch_run("m.txt", "b.csv", "cuda", "unused", "c", 16, False, False, -1, 0, True, 0.3, 99.8, 0.3, 30, None, repair_mask=bad)
    assert not os.path.exists("unused")
