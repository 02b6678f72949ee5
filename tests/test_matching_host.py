"""Matching a second mask to the cells, without a GPU: tests/overlap_numpy.py (the restatement) against np.unique over 64-bit pair keys, and
multiplexed_image_annotator_amd/matching.py -- the owner rule, the per-cell, per-object and pair tables, the agreement at IoU 0.5 .. 0.95 and the
type summary -- against the restatement and against hand-built cases; the CSV texts pinned on one tiny case; the checks of
Annotator.mask_matching on a stub; the command line."""
import types

import numpy as np
import pytest
import torch

import contact_numpy as CN
import expand_numpy as XN
import overlap_numpy as ON
from multiplexed_image_annotator_amd import _lib, matching, ops
from multiplexed_image_annotator_amd.analyses import Analyses


def test_library_version_and_entry_points():
    assert _lib.lib().ribca_version() >= 112
    for name in ("ribca_mask_overlap_ws_bytes", "ribca_mask_overlap", "ribca_mask_compartments"):
        assert hasattr(_lib.lib(), name)
    assert ops.mask_overlap_ws_bytes(64, 64, 10, 8) == 512 + 768 + 256 and ops.mask_overlap_ws_bytes(64, 64, 10, 12) == 0
    assert callable(ops.overlap_pairs) and callable(ops.mask_compartments) and callable(Analyses.mask_matching)


def _case(seed, h=40, w=52, cells=30):
    """two random masks of one shape, their labels and the restated overlap"""
    ma = CN.random_mask(h, w, cells, seed)
    mb = CN.random_mask(h, w, cells + 3, seed + 1000, radius=3.5 + (seed % 3))
    ids_a, ids_b = ON.labels_of(ma), ON.labels_of(mb)
    pairs, area_a, area_b = ON.overlap(ma, ON.id_table(ids_a), len(ids_a), mb, ON.id_table(ids_b), len(ids_b))
    return ma, mb, ids_a, ids_b, pairs, area_a, area_b


def _arrays(pairs):
    return ON.pair_arrays(pairs)


def test_the_restated_pairs_are_np_unique_over_pair_keys():
    for seed in range(6):
        ma, mb, ids_a, ids_b, pairs, area_a, area_b = _case(seed)
        ca, cb = ON.index_image(ma, ON.id_table(ids_a), len(ids_a)), ON.index_image(mb, ON.id_table(ids_b), len(ids_b))
        both = (ca >= 0) & (cb >= 0)
        keys, counts = np.unique((ca[both] << 32) | cb[both], return_counts=True)
        assert {(int(k >> 32), int(k & 0xFFFFFFFF)): int(c) for k, c in zip(keys, counts)} == pairs and len(pairs) > 20
        assert np.array_equal(area_a, np.bincount(ca[ca >= 0], minlength=len(ids_a))) and np.array_equal(area_b, np.bincount(cb[cb >= 0], minlength=len(ids_b)))
        assert ON.id_table(ids_a).tolist() == ops._cell_table(ids_a).tolist()


def _owner_of(ma, mb, percent=50):
    ids_a, ids_b = ON.labels_of(ma), ON.labels_of(mb)
    pairs, area_a, area_b = ON.overlap(ma, ON.id_table(ids_a), len(ids_a), mb, ON.id_table(ids_b), len(ids_b))
    owner, inside = matching.owners(*_arrays(pairs), area_b, percent)
    assert owner.tolist() == ON.owners(pairs, area_b, percent)[0] and inside.tolist() == ON.owners(pairs, area_b, percent)[1]
    assert owner.dtype == np.int32 and inside.dtype == np.int64
    return owner.tolist(), inside.tolist()


def test_owner_rules_on_hand_built_cases():
    # a tie goes to the lowest cell: the object covers two pixels of cell 1 and two of cell 2
    ma = np.array([[1, 1, 2, 2], [1, 1, 2, 2], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int32)
    mb = np.array([[0, 5, 5, 0], [0, 5, 5, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int32)
    assert _owner_of(ma, mb) == ([0], [2])
    assert _owner_of(ma[:, ::-1].copy(), mb) == ([0], [2])                     # cell 2 on the left now: still the lowest INDEX, label 1 -> ... cell 0
    # exactly min_overlap percent is accepted: 4 of 8 pixels at 50 %, 3 of 8 are not
    ma = np.zeros((8, 8), dtype=np.int32)
    mb = np.zeros((8, 8), dtype=np.int32)
    ma[0:2, 0:2] = 3
    mb[0:2, 0:4] = 9
    assert _owner_of(ma, mb, 50) == ([0], [4])
    assert _owner_of(ma, mb, 51) == ([-1], [0])
    ma[1, 1] = 0                                                                    # one pixel less: an orphan
    assert _owner_of(ma, mb, 50) == ([-1], [0])
    mb[0, 3] = 0                                                                    # 3 of 7: 300 >= 42 * 7 = 294, 300 < 43 * 7 = 301
    assert _owner_of(ma, mb, 42) == ([0], [3]) and _owner_of(ma, mb, 43) == ([-1], [0])
    for bad in (0, 101, 50.0, True, None, "50"):
        with pytest.raises(ValueError, match="min_overlap must be an integer percent from 1 to 100"):
            matching.check_min_overlap(bad)
    assert matching.check_min_overlap(np.int64(100)) == 100


def test_the_owner_example_at_37_percent_is_accepted():
    """3 of 8 pixels: 300 >= 37 * 8 holds, 300 >= 38 * 8 = 304 does not -- integers, no rounding of 37.5"""
    ma = np.zeros((4, 4), dtype=np.int32)
    mb = np.zeros((4, 4), dtype=np.int32)
    ma[0, 0:3] = 1
    mb[0:2, 0:4] = 2
    assert _owner_of(ma, mb, 37) == ([0], [3]) and _owner_of(ma, mb, 38) == ([-1], [0])


def _agreement(pairs, area_a, area_b):
    counts, sums = matching.agreement_counts(*_arrays(pairs), area_a, area_b)
    w_counts, w_sums = ON.agreement_counts(pairs, area_a, area_b)
    assert counts.tolist() == w_counts and sums.tolist() == w_sums
    table = matching.agreement_table(counts, sums)
    assert table.tolist() == [[float(v) for v in row] for row in ON.agreement_rows(w_counts, w_sums)]
    return counts, sums, table


def test_iou_of_exactly_one_half_is_no_true_positive():
    """a cell of two pixels, two objects of one pixel inside it: IoU 1/2 each, and 100 > 50 * 2 is false; a solver-free matching must not count
    both"""
    ma = np.array([[1, 1, 0, 0]] + [[0] * 4] * 3, dtype=np.int32)
    mb = np.array([[1, 2, 0, 0]] + [[0] * 4] * 3, dtype=np.int32)
    pairs, area_a, area_b = ON.overlap(ma, ON.id_table([1]), 1, mb, ON.id_table([1, 2]), 2)
    assert pairs == {(0, 0): 1, (0, 1): 1}
    counts, sums, table = _agreement(pairs, area_a, area_b)
    assert counts[:, 2].tolist() == [0] * 10 and not sums.any() and table[0].tolist() == [1, 2, 0, 1, 2, 0, 0, 0, 0, 0]
    mb[0, 1] = 0                                  # one object of one pixel in a cell of two: still IoU 1/2
    pairs, area_a, area_b = ON.overlap(ma, ON.id_table([1]), 1, mb, ON.id_table([1]), 1)
    assert _agreement(pairs, area_a, area_b)[0][:, 2].tolist() == [0] * 10
    ma = np.array([[1, 1, 1, 0]] + [[0] * 4] * 3, dtype=np.int32)      # 2 of 3: IoU 2/3 is a true positive at 50 .. 65, not at 70
    mb = np.array([[2, 2, 0, 0]] + [[0] * 4] * 3, dtype=np.int32)
    pairs, area_a, area_b = ON.overlap(ma, ON.id_table([1]), 1, mb, ON.id_table([2]), 1)
    assert _agreement(pairs, area_a, area_b)[0][:, 2].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0]


def test_no_cell_and_no_object_is_in_two_true_positives():
    seen = 0
    for seed in range(50):
        ma, mb, ids_a, ids_b, pairs, area_a, area_b = _case(seed, 32, 36, 14)
        if seed % 2:                                  # every other pair of masks agrees closely: many true positives
            mb = ON.shifted_second_mask(ma, shift=1, zeroed=1, merged=2)
            ids_b = ON.labels_of(mb)
            pairs, area_a, area_b = ON.overlap(ma, ON.id_table(ids_a), len(ids_a), mb, ON.id_table(ids_b), len(ids_b))
        counts = _agreement(pairs, area_a, area_b)[0]
        for k, t in enumerate(ON.THRESHOLDS):
            tps = ON.true_positives(pairs, area_a, area_b, t)
            assert len(set(i for i, _, _ in tps)) == len(tps) == len(set(j for _, j, _ in tps)) == counts[k, 2]
            seen += len(tps)
        assert (np.diff(counts[:, 2]) <= 0).all()
    assert seen > 500


def test_identical_masks_agree_perfectly_and_an_empty_second_mask_not_at_all():
    ma, _, ids_a, _, _, _, _ = _case(3)
    n = len(ids_a)
    pairs, area_a, area_b = ON.overlap(ma, ON.id_table(ids_a), n, ma, ON.id_table(ids_a), n)
    counts, sums, table = _agreement(pairs, area_a, area_b)
    assert counts.tolist() == [[n, n, n]] * 10 and sums.tolist() == [float(n)] * 10
    assert table[:, 5:].tolist() == [[1.0] * 5] * 10 and table[:, 3:5].tolist() == [[0.0, 0.0]] * 10
    owner, inside = matching.owners(*_arrays(pairs), area_b)
    cells = matching.cell_rows(*_arrays(pairs), area_a, ids_a, owner)
    assert owner.tolist() == list(range(n)) and cells["status"].tolist() == [1] * n and cells["inner_fraction"].tolist() == [1.0] * n
    assert cells["object_id"].tolist() == ids_a
    # an empty B: no object at all
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64))
    owner, inside = matching.owners(*empty, np.zeros(0, np.int64))
    cells = matching.cell_rows(*empty, area_a, [], owner)
    assert len(owner) == 0 and cells["status"].tolist() == [0] * n and not cells["inner_area"].any() and cells["outer_area"].tolist() == area_a.tolist()
    assert len(matching.pair_rows(*empty, area_a, np.zeros(0, np.int64))[0]) == 0
    counts, sums, table = _agreement({}, area_a, np.zeros(0, np.int64))
    assert counts.tolist() == [[n, 0, 0]] * 10 and not table[:, 2].any() and not table[:, 5:].any() and table[:, 3].tolist() == [float(n)] * 10
    assert matching.cells_csv(ids_a, cells) == ON.image_texts(ma, np.zeros_like(ma))["cells_csv"]
    assert matching.objects_csv([], matching.object_rows(*empty, np.zeros(0, np.int64), ids_a, owner, inside)) == "id,area,cells,owner_id,inside,fraction,uncovered,status\n"


def _rows_equal(got, want, status_names):
    for k, row in enumerate(want):
        for key, value in row.items():
            mine = got[key][k]
            assert (status_names[int(mine)] if key == "status" else mine) == value, (k, key)


def test_every_table_is_the_restatement_s_and_the_areas_add_up():
    names = ["a", "b", "c"]
    per_image = []
    for seed in range(8):
        ma, mb, ids_a, ids_b, pairs, area_a, area_b = _case(seed)
        for percent in (50, 20, 100):
            owner, inside = matching.owners(*_arrays(pairs), area_b, percent)
            w_owner, w_inside = ON.owners(pairs, area_b, percent)
            assert owner.tolist() == w_owner and inside.tolist() == w_inside
            cells = matching.cell_rows(*_arrays(pairs), area_a, ids_b, owner)
            objects = matching.object_rows(*_arrays(pairs), area_b, ids_a, owner, inside)
            w_cells, w_objects = ON.cell_rows(pairs, area_a, ids_b, w_owner), ON.object_rows(pairs, area_b, ids_a, w_owner, w_inside)
            _rows_equal(cells, w_cells, matching.CELL_STATUS)
            _rows_equal(objects, w_objects, matching.OBJECT_STATUS)
            assert np.array_equal(cells["inner_area"] + cells["outer_area"], area_a) and (cells["outer_area"] >= cells["foreign_area"]).all()
            covered = np.bincount(_arrays(pairs)[1], weights=_arrays(pairs)[2], minlength=len(ids_b)).astype(np.int64)
            assert np.array_equal(objects["inside"] + (covered - objects["inside"]) + objects["uncovered"], area_b) and (objects["uncovered"] >= 0).all()
            assert int(cells["objects"].sum()) == int((owner >= 0).sum()) and int(cells["inner_area"].sum()) == int(inside.sum())
            types_ = np.arange(len(ids_a)) % 4 - (np.arange(len(ids_a)) % 7 == 0)      # -1 .. 3: labels outside the three names as well
            assert matching.cells_csv(ids_a, cells, types_, names) == ON.cells_csv(ids_a, w_cells, types_, names)
            assert matching.objects_csv(ids_b, objects) == ON.objects_csv(ids_b, w_objects)
            summary = matching.type_summary(types_, 3, cells["status"], cells["inner_fraction"])
            assert matching.summary_csv(names, summary) == ON.summary_csv(names, ON.type_summary(types_, 3, w_cells))
        union, iou = matching.pair_rows(*_arrays(pairs), area_a, area_b)
        assert matching.pairs_csv(ids_a, ids_b, *_arrays(pairs), union, iou) == ON.pairs_csv(ids_a, ids_b, ON.pair_rows(pairs, area_a, area_b))
        per_image.append(_agreement(pairs, area_a, area_b)[:2])
    counts, sums = matching.add_agreement(per_image)
    w_counts, w_sums = ON.add_agreement([ON.agreement_counts(*_case(seed)[4:]) for seed in range(8)])
    assert counts.tolist() == w_counts and sums.tolist() == w_sums
    assert matching.agreement_csv(matching.agreement_table(counts, sums)) == ON.agreement_csv(ON.agreement_rows(w_counts, w_sums))
    assert matching.type_summary([], 2, [], []).tolist()[0][:4] == [0, 0, 0, 0] and np.isnan(matching.type_summary([], 2, [], [])[:, 4:]).all()


def test_an_expanded_mask_against_its_nuclei():
    """A = the nuclei grown by three pixels, B = the nuclei: every object lies inside its own cell"""
    core = XN.random_discs(48, 60, 25, 7)
    grown = XN.expand(core, 3)[0]
    want = ON.image_texts(grown, core)
    ids, area_core, _ = XN.label_rows(core)
    assert want["ids_a"] == want["ids_b"] == ids.tolist() and len(ids) > 15
    assert [o["status"] for o in want["objects"]] == ["matched"] * len(ids) and [o["fraction"] for o in want["objects"]] == [1.0] * len(ids)
    assert [c["inner_area"] for c in want["cells"]] == area_core.tolist() and [c["status"] for c in want["cells"]] == ["single"] * len(ids)
    assert np.array_equal(want["inner"][core > 0], core[core > 0]) and not want["inner"][core <= 0].any()
    assert np.array_equal(want["inner"] + want["outer"], np.where(grown > 0, grown, 0))
    cell, obj, inter = ON.pair_arrays(want["pairs"])
    area_a = np.array([c["area"] for c in want["cells"]])
    owner, inside = matching.owners(cell, obj, inter, area_core)
    cells = matching.cell_rows(cell, obj, inter, area_a, ids, owner)
    assert cells["inner_area"].tolist() == area_core.tolist() and matching.cells_csv(ids, cells) == want["cells_csv"]
    assert (matching.fraction_colour_index(cells["inner_fraction"]) == (cells["inner_fraction"] * 255).astype(int)).all()


TINY_A = np.array([[1, 1, 1, 0, 0, 0],
                   [1, 1, 1, 0, 4, 4],
                   [2, 2, 0, 0, 4, 4],
                   [2, 2, 0, 0, 0, 0]], dtype=np.int32)
TINY_B = np.array([[0, 7, 7, 0, 0, 0],
                   [0, 7, 7, 7, 9, 0],
                   [3, 3, 0, 0, 0, 0],
                   [3, 0, 0, 0, 0, 5]], dtype=np.int32)


def test_every_text_is_pinned_on_one_tiny_case():
    want = ON.image_texts(TINY_A, TINY_B, 50, [1, 0, 7], ["x", "y"])
    cell, obj, inter = ON.pair_arrays(want["pairs"])
    ids_a, ids_b = [1, 2, 4], [3, 5, 7, 9]
    area_a, area_b = np.array([6, 4, 4]), np.array([3, 1, 5, 1])
    owner, inside = matching.owners(cell, obj, inter, area_b)
    cells = matching.cell_rows(cell, obj, inter, area_a, ids_b, owner)
    objects = matching.object_rows(cell, obj, inter, area_b, ids_a, owner, inside)
    union, iou = matching.pair_rows(cell, obj, inter, area_a, area_b)
    texts = (matching.cells_csv(ids_a, cells, [1, 0, 7], ["x", "y"]), matching.objects_csv(ids_b, objects), matching.pairs_csv(ids_a, ids_b, cell, obj, inter, union, iou))
    assert texts == (want["cells_csv"], want["objects_csv"], want["pairs_csv"])
    assert texts[0] == ("id,cell type,area,objects,object_id,inner_area,outer_area,inner_fraction,foreign_area,status\n"
                        "1,y,6,1,7,4,2,0.66666666666666663,0,single\n"
                        "2,x,4,1,3,3,1,0.75,0,single\n"
                        "4,,4,1,9,1,3,0.25,0,single\n")
    assert texts[1] == ("id,area,cells,owner_id,inside,fraction,uncovered,status\n"
                        "3,3,1,2,3,1,0,matched\n"
                        "5,1,0,0,0,0,1,orphan\n"
                        "7,5,1,1,4,0.80000000000000004,1,matched\n"
                        "9,1,1,4,1,1,0,matched\n")
    assert texts[2] == ("cell_id,object_id,intersection,union,iou\n"
                        "1,7,4,7,0.5714285714285714\n"
                        "2,3,3,4,0.75\n"
                        "4,9,1,4,0.25\n")
    counts, sums = matching.agreement_counts(cell, obj, inter, area_a, area_b)
    text = matching.agreement_csv(matching.agreement_table(counts, sums))
    assert text == ON.agreement_csv(ON.agreement_rows(*want["agreement"]))
    rows = text.split("\n")
    assert rows[0] == "threshold_percent,cells,objects,tp,unmatched_cells,unmatched_objects,precision,recall,f1,mean_matched_iou,panoptic_quality"
    assert rows[1] == "50,3,4,2,1,2,0.5,0.66666666666666663,0.5714285714285714,0.6607142857142857,0.37755102040816324"
    assert rows[5] == "70,3,4,1,2,3,0.25,0.33333333333333331,0.2857142857142857,0.75,0.21428571428571427"
    assert rows[6] == "75,3,4,0,3,4,0,0,0,0,0" and rows[10] == "95,3,4,0,3,4,0,0,0,0,0" and rows[11] == ""
    summary = matching.summary_csv(["x", "y"], matching.type_summary([1, 0, 7], 2, cells["status"], cells["inner_fraction"]))
    assert summary == ("cell_type,n,none,single,multi,mean_inner_fraction,median_inner_fraction\n"
                       "x,1,0,1,0,0.75,0.75\n"
                       "y,1,0,1,0,0.66666666666666663,0.66666666666666663\n"
                       "all,3,0,3,0,0.55555555555555547,0.66666666666666663\n")


# ---- Annotator.mask_matching: every error before any state change ---------------------------------------------------------------------------------
class _Stub(Analyses):
    def __init__(self, second_paths=None):
        self.preprocessor = types.SimpleNamespace(masks_dev=[torch.zeros((6, 8), dtype=torch.int32), torch.zeros((5, 5), dtype=torch.int32)], _n_images=2,
                                                  image_ids=[0, 1], second_mask_paths=second_paths)
        self.tile_mode, self.world_size, self.rank = False, 1, 0
        self.annotations, self.cell_types = [], []

    def _image_number(self, i):
        return self.preprocessor.image_ids[i]


def test_mask_matching_raises_before_any_state_change(tmp_path):
    good = [np.zeros((6, 8), dtype=np.int32), np.zeros((5, 5), dtype=np.int64)]
    np.save(tmp_path / "b.npy", np.zeros((6, 9), dtype=np.int32))
    cases = [(dict(), "needs a second mask per image: pass second_masks or add the column second_mask_path"),
             (dict(second_masks=good[:1]), "one second mask per row of the batch CSV, got 1 for 2 images"),
             (dict(second_masks=[good[0], np.zeros((5, 6), dtype=np.int32)]), r"second mask of image 1 must be an integer image of shape \(5, 5\)"),
             (dict(second_masks=[good[0].astype(np.float32), good[1]]), "second mask of image 0 must be an integer image"),
             (dict(second_masks=[str(tmp_path / "b.npy"), good[1]]), r"second mask of image 0 must be an integer image of shape \(6, 8\)"),
             (dict(second_masks=[good[0], None]), "image 1 has no second mask"),
             (dict(second_masks=good, min_overlap=0), "min_overlap must be an integer percent"),
             (dict(second_masks=good, min_overlap=50.0), "min_overlap must be an integer percent")]
    for kwargs, message in cases:
        a = _Stub()
        before = dict(vars(a))
        with pytest.raises(ValueError, match=message):
            a.mask_matching(**kwargs)
        assert vars(a) == before and not hasattr(a, "matching_stats") and not hasattr(a, "intensity_inner")
    a = _Stub(second_paths=[str(tmp_path / "b.npy"), float("nan")])
    with pytest.raises(ValueError, match=r"second mask of image 0 must be an integer image of shape \(6, 8\), got int32 \(6, 9\)"):
        a.mask_matching(intensities=True)
    assert not hasattr(a, "matching_stats") and not hasattr(a, "intensity_inner")
    empty = _Stub()
    empty.preprocessor.masks_dev, empty.preprocessor._n_images = [], 0
    with pytest.raises(ValueError, match="No masks"):
        empty.mask_matching(second_masks=[])


def test_the_batch_csv_column_is_kept(tmp_path):
    import inspect
    from multiplexed_image_annotator_amd import preprocess
    assert "second_mask_path" in inspect.getsource(preprocess.ImageProcessor.__init__)
    assert "compartment must be 'cell', 'core' or 'ring'" in inspect.getsource(Analyses.cell_intensities)      # the compartment names are not extended


def test_the_command_line_flags_default_off_and_reach_the_pipeline():
    from unittest import mock
    import main as cli
    base = ["--marker-list-path", "m.txt", "--batch-id", "b", "--batch-csv", "c.csv"]
    args = cli.parse_args(base)
    assert (args.match_masks, args.match_min_overlap, args.match_intensities, args.match_save_masks, args.second_mask_path) == (False, 50, False, False, None)
    args = cli.parse_args(base + ["--match-masks", "--match-min-overlap", "30", "--match-intensities", "--match-save-masks"])
    assert (args.match_masks, args.match_min_overlap, args.match_intensities, args.match_save_masks) == (True, 30, True, True)
    single = ["--marker-list-path", "m.txt", "--batch-id", "b", "--image-path", "i.npy", "--mask-path", "m.npy"]
    assert cli.parse_args(single + ["--match-masks", "--second-mask-path", "n.npy"]).second_mask_path == "n.npy"
    for bad in (single + ["--match-masks"], base + ["--match-min-overlap", "0"], base + ["--match-min-overlap", "101"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    for match in (None, dict(min_overlap=30, intensities=True, save_masks=False)):
        a = mock.MagicMock()
        a.min_cells_per_image.return_value = 0
        cli._pipeline(a, 16, 0, match=match)
        assert a.mask_matching.call_count == int(match is not None)
        if match is not None:
            assert a.mask_matching.call_args == mock.call(integrate=True, min_overlap=30, intensities=True, save_masks=False)
            order = [c[0] for c in a.method_calls]
            assert order.index("predict") < order.index("mask_matching") < order.index("clear_tmp")
