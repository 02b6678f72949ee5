"""Label expansion without a GPU: the restatement tests/expand_numpy.py against scipy's Euclidean distance transform composed the way
skimage.segmentation.expand_labels composes it -- equal everywhere but on tie pixels, where scipy's scan order picks one of the tied labels --
the text of expand.py, and the ValueErrors of the constructors and the command line."""
import inspect
import os
import types

import numpy as np
import pytest

import expand_numpy as EN
from multiplexed_image_annotator_amd import _lib, expand, ops


def test_version():
    assert _lib.lib().ribca_version() >= 109
    assert ops.EXPAND_MAX_DISTANCE == 32 and ops.EXPAND_TILE == 32


def _scipy_expand(mask, d):
    """skimage.segmentation.expand_labels(mask, d) with every pixel <= 0 as background, and the squared distance beside it"""
    from scipy import ndimage
    dist, idx = ndimage.distance_transform_edt(mask <= 0, return_indices=True)
    grown = (mask <= 0) & (dist <= d)
    out = mask.copy()
    out[grown] = mask[idx[0][grown], idx[1][grown]]
    return out, grown, np.rint(dist * dist).astype(np.int64)


@pytest.mark.parametrize("shape, cells, d, seed", [((67, 131), 40, 1, 1), ((67, 131), 40, 3, 2), ((67, 131), 40, 8, 3), ((67, 131), 40, 16, 4),
                                                   ((67, 131), 12, 32, 5), ((96, 96), 60, 5, 6), ((128, 128), 150, 4, 7)])
def test_the_restatement_against_scipy_s_distance_transform(shape, cells, d, seed):
    mask = EN.random_discs(shape[0], shape[1], cells, seed)
    out, dist2, ties = EN.expand(mask, d)
    ref, grown, ref_d2 = _scipy_expand(mask, d)
    assert np.array_equal((out > 0) & (mask <= 0), grown) and grown.any()
    assert np.array_equal(dist2[grown], ref_d2[grown]) and not dist2[mask > 0].any() and (dist2[(mask <= 0) & ~grown] == -1).all()
    assert not (ties & ~grown).any()
    share = ties.sum() / grown.sum()
    print(f"[expand vs scipy] {shape} {cells} cells D = {d}: {int(grown.sum())} grown, {int(ties.sum())} ties ({100 * share:.1f} %), "
          f"{int((out != ref)[ties].sum())} of them differ")
    assert share < 0.10
    assert np.array_equal(out[~ties], ref[~ties])      # the comparison leaves out tie pixels only
    # on a tie pixel scipy's label is one of the labels at the smallest distance, and never smaller than the restatement's
    labelled = np.argwhere(mask > 0)
    for r, c in np.argwhere(ties):
        d2 = (labelled[:, 0] - r) ** 2 + (labelled[:, 1] - c) ** 2
        tied = mask[labelled[d2 == d2.min(), 0], labelled[d2 == d2.min(), 1]]
        assert d2.min() == dist2[r, c] and ref[r, c] in tied and out[r, c] == tied.min() and len(set(tied.tolist())) > 1


def test_the_restatement_on_hand_written_cases():
    mask = np.zeros((1, 5), dtype=np.int32)
    mask[0, 0], mask[0, 4] = 7, 3
    for m in (mask, mask[:, ::-1].copy()):
        out, dist2, ties = EN.expand(m, 2)
        assert out[0, 2] == 3 and dist2[0, 2] == 4 and ties[0].tolist() == [False, False, True, False, False]
    m = np.array([[0, -4, 0, 0, 9, 0, -2, 0, 0]], dtype=np.int32)
    out, dist2, ties = EN.expand(m, 3)
    assert out.tolist() == [[0, 9, 9, 9, 9, 9, 9, 9, 0]] and dist2.tolist() == [[-1, 9, 4, 1, 0, 1, 4, 9, -1]] and not ties.any()
    out, dist2, _ = EN.expand(m, 1)
    assert out.tolist() == [[0, -4, 0, 9, 9, 9, -2, 0, 0]] and dist2.tolist() == [[-1, -1, -1, 1, 0, 1, -1, -1, -1]]
    diag = np.zeros((4, 4), dtype=np.int32)
    diag[0, 0] = 5
    out, dist2, _ = EN.expand(diag, 2)      # Euclidean: (1, 1) is at squared distance 2, (2, 1) at 5 > 4
    assert out[1, 1] == 5 and dist2[1, 1] == 2 and out[2, 0] == 5 and out[2, 1] == 0 and dist2[2, 1] == -1


def test_the_expansion_table_and_its_text():
    core = np.zeros((8, 9), dtype=np.int32)
    core[1:3, 1:3] = 4
    core[5, 6] = 2
    core[7, 0] = 11
    grown, _, _ = EN.expand(core, 1)
    grown[7, 0], grown[6, 0], grown[7, 1] = 11, 0, 0      # as if label 11 had not grown
    ids, area_core, box_core = EN.label_rows(core)
    _, area_cell, box = EN.label_rows(grown)

    def table(area, b):      # ops.label_table's rows: the box, two sums the text does not use, the area
        return np.concatenate([b, np.zeros((len(b), 2), dtype=np.int64), area[:, None]], axis=1)

    rows = expand.rows(ids, table(area_core, box_core), table(area_cell, box))
    assert rows.dtype == np.int64 and rows.tolist() == [[2, 1, 5, 4, 4, 6, 5, 7], [4, 4, 12, 8, 0, 3, 0, 3], [11, 1, 1, 0, 7, 7, 0, 0]]
    text = expand.cells_csv(rows)
    assert text == "id,area_core,area_cell,grown,rmin,rmax,cmin,cmax\n2,1,5,4,4,6,5,7\n4,4,12,8,0,3,0,3\n11,1,1,0,7,7,0,0\n"
    assert text == EN.expansion_csv(core, grown) and expand.COLUMNS == tuple(text.split("\n")[0].split(","))
    assert expand.stats(rows, 1, 0.25) == {"n": 3, "D": 1, "pixels_grown": 12, "cells_unchanged": 1, "expand_ms": 0.25}
    empty = expand.rows(np.zeros(0), np.zeros((0, 7)), np.zeros((0, 7)))
    assert empty.shape == (0, 8) and expand.cells_csv(empty) == "id,area_core,area_cell,grown,rmin,rmax,cmin,cmax\n"
    assert expand.stats(empty, 5, 0.0)["pixels_grown"] == 0


BAD = (-1, 33, True, False, 2.0, "3", None)


def test_the_distance_check():
    for good in (1, 32, np.int32(7)):
        assert ops.check_expand_distance(good) == int(good)
    assert ops.check_expand_distance(0, "expand_mask", allow_zero=True) == 0
    for bad in BAD + (0,):
        with pytest.raises(ValueError, match="distance must be an integer from 1 to 32 pixels"):
            ops.check_expand_distance(bad)
    with pytest.raises(ValueError, match="expand_labels takes"):
        ops.expand_labels(np.zeros((4, 4), dtype=np.int32), 3)      # not a device tensor: refused before any library call


def test_the_constructors_refuse_a_bad_expand_mask(tmp_path):
    from multiplexed_image_annotator_amd.annotator import Annotator
    from multiplexed_image_annotator_amd.preprocess import ImageProcessor
    markers, batch = str(tmp_path / "markers.txt"), str(tmp_path / "images.csv")
    with open(markers, "w") as f:
        f.write("DAPI\nCD45\nCD20\nCD4\nCD8\nCD3\n")
    with open(batch, "w") as f:
        f.write("image_path,mask_path\nnone.npy,none.npy\n")
    assert inspect.signature(ImageProcessor.__init__).parameters["expand_mask"].default == 0
    assert inspect.signature(Annotator.__init__).parameters["expand_mask"].default == 0
    for bad in BAD:
        with pytest.raises(ValueError, match="expand_mask must be an integer from 0 to 32 pixels"):
            ImageProcessor(batch, None, str(tmp_path / "p"), "cuda", expand_mask=bad)
        with pytest.raises(ValueError, match="expand_mask must be an integer from 0 to 32 pixels"):
            Annotator(markers, batch, "cuda", str(tmp_path / "a"), "x", False, expand_mask=bad)
    pre = ImageProcessor(batch, types.SimpleNamespace(), str(tmp_path / "p"), "cuda", expand_mask=np.int64(4))
    assert pre.expand_mask == 4 and type(pre.expand_mask) is int and pre.masks_core_dev == [] and pre.core_tables == [] and pre.expand_ms == []
    a = Annotator(markers, batch, "cuda", str(tmp_path / "a"), "x", False, expand_mask=32)
    assert a.expand_mask == 32 and a.preprocessor.expand_mask == 32 and a.expansion_stats == []
    assert Annotator(markers, batch, "cuda", str(tmp_path / "b"), "x", False).expand_mask == 0


def test_the_command_line():
    """--expand-mask is 0 by default and refuses what the constructor refuses; run and batch_run raise the constructor's ValueError before anything
    is built; with --intensities an expanded run also writes the core and ring tables, without maps; the parameter stands before ``morphology``"""
    import main as cli
    common = ["--marker-list-path", "m.txt", "--image-path", "i.npy", "--mask-path", "k.npy", "--batch-id", "c"]
    assert cli.parse_args(common).expand_mask == 0
    assert cli.parse_args(common + ["--expand-mask", "32"]).expand_mask == 32
    for bad in ("-1", "33", "2.5"):
        with pytest.raises(SystemExit):
            cli.parse_args(common + ["--expand-mask", bad])
    for fn in (cli._pipeline, cli.run, cli.batch_run):
        params = list(inspect.signature(fn).parameters)
        assert inspect.signature(fn).parameters["expand_mask"].default == 0 and params[params.index("expand_mask") + 1] == "morphology"
    for bad in (33, -1, True, 1.5):
        with pytest.raises(ValueError, match="expand_mask must be an integer from 0 to 32 pixels"):
            cli.run("m.txt", "i.npy", "k.npy", "cuda", "unused", "c", 16, False, False, -1, 0, True, 0.3, 99.8, 0.3, 30, None, 0, expand_mask=bad)
        with pytest.raises(ValueError, match="expand_mask must be an integer from 0 to 32 pixels"):
            cli.batch_run("m.txt", "b.csv", "cuda", "unused", "c", 16, False, False, -1, 0, True, 0.3, 99.8, 0.3, 30, None, expand_mask=bad)
    assert not os.path.exists("unused")

    class Recorder:
        cell_size = 30
        channel_parser = types.SimpleNamespace(immune_base=True, immune_extended=False, immune_full=False, struct=False, nerve=False)

        def __init__(self):
            self.calls = []

        def min_cells_per_image(self):
            return 0

        def __getattr__(self, name):
            return lambda *a, **kw: self.calls.append((name, a, kw))

    off, grown, both = Recorder(), Recorder(), Recorder()
    cli._pipeline(off, 16, 0, intensities=True)
    cli._pipeline(grown, 16, 0, expand_mask=3)
    cli._pipeline(both, 16, 0, expand_mask=3, intensities=True)
    assert [c[2] for c in off.calls if c[0] == "cell_intensities"] == [{"integrate": True}]
    assert "cell_intensities" not in [c[0] for c in grown.calls]
    assert [c[2] for c in both.calls if c[0] == "cell_intensities"] == [
        {"integrate": True}, {"integrate": True, "maps": False, "compartment": "core"}, {"integrate": True, "maps": False, "compartment": "ring"}]
    assert [c[0] for c in both.calls if c[0] != "cell_intensities"] == [c[0] for c in off.calls if c[0] != "cell_intensities"]


def test_a_compartment_is_checked_before_any_state_changes():
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = object.__new__(Annotator)
    a.tile_mode = False
    a.annotations = [["A"]]
    a.cell_types = ["A", "B"]
    a.preprocessor = types.SimpleNamespace(expand_mask=0)
    for compartment in ("core", "ring"):
        with pytest.raises(ValueError, match="expand_mask > 0"):
            a.cell_intensities(compartment=compartment)
    with pytest.raises(ValueError, match="compartment must be"):
        a.cell_intensities(compartment="nucleus")
    assert not hasattr(a, "intensity_stats") and not hasattr(a, "intensity_core")
