"""Annotator.mask_matching end to end on the two-image batch of the cell-type plots, with a batch CSV of its own that carries
``second_mask_path``: (a) a run with expand_mask = 3 matched against the mask file itself -- the nuclei -- reproduces the expansion table, the
core mask and the core / ring intensity tables byte for byte; (b) a second mask made by shifting the first two columns, zeroing three labels
and merging two gives the texts of tests/overlap_numpy.py, the painted map and the counted statistics; reruns, errors, the command line and
two tile-per-rank ranks."""
import io
import os

import numpy as np
import pytest
import torch

import overlap_numpy as ON
from batch_harness import planted_case, result_files, two_image_case, two_ranks, weights
from multiplexed_image_annotator_amd import colors

pytestmark = pytest.mark.gpu


def _write_case(root):
    """the two images, ``second.npy`` beside each mask, and two batch CSVs with the column: ``self.csv`` (B = the mask file) and ``match.csv``"""
    two_image_case(root)
    rows = {"self.csv": [], "match.csv": []}
    for d in ("a", "b"):
        mask = np.load(os.path.join(root, d, "mask.npy")).astype(np.int32)
        np.save(os.path.join(root, d, "second.npy"), ON.shifted_second_mask(mask, shift=2, zeroed=3, merged=2))
        img, mk = os.path.join(root, d, "img.npy"), os.path.join(root, d, "mask.npy")
        rows["self.csv"].append(f"{img},{mk},{mk}")
        rows["match.csv"].append(f"{img},{mk},{os.path.join(root, d, 'second.npy')}")
    for name, lines in rows.items():
        with open(os.path.join(root, name), "w") as f:
            f.write("image_path,mask_path,second_mask_path\n" + "\n".join(lines) + "\n")


def _annotator(root, csv, out, expand_mask=0, predict=True):
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, csv), "cuda", out, "x", False, False, -1, True, 0.3, 99.8, 0.0, 30, None,
                  expand_mask=expand_mask)
    a.set_weights(weights())
    a.preprocess()
    if predict:
        a.predict(16)
        a.export_annotations()
    return a


def _files(out):
    return result_files(out, ("_matching", "intensities_inner", "intensities_outer"))


def _match_both_ways(a):
    assert a.mask_matching(integrate=True) is None
    integrated = list(a.matching_stats)
    assert a.mask_matching(integrate=False) is None
    return integrated


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("matching")
    root = str(tmp / "case")
    os.makedirs(root)
    _write_case(root)
    out = str(tmp / "shifted")
    a = _annotator(root, "match.csv", out)
    integrated = _match_both_ways(a)
    return {"root": root, "tmp": str(tmp), "a": a, "out": out, "integrated": integrated, "files": _files(out)}


def _column(text, name):
    rows = [r.split(",") for r in text.strip().split("\n")]
    k = rows[0].index(name)
    return [r[k] for r in rows[1:]]


def test_an_expanded_run_against_its_own_nuclei(batch):
    """(a): A = the mask grown by three pixels, B = the mask file"""
    out = os.path.join(batch["tmp"], "grown")
    a = _annotator(batch["root"], "self.csv", out, expand_mask=3)
    assert a.mask_matching(intensities=True, save_masks=True, integrate=True) is None
    a.cell_intensities(integrate=True, maps=False, compartment="core")
    a.cell_intensities(integrate=True, maps=False, compartment="ring")
    res = os.path.join(out, "results")
    text = lambda name: open(os.path.join(res, name)).read()      # noqa: E731
    for i in range(2):
        cells = text(f"x_matching_cells_{i}.csv")
        assert _column(cells, "inner_area") == _column(text(f"x_expansion_{i}.csv"), "area_core") and len(_column(cells, "id")) > 100
        assert set(_column(cells, "status")) == {"single"} and _column(cells, "object_id") == _column(cells, "id")
        assert set(_column(text(f"x_matching_objects_{i}.csv"), "status")) == {"matched"}
        assert set(_column(text(f"x_matching_objects_{i}.csv"), "fraction")) == {"1"}
        inner, outer = np.load(os.path.join(res, f"x_matching_inner_{i}.npy")), np.load(os.path.join(res, f"x_matching_outer_{i}.npy"))
        core, grown = a.preprocessor.masks_core_dev[i].cpu().numpy(), a.preprocessor.masks_dev[i].cpu().numpy()
        assert inner.dtype == np.int32 and np.array_equal(inner, core) and np.array_equal(outer, np.where(core > 0, 0, grown)) and (outer > 0).any()
        # the same pixel sets in the same row-major order through the same fixed summation tree: the same bytes
        assert text(f"x_intensities_inner_{i}.csv") == text(f"x_intensities_core_{i}.csv")
        assert text(f"x_intensities_outer_{i}.csv") == text(f"x_intensities_ring_{i}.csv")
        assert np.array_equal(a.intensity_inner[i], a.intensity_core[i], equal_nan=True) and np.array_equal(a.intensity_outer[i], a.intensity_ring[i], equal_nan=True)
    rec = a.matching_stats[0]
    assert rec["none"] == 0 and rec["multi"] == 0 and rec["orphans"] == 0 and rec["n"] == rec["m"] == rec["pairs"]
    assert [f for f in rec["image_files"] if f.endswith("_0.npy") or "intensities" in f and f.endswith("_0.csv")] == [
        "x_matching_inner_0.npy", "x_matching_outer_0.npy", "x_intensities_inner_0.csv", "x_intensities_outer_0.csv"]


def _restated(a, root):
    names = [str(c) for c in a.cell_types]
    out = []
    for i, d in enumerate(("a", "b")):
        mask_a = a.preprocessor.masks_dev[i].cpu().numpy()
        mask_b = np.load(os.path.join(root, d, "second.npy"))
        out.append(ON.image_texts(mask_a, mask_b, 50, a._cell_type_ints(i), names))
        out[-1]["types"], out[-1]["mask_a"] = a._cell_type_ints(i), mask_a
    return names, out


def test_every_file_is_the_restatement_s(batch):
    """(b)"""
    from PIL import Image
    a, files = batch["a"], batch["files"]
    names, want = _restated(a, batch["root"])
    lut = colors.viridis_table()
    expected = []
    for i, w in enumerate(want):
        assert files[f"x_matching_cells_{i}.csv"].decode() == w["cells_csv"]
        assert files[f"x_matching_objects_{i}.csv"].decode() == w["objects_csv"]
        assert files[f"x_matching_pairs_{i}.csv"].decode() == w["pairs_csv"]
        statuses = [c["status"] for c in w["cells"]]
        assert statuses.count("none") >= 3 and statuses.count("multi") + statuses.count("single") > 50
        assert [o["status"] for o in w["objects"]].count("split") + [o["status"] for o in w["objects"]].count("orphan") >= 1
        img = np.array(Image.open(io.BytesIO(files[f"x_matching_fraction_{i}.png"])))
        colour = np.zeros((int(w["mask_a"].max()) + 1, 3), dtype=np.uint8)
        for label, c in zip(w["ids_a"], w["cells"]):
            colour[label] = lut[int(min(max(c["inner_fraction"], 0.0), 1.0) * 255)]
        assert img.shape == w["mask_a"].shape + (3,) and np.array_equal(img, colour[w["mask_a"]])      # every painted pixel, and the background 0
        group = (f"x_matching_agreement_{i}.csv", f"x_matching_summary_{i}.csv")
        assert files[group[0]].decode() == ON.agreement_csv(ON.agreement_rows(*ON.add_agreement([w["agreement"]])))
        assert files[group[1]].decode() == ON.summary_csv(names, ON.type_summary(w["types"], len(names), w["cells"]))
        per_image = [f"x_matching_cells_{i}.csv", f"x_matching_objects_{i}.csv", f"x_matching_pairs_{i}.csv", f"x_matching_fraction_{i}.png"]
        rec = a.matching_stats[i]
        assert rec["files"] == list(group) and rec["file"] == group[0] and rec["image_files"] == per_image
        assert (rec["n"], rec["m"], rec["pairs"]) == (len(w["ids_a"]), len(w["ids_b"]), len(w["pairs"]))
        assert (rec["none"], rec["multi"], rec["orphans"]) == (statuses.count("none"), statuses.count("multi"), sum(1 for o in w["owner"] if o < 0))
        assert rec["slots"] == 8 and rec["min_overlap"] == 50 and rec["annotated"] is True and min(rec["kernel_ms"], rec["draw_ms"]) >= 0.0
        expected += per_image + list(group)
    counts, sums = ON.add_agreement([w["agreement"] for w in want])
    assert files["x_integrated_matching_agreement.csv"].decode() == ON.agreement_csv(ON.agreement_rows(counts, sums))
    assert counts[0][2] > 0 and counts[-1][2] < counts[0][2]      # a shift of two pixels: cells match at IoU 0.5, fewer at 0.95
    types_ = np.concatenate([w["types"] for w in want])
    assert files["x_integrated_matching_summary.csv"].decode() == ON.summary_csv(names, ON.type_summary(types_, len(names), want[0]["cells"] + want[1]["cells"]))
    assert sorted(files) == sorted(expected + ["x_integrated_matching_agreement.csv", "x_integrated_matching_summary.csv"])
    rec = batch["integrated"][0]
    assert len(batch["integrated"]) == 1 and rec["n"] == sum(len(w["ids_a"]) for w in want) and rec["pairs"] == sum(len(w["pairs"]) for w in want)
    assert rec["files"] == ["x_integrated_matching_agreement.csv", "x_integrated_matching_summary.csv"] and len(rec["image_files"]) == 8
    log = open(a.logger.log_file_path).read()
    assert log.count("Mask matching x_integrated_matching_agreement.csv: ") == 1 and log.count("Mask matching x_matching_agreement_1.csv: ") == 1


def test_a_second_run_and_arrays_instead_of_paths_write_the_same_bytes_before_predict_without_types(batch):
    a = batch["a"]
    _match_both_ways(a)
    assert _files(batch["out"]) == batch["files"]
    out = os.path.join(batch["tmp"], "arrays")
    b = _annotator(batch["root"], "images.csv", out, predict=False)      # no column, no predict(): arrays, and tables without cell types
    seconds = [np.load(os.path.join(batch["root"], d, "second.npy")).astype(np.int64) for d in ("a", "b")]
    b.mask_matching(second_masks=seconds, integrate=True)
    got = _files(out)
    for name in got:
        if "_cells_" in name:
            rows, base = got[name].decode().split("\n"), batch["files"][name].decode().split("\n")
            assert [r.split(",")[:1] + r.split(",")[2:] for r in rows] == [r.split(",")[:1] + r.split(",")[2:] for r in base]
            assert set(r.split(",")[1] for r in rows[1:-1]) == {""}
        elif "summary" in name:
            assert got[name].decode().split("\n")[1].startswith("all,") and got[name].decode().split("\n")[1] == batch["files"][name].decode().strip().split("\n")[-1]
        else:
            assert got[name] == batch["files"][name], name
    assert b.matching_stats[0]["annotated"] is False


def test_errors_leave_the_result_directory_as_it_was(batch):
    out = os.path.join(batch["tmp"], "errors")
    b = _annotator(batch["root"], "images.csv", out, predict=False)
    res = os.path.join(out, "results")
    before = {f: os.path.getsize(os.path.join(res, f)) for f in os.listdir(res)}
    with pytest.raises(ValueError, match="needs a second mask per image"):
        b.mask_matching()
    wrong = [np.zeros(tuple(m.shape), dtype=np.int32) for m in b.preprocessor.masks_dev]
    wrong[1] = wrong[1][:, :-1]
    with pytest.raises(ValueError, match="second mask of image 1 must be an integer image of shape"):
        b.mask_matching(second_masks=wrong, intensities=True)
    with pytest.raises(ValueError, match="min_overlap must be an integer percent"):
        b.mask_matching(second_masks=wrong[:1] * 2, min_overlap=0)
    assert {f: os.path.getsize(os.path.join(res, f)) for f in os.listdir(res)} == before and not [f for f in before if "matching" in f]
    assert not hasattr(b, "matching_stats") and not hasattr(b, "intensity_inner")


def test_pipeline_switch(tmp_path):
    """without --match-masks no matching file and no other file changes; with it the integrated set, and the optional files with their flags"""
    import main as cli
    root = str(tmp_path / "case")
    planted_case(root, n_cells=150, h=256, w=300)
    mask = np.load(os.path.join(root, "mask.npy")).astype(np.int32)
    np.save(os.path.join(root, "second.npy"), ON.shifted_second_mask(mask))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        mdir = "src/multiplexed_image_annotator/cell_type_annotation/models"
        os.makedirs(mdir)
        for m, sd in weights().items():
            torch.save({"model": sd}, os.path.join(mdir, m + ".pth"))
        common = ["--marker-list-path", os.path.join(root, "markers.txt"), "--image-path", os.path.join(root, "img.npy"), "--mask-path",
                  os.path.join(root, "mask.npy"), "--batch-id", "c", "--no-infer", "--bs", "16", "--confidence", "0.0", "--n-regions", "0"]
        second = ["--second-mask-path", os.path.join(root, "second.npy")]
        cli.main(common + second + ["--main-dir", str(tmp_path / "off")])
        cli.main(common + second + ["--main-dir", str(tmp_path / "on"), "--match-masks", "--match-intensities", "--match-save-masks", "--match-min-overlap", "60"])
    finally:
        os.chdir(cwd)
    off, on = (sorted(os.listdir(tmp_path / k / "results")) for k in ("off", "on"))
    new = ["c_matching_cells_0.csv", "c_matching_objects_0.csv", "c_matching_pairs_0.csv", "c_matching_fraction_0.png", "c_matching_inner_0.npy",
           "c_matching_outer_0.npy", "c_intensities_inner_0.csv", "c_intensities_outer_0.csv", "c_integrated_matching_agreement.csv",
           "c_integrated_matching_summary.csv"]
    assert not [f for f in off if "matching" in f or "intensities" in f] and sorted(set(on) - set(off)) == sorted(new) and set(off) <= set(on)
    assert open(tmp_path / "off" / "images.csv").read().split("\n")[0] == "image_path,mask_path"
    for f in off:
        if f.endswith(".csv") or f.endswith(".png"):
            assert open(tmp_path / "off" / "results" / f, "rb").read() == open(tmp_path / "on" / "results" / f, "rb").read(), f
    want = ON.image_texts(mask, np.load(os.path.join(root, "second.npy")), 60)
    rows = open(tmp_path / "on" / "results" / "c_matching_objects_0.csv").read()
    assert rows == want["objects_csv"]


def _rank_body(rank, root):
    a = _annotator(root, "match.csv", os.path.join(root, "tiles"))
    assert a.tile_mode
    integrated = _match_both_ways(a)
    return [[s["file"] for s in integrated], [s["file"] for s in a.matching_stats]]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"])
    assert _files(os.path.join(batch["root"], "tiles")) == batch["files"]
    assert wrote == [[["x_integrated_matching_agreement.csv"], ["x_matching_agreement_0.csv"]], [[], ["x_matching_agreement_1.csv"]]]
