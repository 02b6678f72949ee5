"""The cell-type heat map and composition pie: csrc/celltype_stats.hip against tests/celltype_numpy.py bit for bit (workspace and outputs pre-filled
with 0xFF), and Annotator.generate_heatmap() / cell_type_composition() end to end (reference model.py:700-741, 861-912): files, CSV values
against the reference's formulas, PNG rectangles against the numpy rasters of the CSV values, reruns, two ranks in either sharding."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import celltype_numpy as CN
from batch_harness import annotated_batch, load_config1, planted_case, result_files, run_annotator, two_ranks, weights, write_case
from multiplexed_image_annotator_amd import _lib, colors, ops, plots
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

R = CN.R
U = 2.0 ** -53


def _junk(nbytes, dev):
    return torch.full((max(int(nbytes), 1),), 255, dtype=torch.uint8, device=dev)


def _junk_like(shape, dtype, dev):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return _junk(n, dev)[:n].view(dtype).reshape(shape) if n else torch.empty(shape, dtype=dtype, device=dev)


def _gpu_group_sums(x, g, groups, short=0):
    """the entry point itself, on junk-filled outputs and workspace; ``short``: that many bytes fewer than the query asks for"""
    dev = _lib.require_gpu()
    n, c = x.shape
    xd, gd = torch.from_numpy(np.ascontiguousarray(x)).to(dev), torch.from_numpy(np.ascontiguousarray(g, dtype=np.int32)).to(dev)
    sums, counts = _junk_like((groups, c), torch.float64, dev), _junk_like((groups,), torch.int64, dev)
    need = ops.group_sums_ws_bytes(n, c, groups)
    assert need > 0
    ws = _junk(need, dev)
    skipped = ctypes.c_int64(-7)
    status = lib().ribca_group_sums(ptr(xd) if n else None, ptr(gd) if n else None, n, c, groups, ptr(sums), ptr(counts), ctypes.byref(skipped), ptr(ws),
                                    need - short, stream_ptr())
    torch.cuda.synchronize()
    return status, sums.cpu().numpy(), counts.cpu().numpy(), int(skipped.value)


def _values(rng, n, c):
    """both signs, magnitudes 1e-8 .. 1e8: a different order of additions shows in the bits"""
    return rng.choice([-1.0, 1.0], (n, c)) * 10.0 ** rng.uniform(-8, 8, (n, c))


def _ids(rng, n, groups):
    if groups == 5:      # group 2 stays empty; the only row of group 4 is the last one (in the last, partial chunk); -1 and 5 are skipped
        g = rng.choice([0, 1, 3, -1, 5], n)
        if n:
            g[-1] = 4
        return g.astype(np.int32)
    return rng.randint(-1, groups + 1, n).astype(np.int32)


@pytest.mark.parametrize("n", [0, 1, R - 1, R, R + 1, 3 * R + 7])
def test_group_sums_bit_equal_to_the_tree(n):
    rng = np.random.RandomState(n + 1)
    for c in (1, 15, 64):
        for groups in (1, 5, ops.GROUP_SUM_MAX_GROUPS):
            x, g = _values(rng, n, c), _ids(rng, n, groups)
            status, sums, counts, skipped = _gpu_group_sums(x, g, groups)
            assert status == 0, lib().ribca_last_error()
            want, wcounts, wskipped = CN.group_sums(x, g, groups)
            assert np.array_equal(counts, wcounts) and skipped == wskipped, (n, c, groups)
            assert sums.tobytes() == want.tobytes(), (n, c, groups, np.abs(sums - want).max())
            if groups == 5 and n > 1:
                assert counts[2] == 0 and not sums[2].any() and counts[4] == 1 and np.array_equal(sums[4], 0.0 + x[-1]) and skipped > 0
    if n == 0:
        assert not sums.any() and not counts.any() and skipped == 0


def test_group_sums_workspace_one_byte_short_is_a_status():
    rng = np.random.RandomState(3)
    x, g = _values(rng, R + 1, 15), _ids(rng, R + 1, 5)
    status, sums, counts, skipped = _gpu_group_sums(x, g, 5, short=1)
    assert status != 0 and lib().ribca_last_error() == b"ribca_group_sums: workspace too small"
    assert np.isnan(sums).all() and (counts == -1).all() and skipped == -7      # nothing ran: the junk is still there
    with pytest.raises(_lib.RibcaError, match="ribca_group_sums"):
        ops.group_sums(torch.zeros((3, 2), dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"), 257)
    with pytest.raises(ValueError):
        ops.group_sums(torch.zeros((3, 2), dtype=torch.float32, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"), 4)


def test_group_sums_100k_cells_against_np_mean():
    rng = np.random.RandomState(11)
    n, c, groups = 100000, 15, 12
    x = rng.uniform(0.0, 1.0, (n, c)) * 10.0 ** rng.uniform(-3, 0, (n, c))      # intensity rows lie in [0, 1]
    g = rng.randint(0, groups, n).astype(np.int32)
    dev = _lib.require_gpu()
    sums, counts, skipped = ops.group_sums(torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev), groups)
    again = ops.group_sums(torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev), groups, ws=_junk(ops.group_sums_ws_bytes(n, c, groups) + 4096, dev))
    assert torch.equal(sums, again[0]) and torch.equal(counts, again[1])
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    assert skipped == 0 and counts.sum() == n
    worst = 0.0
    for k in range(groups):
        rows = x[g == k]
        n_g = len(rows)
        assert counts[k] == n_g
        mean = np.mean(rows, axis=0)
        # two fp64 sums of n_g terms, each within (n_g - 1) u sum|x| of the exact sum; then each side divides once (u |mean| each)
        bound = 2.0 * (n_g - 1) * U * np.abs(rows).sum(axis=0) / n_g + 2.0 * U * np.abs(mean)
        diff = np.abs(sums[k] / n_g - mean)
        worst = max(worst, float((diff / bound).max()))
        assert (diff <= bound).all()
    print(f"[group_sums 100k x 15] worst |mean - np.mean| / bound = {worst:.3g}")


def _gpu_heatmap(sums, counts, cell, gap, short=0):
    dev = _lib.require_gpu()
    t, c = sums.shape
    sd, cd = torch.from_numpy(np.ascontiguousarray(sums, dtype=np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).to(dev)
    lut = torch.from_numpy(colors.diverging_table()).to(dev)
    out = _junk_like((t * cell, c * cell, 3), torch.uint8, dev)
    need = int(lib().ribca_heatmap_raster_ws_bytes(t, c, cell, gap))
    ws = _junk(need, dev)
    vmin, vmax = ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    status = lib().ribca_heatmap_raster(ptr(sd), ptr(cd), t, c, ptr(lut), cell, gap, ptr(out), ctypes.byref(vmin), ctypes.byref(vmax), ptr(ws), need - short,
                                        stream_ptr())
    torch.cuda.synchronize()
    return status, out.cpu().numpy(), vmin.value, vmax.value


HEAT_CASES = {
    "one cell": (np.array([[3.5]]), np.array([2])),
    "3 x 4 with an empty row": (np.array([[1.0, 2.0, 3.0, 4.0], [9.0, 9.0, 9.0, 9.0], [0.3, 7.0, 0.9, 2.5]]), np.array([3, 0, 7])),
    "constant table": (np.array([[0.6, 0.6], [1.2, 1.2]]), np.array([1, 2])),
    "a cell equal to vmax": (np.array([[0.25, 0.5], [1.5, 2.0]]), np.array([1, 2])),
    "random 7 x 15": None,
}


@pytest.mark.parametrize("case", list(HEAT_CASES))
def test_heatmap_raster_bit_equal_to_numpy(case):
    if HEAT_CASES[case] is None:
        rng = np.random.RandomState(2)
        counts = rng.randint(0, 50, 7)
        sums = rng.uniform(0, 1, (7, 15)) * counts[:, None]
    else:
        sums, counts = HEAT_CASES[case]
    lut = colors.diverging_table()
    for cell, gap in ((24, 1), (5, 0), (1, 0)):
        status, img, vmin, vmax = _gpu_heatmap(sums, counts, cell, gap)
        assert status == 0, lib().ribca_last_error()
        want, wmin, wmax = CN.heatmap_raster(CN.means_of(sums, counts), lut, cell, gap)
        assert (vmin, vmax) == (wmin, wmax) and np.array_equal(img, want), case
    means = CN.means_of(sums, counts)
    mid = lambda t, j: img[t, j]      # cell = 1: one pixel per table cell
    if case == "one cell":
        assert (vmin, vmax) == (1.75, 1.75) and (mid(0, 0) == lut[0]).all()
    if case == "3 x 4 with an empty row":
        assert (img[1] == 192).all() and vmax == 4.0 / 3.0 and vmin == 0.3 / 7.0      # the empty row is silver and outside vmin / vmax
    if case == "constant table":
        assert vmin == vmax == 0.6 and (img == lut[0]).all()
    if case == "a cell equal to vmax":
        assert means[1, 1] == vmax == 1.0 and (mid(1, 1) == lut[255]).all() and (mid(0, 0) == lut[0]).all()


def test_heatmap_raster_workspace_one_byte_short_is_a_status():
    sums, counts = HEAT_CASES["a cell equal to vmax"]
    status, img, vmin, vmax = _gpu_heatmap(sums, counts, 8, 1, short=1)
    assert status != 0 and lib().ribca_last_error() == b"ribca_heatmap_raster: workspace too small"
    assert (img == 255).all() and (vmin, vmax) == (-7.0, -7.0)
    dev = _lib.require_gpu()
    with pytest.raises(_lib.RibcaError, match="ribca_heatmap_raster"):
        ops.heatmap_raster(torch.zeros((2, 2), dtype=torch.float64, device=dev), torch.ones(2, dtype=torch.int64, device=dev),
                           torch.from_numpy(colors.diverging_table()).to(dev), 8, 4)


def _gpu_pie(rays, rgb, size, radius):
    dev = _lib.require_gpu()
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 2)
    m = len(rays)
    rd, cd = torch.from_numpy(rays).to(dev), torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.uint8)).to(dev)
    out = _junk_like((size, size, 3), torch.uint8, dev)
    out[..., 1] = 254      # junk that is not white either
    status = lib().ribca_pie_raster(ptr(rd) if m else None, m, ptr(cd), size, radius, ptr(out), stream_ptr())
    torch.cuda.synchronize()
    return status, out.cpu().numpy()


@pytest.mark.parametrize("counts", [(7,), (4, 4), (2, 11, 3, 4), (5, 3, 0, 9)], ids=["m=0", "two halves", "one wedge wider than pi", "17 cells"])
def test_pie_raster_bit_equal_to_numpy(counts):
    kept, rays = plots.pie_wedges(counts)
    rgb = np.array(colors.get_colors(len(counts) + 1), dtype=np.uint8)[kept]
    status, img = _gpu_pie(rays, rgb, 65, 30)
    assert status == 0, lib().ribca_last_error()
    assert len(rays) == len(kept) - 1
    want = CN.pie_raster(rays, rgb, 65, 30)
    assert np.array_equal(img, want)
    wedge = CN.pie_wedge_index(rays, 65, 30)
    assert (img[wedge < 0] == 255).all() and (wedge >= 0).sum() == 2821      # the lattice points with dx^2 + dy^2 <= 900
    assert (img[32, 32] == rgb[0]).all() and set(np.unique(wedge)) == set(range(-1, len(kept)))
    if counts == (2, 11, 3, 4):
        assert (wedge == 1).sum() > (wedge >= 0).sum() / 2
    if counts == (4, 4):
        assert (wedge[:32][wedge[:32] >= 0] == 0).all() and (wedge[33:][wedge[33:] >= 0] == 1).all()
    # another canvas: even size, the disc clipped by it
    status, img = _gpu_pie(rays, rgb, 40, 30)
    assert status == 0 and np.array_equal(img, CN.pie_raster(rays, rgb, 40, 30))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _plot_all(a):
    """the four calls; every one returns None"""
    assert a.generate_heatmap(integrate=True) is None
    integrated = list(a.heatmap_stats)
    assert a.generate_heatmap(integrate=False) is None
    assert a.cell_type_composition(integrate=True) is None
    pies = list(a.composition_stats)
    assert a.cell_type_composition() is None
    return integrated, pies


NEEDLES = ("heatmap", "composition")
EXPECTED = sorted([f"x_{stem}.{ext}" for stem in ("Integrated_heatmap", "heatmap_0", "heatmap_1", "integrated_cell-type_composition",
                                                  "cell-type_composition_0", "cell-type_composition_1") for ext in ("png", "csv")])


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two-image batch annotated once, with a confidence threshold at the median so that "Others" is one of the cell types, and plotted"""
    b = annotated_batch(tmp_path_factory, "plots", _plot_all, NEEDLES)
    b["integrated"], b["pies"] = b["integrated"]
    return b


def _read_heatmap_csv(text):
    lines = text.strip().split("\n")
    head = lines[0].split(",")
    names = [l.split(",")[0] for l in lines[1:]]
    means = np.array([[float(v) for v in l.split(",")[1:-1]] for l in lines[1:]])
    cells = [int(l.split(",")[-1]) for l in lines[1:]]
    return head, names, means, cells


def _check_heatmap(a, files, stem, images, stats):
    """the CSV against the reference's formula over the given images, the PNG's data rectangle against the numpy raster of the CSV's values"""
    import io
    from PIL import Image
    head, names, means, cells = _read_heatmap_csv(files[stem + ".csv"].decode())
    assert head == ["cell_type"] + list(a.channel_parser.markers) + ["cells"]
    labels = [n for i in images for n in a.annotations[i]]
    x = np.concatenate([a.preprocessor.intensity_full[i] for i in images], axis=0)
    assert names == np.unique(labels).tolist() and len(names) >= 2
    for name, row, k in zip(names, means, cells):
        rows = x[[n == name for n in labels]]
        assert k == len(rows) > 0
        ref = np.mean(rows, axis=0)      # model.py:715 / 735
        bound = 2.0 * (k - 1) * U * np.abs(rows).sum(axis=0) / k + 2.0 * U * np.abs(ref)
        assert (np.abs(row - ref) <= bound).all(), (name, np.abs(row - ref).max())
    img = np.array(Image.open(io.BytesIO(files[stem + ".png"])))
    cell, gap = a.HEATMAP_CELL, a.HEATMAP_GAP
    want, vmin, vmax = CN.heatmap_raster(means, colors.diverging_table(), cell, gap)
    top, left = stats["rect"]
    assert np.array_equal(img[top:top + len(names) * cell, left:left + means.shape[1] * cell], want)
    assert (stats["vmin"], stats["vmax"]) == (vmin, vmax) == (means.min(), means.max())
    assert stats["rows"] == len(names) and stats["columns"] == means.shape[1] and stats["cells"] == len(labels) and stats["skipped"] == 0
    assert stats["file"] == stem + ".png" and all(stats[k] >= 0.0 for k in ("sums_ms", "raster_ms", "draw_ms"))


def test_heatmaps_end_to_end(batch):
    a, files = batch["a"], batch["files"]
    assert sorted(files) == EXPECTED
    assert "Others" in a.annotations[0] and len(a.annotations) == 2
    _check_heatmap(a, files, "x_Integrated_heatmap", [0, 1], batch["integrated"][0])
    assert len(batch["integrated"]) == 1 and len(a.heatmap_stats) == 2
    for i in (0, 1):
        _check_heatmap(a, files, f"x_heatmap_{i}", [i], a.heatmap_stats[i])
    log = open(a.logger.log_file_path).read()
    assert "skipped (plotting" not in log and log.count("Heat map x_Integrated_heatmap.png: ") == 1 and "Composition x_integrated_cell-type_composition.png: " in log


def _check_pie(a, files, stem, images, stats, reduction=True):
    import io
    from PIL import Image
    lines = files[stem + ".csv"].decode().strip().split("\n")
    assert lines[0] == "cell_type,cells,fraction"
    names = [l.split(",")[0] for l in lines[1:]]
    cells = [int(l.split(",")[1]) for l in lines[1:]]
    frac = [float(l.split(",")[2]) for l in lines[1:]]
    want = collections.Counter(n for i in images for n in a.annotations[i])
    assert names == [str(c) for c in a.cell_types] and cells == [want[n] for n in names] and sum(cells) == sum(want.values())
    assert frac == [c / sum(cells) for c in cells]
    img = np.array(Image.open(io.BytesIO(files[stem + ".png"])))
    kept, rays = plots.pie_wedges(cells)
    disc = CN.pie_raster(rays, np.array(a.colors, dtype=np.uint8)[kept], a.PIE_CANVAS, a.PIE_RADIUS)
    top, left = stats["rect"]
    assert np.array_equal(img[top:top + a.PIE_CANVAS, left:left + a.PIE_CANVAS], disc) and img.shape[1] > a.PIE_CANVAS
    assert stats["cells"] == sum(cells) and stats["wedges"] == len(kept) >= 2 and stats["skipped"] == 0 and stats["file"] == stem + ".png"


def test_compositions_end_to_end(batch):
    a, files = batch["a"], batch["files"]
    _check_pie(a, files, "x_integrated_cell-type_composition", [0, 1], batch["pies"][0])
    assert len(batch["pies"]) == 1 and len(a.composition_stats) == 2
    for i in (0, 1):
        _check_pie(a, files, f"x_cell-type_composition_{i}", [i], a.composition_stats[i])
    # reduction=False changes the legend (the reference's raw count x 100), not the disc or the CSV
    a.cell_type_composition(reduction=False, integrate=True)
    again = result_files(batch["out"], NEEDLES)
    stem = "x_integrated_cell-type_composition"
    assert again[stem + ".csv"] == files[stem + ".csv"] and again[stem + ".png"] != files[stem + ".png"]
    _check_pie(a, again, stem, [0, 1], a.composition_stats[0])
    a.cell_type_composition(integrate=True)
    assert result_files(batch["out"], NEEDLES) == files


def test_a_second_run_writes_the_same_bytes(batch):
    out = os.path.join(batch["tmp"], "two")
    b = run_annotator(batch["root"], out, -1, batch["thr"])
    _plot_all(b)
    assert result_files(out, NEEDLES) == batch["files"]


def test_additional_types_get_a_row(batch):
    out = os.path.join(batch["tmp"], "extra")
    a = run_annotator(batch["root"], out, 20, batch["thr"])
    assert any(n.startswith("Additional type") for n in a.cell_types)
    integrated, pies = _plot_all(a)
    files = result_files(out, NEEDLES)
    head, names, means, cells = _read_heatmap_csv(files["x_Integrated_heatmap.csv"].decode())
    assert any(n.startswith("Additional type") for n in names) and names == sorted(names)
    _check_heatmap(a, files, "x_Integrated_heatmap", [0, 1], integrated[0])
    _check_pie(a, files, "x_integrated_cell-type_composition", [0, 1], pies[0])


def test_config1_heatmap_matches_the_reference_golden(golden_dir, tmp_path):
    """the heat-map table of BASELINE config 1's stand-in against np.mean over the reference run's own intensity rows grouped by its own labels"""
    from multiplexed_image_annotator_amd.annotator import Annotator
    meta, arrs, raw, mask, weights, mf = load_config1(golden_dir, tmp_path)
    _, csv = write_case(tmp_path, raw, mask, meta["markers"])
    a = Annotator(mf, csv, "cuda", str(tmp_path), "c1", True, False, -1, True, meta["blur"], meta["amax"], meta["conf"], 30, None)
    a.set_weights(weights)
    a.preprocess()
    a.predict(meta["batch_size"])
    assert a.generate_heatmap(integrate=True) is None
    head, names, means, cells = _read_heatmap_csv(open(tmp_path / "results" / "c1_Integrated_heatmap.csv").read())
    labels = np.array(meta["labels"])
    assert len(labels) == 1850 and head[1:-1] == meta["markers"] and names == np.unique(labels).tolist() and sum(cells) == 1850
    for name, row, k in zip(names, means, cells):
        rows = arrs["intensity"][labels == name]
        assert k == len(rows)
        ref = np.mean(rows, axis=0)
        # the summation bound, and the rtol 1e-12 / atol 1e-14 test_config1_matches_reference_golden grants every intensity row
        bound = 2.0 * (k - 1) * U * np.abs(rows).sum(axis=0) / k + 2.0 * U * np.abs(ref) + 1e-12 * np.abs(rows).mean(axis=0) + 1e-14
        assert (np.abs(row - ref) <= bound).all(), (name, np.abs(row - ref).max())


def test_errors_before_predict(tmp_path):
    from multiplexed_image_annotator_amd.annotator import Annotator
    root = str(tmp_path / "case")
    planted_case(root, n_cells=150, h=256, w=300)
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", str(tmp_path / "o"), "t", False, False, -1, True, 0.3,
                  99.8, 0.0, 30, None)
    with pytest.raises(ValueError, match="No annotations to generate heatmap"):
        a.generate_heatmap(integrate=True)
    with pytest.raises(ValueError, match="No annotations to analyze"):
        a.cell_type_composition()
    assert not [f for f in os.listdir(str(tmp_path / "o" / "results")) if "heatmap" in f or "composition" in f]
    assert not hasattr(a, "_skip")


def test_pipeline_leaves_both_integrated_figures(tmp_path):
    import main as cli
    root = str(tmp_path / "case")
    planted_case(root, n_cells=150, h=256, w=300)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        mdir = "src/multiplexed_image_annotator/cell_type_annotation/models"
        os.makedirs(mdir)
        for m, sd in weights().items():
            torch.save({"model": sd}, os.path.join(mdir, m + ".pth"))
        cli.main(["--marker-list-path", os.path.join(root, "markers.txt"), "--image-path", os.path.join(root, "img.npy"), "--mask-path",
                  os.path.join(root, "mask.npy"), "--batch-id", "c", "--main-dir", str(tmp_path / "out"), "--no-infer", "--bs", "16", "--confidence", "0.0"])
    finally:
        os.chdir(cwd)
    res = tmp_path / "out" / "results"
    for f in ("c_Integrated_heatmap.png", "c_Integrated_heatmap.csv", "c_integrated_cell-type_composition.png", "c_integrated_cell-type_composition.csv",
              "c_cell-type_composition_0.png"):
        assert (res / f).exists(), f


def _rank_body(rank, root, thr, tile):
    out = os.path.join(root, "tiles" if tile else "sharded")
    a = run_annotator(root, out, -1, thr)
    assert a.tile_mode == bool(tile)
    _plot_all(a)
    return {"heatmaps": [s["file"] for s in a.heatmap_stats], "pies": [s["file"] for s in a.composition_stats]}


@pytest.mark.parametrize("tile", [0, 1], ids=["cell-sharded", "tile-per-rank"])
def test_two_ranks_write_the_single_rank_bytes(batch, tile):
    wrote = two_ranks(_rank_body, batch["root"], batch["thr"], tile, tile=tile)
    name = "tiles" if tile else "sharded"
    assert result_files(os.path.join(batch["root"], name), NEEDLES) == batch["files"]
    if tile:      # the per-image figures come from the rank that owns the image (after the calls of _plot_all: the per-image ones are the last)
        assert wrote[0] == {"heatmaps": ["x_heatmap_0.png"], "pies": ["x_cell-type_composition_0.png"]}
        assert wrote[1] == {"heatmaps": ["x_heatmap_1.png"], "pies": ["x_cell-type_composition_1.png"]}
    else:
        assert wrote[0] == {"heatmaps": ["x_heatmap_0.png", "x_heatmap_1.png"], "pies": ["x_cell-type_composition_0.png", "x_cell-type_composition_1.png"]}
        assert wrote[1] == {"heatmaps": [], "pies": []}
