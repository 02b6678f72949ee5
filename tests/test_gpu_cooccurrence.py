"""The co-occurrence by distance on the GPU: ribca_radial_pair_counts (csrc/cooccurrence.hip) against tests/cooccurrence_numpy.py bit for bit
(the output pre-loaded, the workspace junk-filled), exact ties on an integer grid, properties that need no oracle, the refusals, and
Annotator.cooccurrence_by_distance() end to end: files, the table against the oracle computed from the same cell tables, the PNG rectangles
against the rasteriser, reruns, anchors, the command line, two ranks."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import cooccurrence_numpy as CO
from batch_harness import annotated_batch, cli_runs, result_files, run_annotator, two_ranks
from multiplexed_image_annotator_amd import _lib, colors, cooccurrence, enrichment, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

#: the launch geometry of csrc/cooccurrence.hip
TILE = 512                  # CO_TILE: candidates of one LDS tile
SPLIT = 8                   # CO_SPLIT: candidate slices (gridDim.y) at most; n = SPLIT * TILE + 1 gives slice 0 a second tile of one candidate
LDS_SMALL, LDS_MID, LDS_MAX = 4096, 8192, 16384      # B T^2 up to which each of the three LDS forms counts; above LDS_MAX: global atomics
CAP = 1 << 21               # CO_N_MAX


def _edges(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def _gpu_counts(x, y, labels, t, r2, counts=None, n=None):
    """the entry point itself; ``counts``: accumulate into this device tensor.  The library asks for no workspace; the one handed over all the
    same is junk before and must be the same junk after."""
    dev = _lib.require_gpu()
    n = len(x) if n is None else n
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
    if counts is None:
        counts = torch.zeros((len(r2), t, t), dtype=torch.int64, device=dev)
    assert ops.radial_pair_counts_ws_bytes(n, t, len(r2)) == 0
    ws = torch.full((256,), 255, dtype=torch.uint8, device=dev)
    status = lib().ribca_radial_pair_counts(ptr(xd), ptr(yd), ptr(td), n, t, _edges(r2), len(r2), ptr(counts), ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert (ws == 255).all()
    return status, counts


def _radii(bands):
    return np.array([150.0]) if bands == 1 else np.linspace(20.0, 400.0, bands)


#: (what, n, T, B)
SHAPES = [("one cell", 1, 3, 4), ("two cells", 2, 2, 2), ("one full workgroup", 256, 5, 16), ("one past a workgroup", 257, 5, 16),
          ("one past the candidate tile", TILE + 1, 12, 16), ("ragged last workgroup, two slices", 1000, 12, 32),
          ("one past the candidate split", SPLIT * TILE + 1, 12, 16), ("one band", 300, 7, 1), ("one type", 300, 1, 32),
          ("small LDS form, full", 600, 16, 16), ("middle LDS form, first", 600, 16, 17), ("middle LDS form, full", 600, 16, 32),
          ("large LDS form, first", 600, 53, 3), ("large LDS form, full", 600, 32, 16), ("global form, first", 600, 23, 31),
          ("254 types", 1000, 254, 2)]


def test_the_shapes_sit_where_the_forms_change():
    words = {what: b * t * t for what, _, t, b in SHAPES}
    assert words["small LDS form, full"] == LDS_SMALL and LDS_SMALL < words["middle LDS form, first"] and words["middle LDS form, full"] == LDS_MID
    assert LDS_MID < words["large LDS form, first"] and words["large LDS form, full"] == LDS_MAX and LDS_MAX * 4 == 64 * 1024
    # no B <= 32 and T <= 254 has B T^2 between LDS_MAX and this one
    assert words["global form, first"] == min(b * t * t for b in range(1, 33) for t in range(1, 255) if b * t * t > LDS_MAX)
    assert words["254 types"] > LDS_MAX


@pytest.mark.parametrize("what,n,t,bands", SHAPES, ids=[s[0] for s in SHAPES])
def test_counts_bit_equal_to_numpy(what, n, t, bands):
    rng = np.random.RandomState(n + 7 * t + bands)
    x, y = rng.uniform(0, 1000, n), rng.uniform(0, 1000, n)
    labels = rng.randint(0, t, n)
    r2 = _radii(bands) ** 2
    before = torch.from_numpy(rng.randint(0, 1000, (bands, t, t))).cuda()
    status, counts = _gpu_counts(x, y, labels, t, r2, counts=before.clone())
    assert status == 0, lib().ribca_last_error()
    got = (counts - before).cpu().numpy()
    want = CO.pair_counts(x, y, labels, t, r2)
    assert np.array_equal(got, want), what
    assert np.array_equal(got, got.transpose(0, 2, 1))
    if n == 1:
        assert not got.any()
    elif n > 2:
        assert got.any()


def test_labels_outside_the_range_are_skipped_on_both_sides():
    n, t = 700, 4
    rng = np.random.RandomState(11)
    x, y = rng.uniform(0, 300, n), rng.uniform(0, 300, n)
    labels = rng.randint(0, t, n)
    labels[[0, 3, 255, 256, 511, 512, 699]] = [t, -1, 2 ** 31 - 1, -2 ** 31, t + 1, -1, 254]
    r2 = np.array([30.0, 80.0, 1000.0]) ** 2      # the last radius passes the diameter: every valid pair is counted
    status, counts = _gpu_counts(x, y, labels, t, r2)
    assert status == 0, lib().ribca_last_error()
    got = counts.cpu().numpy()
    v = n - 7
    assert got.sum() == v * (v - 1)
    assert np.array_equal(got, CO.pair_counts(x, y, labels, t, r2))
    valid = np.bincount(labels[(labels >= 0) & (labels < t)], minlength=t)
    assert np.array_equal(got.sum(axis=(0, 2)), valid * (v - 1))      # every valid cell meets every other valid cell once


def test_exact_ties_land_in_the_band_that_ends_at_them():
    """integer coordinates on a 6 x 6 grid, 300 cells (so groups of identical points), r2 = 1, 2, 25: the bands by integer arithmetic"""
    rng = np.random.RandomState(5)
    n, t = 300, 3
    xi, yi = rng.randint(0, 6, n), rng.randint(0, 6, n)
    labels = rng.randint(0, t, n)
    d2 = (xi[:, None] - xi[None, :]) ** 2 + (yi[:, None] - yi[None, :]) ** 2
    off = ~np.eye(n, dtype=bool)
    want = np.zeros((3, t, t), dtype=np.int64)
    for b, (lo, hi) in enumerate(((-1, 1), (1, 2), (2, 25))):
        sel = (d2 > lo) & (d2 <= hi) & off
        np.add.at(want[b], (labels[np.nonzero(sel)[0]], labels[np.nonzero(sel)[1]]), 1)
    assert ((d2 == 25) & off).sum() > 0 and ((d2 == 0) & off).sum() > 0 and (d2 > 25).any()
    status, counts = _gpu_counts(xi.astype(np.float64), yi.astype(np.float64), labels, t, [1.0, 2.0, 25.0])
    assert status == 0, lib().ribca_last_error()
    got = counts.cpu().numpy()
    assert np.array_equal(got, want)
    assert got[0].sum() == ((d2 <= 1) & off).sum() and got[1].sum() == (d2 == 2).sum() and got[2].sum() == ((d2 > 2) & (d2 <= 25)).sum()
    # 3-4-5 alone: two cells 5 apart, edges 24.999.. < 25 <= 25
    status, counts = _gpu_counts(np.array([0.0, 3.0]), np.array([0.0, 4.0]), [0, 1], 2, [np.nextafter(25.0, 0.0), 25.0])
    assert status == 0 and counts.cpu().numpy().tolist() == [[[0, 0], [0, 0]], [[0, 1], [1, 0]]]
    status, counts = _gpu_counts(np.array([0.0, 3.0]), np.array([0.0, 4.0]), [0, 1], 2, [25.0, 26.0])
    assert status == 0 and counts.cpu().numpy().tolist() == [[[0, 1], [1, 0]], [[0, 0], [0, 0]]]
    assert np.array_equal(got, CO.pair_counts(xi, yi, labels, t, [1.0, 2.0, 25.0]))


def test_merged_bands_and_a_second_call_doubles():
    n, t = 900, 6
    rng = np.random.RandomState(2)
    x, y, labels = rng.uniform(0, 500, n), rng.uniform(0, 500, n), rng.randint(0, t, n)
    r1, r2, r3 = 40.0, 95.5, 210.0
    fine = ops.radial_pair_counts(x, y, labels, t, [r1, r2, r3])
    coarse = ops.radial_pair_counts(x, y, labels, t, [r1, r3])
    assert fine.dtype == torch.int64 and fine.shape == (3, t, t) and coarse.shape == (2, t, t)
    assert torch.equal(coarse[0], fine[0]) and torch.equal(coarse[1], fine[1] + fine[2]) and fine[1].any() and fine[2].any()
    assert np.array_equal(fine.cpu().numpy(), CO.pair_counts(x, y, labels, t, np.array([r1, r2, r3]) ** 2))      # the wrapper squares in fp64
    out = fine.clone()
    assert ops.radial_pair_counts(x, y, labels, t, [r1, r2, r3], out=out) is out and torch.equal(out, 2 * fine)
    everything = ops.radial_pair_counts(x, y, labels, t, [1000.0])
    assert int(everything.sum()) == n * (n - 1)
    with pytest.raises(ValueError, match="out must be"):
        ops.radial_pair_counts(x, y, labels, t, [r1, r3], out=out)


def test_refusals_are_a_status_and_nothing_runs():
    dev = _lib.require_gpu()
    x = np.arange(8.0)
    junk = torch.full((2, 3, 3), -1, dtype=torch.int64, device=dev)
    status, counts = _gpu_counts(x, x, np.zeros(8), 3, [1.0, 4.0], counts=junk.clone(), n=CAP + 1)      # refused before any buffer is read
    assert status == 1 and lib().ribca_last_error() == b"ribca_radial_pair_counts: needs 1 <= n <= 2^21" and torch.equal(counts, junk)
    status, counts = _gpu_counts(x, x, np.zeros(8), 3, [4.0, 1.0], counts=junk.clone())
    assert status == 1 and lib().ribca_last_error().startswith(b"ribca_radial_pair_counts: the squared radii") and torch.equal(counts, junk)
    status, counts = _gpu_counts(x, x, np.zeros(8), 255, [1.0, 4.0], counts=junk.clone())
    assert status == 1 and lib().ribca_last_error() == b"ribca_radial_pair_counts: needs 1 <= T <= 254" and torch.equal(counts, junk)
    with pytest.raises(_lib.RibcaError, match="needs 1 <= B <= 32"):
        ops.radial_pair_counts(x, x, np.zeros(8), 3, np.arange(1.0, 34.0))
    with pytest.raises(_lib.RibcaError, match="squared radii"):
        ops.radial_pair_counts(x, x, np.zeros(8), 3, [2.0, 2.0])


def test_adjacent_pairs_of_two_types_attract_near_and_not_far():
    """2000 couples, a cell of type 0 with a cell of type 1 one pixel to its right, the couples uniform on 1000 x 1000: the first band (1.5 px)
    holds the partners and next to nothing else (expected strangers: 4000^2 pi 1.5^2 / 1e6 = 113 of 4000 + 113 pairs), so the lift of (0, 1) is
    near 2 there and that of (0, 0) near 0.  In the ring 200 .. 300 px every type pair expects about 2000^2 pi (300^2 - 200^2) / 1e6 = 6e5 pairs
    (less at the border, alike for all four), relative scatter below 1 %: the lift is within 0.97 .. 1.03."""
    rng = np.random.RandomState(1)
    px, py = rng.uniform(0, 1000, 2000), rng.uniform(0, 1000, 2000)
    x, y = np.concatenate([px, px + 1.0]), np.concatenate([py, py])
    labels = np.repeat([0, 1], 2000)
    counts = ops.radial_pair_counts(x, y, labels, 2, [1.5, 200.0, 300.0]).cpu().numpy()
    lift = cooccurrence.lift(counts)
    print("lift near", lift[0].tolist(), "far", lift[2].tolist(), "counts", counts[0].tolist(), counts[2].tolist())
    assert counts[0, 0, 1] >= 2000 and lift[0, 0, 1] > 1.5 and lift[0, 0, 0] < 0.5
    assert (np.abs(lift[2] - 1.0) < 0.03).all()
    assert np.array_equal(counts, CO.pair_counts(x, y, labels, 2, np.array([1.5, 200.0, 300.0]) ** 2))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
RADII = [25.0, 60.0, 120.0, 250.0]


def _analyse(a):
    assert a.cooccurrence_by_distance(radii=RADII, integrate=True) is None
    integrated = list(a.cooccurrence_stats)
    assert a.cooccurrence_by_distance(radii=RADII, integrate=False) is None
    return integrated


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two-image batch of the cell-type plots, annotated once with "Others" among the cell types, and analysed"""
    return annotated_batch(tmp_path_factory, "cooc", _analyse, "cooccurrence")


def _oracle_counts(a, images):
    t = len(a.cell_types)
    total = np.zeros((len(RADII), t, t), dtype=np.int64)
    present = np.zeros(t, dtype=np.int64)
    for i in images:
        tab = a.preprocessor.cell_tables[i]
        x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
        y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
        types = a._cell_type_ints(i)
        total += CO.pair_counts(x, y, types, t, np.array(RADII) ** 2)      # pairs within one image only
        present += np.bincount(types, minlength=t)
    return total, present


def _check_group(a, files, stem, tail, images, stats):
    from PIL import Image
    t = len(a.cell_types)
    names = [str(c) for c in a.cell_types]
    counts, present = _oracle_counts(a, images)
    assert files[f"{stem}{tail}.csv"].decode() == CO.table_csv(names, RADII, counts)
    anchors = [k for k in range(t) if present[k] > 0]
    pngs = [f"{stem}_{cooccurrence.slug(names[k])}{tail}.png" for k in anchors]
    assert stats["files"] == [f"{stem}{tail}.csv"] + pngs and stats["file"] == f"{stem}{tail}.csv"
    assert stats["n"] == sum(len(a.preprocessor.cell_ids[i]) for i in images) and stats["T"] == t and stats["B"] == len(RADII) and stats["radii"] == RADII
    assert stats["pairs"] == int(counts.sum()) and stats["count_ms"] >= 0.0 and stats["draw_ms"] >= 0.0
    values = cooccurrence.figure_values(counts, CO.lift(counts))
    dev = _lib.require_gpu()
    lut = colors.diverging_table()
    cell = a.HEATMAP_CELL
    for k, name, fig in zip(anchors, pngs, stats["figures"]):
        table = np.ascontiguousarray(values[:, k, :].T)
        lim = enrichment.colour_limit(table)
        assert fig["file"] == name and fig["anchor"] == names[k] and fig["limit"] == lim
        img = np.array(Image.open(io.BytesIO(files[name])))
        top, left = fig["rect"]
        want = ops.table_raster(torch.from_numpy(table).to(dev), torch.from_numpy(lut).to(dev), cell, a.HEATMAP_GAP, -lim, lim).cpu().numpy()
        assert want.shape == (t * cell, len(RADII) * cell, 3)
        assert np.array_equal(img[top:top + t * cell, left:left + len(RADII) * cell], want), name
    return counts, pngs


def test_files_tables_and_figures_are_the_oracle_s(batch):
    a, files = batch["a"], batch["files"]
    assert len(a.cell_types) >= 3 and len(batch["integrated"]) == 1 and len(a.cooccurrence_stats) == 2
    counts, expected = _check_group(a, files, "x_integrated_cooccurrence", "", [0, 1], batch["integrated"][0])
    expected = expected + ["x_integrated_cooccurrence.csv"]
    assert counts.any() and np.isfinite(cooccurrence.lift(counts)).any()
    for i in (0, 1):
        _, pngs = _check_group(a, files, "x_cooccurrence", f"_{i}", [i], a.cooccurrence_stats[i])
        expected += pngs + [f"x_cooccurrence_{i}.csv"]
    assert sorted(files) == sorted(expected)
    assert files["x_integrated_cooccurrence.csv"] != files["x_cooccurrence_0.csv"] and files["x_cooccurrence_0.csv"] != files["x_cooccurrence_1.csv"]
    if "Proliferating/tumor cell" in a.cell_types:
        assert "x_integrated_cooccurrence_Proliferating_tumor_cell.png" in files
    log = open(a.logger.log_file_path).read()
    assert log.count("Co-occurrence by distance x_integrated_cooccurrence.csv: ") == 1


def test_anchors_restrict_the_figures_and_a_second_run_writes_the_same_bytes(batch):
    out = os.path.join(batch["tmp"], "two")
    b = run_annotator(batch["root"], out, -1, batch["thr"])
    names = [str(c) for c in b.cell_types]
    b.cooccurrence_by_distance(radii=RADII, integrate=True, anchors=[names[1], 0])
    wanted = [f"x_integrated_cooccurrence_{cooccurrence.slug(names[k])}.png" for k in (1, 0)]
    assert b.cooccurrence_stats[0]["files"] == ["x_integrated_cooccurrence.csv"] + wanted
    first = result_files(out, "cooccurrence")
    assert sorted(first) == sorted(["x_integrated_cooccurrence.csv"] + wanted)
    assert all(first[f] == batch["files"][f] for f in first)
    _analyse(b)
    assert result_files(out, "cooccurrence") == batch["files"]
    # the default radii: 16 bands of one cell size
    b.cooccurrence_by_distance(integrate=True, anchors=[0])
    assert b.cooccurrence_stats[0]["radii"] == [30.0 * k for k in range(1, 17)] and b.cooccurrence_stats[0]["B"] == 16


def test_errors_leave_the_files_alone(batch):
    a = batch["a"]
    with pytest.raises(ValueError, match="1 to 32 radii"):
        a.cooccurrence_by_distance(radii=np.arange(1.0, 34.0))
    for bad in ([], [10.0, 10.0], [20.0, 10.0], [-1.0, 5.0], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError):
            a.cooccurrence_by_distance(radii=bad)
    with pytest.raises(ValueError, match="is not one of the cell types"):
        a.cooccurrence_by_distance(radii=RADII, anchors=["no such cell"])
    with pytest.raises(ValueError, match="is not one of the cell types"):
        a.cooccurrence_by_distance(radii=RADII, anchors=[len(a.cell_types)])
    assert result_files(batch["out"], "cooccurrence") == batch["files"]
    from multiplexed_image_annotator_amd.annotator import Annotator
    root = batch["root"]
    fresh = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", os.path.join(batch["tmp"], "fresh"), "x", False, False,
                      -1, True, 0.3, 99.8, 0.3, 30, None)
    with pytest.raises(ValueError, match="No annotations"):
        fresh.cooccurrence_by_distance()


def test_pipeline_switch(tmp_path):
    """--cooccurrence-bands 0 (the default) writes no co-occurrence file; N > 0 writes the integrated table and its figures, N bands of one cell size"""
    import main as cli
    listing, common = cli_runs(tmp_path, {"off": [], "on": ["--cooccurrence-bands", "4"]}, "cooccurrence")
    on = listing["on"]
    added = [f for f in on if "cooccurrence" in f]
    assert "c_integrated_cooccurrence.csv" in added and len(added) >= 2
    assert all(f.startswith("c_integrated_cooccurrence_") and f.endswith(".png") for f in added if f != "c_integrated_cooccurrence.csv")
    rows = open(tmp_path / "on" / "results" / "c_integrated_cooccurrence.csv").read().strip().split("\n")
    assert rows[0] == "band,r_lo,r_hi,cell_type,neighbor_type,count,lift,cum_count,cum_lift"
    assert sorted({(r.split(",")[0], r.split(",")[2]) for r in rows[1:]}) == [("0", "30.0"), ("1", "60.0"), ("2", "90.0"), ("3", "120.0")]
    assert cli.parse_args(common + ["--main-dir", "x"]).cooccurrence_bands == 0


def _rank_body(rank, root, thr):
    a = run_annotator(root, os.path.join(root, "tiles"), -1, thr)
    assert a.tile_mode
    integrated = _analyse(a)
    return [[s["file"] for s in integrated], [s["file"] for s in a.cooccurrence_stats]]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], batch["thr"])
    assert result_files(os.path.join(batch["root"], "tiles"), "cooccurrence") == batch["files"]
    assert wrote == [[["x_integrated_cooccurrence.csv"], ["x_cooccurrence_0.csv"]], [[], ["x_cooccurrence_1.csv"]]]
