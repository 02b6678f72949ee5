"""The neighbourhood enrichment on the GPU: ribca_knn_neighbours, ribca_nhood_perm_counts (csrc/enrichment.hip) and ribca_table_raster against
tests/enrichment_numpy.py bit for bit (workspace and outputs pre-filled with junk), and Annotator.neighborhood_analysis() /
neighborhood_enrichment() end to end: files, the PNG rectangles against the rasteriser, the table against the oracle computed from the same cell
tables, reruns, seeds, two ranks."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import enrichment_numpy as EN
from batch_harness import annotated_batch, cli_runs, result_files, run_annotator, two_ranks
from multiplexed_image_annotator_amd import _lib, colors, enrichment, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _junk(nbytes, dev):
    return torch.full((max(int(nbytes), 1),), 255, dtype=torch.uint8, device=dev)


# ---- neighbour list --------------------------------------------------------------------------------------------------------------------------
def _points(case):
    rng = np.random.RandomState(len(case))
    if case == "duplicates":      # integer coordinates on a 6 x 6 grid: exact ties, among them whole groups of identical points
        return rng.randint(0, 6, 300).astype(np.float64), rng.randint(0, 6, 300).astype(np.float64), 25
    n, k = {"register list full": (33, 32), "ragged second workgroup": (257, 25), "one candidate in the second tile": (1025, 2)}[case]
    return rng.uniform(0, 1000, n), rng.uniform(0, 1000, n), k


@pytest.mark.parametrize("case", ["register list full", "ragged second workgroup", "one candidate in the second tile", "duplicates"])
def test_neighbour_list_bit_equal_to_numpy(case):
    x, y, k = _points(case)
    n = len(x)
    idx = ops.knn_neighbours(x, y, k)
    assert idx.shape == (n, k - 1) and idx.dtype == torch.int32
    got = idx.cpu().numpy()
    assert np.array_equal(got, EN.knn_list(x, y, k)), case
    assert (got != np.arange(n)[:, None]).all() or case == "duplicates"      # the cell itself is dropped (a duplicate of lower index may stand in)
    # counting over the list with the true labels is the co-occurrence matrix
    for t in (5, 40):      # the LDS histogram and the straight-to-global form of the counting kernel
        labels = np.random.RandomState(n).randint(0, t, n)
        want = ops.knn_cooccurrence(x, y, labels, t, k).cpu().numpy()
        assert np.array_equal(EN.pair_counts(got, labels, t), want), (case, t)


# ---- permutation counts ------------------------------------------------------------------------------------------------------------------------
def _gpu_perm(idx, labels, t, seed, image, p0, p, counts=None, short=0):
    """the entry point itself on a junk-filled workspace; ``counts``: accumulate into this device tensor"""
    dev = _lib.require_gpu()
    n, m = idx.shape
    idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
    lab_d = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
    if counts is None:
        counts = torch.zeros((p, t, t), dtype=torch.int64, device=dev)
    need = ops.nhood_perm_counts_ws_bytes(n, p)
    assert need >= min(p, 128) * n
    ws = _junk(need, dev)
    status = lib().ribca_nhood_perm_counts(ptr(idx_d), ptr(lab_d), n, m, t, seed, image, p0, p, ptr(counts), ptr(ws), need - short, stream_ptr())
    torch.cuda.synchronize()
    return status, counts


#: (n, T, m): n = 2 .. 1000 of one slab, 4097 and 9000 of two and three (the last one ragged); T on both sides of 32 and at 64; m = 1, 24, 31
PERM_SHAPES = [(2, 1, 1), (5, 3, 31), (17, 3, 24), (256, 32, 24), (257, 33, 1), (1000, 64, 31), (1000, 3, 24), (4097, 12, 24), (9000, 33, 3)]


@pytest.mark.parametrize("n,t,m", PERM_SHAPES)
def test_perm_counts_bit_equal_to_numpy(n, t, m):
    rng = np.random.RandomState(n + t + m)
    idx = rng.randint(0, n, (n, m))
    labels = rng.randint(0, t, n)
    n_a = np.bincount(labels, minlength=t)
    for p, seed, image, p0 in ((1, 0, 0, 0), (7, 12345678901234567890, 3, 40)):
        status, counts = _gpu_perm(idx, labels, t, seed, image, p0, p)
        assert status == 0, lib().ribca_last_error()
        got = counts.cpu().numpy()
        # independent of the oracle: every pair is counted once, and a permutation keeps the number of cells of each type
        assert (got.sum(axis=(1, 2)) == n * m).all() and (got.sum(axis=2) == m * n_a[None, :]).all(), (n, t, m, p)
        assert np.array_equal(got, EN.perm_counts(idx, labels, t, seed, image, p0, p)), (n, t, m, p)


@pytest.mark.parametrize("n,m", [(2, 1), (5, 4), (17, 24), (64, 31)])
def test_sigma_is_a_bijection_on_the_device(n, m):
    """T = n and labels 0 .. n - 1: every cell keeps a label of its own, so every row of every slice sums to m"""
    idx = np.random.RandomState(n).randint(0, n, (n, m))
    status, counts = _gpu_perm(idx, np.arange(n), n, 9, 1, 0, 7)
    assert status == 0, lib().ribca_last_error()
    got = counts.cpu().numpy()
    assert (got.sum(axis=2) == m).all()
    assert np.array_equal(got, EN.perm_counts(idx, np.arange(n), n, 9, 1, 0, 7))


def test_perm_batches_compose_and_calls_accumulate():
    n, t, m = 300, 5, 24
    rng = np.random.RandomState(8)
    idx, labels = rng.randint(0, n, (n, m)), rng.randint(0, t, n)
    status, all7 = _gpu_perm(idx, labels, t, 4, 2, 0, 7)
    assert status == 0
    status, last2 = _gpu_perm(idx, labels, t, 4, 2, 5, 2)
    assert status == 0 and torch.equal(all7[5:], last2)
    assert not torch.equal(all7[0], all7[1])
    status, twice = _gpu_perm(idx, labels, t, 4, 2, 0, 7, counts=all7.clone())
    assert status == 0 and torch.equal(twice, 2 * all7)
    # the wrapper: the same numbers, accumulated into out; another image number, other permutations
    idx_d = torch.from_numpy(idx.astype(np.int32)).cuda()
    out = ops.nhood_perm_counts(idx_d, labels, t, 4, 2, 0, 7)
    assert torch.equal(out, all7) and ops.nhood_perm_counts(idx_d, labels, t, 4, 2, 0, 7, out=out) is out and torch.equal(out, 2 * all7)
    assert not torch.equal(ops.nhood_perm_counts(idx_d, labels, t, 4, 3, 0, 7), all7)
    # more permutations than one batch of label rows holds (128): the host loop
    n, t, m, p = 50, 3, 2, 130
    idx, labels = rng.randint(0, n, (n, m)), rng.randint(0, t, n)
    status, counts = _gpu_perm(idx, labels, t, 0, 0, 0, p)
    assert status == 0 and np.array_equal(counts.cpu().numpy(), EN.perm_counts(idx, labels, t, 0, 0, 0, p))


def test_labels_and_neighbours_out_of_range_are_skipped():
    """the C entry point never indexes with them (ops.nhood_perm_counts refuses such labels before it gets there)"""
    n, t, m = 200, 4, 6
    rng = np.random.RandomState(5)
    idx, labels = rng.randint(0, n, (n, m)), rng.randint(0, t, n)
    labels[[3, 50, 51]] = [t, -1, 2 ** 31 - 1]
    idx[7, 2], idx[9, 0], idx[11, 5] = n, -1, 2 ** 31 - 1
    status, counts = _gpu_perm(idx, labels, t, 1, 0, 0, 3)
    assert status == 0
    want = np.zeros((3, t, t), dtype=np.int64)
    for j in range(3):
        lab = labels[EN.sigma(n, 1, 0, j)]
        for i in range(n):
            for q in range(m):
                if 0 <= idx[i, q] < n and 0 <= lab[i] < t and 0 <= lab[idx[i, q]] < t:
                    want[j, lab[i], lab[idx[i, q]]] += 1
    assert np.array_equal(counts.cpu().numpy(), want) and (want.sum(axis=(1, 2)) < n * m).all()
    with pytest.raises(ValueError, match="labels must lie in"):
        ops.nhood_perm_counts(torch.from_numpy(idx.astype(np.int32)).cuda(), labels, t, 1, 0, 0, 3)


# ---- raster ------------------------------------------------------------------------------------------------------------------------------------
def _gpu_table(values, cell, gap, vmin, vmax):
    dev = _lib.require_gpu()
    r, c = values.shape
    vd = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(dev)
    lut = torch.from_numpy(colors.diverging_table()).to(dev)
    n = r * cell * c * cell * 3
    out = _junk(n, dev)[:n].reshape(r * cell, c * cell, 3)
    out[..., 1] = 254      # junk that is not white either
    status = lib().ribca_table_raster(ptr(vd), r, c, ptr(lut), cell, gap, vmin, vmax, ptr(out), stream_ptr())
    torch.cuda.synchronize()
    return status, out.cpu().numpy()


def test_table_raster_bit_equal_to_numpy():
    lut = colors.diverging_table()
    v = np.array([[-3.0, -1.0, 0.0, 0.3], [np.nan, 1.0, 2.5, -0.999], [np.inf, -np.inf, 0.999, 1e-300]])      # beyond each limit, a NaN, the limits
    for cell, gap in ((24, 1), (5, 0), (1, 0)):
        for vmin, vmax in ((-1.0, 1.0), (-3.0, 2.5), (0.3, 0.3), (0.0, 1e-300)):
            status, img = _gpu_table(v, cell, gap, vmin, vmax)
            assert status == 0, lib().ribca_last_error()
            assert np.array_equal(img, EN.table_raster(v, lut, cell, gap, vmin, vmax)), (cell, gap, vmin, vmax)
    status, img = _gpu_table(v, 1, 0, -1.0, 1.0)
    assert (img[0, 0] == lut[0]).all() and (img[0, 1] == lut[0]).all() and (img[0, 2] == lut[128]).all() and (img[1, 0] == 192).all()
    assert (img[1, 1] == lut[255]).all() and (img[1, 2] == lut[255]).all() and (img[2, 0] == lut[255]).all() and (img[2, 1] == lut[0]).all()
    status, img = _gpu_table(v, 1, 0, 0.3, 0.3)
    assert (img[~np.isnan(v)] == lut[128]).all() and (img[1, 0] == 192).all()
    dev = _lib.require_gpu()
    got = ops.table_raster(torch.from_numpy(v).to(dev), torch.from_numpy(lut).to(dev), 24, 1, -1.0, 1.0).cpu().numpy()
    assert np.array_equal(got, EN.table_raster(v, lut, 24, 1, -1.0, 1.0))
    # ribca_heatmap_raster's own scale given by hand paints what it paints (no value lies outside it, the scale is not a point)
    sums, counts = np.array([[0.25, 0.5], [1.5, 2.0]]), np.array([1, 2])
    rect, lo, hi = ops.heatmap_raster(torch.from_numpy(sums).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(lut).to(dev), 8, 1)
    same = ops.table_raster(torch.from_numpy(sums / counts[:, None]).to(dev), torch.from_numpy(lut).to(dev), 8, 1, lo, hi)
    assert torch.equal(rect, same)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_a_status_and_nothing_runs():
    dev = _lib.require_gpu()
    rng = np.random.RandomState(1)
    n, m = 100, 24
    idx, labels = rng.randint(0, n, (n, m)), rng.randint(0, 65, n)
    junk = torch.full((2, 65, 65), -1, dtype=torch.int64, device=dev)
    status, counts = _gpu_perm(idx, labels, 65, 0, 0, 0, 2, counts=junk.clone())
    assert status == 1 and lib().ribca_last_error() == b"ribca_nhood_perm_counts: needs 1 <= T <= 64" and torch.equal(counts, junk)
    status, counts = _gpu_perm(idx, labels % 12, 12, 0, 0, 0, 2, counts=junk[:, :12, :12].clone().contiguous(), short=1)
    assert status == 1 and lib().ribca_last_error() == b"ribca_nhood_perm_counts: workspace too small" and (counts == -1).all()
    ws = _junk(4096, dev)
    idx_d, lab_d = torch.from_numpy(idx.astype(np.int32)).to(dev), torch.from_numpy((labels % 12).astype(np.int32)).to(dev)
    assert lib().ribca_nhood_perm_counts(ptr(idx_d), ptr(lab_d), n, m, 12, 0, 0, 0, 2, None, ptr(ws), 4096, stream_ptr()) == 1
    assert lib().ribca_last_error() == b"ribca_nhood_perm_counts: NULL buffer"
    x = torch.from_numpy(rng.uniform(0, 1, 40)).to(dev)
    out = torch.full((40, 32), -1, dtype=torch.int32, device=dev)
    assert lib().ribca_knn_neighbours(ptr(x), ptr(x), 40, 33, ptr(out), stream_ptr()) == 1
    assert lib().ribca_last_error() == b"ribca_knn_neighbours: k must be in [2, 32]"
    assert lib().ribca_knn_neighbours(ptr(x), ptr(x), 20, 25, ptr(out), stream_ptr()) == 1
    assert lib().ribca_last_error() == b"ribca_knn_neighbours: k exceeds the number of cells"
    assert lib().ribca_knn_neighbours(ptr(x), None, 40, 25, ptr(out), stream_ptr()) == 1
    assert lib().ribca_last_error() == b"ribca_knn_neighbours: NULL buffer"
    torch.cuda.synchronize()
    assert (out == -1).all()
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        ops.knn_neighbours(np.zeros(5), np.zeros(5), 6)
    with pytest.raises(_lib.RibcaError, match="ribca_knn_neighbours"):
        ops.knn_neighbours(np.zeros(50), np.zeros(50), 33)
    with pytest.raises(_lib.RibcaError, match="ribca_nhood_perm_counts"):
        ops.nhood_perm_counts(torch.zeros((10, 32), dtype=torch.int32, device=dev), np.zeros(10), 2, 0, 0, 0, 1)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
P_TEST = 40


def _analyse(a):
    a.neighborhood_analysis(integrate=True)
    integrated = list(a.neighborhood_stats)
    a.neighborhood_analysis(integrate=False)
    assert a.neighborhood_enrichment(n_perms=P_TEST, integrate=True) is None
    enriched = list(a.enrichment_stats)
    assert a.neighborhood_enrichment(n_perms=P_TEST, integrate=False) is None
    return integrated, enriched


EXPECTED = sorted([f"x_{s}.{e}" for s in ("integrated_neighborhood", "neighborhood_0", "neighborhood_1") for e in ("csv", "png")]
                  + [f"x_integrated_neighborhood_enrichment{t}" for t in (".csv", ".png", "_table.csv")]
                  + [f"x_neighborhood_enrichment{t}" for i in (0, 1) for t in (f"_{i}.csv", f"_{i}.png", f"_table_{i}.csv")])


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two-image batch of the cell-type plots, annotated once with "Others" among the cell types, and analysed"""
    os.environ.pop("RIBCA_ENRICH_SEED", None)
    b = annotated_batch(tmp_path_factory, "enrich", _analyse, "neighborhood")
    b["integrated"], b["enriched"] = b["integrated"]
    return b


def _rect_of(files, name, stats, t, cell):
    from PIL import Image
    img = np.array(Image.open(io.BytesIO(files[name])))
    top, left = stats["rect"]
    return img[top:top + t * cell, left:left + t * cell]


def test_neighbourhood_png_holds_the_raster(batch):
    a, files = batch["a"], batch["files"]
    assert sorted(files) == EXPECTED
    t = len(a.cell_types)
    assert t >= 3
    for name, images, stats in [("x_integrated_neighborhood.png", [0, 1], batch["integrated"][0]), ("x_neighborhood_0.png", [0], a.neighborhood_stats[0]),
                                ("x_neighborhood_1.png", [1], a.neighborhood_stats[1])]:
        m = a.neighborhood_matrix(images, 25)
        sums = m.sum(axis=1, keepdims=True)
        m = np.divide(m, sums, out=m.copy(), where=sums > 0)
        assert stats["file"] == name and (stats["vmin"], stats["vmax"]) == (m.min(), m.max()) and m.max() > m.min()
        dev = _lib.require_gpu()
        lut = colors.diverging_table()
        want = ops.table_raster(torch.from_numpy(m).to(dev), torch.from_numpy(lut).to(dev), a.HEATMAP_CELL, a.HEATMAP_GAP, m.min(), m.max()).cpu().numpy()
        got = _rect_of(files, name, stats, t, a.HEATMAP_CELL)
        assert np.array_equal(got, want) and np.array_equal(got, EN.table_raster(m, lut, a.HEATMAP_CELL, a.HEATMAP_GAP, m.min(), m.max()))
        # the CSV beside it is what it was: the matrix with three decimals
        rows = files[name[:-4] + ".csv"].decode().strip().split("\n")
        assert rows[0] == "cell_type," + "".join(f"{c}," for c in a.cell_types)
        assert rows[1:] == [f"{c}," + "".join(f"{m[r][j]:.3f}," for j in range(t)) for r, c in enumerate(a.cell_types)]


def _oracle(a, images, seed, p):
    t = len(a.cell_types)
    observed, null = np.zeros((t, t), dtype=np.int64), np.zeros((p, t, t), dtype=np.int64)
    for i in images:
        tab = a.preprocessor.cell_tables[i]
        x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
        y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
        types = a._cell_type_ints(i)
        idx = EN.knn_list(x, y, 25)
        observed += EN.pair_counts(idx, types, t)
        null += EN.perm_counts(idx, types, t, seed, a._image_number(i), 0, p)      # keyed with the batch-wide image number
    return observed, EN.z_scores(observed, null)


def _read_table(text):
    lines = text.strip().split("\n")
    assert lines[0] == "cell_type,neighbour,observed,null_mean,null_std,z,n_ge,n_le"
    return [l.split(",") for l in lines[1:]]


def _check_enrichment(a, files, stem, tail, images, stats, seed=0):
    t = len(a.cell_types)
    names = [str(c) for c in a.cell_types]
    observed, want = _oracle(a, images, seed, P_TEST)
    rows = _read_table(files[f"{stem}_table{tail}.csv"].decode())
    assert [(r[0], r[1]) for r in rows] == [(x, y) for x in names for y in names]
    for r, row in enumerate(rows):
        pos = divmod(r, t)
        assert int(row[2]) == observed[pos] and int(row[6]) == want["n_ge"][pos] and int(row[7]) == want["n_le"][pos]
        for text, key in ((row[3], "mean"), (row[4], "std"), (row[5], "z")):
            assert np.array([float(text)]).tobytes() == np.array([want[key][pos]]).tobytes(), (pos, key, text, want[key][pos])
    assert files[f"{stem}{tail}.csv"].decode() == enrichment.matrix_csv(names, want["z"])
    lim = enrichment.colour_limit(want["z"])
    assert stats["file"] == f"{stem}{tail}.png" and stats["limit"] == lim and stats["P"] == P_TEST and stats["T"] == t and stats["seed"] == seed
    assert stats["n"] == sum(len(a.preprocessor.cell_ids[i]) for i in images) and all(stats[k] >= 0.0 for k in ("knn_ms", "perm_ms", "draw_ms"))
    rect = _rect_of(files, f"{stem}{tail}.png", stats, t, a.HEATMAP_CELL)
    assert np.array_equal(rect, EN.table_raster(want["z"], colors.diverging_table(), a.HEATMAP_CELL, a.HEATMAP_GAP, -lim, lim))
    return want


def test_enrichment_table_is_the_oracle_s(batch):
    a, files = batch["a"], batch["files"]
    assert len(batch["enriched"]) == 1 and len(a.enrichment_stats) == 2
    want = _check_enrichment(a, files, "x_integrated_neighborhood_enrichment", "", [0, 1], batch["enriched"][0])
    assert np.isfinite(want["z"]).any() and (want["std"] > 0).any()
    for i in (0, 1):
        _check_enrichment(a, files, "x_neighborhood_enrichment", f"_{i}", [i], a.enrichment_stats[i])
    log = open(a.logger.log_file_path).read()
    assert log.count("Neighbourhood enrichment x_integrated_neighborhood_enrichment.png: ") == 1


def test_a_second_run_writes_the_same_bytes_and_a_seed_changes_z(batch, monkeypatch):
    out = os.path.join(batch["tmp"], "two")
    b = run_annotator(batch["root"], out, -1, batch["thr"])
    _analyse(b)
    assert result_files(out, "neighborhood") == batch["files"]
    monkeypatch.setenv("RIBCA_ENRICH_SEED", "5")
    b.neighborhood_enrichment(n_perms=P_TEST, integrate=True)
    seeded = result_files(out, "neighborhood")
    name = "x_integrated_neighborhood_enrichment_table.csv"
    assert seeded[name] != batch["files"][name] and b.enrichment_stats[0]["seed"] == 5
    assert [r[:3] for r in _read_table(seeded[name].decode())] == [r[:3] for r in _read_table(batch["files"][name].decode())]      # observed stays
    _check_enrichment(b, seeded, "x_integrated_neighborhood_enrichment", "", [0, 1], b.enrichment_stats[0], seed=5)
    assert {k: v for k, v in seeded.items() if "integrated_neighborhood_enrichment" not in k} == \
           {k: v for k, v in batch["files"].items() if "integrated_neighborhood_enrichment" not in k}


def test_errors_leave_the_files_alone(batch):
    a = batch["a"]
    with pytest.raises(ValueError, match="n_perms"):
        a.neighborhood_enrichment(n_perms=0)
    with pytest.raises(_lib.RibcaError, match="n_neighbors must be in"):      # what neighborhood_analysis raises for a list this long
        a.neighborhood_enrichment(n_neighbors=33, n_perms=2, integrate=False)
    assert result_files(batch["out"], "neighborhood") == batch["files"]


def test_pipeline_switch(tmp_path):
    """--enrichment-perms 0 (the default) writes no enrichment file; N > 0 writes the three integrated ones after the neighbourhood matrix"""
    import main as cli
    listing, common = cli_runs(tmp_path, {"off": [], "on": ["--enrichment-perms", "20"]}, "enrichment")
    off, on = listing["off"], listing["on"]
    assert "c_integrated_neighborhood.png" in off and "c_integrated_neighborhood.csv" in off
    assert [f for f in on if "enrichment" in f] == ["c_integrated_neighborhood_enrichment.csv", "c_integrated_neighborhood_enrichment.png",
                                                    "c_integrated_neighborhood_enrichment_table.csv"]
    assert cli.parse_args(common + ["--main-dir", "x"]).enrichment_perms == 0


def _rank_body(rank, root, thr):
    a = run_annotator(root, os.path.join(root, "tiles"), -1, thr)
    assert a.tile_mode
    _analyse(a)
    return [s["file"] for s in a.enrichment_stats]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], batch["thr"], unset=("RIBCA_ENRICH_SEED",))
    assert result_files(os.path.join(batch["root"], "tiles"), "neighborhood") == batch["files"]
    assert wrote == [["x_neighborhood_enrichment_0.png"], ["x_neighborhood_enrichment_1.png"]]      # the per-image call came last
