"""The nearest cell of every type on the GPU: ribca_nearest_by_type and ribca_nearest_perm_counts (csrc/nearest.hip) against
tests/nearest_numpy.py for EQUALITY, bit for bit (near2 as raw uint64), every output and workspace junk-filled before every call; exact ties on
an integer lattice, labels outside the range, purity in the permutation window, and Annotator.nearest_type_distances() end to end: files, the
per-cell table against the ops results, the tables against the oracle computed from the same cell tables, the maps, reruns, targets, the
refusals, two ranks."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import enrichment_numpy as EN
import nearest_numpy as NN
from batch_harness import annotated_batch, result_files, run_annotator, two_ranks
from multiplexed_image_annotator_amd import _lib, colors, cooccurrence, nearest, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

#: the launch geometry of csrc/nearest.hip
TILE = 512          # NR_TILE: candidates of one LDS tile; a segment of 2 TILE + 1 slots takes a third tile of one candidate
SORT = 1024         # NR_SORT: cells of one workgroup of the counting sort
BATCH = 32          # NR_BATCH: permutations of one internal batch


def _edges(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def _dev(x, y, labels):
    dev = _lib.require_gpu()
    return (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev),
            torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev), dev)


def _gpu_table(x, y, labels, t, junk=0xA5):
    """the entry point itself on junk-filled outputs and a junk-filled workspace of exactly the size the query asks for"""
    xd, yd, td, dev = _dev(x, y, labels)
    n = len(x)
    near2 = torch.full((n, t), float(junk), dtype=torch.float64, device=dev)
    arg = torch.full((n, t), junk, dtype=torch.int32, device=dev)
    ws = torch.full((ops.nearest_by_type_ws_bytes(n, t),), junk, dtype=torch.uint8, device=dev)
    status = lib().ribca_nearest_by_type(ptr(xd), ptr(yd), ptr(td), n, t, ptr(near2), ptr(arg), ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    return near2.cpu().numpy(), arg.cpu().numpy()


def _gpu_perm(x, y, labels, t, r2, seed, image, p0, n_perms, counts=None, junk=0x5A):
    xd, yd, td, dev = _dev(x, y, labels)
    n = len(x)
    if counts is None:
        counts = torch.zeros((n_perms, len(r2), t, t), dtype=torch.int64, device=dev)
    ws = torch.full((ops.nearest_perm_counts_ws_bytes(n, t, n_perms),), junk, dtype=torch.uint8, device=dev)
    status = lib().ribca_nearest_perm_counts(ptr(xd), ptr(yd), ptr(td), n, t, _edges(r2), len(r2), seed, image, p0, n_perms, ptr(counts), ptr(ws),
                                             ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    return counts


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


def _case(n, t, seed):
    """uniform cells on 1000 x 1000 with labels in [0, t); for t > 1 the last type has no cell"""
    rng = np.random.RandomState(seed)
    x, y = rng.uniform(0, 1000, n), rng.uniform(0, 1000, n)
    labels = rng.randint(0, t, n)
    if t > 1:
        labels[labels == t - 1] = 0
    return x, y, labels


def _radii(bands):
    return np.array([150.0]) if bands == 1 else np.linspace(20.0, 400.0, bands)


#: (what, n, T, B, P)
SHAPES = [("one cell", 1, 3, 4, 2), ("two cells", 2, 2, 2, 3), ("five cells", 5, 3, 1, 3), ("one short of a workgroup", 255, 3, 16, 2),
          ("one full workgroup, one type", 256, 1, 32, 2), ("one past a workgroup", 257, 3, 2, 2), ("one past the tile, 33 types", 513, 33, 16, 2),
          ("64 types, 32 bands", 600, 64, 32, 2), ("64 types, one band", 600, 64, 1, 2),
          ("one segment past two tiles, two sort chunks", 2 * TILE + 60, 1, 16, 2), ("three sort chunks", 2 * SORT + 52, 3, 2, 2)]


@pytest.mark.parametrize("what,n,t,bands,perms", SHAPES, ids=[s[0] for s in SHAPES])
def test_both_entry_points_bit_equal_to_numpy(what, n, t, bands, perms):
    x, y, labels = _case(n, t, n + 7 * t + bands)
    r2 = _radii(bands) ** 2
    near2, arg = _gpu_table(x, y, labels, t)
    want2, want_arg = NN.nearest_by_type(x, y, labels, t)
    assert _same_bits(near2, want2), what
    assert np.array_equal(arg, want_arg), what
    if t > 1:
        assert np.isinf(near2[:, t - 1]).all() and (arg[:, t - 1] == -1).all()
    if n == 1:
        assert np.isinf(near2).all() and (arg == -1).all()
    # the observed counts are the permutation counts of the identity labelling
    observed = nearest.observed_counts(near2, labels, t, r2)
    assert np.array_equal(observed, NN.band_counts(want2, labels, t, r2))
    before = torch.from_numpy(np.random.RandomState(1).randint(0, 1000, (perms, bands, t, t))).cuda()
    counts = _gpu_perm(x, y, labels, t, r2, 9, 4, 3, perms, counts=before.clone())
    got = (counts - before).cpu().numpy()
    want = NN.perm_counts(x, y, labels, t, r2, 9, 4, 3, perms)
    assert np.array_equal(got, want), what
    carried = np.bincount(labels, minlength=t)
    assert (got.sum(axis=1) <= carried[None, :, None]).all()      # per permutation, anchor and target: no more cells than carry the anchor type
    if n > 2:
        assert got.any() or bands == 1


def test_the_distance_table_at_254_types():
    n, t = 1000, 254
    x, y, labels = _case(n, t, 254)
    near2, arg = _gpu_table(x, y, labels, t)
    want2, want_arg = NN.nearest_by_type(x, y, labels, t)
    assert _same_bits(near2, want2) and np.array_equal(arg, want_arg)
    assert np.isfinite(near2).any() and np.isinf(near2[:, t - 1]).all()


def test_exact_ties_on_an_integer_lattice():
    """300 cells on a 6 x 6 grid (so groups of identical points), r2 = 1, 2, 25: the lowest index among equals, d2 == 0 in band 0, a distance on a
    band edge in the band that ends at it -- all by integer arithmetic"""
    rng = np.random.RandomState(5)
    n, t = 300, 3
    xi, yi = rng.randint(0, 6, n), rng.randint(0, 6, n)
    labels = rng.randint(0, t, n)
    d2 = (xi[:, None] - xi[None, :]) ** 2 + (yi[:, None] - yi[None, :]) ** 2
    big = 10 ** 6
    near2, arg = _gpu_table(xi.astype(np.float64), yi.astype(np.float64), labels, t)
    want_m = np.zeros((n, t), dtype=np.int64)
    for b in range(t):
        masked = np.where((labels[None, :] == b) & ~np.eye(n, dtype=bool), d2, big)
        want_m[:, b] = masked.min(axis=1)
        assert np.array_equal(arg[:, b], masked.argmin(axis=1))      # argmin: the first = the lowest index
    assert (want_m < big).all() and np.array_equal(near2, want_m.astype(np.float64))
    assert (want_m == 0).any() and (want_m == 1).any()
    r2 = [1.0, 2.0, 25.0]
    want = np.zeros((3, t, t), dtype=np.int64)
    for band, (lo, hi) in enumerate(((-1, 1), (1, 2), (2, 25))):
        for a in range(t):
            want[band, a] = ((want_m > lo) & (want_m <= hi))[labels == a].sum(axis=0)
    assert np.array_equal(nearest.observed_counts(near2, labels, t, r2), want) and want[0].any()
    got = _gpu_perm(xi.astype(np.float64), yi.astype(np.float64), labels, t, r2, 0, 0, 0, 3).cpu().numpy()
    assert np.array_equal(got, NN.perm_counts(xi, yi, labels, t, r2, 0, 0, 0, 3))
    # 3-4-5 alone, one cell of each type: the distance 5 against the edges 24.99.. < 25 and 25 < 26, under every labelling
    x2, y2 = np.array([0.0, 3.0]), np.array([0.0, 4.0])
    for edges, band in (([np.nextafter(25.0, 0.0), 25.0], 1), ([25.0, 26.0], 0)):
        got = _gpu_perm(x2, y2, [0, 1], 2, edges, 0, 0, 0, 4).cpu().numpy()
        want = np.zeros((2, 2, 2), dtype=np.int64)
        want[band, 0, 1] = want[band, 1, 0] = 1
        assert all(np.array_equal(got[j], want) for j in range(4))
    got = _gpu_perm(x2, y2, [0, 1], 2, [np.nextafter(25.0, 0.0)], 0, 0, 0, 2).cpu().numpy()
    assert not got.any()


def test_labels_outside_the_range():
    n, t = 700, 4
    rng = np.random.RandomState(11)
    x, y = rng.uniform(0, 300, n), rng.uniform(0, 300, n)
    labels = rng.randint(0, t, n).astype(np.int64)
    odd = [0, 3, 255, 256, 511, 512, 699]
    labels[odd] = [t, -1, 2 ** 31 - 1, -2 ** 31, t + 1, -1, 254]
    near2, arg = _gpu_table(x, y, labels, t)
    want2, want_arg = NN.nearest_by_type(x, y, labels, t)
    assert _same_bits(near2, want2) and np.array_equal(arg, want_arg)
    assert np.isfinite(near2[odd]).all() and not np.isin(arg, odd).any()      # such a cell has its row and is nobody's nearest
    r2 = np.array([10.0, 30.0, 1000.0]) ** 2      # the last radius passes the diameter: every valid cell is counted once per target type
    got = _gpu_perm(x, y, labels, t, r2, 2, 1, 0, 3).cpu().numpy()
    assert np.array_equal(got, NN.perm_counts(x, y, labels, t, r2, 2, 1, 0, 3))
    valid = np.bincount(labels[(labels >= 0) & (labels < t)], minlength=t)
    assert np.array_equal(got.sum(axis=1), np.broadcast_to(valid[None, :, None], (3, t, t)))
    assert np.array_equal(nearest.observed_counts(near2, labels, t, r2).sum(axis=0), np.broadcast_to(valid[:, None], (t, t)))


def test_purity_in_the_permutation_window_and_accumulation():
    n, t = 400, 5
    x, y, labels = _case(n, t, 21)
    r2 = _radii(4) ** 2
    whole = _gpu_perm(x, y, labels, t, r2, 7, 2, 0, 7)
    part = _gpu_perm(x, y, labels, t, r2, 7, 2, 5, 2, junk=0x11)
    assert torch.equal(whole[5:], part) and whole.any()
    assert not torch.equal(whole[0], whole[1])
    assert not torch.equal(whole[:2], _gpu_perm(x, y, labels, t, r2, 8, 2, 0, 2)) and not torch.equal(whole[:2], _gpu_perm(x, y, labels, t, r2, 7, 3, 0, 2))
    again = _gpu_perm(x, y, labels, t, r2, 7, 2, 0, 7, counts=whole.clone(), junk=0xEE)
    assert torch.equal(again, 2 * whole)      # ACCUMULATED
    # one past the internal batch: permutation 32 of a call of 33 is the single permutation of a call that starts there
    m = 60
    long = _gpu_perm(x[:m], y[:m], labels[:m], t, r2, 1, 0, 0, BATCH + 1)
    assert torch.equal(long[BATCH:], _gpu_perm(x[:m], y[:m], labels[:m], t, r2, 1, 0, BATCH, 1))
    assert np.array_equal(long[BATCH].cpu().numpy(), NN.perm_counts(x[:m], y[:m], labels[:m], t, r2, 1, 0, BATCH, 1)[0])
    first = _gpu_table(x, y, labels, t, junk=0x00)
    second = _gpu_table(x, y, labels, t, junk=0xFF)
    assert _same_bits(first[0], second[0]) and np.array_equal(first[1], second[1])
    # the wrappers: the same bits, radii squared in fp64
    near2, arg = ops.nearest_by_type(x, y, labels, t)
    assert near2.dtype == torch.float64 and arg.dtype == torch.int32 and _same_bits(near2.cpu().numpy(), first[0]) and np.array_equal(arg.cpu().numpy(), first[1])
    out = ops.nearest_perm_counts(x, y, labels, t, _radii(4), 7, 2, 0, 7)
    assert out.dtype == torch.int64 and torch.equal(out, whole)
    assert ops.nearest_perm_counts(x, y, labels, t, _radii(4), 7, 2, 0, 7, out=out) is out and torch.equal(out, 2 * whole)
    with pytest.raises(ValueError, match="out must be"):
        ops.nearest_perm_counts(x, y, labels, t, _radii(3), 7, 2, 0, 7, out=out)
    with pytest.raises(_lib.RibcaError, match="needs 1 <= T <= 64"):
        ops.nearest_perm_counts(x, y, labels, 65, _radii(3), 7, 2, 0, 1)
    with pytest.raises(_lib.RibcaError, match="needs 1 <= T <= 254"):
        ops.nearest_by_type(x, y, labels, 255)


def test_planted_attraction_on_the_gpu():
    """the layout of tests/test_nearest_host.py, 50 permutations: the GPU's counts are the restatement's, so its z-scores are"""
    rng = np.random.RandomState(400)
    ax, ay = rng.uniform(0, 1000, 120), rng.uniform(0, 1000, 120)
    theta = rng.uniform(0, 2 * np.pi, 120)
    cx, cy = rng.uniform(0, 1000, 160), rng.uniform(0, 1000, 160)
    x = np.concatenate([ax, ax + 12.0 * np.cos(theta), cx])
    y = np.concatenate([ay, ay + 12.0 * np.sin(theta), cy])
    labels = np.repeat([0, 1, 2], [120, 120, 160])
    radii = 30.0 * np.arange(1, 9)
    near2 = ops.nearest_by_type(x, y, labels, 3)[0].cpu().numpy()
    observed = nearest.observed_counts(near2, labels, 3, radii ** 2)
    null = ops.nearest_perm_counts(x, y, labels, 3, radii, 0, 0, 0, 50).cpu().numpy()
    assert np.array_equal(null, NN.perm_counts(x, y, labels, 3, radii ** 2, 0, 0, 0, 50))
    s = nearest.statistics(observed, null, np.bincount(labels, minlength=3))
    print("z[0][A][B]", s["z"][0, 0, 1], "z[0][B][A]", s["z"][0, 1, 0], "G_AB(30)", s["G"][0, 0, 1])
    assert s["G"][0, 0, 1] == 1.0 and s["z"][0, 0, 1] > 8.0 and s["z"][0, 1, 0] > 8.0


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
RADII = [25.0, 60.0, 120.0, 250.0]
PERMS = 6


def _analyse(a, **kw):
    assert a.nearest_type_distances(radii=RADII, n_perms=PERMS, integrate=True, **kw) is None
    integrated = list(a.nearest_stats)
    assert a.nearest_type_distances(radii=RADII, n_perms=PERMS, integrate=False, **kw) is None
    return integrated


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two-image batch of the cell-type plots, annotated once with "Others" among the cell types, and analysed"""
    return annotated_batch(tmp_path_factory, "nearest", _analyse, "_nearest_")


def _xy(a, i):
    tab = a.preprocessor.cell_tables[i]
    return tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64), tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)


def _oracle(a, images):
    t = len(a.cell_types)
    r2 = np.array(RADII) ** 2
    observed, null, present = np.zeros((len(RADII), t, t), dtype=np.int64), np.zeros((PERMS, len(RADII), t, t), dtype=np.int64), np.zeros(t, dtype=np.int64)
    for i in images:
        x, y = _xy(a, i)
        types = a._cell_type_ints(i)
        observed += NN.band_counts(NN.nearest_by_type(x, y, types, t)[0], types, t, r2)
        null += NN.perm_counts(x, y, types, t, r2, 0, a._image_number(i), 0, PERMS)
        present += np.bincount(types, minlength=t)
    return observed, null, present


def _check_group(a, files, stem, tail, images, stats):
    from PIL import Image
    t = len(a.cell_types)
    names = [str(c) for c in a.cell_types]
    observed, null, present = _oracle(a, images)
    want = NN.statistics(observed, null, present)
    assert files[f"{stem}{tail}.csv"].decode() == nearest.table_csv(names, RADII, observed, present, want)
    pngs = []
    for k in range(t):
        if present[k] > 0:
            pngs += [f"{stem}_{cooccurrence.slug(names[k])}{tail}.png", f"{stem}_{cooccurrence.slug(names[k])}_z{tail}.png"]
    assert stats["files"] == [f"{stem}{tail}.csv"] + pngs and stats["file"] == f"{stem}{tail}.csv"
    assert stats["n"] == sum(len(a.preprocessor.cell_ids[i]) for i in images) and stats["T"] == t and stats["B"] == len(RADII) and stats["P"] == PERMS
    assert stats["seed"] == 0 and stats["radii"] == RADII and min(stats["distance_ms"], stats["perm_ms"], stats["draw_ms"]) >= 0.0
    dev = _lib.require_gpu()
    lut = colors.diverging_table()
    cell = a.HEATMAP_CELL
    for fig in stats["figures"]:
        k = names.index(fig["anchor"])
        table = np.ascontiguousarray(want["G" if fig["what"] == "G" else "z"][:, k, :].T)
        lo, hi = (0.0, 1.0) if fig["what"] == "G" else (-fig["limit"], fig["limit"])
        img = np.array(Image.open(io.BytesIO(files[fig["file"]])))
        top, left = fig["rect"]
        rect = ops.table_raster(torch.from_numpy(table).to(dev), torch.from_numpy(lut).to(dev), cell, a.HEATMAP_GAP, lo, hi).cpu().numpy()
        assert np.array_equal(img[top:top + t * cell, left:left + len(RADII) * cell], rect), fig["file"]
    return pngs + [f"{stem}{tail}.csv"]


def _check_image(a, files, i):
    """the per-cell table against ops, the maps against the viridis entry computed here"""
    from PIL import Image
    t = len(a.cell_types)
    names = [str(c) for c in a.cell_types]
    ids = a.preprocessor.cell_ids[i]
    x, y = _xy(a, i)
    types = a._cell_type_ints(i)
    near2, arg = (v.cpu().numpy() for v in ops.nearest_by_type(x, y, types, t))
    number = a._image_number(i)
    rows = files[f"x_nearest_{number}.csv"].decode().strip().split("\n")
    assert rows[0] == "cell_id,cell_type," + ",".join(f"d_{cooccurrence.slug(c)},id_{cooccurrence.slug(c)}" for c in names) and len(rows) == 1 + len(ids)
    cells = [r.split(",") for r in rows[1:]]
    assert [int(c[0]) for c in cells] == [int(v) for v in ids] and [c[1] for c in cells] == [names[k] for k in types]
    assert np.array_equal(np.array([[float(c[2 + 2 * b]) for b in range(t)] for c in cells]), np.sqrt(near2))
    assert [[c[3 + 2 * b] for b in range(t)] for c in cells] == [[str(int(ids[j])) if j >= 0 else "" for j in row] for row in arg]
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    lut = colors.viridis_table()
    here = np.bincount(types, minlength=t)
    maps = []
    for b in range(t):
        name = f"x_nearest_{cooccurrence.slug(names[b])}_{number}.png"
        if here[b] == 0:
            assert name not in files
            continue
        maps.append(name)
        img = np.array(Image.open(io.BytesIO(files[name])))
        assert img.shape == mask.shape + (3,)
        for j in (0, len(ids) // 2, len(ids) - 1):      # a pixel of a known cell
            r, c = np.argwhere(mask == ids[j])[0]
            d = float(np.sqrt(near2[j, b]))
            assert img[r, c].tolist() == lut[int(min(d / RADII[-1], 1.0) * 255)].tolist(), (name, j)
        assert (img[mask == 0] == 0).all()
    return maps + [f"x_nearest_{number}.csv"]


def test_files_tables_and_maps_are_the_oracle_s(batch):
    a, files = batch["a"], batch["files"]
    assert len(a.cell_types) >= 3 and len(batch["integrated"]) == 1 and len(a.nearest_stats) == 2
    expected = _check_group(a, files, "x_integrated_nearest_table", "", [0, 1], batch["integrated"][0])
    for i in (0, 1):
        expected += _check_group(a, files, "x_nearest_table", f"_{i}", [i], a.nearest_stats[i])
        per_image = _check_image(a, files, i)
        assert sorted(a.nearest_stats[i]["image_files"]) == sorted(per_image)
        expected += per_image
    assert sorted(files) == sorted(expected)
    log = open(a.logger.log_file_path).read()
    assert log.count("Nearest cell of every type x_integrated_nearest_table.csv: ") == 1


def test_targets_restrict_the_maps_and_a_second_run_writes_the_same_bytes(batch):
    out = os.path.join(batch["tmp"], "two")
    b = run_annotator(batch["root"], out, -1, batch["thr"])
    names = [str(c) for c in b.cell_types]
    b.nearest_type_distances(radii=RADII, n_perms=0, integrate=False, targets=[names[1], 0])
    maps = sorted(f for f in result_files(out, "_nearest_") if f.endswith(".png") and "_table" not in f)
    assert maps == sorted(f"x_nearest_{cooccurrence.slug(names[k])}_{i}.png" for k in (1, 0) for i in (0, 1))
    # without a null: no z figure, and the table has the seven columns
    assert not [f for f in result_files(out, "_nearest_") if f.endswith("_z_0.png")]
    assert result_files(out, "_nearest_")["x_nearest_table_0.csv"].decode().split("\n")[0] == "anchor,target,anchor_cells,r,count,cum_count,G"
    assert all(result_files(out, "_nearest_")[f] == batch["files"][f] for f in maps if f in batch["files"])
    for f in os.listdir(os.path.join(out, "results")):
        if "_nearest_" in f:
            os.remove(os.path.join(out, "results", f))
    _analyse(b)
    assert result_files(out, "_nearest_") == batch["files"]
    # the default radii: 16 of one cell size
    b.nearest_type_distances(integrate=True, targets=[0])
    assert b.nearest_stats[0]["radii"] == [30.0 * k for k in range(1, 17)] and b.nearest_stats[0]["B"] == 16 and b.nearest_stats[0]["P"] == 0


def test_errors_leave_the_files_alone(batch, monkeypatch):
    a = batch["a"]
    with pytest.raises(ValueError, match="1 to 32 radii"):
        a.nearest_type_distances(radii=np.arange(1.0, 34.0))
    for bad in ([], [10.0, 10.0], [20.0, 10.0], [-1.0, 5.0], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError):
            a.nearest_type_distances(radii=bad)
    with pytest.raises(ValueError, match="is not one of the cell types"):
        a.nearest_type_distances(radii=RADII, targets=["no such cell"])
    with pytest.raises(ValueError, match="is not one of the cell types"):
        a.nearest_type_distances(radii=RADII, targets=[len(a.cell_types)])
    with pytest.raises(ValueError, match="must not be negative"):
        a.nearest_type_distances(radii=RADII, n_perms=-1)
    kept = a.cell_types
    try:
        a.cell_types = [str(c) for c in kept] + [f"type {k}" for k in range(65 - len(kept))]
        with pytest.raises(ValueError, match="at most 64 cell types"):
            a.nearest_type_distances(radii=RADII, n_perms=1)
        a.cell_types = [str(c) for c in kept] + [f"type {k}" for k in range(255 - len(kept))]
        with pytest.raises(ValueError, match="at most 254 cell types"):
            a.nearest_type_distances(radii=RADII)
    finally:
        a.cell_types = kept
    monkeypatch.setattr(ops, "NEAREST_MAX_CELLS", 10)
    with pytest.raises(ValueError, match="at most 10 cells per image"):
        a.nearest_type_distances(radii=RADII)
    monkeypatch.undo()
    assert result_files(batch["out"], "_nearest_") == batch["files"]
    from multiplexed_image_annotator_amd.annotator import Annotator
    root = batch["root"]
    fresh = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", os.path.join(batch["tmp"], "fresh"), "x", False, False,
                      -1, True, 0.3, 99.8, 0.3, 30, None)
    with pytest.raises(ValueError, match="No annotations"):
        fresh.nearest_type_distances()


def test_the_seed_switch_moves_the_null_and_nothing_else(batch, monkeypatch):
    out = os.path.join(batch["tmp"], "seeded")
    b = run_annotator(batch["root"], out, -1, batch["thr"])
    monkeypatch.setenv("RIBCA_NEAREST_SEED", "5")
    b.nearest_type_distances(radii=RADII, n_perms=PERMS, integrate=True)
    assert b.nearest_stats[0]["seed"] == 5
    got = result_files(out, "_nearest_")
    assert got["x_nearest_0.csv"] == batch["files"]["x_nearest_0.csv"]
    rows, base = got["x_integrated_nearest_table.csv"].decode().split("\n"), batch["files"]["x_integrated_nearest_table.csv"].decode().split("\n")
    assert [r.split(",")[:7] for r in rows] == [r.split(",")[:7] for r in base] and rows != base


def _rank_body(rank, root, thr):
    a = run_annotator(root, os.path.join(root, "tiles"), -1, thr)
    assert a.tile_mode
    integrated = _analyse(a)
    return [[s["file"] for s in integrated], [s["file"] for s in a.nearest_stats]]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], batch["thr"])
    assert result_files(os.path.join(batch["root"], "tiles"), "_nearest_") == batch["files"]
    assert wrote == [[["x_integrated_nearest_table.csv"], ["x_nearest_table_0.csv"]], [[], ["x_nearest_table_1.csv"]]]
