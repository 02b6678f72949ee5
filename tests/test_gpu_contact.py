"""The cell contact graph on the GPU: ribca_contact_table and ribca_edge_perm_counts (csrc/contact.hip) against tests/contact_numpy.py for
EQUALITY, every output and workspace junk-filled to exactly the queried size before every call: masks that are and are not a multiple of the
pixel tile, an image thinner than the reach, contacts on and across the tile seams, every kind of label that is no cell, more distinct pairs
than a workgroup's table holds, the retry and the overflow report; the null over an edge list with its purity and accumulation; and
Annotator.contact_analysis() end to end: files, tables against the restatement run on the same masks and labels, reruns, the pipeline switch,
two ranks."""
import io
import os

import numpy as np
import pytest
import torch

import contact_numpy as CN
from batch_harness import MARKERS, SEED, annotated_batch, cli_runs, result_files, run_annotator, two_ranks
from multiplexed_image_annotator_amd import _lib, colors, contact, enrichment, ops, synth
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

TILE = 32          # CT_TILE of csrc/contact.hip: a workgroup's pixel tile
REACHES = (1, 2, 3, 8)


def _gpu_table(mask, table, n, d, slots, junk=0xA5):
    """the entry point itself on junk-filled outputs and a junk-filled workspace of exactly the size the query asks for"""
    dev = _lib.require_gpu()
    md = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.int32)).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(dev)
    h, w = mask.shape
    nbr = torch.full((n, slots), junk, dtype=torch.int32, device=dev)
    pairs = torch.full((n, slots), junk, dtype=torch.int64, device=dev)
    degree = torch.full((n,), junk, dtype=torch.int32, device=dev)
    over = torch.full((2,), junk, dtype=torch.int32, device=dev)
    ws = torch.full((ops.contact_table_ws_bytes(h, w, n, slots),), junk, dtype=torch.uint8, device=dev)
    status = lib().ribca_contact_table(ptr(md), h, w, ptr(td), len(table), n, d, slots, ptr(nbr), ptr(pairs), ptr(degree), ptr(over), ptr(ws),
                                       ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    return nbr.cpu().numpy(), pairs.cpu().numpy(), degree.cpu().numpy(), over.cpu().numpy()


def _equal_to_the_restatement(mask, table, n, d, slots=32, junk=0xA5):
    want = CN.pair_weights(mask, table, n, d)
    nbr, pairs, degree, over = _gpu_table(mask, table, n, d, slots, junk)
    w_nbr, w_pairs, w_degree = CN.table(want, n, slots)
    assert over.tolist() == [0, -1]
    assert np.array_equal(degree, w_degree) and np.array_equal(nbr, w_nbr) and np.array_equal(pairs, w_pairs), (mask.shape, d, slots)
    return want


def _odd_labels(mask):
    """the mask with every kind of label that is no cell, and its table: label 0, negative labels, labels >= L, a label mapped to -1, one mapped
    past the cells, even label ids only (2 k -> cell k - 1), one label in two blobs"""
    m = mask.astype(np.int32) * 2
    top = int(m.max())
    table = np.full(top + 1, -1, dtype=np.int32)
    table[2::2] = np.arange(top // 2)
    n = top // 2
    m[m == 14] = top + 40                      # a label past the table
    m[0:2, 0:3] = -6                           # negative labels
    m[-2:, -9:] = 6                            # the label 6 in a second blob
    m[1, 5:8] = 7                              # an odd label: inside the table, mapped to -1
    table[10] = -1                             # an unmapped label
    table[18] = n + 5                          # mapped past the cells
    return m, table, n


@pytest.mark.parametrize("shape, cells, seed", [((37, 53), 30, 21), ((64, 96), 80, 22)])
def test_the_table_is_the_restatement_s(shape, cells, seed):
    """37 x 53 is no multiple of the tile, 64 x 96 is exactly 2 x 3 tiles; plain labels and the odd ones"""
    mask = CN.random_mask(shape[0], shape[1], cells, seed)
    table, n = CN.identity_table(mask)
    odd, odd_table, odd_n = _odd_labels(mask)
    for d in REACHES:
        got = _equal_to_the_restatement(mask, table, n, d)
        assert len(got) > cells
        got = _equal_to_the_restatement(odd, odd_table, odd_n, d, junk=0x5A)
        assert got and not [k for k in got if 4 in k or 8 in k or 6 in k]      # the cells of the labels 10, 18 and 14 own no pixel


def test_an_image_thinner_than_the_reach():
    mask = np.zeros((3, 50), dtype=np.int32)
    for k in range(10):
        mask[:, 5 * k:5 * k + 4] = k + 1      # ten 3 x 4 cells, one empty column between them
    mask[1, 22:30] = 0
    table, n = CN.identity_table(mask)
    got = _equal_to_the_restatement(mask, table, n, 8)
    assert (0, 2) in got and (0, 3) not in got      # columns 3 and 10 are 7 apart, 3 and 15 are 12 apart
    _equal_to_the_restatement(mask.T.copy(), table, n, 8)
    _equal_to_the_restatement(mask[:1], table, n, 1)


@pytest.mark.parametrize("d", REACHES)
def test_contacts_on_the_tile_seams_and_the_image_borders(d):
    """64 x 96 = 2 x 3 tiles: cells in all four corners with a neighbour each, a vertical contact on the columns 31 | 32 and a horizontal one on
    the rows 31 | 32, and two pairs exactly d apart across either seam (one pixel further and they would not be in contact)"""
    mask = np.zeros((2 * TILE, 3 * TILE), dtype=np.int32)
    h, w = mask.shape
    mask[0:3, 0:3], mask[0:3, 3:6] = 1, 2
    mask[0:3, w - 3:w], mask[3:6, w - 3:w] = 3, 4
    mask[h - 3:h, 0:3], mask[h - 6:h - 3, 0:3] = 5, 6
    mask[h - 3:h, w - 3:w], mask[h - 3:h, w - 6:w - 3] = 7, 8
    mask[10:20, 28:32], mask[10:20, 32:36] = 9, 10                  # vertical contact on the seam 31 | 32
    mask[28:32, 40:50], mask[32:36, 40:50] = 11, 12                 # horizontal contact on the seam 31 | 32
    mask[40:44, 28:32], mask[40:44, 31 + d:35 + d] = 13, 14         # columns 31 and 31 + d: exactly d apart across the seam
    mask[28:32, 70:74], mask[31 + d:35 + d, 70:74] = 15, 16         # rows 31 and 31 + d
    mask[50:54, 60:64], mask[50:54, 64 + d:68 + d] = 17, 18         # columns 63 and 64 + d: d + 1 apart, no contact
    table, n = CN.identity_table(mask)
    got = _equal_to_the_restatement(mask, table, n, d)
    for a, b in ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)):
        assert got[(a - 1, b - 1)] == got[(b - 1, a - 1)] > 0
    assert got[(8, 9)] >= 10 and (16, 17) not in got
    if d == 1:
        assert got[(8, 9)] == 10 and got[(10, 11)] == 10 and got[(12, 13)] == 4 and got[(0, 1)] == 3


def _checkerboard():
    mask = np.arange(1, TILE * TILE + 1, dtype=np.int32).reshape(TILE, TILE)
    table, n = CN.identity_table(mask)
    return mask, table, n


def test_more_pairs_than_a_workgroup_s_table_and_the_retry():
    """32 x 32 cells of one pixel at d = 4: up to 48 neighbours each and 44 000 distinct pairs in one tile; 32 slots overflow, 64 fit"""
    mask, table, n = _checkerboard()
    want = CN.pair_weights(mask, table, n, 4)
    degree = np.bincount([k[0] for k in want], minlength=n)
    assert degree.max() == 48 and len(want) > 40000 and set(want.values()) == {1}
    _, _, _, over = _gpu_table(mask, table, n, 4, 32)
    assert over.tolist() == [int((degree > 32).sum()), int(np.argmax(degree > 32))]
    _equal_to_the_restatement(mask, table, n, 4, slots=64)
    g = ops.contact_graph(torch.from_numpy(mask).to(_lib.require_gpu()), np.arange(1, n + 1), 4)
    src, dst, pairs = CN.edge_list(want)
    assert g["slots"] == 64 and np.array_equal(g["src"], src) and np.array_equal(g["dst"], dst) and np.array_equal(g["pairs"], pairs)
    assert g["src"].dtype == np.int32 and g["dst"].dtype == np.int32 and g["pairs"].dtype == np.int64 and np.array_equal(g["degree"], degree)


def test_every_row_length_that_fits_gives_the_same_edges_and_two_runs_the_same_bytes():
    mask = CN.random_mask(64, 96, 80, 22)
    table, n = CN.identity_table(mask)
    lists = []
    for slots in (64, 256, 8, 1024):
        nbr, pairs, degree, over = _gpu_table(mask, table, n, 3, slots, junk=slots & 0xFF)
        assert over.tolist() == [0, -1] and degree.max() <= 8
        keep = np.arange(slots)[None, :] < degree[:, None]
        lists.append((np.repeat(np.arange(n), degree).tolist(), nbr[keep].tolist(), pairs[keep].tolist()))
        again = _gpu_table(mask, table, n, 3, slots, junk=0x3C)
        assert all(np.array_equal(a, b) and a.tobytes() == b.tobytes() for a, b in zip((nbr, pairs, degree, over), again))
    assert lists[0] == lists[1] == lists[2] == lists[3]


def test_a_generated_mask_through_the_wrapper():
    """about 150 cells on 256 x 300 from the generator of the other GPU tests, through ops.contact_graph at every reach"""
    mk = synth.make_mask_and_image(256, 300, 150, len(MARKERS), SEED, want_image=False)[0].numpy().astype(np.int32)
    ids = np.unique(mk[mk > 0])
    table = np.full(int(ids.max()) + 1, -1, dtype=np.int32)
    table[ids] = np.arange(len(ids))
    md = torch.from_numpy(mk).to(_lib.require_gpu())
    for d in REACHES:
        want = CN.pair_weights(mk, table, len(ids), d)
        src, dst, pairs = CN.edge_list(want)
        g = ops.contact_graph(md, ids, d)
        assert len(src) > 30 and np.array_equal(g["src"], src) and np.array_equal(g["dst"], dst) and np.array_equal(g["pairs"], pairs)
        assert np.array_equal(g["degree"], np.bincount(src, minlength=len(ids))) and g["slots"] == 32
    empty = ops.contact_graph(md, np.zeros(0, dtype=np.int64), 2)
    assert len(empty["src"]) == 0 and len(empty["degree"]) == 0


def test_a_background_labelled_as_a_cell_overflows_and_is_named():
    """200 x 200, the background carries the label 2501 and is mapped to a cell; 2500 cells of one pixel on a 4-px grid all touch it at d = 1"""
    mask = np.full((200, 200), 2501, dtype=np.int32)
    mask[1::4, 1::4] = np.arange(1, 2501, dtype=np.int32).reshape(50, 50)
    ids = np.arange(1, 2502)
    with pytest.raises(ValueError, match=r"mask label 2501; a background region labelled as a cell is the usual cause"):
        ops.contact_graph(torch.from_numpy(mask).to(_lib.require_gpu()), ids, 1)
    table, n = CN.identity_table(mask)
    _, _, _, over = _gpu_table(mask, table, n, 1, 1024)
    assert n == 2501 and over.tolist() == [1, 2500]


# ---- the null over an edge list ---------------------------------------------------------------------------------------------------------------------
def _gpu_null(src, dst, labels, t, seed, image, p0, n_perms, counts=None, junk=0x5A):
    dev = _lib.require_gpu()
    sd = torch.from_numpy(np.ascontiguousarray(src, dtype=np.int32)).to(dev)
    dd = torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int32)).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)
    n = len(labels)
    if counts is None:
        counts = torch.zeros((n_perms, t, t), dtype=torch.int64, device=dev)
    ws = torch.full((ops.edge_perm_counts_ws_bytes(n, n_perms),), junk, dtype=torch.uint8, device=dev)
    status = lib().ribca_edge_perm_counts(ptr(sd), ptr(dd), len(src), ptr(td), n, t, seed, image, p0, n_perms, ptr(counts), ptr(ws), ws.numel(),
                                          stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    return counts


def _random_graph(n, e, t, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, n, e), rng.randint(0, n, e), rng.randint(0, t, n)


@pytest.mark.parametrize("n, e, t, perms", [(300, 700, 1, 5), (300, 700, 4, 5), (700, 9000, 64, 3), (50, 200, 4, 1), (50, 200, 3, 130)])
def test_the_null_is_the_restatement_s(n, e, t, perms):
    """one type, a few, the most; more edges than one workgroup's slab (4096); one permutation; more permutations than one batch (128)"""
    src, dst, labels = _random_graph(n, e, t, 31 + t)
    got = _gpu_null(src, dst, labels, t, 7, 2, 3, perms).cpu().numpy()
    assert np.array_equal(got, CN.edge_perm_counts(src, dst, labels, t, 7, 2, 3, perms))
    assert (got.sum(axis=(1, 2)) == e).all()


def test_the_null_skips_what_is_out_of_range():
    src, dst, labels = _random_graph(200, 900, 4, 41)
    labels = labels.copy()
    labels[::7] = 4
    labels[3::11] = -1
    labels[5::13] = 300
    src, dst = src.copy(), dst.copy()
    src[::9], dst[4::10], src[7::31] = 200, -1, 1 << 30
    got = _gpu_null(src, dst, labels, 4, 1, 0, 0, 6).cpu().numpy()
    assert np.array_equal(got, CN.edge_perm_counts(src, dst, labels, 4, 1, 0, 0, 6)) and 0 < got[0].sum() < 900


def test_the_null_is_pure_in_the_permutation_and_accumulates():
    src, dst, labels = _random_graph(400, 1500, 5, 51)
    whole = _gpu_null(src, dst, labels, 5, 9, 4, 0, 50).cpu().numpy()
    first = _gpu_null(src, dst, labels, 5, 9, 4, 0, 20, junk=0x11).cpu().numpy()
    rest = _gpu_null(src, dst, labels, 5, 9, 4, 20, 30, junk=0xEE).cpu().numpy()
    assert np.array_equal(whole, np.concatenate([first, rest])) and not np.array_equal(whole[0], whole[1])
    # two images into one tensor, through the wrapper and its out=
    src2, dst2, labels2 = _random_graph(90, 300, 5, 52)
    acc = ops.edge_perm_counts(src, dst, labels, 5, 9, 4, 0, 8)
    same = ops.edge_perm_counts(src2, dst2, labels2, 5, 9, 5, 0, 8, out=acc)
    assert same is acc
    want = CN.edge_perm_counts(src, dst, labels, 5, 9, 4, 0, 8) + CN.edge_perm_counts(src2, dst2, labels2, 5, 9, 5, 0, 8)
    assert np.array_equal(acc.cpu().numpy(), want)
    with pytest.raises(ValueError, match="out must be"):
        ops.edge_perm_counts(src, dst, labels, 5, 9, 4, 0, 7, out=acc)
    with pytest.raises(_lib.RibcaError, match="needs 1 <= T <= 64"):
        ops.edge_perm_counts(src, dst, labels, 65, 9, 4, 0, 1)


def test_planted_contact_on_the_gpu():
    """the layout of tests/test_contact_host.py, 50 permutations: the GPU's graph and counts are the restatement's, so its z-scores are"""
    mask, labels = CN.planted_mask()
    ids = np.arange(1, 521)
    table, n = CN.identity_table(mask)
    md = torch.from_numpy(mask).to(_lib.require_gpu())
    for d, bound in ((1, 20.7), (4, 17.3)):
        g = ops.contact_graph(md, ids, d)
        src, dst, pairs = CN.edge_list(CN.pair_weights(mask, table, n, d))
        assert np.array_equal(g["src"], src) and np.array_equal(g["dst"], dst) and np.array_equal(g["pairs"], pairs)
        null = ops.edge_perm_counts(g["src"], g["dst"], labels, 4, 0, 0, 0, 50).cpu().numpy()
        assert np.array_equal(null, CN.edge_perm_counts(src, dst, labels, 4, 0, 0, 0, 50))
        z = enrichment.z_scores(contact.observed(g["src"], g["dst"], g["pairs"], labels, 4)[0], null)["z"]
        print("d", d, "z[A][B]", z[0, 1])
        assert z[0, 1] > bound and z[1, 0] > bound


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
REACH = 3
PERMS = 6


def _analyse(a):
    assert a.contact_analysis(distance=REACH, n_perms=PERMS, integrate=True) is None
    integrated = list(a.contact_stats)
    assert a.contact_analysis(distance=REACH, n_perms=PERMS, integrate=False) is None
    return integrated


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two-image batch of the cell-type plots, annotated once with "Others" among the cell types, and analysed"""
    return annotated_batch(tmp_path_factory, "contact", _analyse, "_contact")


def _restated_graph(a, i):
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    ids = np.asarray(a.preprocessor.cell_ids[i], dtype=np.int64)
    table = np.full(int(ids.max()) + 1, -1, dtype=np.int32)
    table[ids] = np.arange(len(ids))
    return CN.edge_list(CN.pair_weights(mask, table, len(ids), REACH))


def _check_group(a, files, stem, tail, images, stats, perms=PERMS):
    from PIL import Image
    t = len(a.cell_types)
    names = [str(c) for c in a.cell_types]
    edges, weight, null, n_edges = np.zeros((t, t), dtype=np.int64), np.zeros((t, t), dtype=np.int64), np.zeros((perms, t, t), dtype=np.int64), 0
    for i in images:
        src, dst, pairs = _restated_graph(a, i)
        types = a._cell_type_ints(i)
        here = contact.observed(src, dst, pairs, types, t)
        edges, weight, n_edges = edges + here[0], weight + here[1], n_edges + len(src)
        null += CN.edge_perm_counts(src, dst, types, t, 0, a._image_number(i), 0, perms)
    want = enrichment.z_scores(edges, null)
    assert n_edges > 100 and np.isfinite(want["z"]).any()
    assert files[f"{stem}_table{tail}.csv"].decode() == contact.table_csv(names, edges, weight, want)
    assert files[f"{stem}{tail}.csv"].decode() == enrichment.matrix_csv(names, want["z"])
    expected = [f"{stem}_table{tail}.csv", f"{stem}_pairs{tail}.png", f"{stem}{tail}.csv", f"{stem}{tail}.png"]
    assert stats["files"] == expected and stats["file"] == expected[0]
    assert stats["n"] == sum(len(a.preprocessor.cell_ids[i]) for i in images) and stats["E"] == n_edges and stats["T"] == t and stats["P"] == perms
    assert stats["d"] == REACH and stats["seed"] == 0 and stats["slots"] == 32 and 1 <= stats["max_degree"] <= 32
    assert min(stats["graph_ms"], stats["perm_ms"], stats["draw_ms"]) >= 0.0
    dev = _lib.require_gpu()
    lut = colors.diverging_table()
    cell = a.HEATMAP_CELL
    share = contact.row_normalised(weight)
    for fig, table, lo, hi in ((stats["figures"][0], share, 0.0, float(share.max())), (stats["figures"][1], want["z"], None, None)):
        if lo is None:
            lo, hi = -enrichment.colour_limit(want["z"]), enrichment.colour_limit(want["z"])
        img = np.array(Image.open(io.BytesIO(files[fig["file"]])))
        top, left = fig["rect"]
        rect = ops.table_raster(torch.from_numpy(np.ascontiguousarray(table)).to(dev), torch.from_numpy(lut).to(dev), cell, a.HEATMAP_GAP, lo, hi).cpu().numpy()
        assert np.array_equal(img[top:top + t * cell, left:left + t * cell], rect), fig["file"]
    assert [f["what"] for f in stats["figures"]] == ["pairs", "z"]
    return expected


def _check_image(a, files, i):
    """the two per-image tables against ops.contact_graph, the degree map against the viridis entry computed here"""
    from PIL import Image
    names = [str(c) for c in a.cell_types]
    ids = a.preprocessor.cell_ids[i]
    types = a._cell_type_ints(i)
    g = ops.contact_graph(a.preprocessor.masks_dev[i], ids, REACH)
    src, dst, pairs = _restated_graph(a, i)
    assert np.array_equal(g["src"], src) and np.array_equal(g["dst"], dst) and np.array_equal(g["pairs"], pairs)
    number = a._image_number(i)
    assert files[f"x_contact_cells_{number}.csv"].decode() == contact.cells_csv(ids, types, names, g["src"], g["dst"], g["pairs"], g["degree"])
    rows = [r.split(",") for r in files[f"x_contact_cells_{number}.csv"].decode().strip().split("\n")]
    assert rows[0][:4] == ["cell_id", "cell_type", "degree", "pixel_pairs"] and len(rows) == 1 + len(ids)
    assert [int(r[0]) for r in rows[1:]] == [int(v) for v in ids] and [int(r[2]) for r in rows[1:]] == g["degree"].tolist()
    assert [sum(int(v) for v in r[4:]) for r in rows[1:]] == g["degree"].tolist()      # every neighbour has a type
    assert files[f"x_contact_edges_{number}.csv"].decode() == contact.edges_csv(ids, types, names, g["src"], g["dst"], g["pairs"])
    edge_rows = files[f"x_contact_edges_{number}.csv"].decode().strip().split("\n")[1:]
    assert len(edge_rows) * 2 == len(src) and all(int(r.split(",")[0]) < int(r.split(",")[1]) for r in edge_rows)
    mask = a.preprocessor.masks_dev[i].cpu().numpy()
    lut = colors.viridis_table()
    img = np.array(Image.open(io.BytesIO(files[f"x_contact_degree_{number}.png"])))
    assert img.shape == mask.shape + (3,) and (img[mask == 0] == 0).all()
    for j in (0, len(ids) // 2, len(ids) - 1, int(np.argmax(g["degree"]))):      # a pixel of a known cell
        r, c = np.argwhere(mask == ids[j])[0]
        assert img[r, c].tolist() == lut[int(min(int(g["degree"][j]) / 12, 1.0) * 255)].tolist(), j
    return [f"x_contact_edges_{number}.csv", f"x_contact_cells_{number}.csv", f"x_contact_degree_{number}.png"]


def test_files_tables_and_maps_are_the_restatement_s(batch):
    a, files = batch["a"], batch["files"]
    assert len(a.cell_types) >= 3 and len(batch["integrated"]) == 1 and len(a.contact_stats) == 2
    expected = _check_group(a, files, "x_integrated_contact", "", [0, 1], batch["integrated"][0])
    for i in (0, 1):
        expected += _check_group(a, files, "x_contact", f"_{i}", [i], a.contact_stats[i])
        per_image = _check_image(a, files, i)
        assert a.contact_stats[i]["image_files"] == per_image
        expected += per_image
    assert sorted(files) == sorted(expected)
    assert sorted(batch["integrated"][0]["image_files"]) == sorted(f for f in expected if "_edges_" in f or "_cells_" in f or "_degree_" in f)
    log = open(a.logger.log_file_path).read()
    assert log.count("Contact graph x_integrated_contact_table.csv: ") == 1 and log.count("Contact graph x_contact_table_1.csv: ") == 1


def test_a_second_run_writes_the_same_bytes_and_no_null_means_no_z_files(batch, monkeypatch):
    out = os.path.join(batch["tmp"], "two")
    b = run_annotator(batch["root"], out, -1, batch["thr"])
    b.contact_analysis(distance=REACH, integrate=False)
    got = result_files(out, "_contact")
    assert sorted(got) == sorted(f for f in batch["files"] if "integrated" not in f and f not in [f"x_contact_{i}.{e}" for i in (0, 1) for e in ("csv", "png")])
    assert got["x_contact_table_0.csv"].decode().split("\n")[0] == "cell_type,neighbour,edges,pixel_pairs" and b.contact_stats[0]["P"] == 0
    assert all(got[f] == batch["files"][f] for f in got if "_table_" not in f)
    _analyse(b)
    assert result_files(out, "_contact") == batch["files"]
    # the seed moves the null and nothing else
    monkeypatch.setenv("RIBCA_CONTACT_SEED", "5")
    b.contact_analysis(distance=REACH, n_perms=PERMS, integrate=True)
    assert b.contact_stats[0]["seed"] == 5
    seeded = result_files(out, "_contact")
    name = "x_integrated_contact_table.csv"
    rows, base = seeded[name].decode().split("\n"), batch["files"][name].decode().split("\n")
    assert [r.split(",")[:4] for r in rows] == [r.split(",")[:4] for r in base] and rows != base
    assert all(seeded[f] == batch["files"][f] for f in seeded if "integrated" not in f or "_pairs" in f)


def test_errors_leave_the_files_alone(batch):
    a = batch["a"]
    with pytest.raises(ValueError, match="distance must be an integer from 1 to 8"):
        a.contact_analysis(distance=9)
    with pytest.raises(ValueError, match="must not be negative"):
        a.contact_analysis(n_perms=-1)
    assert result_files(batch["out"], "_contact") == batch["files"]
    from multiplexed_image_annotator_amd.annotator import Annotator
    root = batch["root"]
    fresh = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", os.path.join(batch["tmp"], "fresh"), "x", False, False,
                      -1, True, 0.3, 99.8, 0.3, 30, None)
    with pytest.raises(ValueError, match="No annotations"):
        fresh.contact_analysis()


def test_pipeline_switch(tmp_path):
    """--contact-distance 0 (the default) writes no contact file and changes no other; D > 0 writes the per-image and the integrated ones"""
    import main as cli
    listing, common = cli_runs(tmp_path, {"off": [], "on": ["--contact-distance", "2", "--contact-perms", "5"], "bare": ["--contact-distance", "2"]},
                               "contact")
    off, on, bare = listing["off"], listing["on"], listing["bare"]
    assert [f for f in on if "contact" in f] == sorted(["c_contact_edges_0.csv", "c_contact_cells_0.csv", "c_contact_degree_0.png", "c_integrated_contact_table.csv",
                                                       "c_integrated_contact_pairs.png", "c_integrated_contact.csv", "c_integrated_contact.png"])
    assert [f for f in bare if "contact" in f] == sorted(["c_contact_edges_0.csv", "c_contact_cells_0.csv", "c_contact_degree_0.png",
                                                         "c_integrated_contact_table.csv", "c_integrated_contact_pairs.png"])
    for f in off:
        if f.endswith(".csv") or f.endswith(".png"):
            assert open(tmp_path / "off" / "results" / f, "rb").read() == open(tmp_path / "on" / "results" / f, "rb").read(), f
    rows = open(tmp_path / "on" / "results" / "c_integrated_contact_table.csv").read().split("\n")
    assert rows[0] == "cell_type,neighbour,edges,pixel_pairs,null_mean,null_std,z,n_ge,n_le"
    assert cli.parse_args(common + ["--main-dir", "x"]).contact_distance == 0


def _rank_body(rank, root, thr):
    a = run_annotator(root, os.path.join(root, "tiles"), -1, thr)
    assert a.tile_mode
    integrated = _analyse(a)
    return [[s["file"] for s in integrated], [s["file"] for s in a.contact_stats]]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], batch["thr"], unset=("RIBCA_CONTACT_SEED",))
    assert result_files(os.path.join(batch["root"], "tiles"), "_contact") == batch["files"]
    assert wrote == [[["x_integrated_contact_table.csv"], ["x_contact_table_0.csv"]], [[], ["x_contact_table_1.csv"]]]
