"""The contingency table of two masks on the GPU: ribca_mask_overlap and ribca_mask_compartments (csrc/overlap.hip) against
tests/overlap_numpy.py for EQUALITY, every output and the workspace junk-filled to exactly the queried size before every call: an image
smaller than a tile, ragged edges, tile seams, rows that take the 16-byte loads and rows that cannot, every kind of label that is no cell or no
object in both masks, one mask against itself, more partners than the longest row, more distinct pairs than a workgroup's table holds, the
retry of ops.overlap_pairs and its overflow report, the split into inner and outer, and every refusal."""
import numpy as np
import pytest
import torch

import contact_numpy as CN
import overlap_numpy as ON
from multiplexed_image_annotator_amd import _lib, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_lib.require_gpu())


def _misaligned(a):
    """the same (H, W) int32 values in device memory that starts 4 bytes past a 16-byte boundary"""
    flat = torch.empty(a.size + 1, dtype=torch.int32, device=_lib.require_gpu())
    view = flat[1:].view(a.shape)
    view.copy_(_dev(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _gpu_overlap(ma, ta, n, mb, tb, m, slots, junk=0xA5, same=False, misaligned=False):
    """the entry point itself on junk-filled outputs and a junk-filled workspace of exactly the size the query asks for"""
    dev = _lib.require_gpu()
    h, w = ma.shape
    ad = _misaligned(ma) if misaligned else _dev(ma)
    bd = ad if same else (_misaligned(mb) if misaligned else _dev(mb))
    tad, tbd = _dev(ta), _dev(tb)
    partner = torch.full((n, slots), junk, dtype=torch.int32, device=dev)
    inter = torch.full((n, slots), junk, dtype=torch.int64, device=dev)
    degree = torch.full((n,), junk, dtype=torch.int32, device=dev)
    area_a = torch.full((n,), junk, dtype=torch.int32, device=dev)
    area_b = torch.full((m,), junk, dtype=torch.int32, device=dev)
    over = torch.full((2,), junk, dtype=torch.int32, device=dev)
    ws = torch.full((ops.mask_overlap_ws_bytes(h, w, n, slots),), junk, dtype=torch.uint8, device=dev)
    status = lib().ribca_mask_overlap(ptr(ad), ptr(bd), h, w, ptr(tad), len(ta), n, ptr(tbd), len(tb), m, slots, ptr(partner), ptr(inter), ptr(degree),
                                      ptr(area_a), ptr(area_b), ptr(over), ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    return tuple(t.cpu().numpy() for t in (partner, inter, degree, area_a, area_b, over))


def _equal_to_the_restatement(ma, ta, n, mb, tb, m, slots=16, **kw):
    pairs, w_area_a, w_area_b = ON.overlap(ma, ta, n, mb, tb, m)
    partner, inter, degree, area_a, area_b, over = _gpu_overlap(ma, ta, n, mb, tb, m, slots, **kw)
    w_partner, w_inter, w_degree = ON.table(pairs, n, slots)
    assert over.tolist() == [0, -1]
    assert np.array_equal(area_a, w_area_a) and np.array_equal(area_b, w_area_b), ma.shape
    assert np.array_equal(degree, w_degree) and np.array_equal(partner, w_partner) and np.array_equal(inter, w_inter), (ma.shape, slots)
    return pairs


def _table(cells):
    """labels 1 .. cells -> 0 .. cells - 1, label 0 -> none"""
    return np.arange(-1, cells, dtype=np.int32)


def _two_masks(shape, cells, seed):
    return CN.random_mask(shape[0], shape[1], cells, seed), CN.random_mask(shape[0], shape[1], max(cells - 1, 2), seed + 100, radius=4.0)


@pytest.mark.parametrize("shape, cells, seed", [((1, 1), 3, 1), ((1, 70), 5, 2), ((33, 65), 40, 3), ((70, 45), 60, 4), ((96, 96), 200, 5)])
def test_the_table_is_the_restatement_s(shape, cells, seed):
    """an image smaller than a tile, one row across three tiles, ragged edges in either direction, exactly 3 x 3 tiles (the 16-byte loads)"""
    ma, mb = _two_masks(shape, cells, seed)
    m = max(cells - 1, 2)
    pairs = _equal_to_the_restatement(ma, _table(cells), cells, mb, _table(m), m)
    if shape != (1, 1):
        assert len(pairs) >= 3
    pairs_t = _equal_to_the_restatement(mb, _table(m), m, ma, _table(cells), cells, junk=0x5A)
    assert {(j, i): v for (i, j), v in pairs.items()} == pairs_t


def test_aligned_rows_in_misaligned_memory_take_the_scalar_loads():
    ma, mb = _two_masks((96, 96), 200, 5)
    _equal_to_the_restatement(ma, _table(200), 200, mb, _table(199), 199, misaligned=True)


def _odd_labels(mask):
    """the mask with every kind of label that is no cell, and its table: negative labels, labels past the table, a label mapped to -1, one mapped
    past the cells, even labels only (2 k -> k - 1), one label in two blobs"""
    m = mask.astype(np.int32) * 2
    top = int(m.max())
    table = np.full(top + 1, -1, dtype=np.int32)
    table[2::2] = np.arange(top // 2)
    n = top // 2
    m[m == 14] = top + 40
    m[0:2, 0:3] = -6
    m[-2:, -9:] = 6
    m[1, 5:8] = 7
    table[10] = -1
    table[18] = n + 5
    return m, table, n


def test_labels_that_are_no_cell_and_no_object():
    ma, mb = _two_masks((70, 45), 60, 4)
    oa, ta, n = _odd_labels(ma)
    ob, tb, m = _odd_labels(mb)
    pairs = _equal_to_the_restatement(oa, ta, n, ob, tb, m)
    assert pairs and not [k for k in pairs if k[0] in (4, 8, 6) or k[1] in (4, 8, 6)]      # the indices of the labels 10, 18 and 14 own no pixel


def test_a_mask_against_itself():
    ma = CN.random_mask(70, 45, 60, 4)
    partner, inter, degree, area_a, area_b, over = _gpu_overlap(ma, _table(60), 60, ma, _table(60), 60, 8, same=True)
    here = area_a > 0
    assert over.tolist() == [0, -1] and here.sum() > 30 and np.array_equal(area_a, area_b)
    assert (degree[here] == 1).all() and (degree[~here] == 0).all()
    assert np.array_equal(partner[here, 0], np.flatnonzero(here)) and np.array_equal(inter[here, 0], area_a[here])
    assert np.array_equal(area_a, np.bincount(ma[ma > 0] - 1, minlength=60))


def test_more_partners_than_the_longest_row():
    """one 64 x 64 cell (label 7, cell 2 of 3) over a B whose every pixel is its own object: 4096 partners"""
    ma = np.full((64, 64), 7, dtype=np.int32)
    mb = np.arange(1, 4097, dtype=np.int32).reshape(64, 64)
    ta = np.full(8, -1, dtype=np.int32)
    ta[3], ta[5], ta[7] = 0, 1, 2
    _, _, _, area_a, area_b, over = _gpu_overlap(ma, ta, 3, mb, _table(4096), 4096, 1024)
    assert over.tolist() == [1, 2]
    assert area_a.tolist() == [0, 0, 4096] and (area_b == 1).all()      # the areas stay exact
    with pytest.raises(ValueError, match=r"overlap more than 1024 objects of the second mask, the lowest of them mask label 7; a background region"):
        ops.overlap_pairs(_dev(ma), [7], _dev(mb), np.arange(1, 4097))


def test_a_row_of_1024_partners_is_reached_by_doubling():
    ma = np.full((64, 64), 7, dtype=np.int32)
    mb = (np.arange(32)[:, None] * 32 + np.arange(32)[None, :] + 1).astype(np.int32).repeat(2, axis=0).repeat(2, axis=1)
    for slots in (8, 512):
        assert _gpu_overlap(ma, ON.id_table([7]), 1, mb, _table(1024), 1024, slots)[5].tolist() == [1, 0]
    _equal_to_the_restatement(ma, ON.id_table([7]), 1, mb, _table(1024), 1024, slots=1024)
    g = ops.overlap_pairs(_dev(ma), [7], _dev(mb), np.arange(1, 1025))
    assert g["slots"] == 1024 and g["degree"].tolist() == [1024] and (g["inter"] == 4).all() and np.array_equal(g["obj"], np.arange(1024))
    assert g["cell"].dtype == np.int32 and g["obj"].dtype == np.int32 and g["inter"].dtype == np.int64 and g["area_a"].tolist() == [4096]


def test_more_distinct_pairs_than_a_workgroup_s_table():
    """per-pixel-distinct labels in BOTH masks, 64 x 64: 1024 distinct pairs per tile, and as many (cell, none) and (none, object) entries"""
    ma = np.arange(1, 4097, dtype=np.int32).reshape(64, 64)
    mb = ma[::-1, ::-1].copy()
    pairs = _equal_to_the_restatement(ma, _table(4096), 4096, mb, _table(4096), 4096, slots=8)
    assert len(pairs) == 4096 and set(pairs.values()) == {1}


def test_every_row_length_that_fits_gives_the_same_pairs_and_two_runs_the_same_bytes():
    ma, mb = _two_masks((96, 96), 200, 5)
    lists = []
    for slots in (64, 256, 8, 1024):
        got = _gpu_overlap(ma, _table(200), 200, mb, _table(199), 199, slots, junk=slots & 0xFF)
        partner, inter, degree = got[:3]
        assert got[5].tolist() == [0, -1] and degree.max() <= 8
        keep = np.arange(slots)[None, :] < degree[:, None]
        lists.append((np.repeat(np.arange(200), degree).tolist(), partner[keep].tolist(), inter[keep].tolist(), got[3].tolist(), got[4].tolist()))
        again = _gpu_overlap(ma, _table(200), 200, mb, _table(199), 199, slots, junk=0x3C)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    assert lists[0] == lists[1] == lists[2] == lists[3]


def test_the_wrapper_on_two_masks():
    ma, mb = _two_masks((70, 45), 60, 4)
    ids_a, ids_b = ON.labels_of(ma), ON.labels_of(mb)
    pairs, area_a, area_b = ON.overlap(ma, ON.id_table(ids_a), len(ids_a), mb, ON.id_table(ids_b), len(ids_b))
    cell, obj, inter = ON.pair_arrays(pairs)
    g = ops.overlap_pairs(_dev(ma), ids_a, _dev(mb), ids_b)
    assert np.array_equal(g["cell"], cell) and np.array_equal(g["obj"], obj) and np.array_equal(g["inter"], inter) and g["slots"] == 8
    assert np.array_equal(g["area_a"], area_a) and np.array_equal(g["area_b"], area_b) and np.array_equal(g["degree"], np.bincount(cell, minlength=len(ids_a)))
    empty = ops.overlap_pairs(_dev(ma), ids_a, _dev(np.zeros_like(mb)), [])
    assert len(empty["cell"]) == 0 and np.array_equal(empty["area_a"], area_a) and len(empty["area_b"]) == 0 and not empty["degree"].any()
    none = ops.overlap_pairs(_dev(ma), [], _dev(mb), ids_b)
    assert len(none["inter"]) == 0 and len(none["degree"]) == 0 and np.array_equal(none["area_b"], area_b)


# ---- compartments ----------------------------------------------------------------------------------------------------------------------------------
def _gpu_compartments(ma, ta, n, mb, tb, m, owner, junk=0x77, misaligned=False):
    dev = _lib.require_gpu()
    h, w = ma.shape
    ad, bd = (_misaligned(ma), _misaligned(mb)) if misaligned else (_dev(ma), _dev(mb))
    tad, tbd, od = _dev(ta), _dev(tb), _dev(owner)
    inner = torch.full((h, w), junk, dtype=torch.int32, device=dev)
    outer = torch.full((h, w), junk, dtype=torch.int32, device=dev)
    status = lib().ribca_mask_compartments(ptr(ad), ptr(bd), h, w, ptr(tad), len(ta), n, ptr(tbd), len(tb), m, ptr(od), ptr(inner), ptr(outer),
                                           stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    return inner.cpu().numpy(), outer.cpu().numpy()


@pytest.mark.parametrize("shape, cells, seed, misaligned", [((1, 1), 3, 1, False), ((33, 65), 40, 3, False), ((96, 96), 200, 5, False),
                                                            ((96, 96), 200, 5, True), ((70, 45), 60, 4, False)])
def test_inner_and_outer_are_the_restatement_s(shape, cells, seed, misaligned):
    ma, mb = _two_masks(shape, cells, seed)
    if shape == (70, 45):
        (ma, ta, n), (mb, tb, m) = _odd_labels(ma), _odd_labels(mb)
    else:
        ta, n, tb, m = _table(cells), cells, _table(max(cells - 1, 2)), max(cells - 1, 2)
    pairs, _, area_b = ON.overlap(ma, ta, n, mb, tb, m)
    owner = np.array(ON.owners(pairs, area_b, 50)[0], dtype=np.int32)
    inner, outer = _gpu_compartments(ma, ta, n, mb, tb, m, owner, misaligned=misaligned)
    w_inner, w_outer = ON.compartments(ma, ta, n, mb, tb, m, owner)
    assert np.array_equal(inner, w_inner) and np.array_equal(outer, w_outer)
    is_cell = ON.index_image(ma, ta, n) >= 0
    assert np.array_equal((inner > 0).astype(int) + (outer > 0).astype(int), is_cell.astype(int))
    if shape != (1, 1):
        assert (inner > 0).any() and (outer > 0).any()
    nobody = np.full(m, -1, dtype=np.int32)
    inner, outer = _gpu_compartments(ma, ta, n, mb, tb, m, nobody, junk=0x11, misaligned=misaligned)
    assert not inner.any() and np.array_equal(outer, np.where(is_cell, ma, 0))


def test_the_compartments_wrapper():
    ma, mb = _two_masks((70, 45), 60, 4)
    ids_a, ids_b = ON.labels_of(ma), ON.labels_of(mb)
    want = ON.image_texts(ma, mb)
    inner, outer = ops.mask_compartments(_dev(ma), ids_a, _dev(mb), ids_b, want["owner"])
    assert np.array_equal(inner.cpu().numpy(), want["inner"]) and np.array_equal(outer.cpu().numpy(), want["outer"])
    inner, outer = ops.mask_compartments(_dev(ma), ids_a, _dev(np.zeros_like(mb)), [], [])
    assert not inner.cpu().numpy().any() and np.array_equal(outer.cpu().numpy(), ma)
    inner, outer = ops.mask_compartments(_dev(ma), [], _dev(mb), ids_b, np.full(len(ids_b), -1))
    assert not inner.cpu().numpy().any() and not outer.cpu().numpy().any()
    with pytest.raises(ValueError, match="one owner per object"):
        ops.mask_compartments(_dev(ma), ids_a, _dev(mb), ids_b, [0])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_a_status_that_names_the_entry_point_and_writes_nothing():
    dev = _lib.require_gpu()
    h, w, n, m, s = 8, 12, 4, 5, 8
    ma, mb = torch.zeros((h, w), dtype=torch.int32, device=dev), torch.zeros((h, w), dtype=torch.int32, device=dev)
    ta, tb = torch.zeros(6, dtype=torch.int32, device=dev), torch.zeros(7, dtype=torch.int32, device=dev)
    outs = {"partner": torch.full((n, s), 0x5B, dtype=torch.int32, device=dev), "inter": torch.full((n, s), 0x5B, dtype=torch.int64, device=dev),
            "degree": torch.full((n,), 0x5B, dtype=torch.int32, device=dev), "area_a": torch.full((n,), 0x5B, dtype=torch.int32, device=dev),
            "area_b": torch.full((m,), 0x5B, dtype=torch.int32, device=dev), "over": torch.full((2,), 0x5B, dtype=torch.int32, device=dev)}
    ws = torch.full((ops.mask_overlap_ws_bytes(h, w, n, s),), 0x5B, dtype=torch.uint8, device=dev)
    assert ws.numel() > 0

    def overlap(**kw):
        a = dict(mask_a=ptr(ma), mask_b=ptr(mb), H=h, W=w, ta=ptr(ta), La=6, n=n, tb=ptr(tb), Lb=7, m=m, S=s, ws=ptr(ws), ws_bytes=ws.numel())
        a.update({k: ptr(v) for k, v in outs.items()})
        a.update(kw)
        return lib().ribca_mask_overlap(a["mask_a"], a["mask_b"], a["H"], a["W"], a["ta"], a["La"], a["n"], a["tb"], a["Lb"], a["m"], a["S"], a["partner"],
                                        a["inter"], a["degree"], a["area_a"], a["area_b"], a["over"], a["ws"], a["ws_bytes"], stream_ptr())

    def refused(status, text):
        assert status != 0 and text in lib().ribca_last_error().decode(), lib().ribca_last_error()

    for name in ("mask_a", "mask_b", "ta", "tb", "partner", "inter", "degree", "area_a", "area_b", "over", "ws"):
        refused(overlap(**{name: None}), "ribca_mask_overlap: NULL buffer")
    for kw in (dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15)):
        refused(overlap(**kw), "ribca_mask_overlap: needs 1 <= H, W and H W < 2^31")
    for kw in (dict(La=0), dict(Lb=0)):
        refused(overlap(**kw), "ribca_mask_overlap: needs 1 <= La, Lb")
    for kw in (dict(n=0), dict(m=0), dict(n=(1 << 21) + 1), dict(m=(1 << 21) + 1)):
        refused(overlap(**kw), "ribca_mask_overlap: needs 1 <= n, m <= 2^21")
    for bad in (0, 4, 12, 2048):
        refused(overlap(S=bad), "ribca_mask_overlap: S must be a power of two in 8 .. 1024")
        assert ops.mask_overlap_ws_bytes(h, w, n, bad) == 0
    refused(overlap(ws_bytes=ws.numel() - 1), "ribca_mask_overlap: workspace too small")
    for kw in (dict(partner=ptr(outs["inter"])), dict(degree=ptr(outs["area_a"])), dict(area_b=ptr(mb)), dict(over=ptr(ta)), dict(ws=ptr(outs["inter"])),
               dict(area_a=ptr(ma))):
        refused(overlap(**kw), "ribca_mask_overlap: the outputs and ws must not overlap")
    torch.cuda.synchronize()
    assert all((v == 0x5B).all().item() for v in outs.values()) and (ws == 0x5B).all().item()
    assert overlap(mask_b=ptr(ma)) == 0      # one mask twice is allowed
    torch.cuda.synchronize()
    assert outs["over"].tolist() == [0, -1]

    owner = torch.full((m,), -1, dtype=torch.int32, device=dev)
    inner = torch.full((h, w), 0x5B, dtype=torch.int32, device=dev)
    outer = torch.full((h, w), 0x5B, dtype=torch.int32, device=dev)

    def split(**kw):
        a = dict(mask_a=ptr(ma), mask_b=ptr(mb), H=h, W=w, ta=ptr(ta), La=6, n=n, tb=ptr(tb), Lb=7, m=m, owner=ptr(owner), inner=ptr(inner), outer=ptr(outer))
        a.update(kw)
        return lib().ribca_mask_compartments(a["mask_a"], a["mask_b"], a["H"], a["W"], a["ta"], a["La"], a["n"], a["tb"], a["Lb"], a["m"], a["owner"],
                                             a["inner"], a["outer"], stream_ptr())

    for name in ("mask_a", "mask_b", "ta", "tb", "owner", "inner", "outer"):
        refused(split(**{name: None}), "ribca_mask_compartments: NULL buffer")
    refused(split(H=0), "ribca_mask_compartments: needs 1 <= H, W and H W < 2^31")
    refused(split(Lb=0), "ribca_mask_compartments: needs 1 <= La, Lb")
    refused(split(m=0), "ribca_mask_compartments: needs 1 <= n, m <= 2^21")
    for kw in (dict(inner=ptr(outer)), dict(outer=ptr(ma)), dict(inner=ptr(mb)), dict(outer=ptr(owner))):
        refused(split(**kw), "ribca_mask_compartments: inner and outer must not overlap")
    torch.cuda.synchronize()
    assert (inner == 0x5B).all().item() and (outer == 0x5B).all().item()
    assert split(mask_b=ptr(ma)) == 0
    torch.cuda.synchronize()
    assert not inner.any().item() and not outer.any().item()      # label 0 maps to cell 0 of the zero table: owner -1, so outer = mask_a = 0
