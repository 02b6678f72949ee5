"""Cell outlines on the GPU: ribca_mask_rings and ribca_mask_ring_vertices (csrc/outlines.hip) against tests/outlines_numpy.py for EQUALITY of the
bytes of the sorted ring rows and of the vertices, outputs and workspace junk-filled to exactly the queried size before every call and the input
unchanged after it: damaged discs over 3 x 5 ragged tiles with bars across every seam and cells on all four borders, the special shapes of
tests/components_numpy.py, thin, tiny and uniform masks, a checkerboard, a nested ring, labels that map to no cell and two labels that map to
one; the even-odd fill of the GPU's rings gives the owned pixels back; area, perimeter and Euler number agree with ops.mask_morphology; the cap
protocol; ring rows that do not fit the mask; the refusals."""
import numpy as np
import pytest
import torch

import components_numpy as CN
import outlines_numpy as ON
from multiplexed_image_annotator_amd import _lib, morphology, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

T = ops.OUTLINES_TILE
JUNK = 0x5A


def _rings(mask, table, n, cap, junk=JUNK):
    """ribca_mask_rings itself on junk-filled outputs and a junk-filled workspace of exactly the size the query asks for"""
    dev = _lib.require_gpu()
    mask = np.ascontiguousarray(mask, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.int32)
    md, td = torch.from_numpy(mask).to(dev), torch.from_numpy(table).to(dev)
    h, w = mask.shape
    rings = torch.full((cap, 6), junk, dtype=torch.int64, device=dev)
    total = torch.full((1,), junk, dtype=torch.int64, device=dev)
    ws = torch.full((ops.mask_rings_ws_bytes(h, w, n),), junk, dtype=torch.uint8, device=dev)
    assert ws.numel() > 0
    status = lib().ribca_mask_rings(ptr(md), h, w, ptr(td), len(table), n, cap, ptr(rings), ptr(total), ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    assert np.array_equal(md.cpu().numpy(), mask) and np.array_equal(td.cpu().numpy(), table)      # the inputs are read only
    return rings.cpu().numpy(), int(total.item())


def _vertices(mask, table, n, rings, first, junk=JUNK):
    """ribca_mask_ring_vertices itself on junk-filled outputs"""
    dev = _lib.require_gpu()
    mask = np.ascontiguousarray(mask, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.int32)
    md, td = torch.from_numpy(mask).to(dev), torch.from_numpy(table).to(dev)
    rows = np.ascontiguousarray(rings, dtype=np.int64).reshape(-1, 6)
    rd = torch.from_numpy(rows if len(rows) else np.full((1, 6), junk, dtype=np.int64)).to(dev)      # R = 0: a row nobody reads, a pointer to pass
    fd =torch.from_numpy(np.ascontiguousarray(first, dtype=np.int64)).to(dev)
    h, w = mask.shape
    out = torch.full((max(int(first[-1]), 1), 2), junk, dtype=torch.int32, device=dev)      # one junk row where there is no vertex: a pointer to pass
    bad = torch.full((1,), junk, dtype=torch.int32, device=dev)
    status = lib().ribca_mask_ring_vertices(ptr(md), h, w, ptr(td), len(table), n, ptr(rd), len(rings), ptr(fd), ptr(out), ptr(bad), stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    assert np.array_equal(md.cpu().numpy(), mask) and np.array_equal(rd.cpu().numpy()[:len(rows)], rows)
    return out.cpu().numpy()[:int(first[-1])], int(bad.item())


def _sorted(rows):
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


def _equal_to_the_restatement(mask, table=None, n=None):
    """both entry points against the restatement, byte for byte; returns (rings, first, vertices) of the GPU"""
    if table is None:
        table, ids = ON.label_table(mask)
        n = len(ids)
    want_rings, want_first, want_vertices = ON.trace(mask, table, n)
    cap = len(want_rings) + 3
    rows, total = _rings(mask, table, n, cap)
    assert total == len(want_rings), (mask.shape, total, len(want_rings))
    assert (rows[total:] == -1).all()                                   # the unused rows
    got = _sorted(rows[:total])
    assert got.dtype == np.int64 and got.tobytes() == want_rings.tobytes(), (mask.shape, np.argwhere(got != want_rings)[:5].tolist())
    vertices, bad = _vertices(mask, table, n, got, want_first)
    assert bad == 0
    assert vertices.dtype == np.int32 and vertices.tobytes() == want_vertices.tobytes(), mask.shape
    h, w = mask.shape
    assert np.array_equal(ON.rasterise(got, want_first, vertices, h, w), ON.owners(mask, table, n))
    return got, want_first, vertices


def _agrees_with_morphology(mask, rings):
    """per cell: the sum of area2 is twice the area, the sum of edges is columns 6 + 7 + 8 of ribca_mask_morphology, and exterior rings minus
    holes is the Euler number morphology.features reports"""
    dev = _lib.require_gpu()
    table, ids = ON.label_table(mask)
    got = ops.mask_morphology(torch.from_numpy(np.ascontiguousarray(mask, dtype=np.int32)).to(dev), ids)
    n = len(ids)
    area2 = np.bincount(rings[:, 0], weights=rings[:, 4], minlength=n).astype(np.int64)
    edges = np.bincount(rings[:, 0], weights=rings[:, 3], minlength=n).astype(np.int64)
    euler = np.bincount(rings[:, 0], weights=np.sign(rings[:, 4]), minlength=n).astype(np.int64)
    sums = got["sums"]
    assert np.array_equal(area2, 2 * sums[:, 0]) and np.array_equal(edges, sums[:, 6] + sums[:, 7] + sums[:, 8])
    assert np.array_equal(euler, morphology.features(sums, got["bbox"])["euler"].astype(np.int64))


@pytest.fixture(scope="module")
def discs():
    assert T == 32
    mask = ON.seam_discs()
    assert mask.shape == (67, 131) and mask[0].any() and mask[-1].any() and mask[:, 0].any() and mask[:, -1].any()
    return mask


@pytest.fixture(scope="module")
def disc_result(discs):
    return _equal_to_the_restatement(discs)


def test_damaged_discs_across_tile_seams_and_image_borders(discs, disc_result):
    rings, first, vertices = disc_result
    assert len(rings) > 45 and (rings[:, 4] < 0).any() and (rings[:, 5] > 0).any()      # holes and saddles are there
    assert len(np.unique(rings[:, 0])) < len(rings[rings[:, 4] > 0])                     # and a label in several blobs
    _agrees_with_morphology(discs, rings)


@pytest.fixture(scope="module")
def special():
    return {name: (m,) + _equal_to_the_restatement(m) for name, m in ON.special_masks(T).items()}


def test_the_special_shapes(special):
    counts = {name: (len(r), int(f[-1])) for name, (m, r, f, v) in special.items()}
    assert counts == {"diagonal_down": (1, 8), "diagonal_up": (1, 8), "diagonal_ring": (2, 16), "side_by_side": (2, 8), "two_blobs": (2, 8),
                      "serpentine": (1, 194), "channel": (48, 192), "comb": (1, 132), "near_int32_max": (3, 12), "negative": (11, 188)}
    for name, (m, r, f, v) in special.items():
        _agrees_with_morphology(m, r)
    m, r, f, v = special["diagonal_ring"]
    assert r[:, 5].tolist() == [4, 4] and (r[:, 4] > 0).tolist() == [True, False]      # one exterior, one hole, joined at four saddles
    m, r, f, v = special["diagonal_down"]
    assert r[0].tolist() == [0, (T - 1) * (2 * T + 1) + T - 1, 8, 8, 4, 2]              # two pixels that touch at a corner are one ring


@pytest.mark.parametrize("name", sorted(ON.small_masks()))
def test_thin_tiny_and_uniform_masks_the_checkerboard_and_the_nested_ring(name):
    mask = ON.small_masks()[name]
    rings, first, vertices = _equal_to_the_restatement(mask)
    want = {"row": (3, 12), "column": (3, 12), "pixel": (1, 4), "lone": (1, 4), "uniform": (1, 4), "background": (0, 0), "checkerboard": (19, 128),
            "nested": (3, 12)}[name]
    assert (len(rings), int(first[-1])) == want
    if name == "lone":
        assert rings[0].tolist() == [0, 32 * 34 + 32, 4, 4, 2, 0] and vertices.tolist() == [[32, 32], [32, 33], [33, 33], [33, 32]]
    if name != "background":
        _agrees_with_morphology(mask, rings)


def test_labels_that_are_no_cell_and_two_labels_that_are_one(discs):
    ids = np.unique(discs[discs > 0])
    mask = discs.copy()
    mask[40:44, 3:9] = -7                                  # negative pixels
    mask[50:53, 20:24] = int(ids.max()) + 5                # a label at or above L
    table, _ = ON.label_table(discs)
    n = len(ids)
    table[ids[3]] = -1                                     # an unmapped label
    table[ids[5]] = n + 2                                  # an entry that names no cell
    table[ids[7]] = table[ids[8]]                          # two labels, ONE cell
    table[ids[10]] = table[ids[30]]
    rings, first, vertices = _equal_to_the_restatement(mask, table, n)
    cells = set(rings[:, 0].tolist())
    assert 3 not in cells and 5 not in cells and 7 not in cells and 10 not in cells and 8 in cells and 30 in cells
    own = ON.owners(mask, table, n)
    assert (own[np.isin(mask, ids[[7, 8]])] == 8).all() and (own[mask < 0] == -1).all() and (own[mask > ids.max()] == -1).all()


def test_the_cap_protocol(discs, disc_result):
    dev = _lib.require_gpu()
    table, ids = ON.label_table(discs)
    want = disc_result[0]
    rows, total = _rings(discs, table, len(ids), 1)
    assert total == len(want) > 1                          # status 0, the exact total, rows undefined
    rows, total = _rings(discs, table, len(ids), len(want))
    assert total == len(want) and _sorted(rows).tobytes() == want.tobytes()      # a cap that just fits
    rows, total = _rings(discs, table, len(ids), len(want) + 40, junk=0x33)
    assert (rows[total:] == -1).all() and _sorted(rows[:total]).tobytes() == want.tobytes()
    md = torch.from_numpy(discs).to(dev)
    got = ops.mask_rings(md, ids, first_cap=1)
    assert got["calls"] == 2
    once = ops.mask_rings(md, ids)
    assert once["calls"] == 1
    for g in (got, once):
        assert g["rings"].tobytes() == want.tobytes() and g["first"].tobytes() == disc_result[1].tobytes()
        assert g["vertices"].tobytes() == disc_result[2].tobytes()
    none = ops.mask_rings(torch.zeros((5, 9), dtype=torch.int32, device=dev), np.zeros(0, np.int64))
    assert none["calls"] == 0 and none["rings"].shape == (0, 6) and none["first"].tolist() == [0] and none["vertices"].shape == (0, 2)
    for bad in (md.to(torch.int64), md.cpu(), md.reshape(-1), discs):
        with pytest.raises(ValueError):
            ops.mask_rings(bad, ids)


def test_rows_that_do_not_fit_the_mask_count_as_bad_and_stay_in_their_range(discs, disc_result):
    rings, first, vertices = disc_result
    table, ids = ON.label_table(discs)
    n = len(ids)
    order = np.random.RandomState(5).permutation(len(rings))      # any order the caller chose
    shuffled = rings[order]
    sfirst = np.zeros(len(rings) + 1, dtype=np.int64)
    sfirst[1:] = np.cumsum(shuffled[:, 2])
    good, bad = _vertices(discs, table, n, shuffled, sfirst)
    assert bad == 0
    for k, o in enumerate(order):
        assert np.array_equal(good[sfirst[k]:sfirst[k + 1]], vertices[first[o]:first[o + 1]])
    rows = shuffled.copy()
    rows[4, 1] += 1                    # no ring of that cell starts one vertex to the right
    rows[9, 0] = (rows[9, 0] + 1) % n  # the start of another cell's ring
    rows[20, 2] += 2                   # the walk finds two vertices fewer than the row says
    rows[31, 2] -= 2 if rows[31, 2] > 4 else -4      # ... or more
    rows[40, 1] = -5                   # no vertex at all
    rfirst = np.zeros(len(rows) + 1, dtype=np.int64)
    rfirst[1:] = np.cumsum(rows[:, 2])
    got, bad = _vertices(discs, table, n, rows, rfirst)
    assert bad == 5
    wrong = {4, 9, 20, 31, 40}
    for k, o in enumerate(order):
        mine = got[rfirst[k]:rfirst[k + 1]]
        if k in wrong:
            assert (mine == -1).all() and len(mine) == rows[k, 2]
        else:
            assert np.array_equal(mine, vertices[first[o]:first[o + 1]])
    # ``first`` that does not match the rows' counts: reported in bad -- it lives on the device --, every range written is the row's own
    off = sfirst.copy()
    off[11:] += 1                      # row 10 has room for one vertex more than its count
    got, bad = _vertices(discs, table, n, shuffled, off)
    assert bad == 1 and (got[off[10]:off[11]] == -1).all()
    assert np.array_equal(got[:off[10]], good[:sfirst[10]]) and np.array_equal(got[off[11]:], good[sfirst[11]:])
    past = sfirst.copy()
    past[-2] = past[-1] + 3            # the last two rows have no range inside the buffer: counted, nothing written
    got, bad = _vertices(discs, table, n, shuffled, past)
    assert bad == 2 and (got[sfirst[-3]:] == JUNK).all() and np.array_equal(got[:sfirst[-3]], good[:sfirst[-3]])


def test_labels_at_or_above_the_table_own_nothing():
    mask = CN.special_masks(T)["near_int32_max"]
    assert mask.max() == 2 ** 31 - 1
    table = np.array([-1, 0, 1, 0, 1, 0, 1, 0], dtype=np.int32)
    rings, first, vertices = _equal_to_the_restatement(mask, table, 2)
    assert len(rings) == 0
    mask = mask.copy()
    mask[20:22, 5:8] = 6               # and a label inside the table among them
    rings, first, vertices = _equal_to_the_restatement(mask, table, 2)
    assert rings.tolist() == [[1, 20 * (mask.shape[1] + 1) + 5, 4, 10, 12, 0]]


def test_two_calls_give_equal_sets(special):
    mask, rings, first, vertices = special["channel"]
    table, ids = ON.label_table(mask)
    rows, total = _rings(mask, table, len(ids), 64, junk=0x33)
    assert _sorted(rows[:total]).tobytes() == rings.tobytes()


def test_refused_arguments_return_a_status_and_leave_the_process_alive(discs, disc_result):
    dev = _lib.require_gpu()
    table, ids = ON.label_table(discs)
    n, L = len(ids), len(table)
    rings, first, vertices = disc_result
    R = len(rings)
    md, td = torch.from_numpy(discs).to(dev), torch.from_numpy(table).to(dev)
    h, w = discs.shape
    rows = torch.full((R, 6), 0x11, dtype=torch.int64, device=dev)
    total = torch.full((1,), 0x11, dtype=torch.int64, device=dev)
    ws = torch.zeros(ops.mask_rings_ws_bytes(h, w, n), dtype=torch.uint8, device=dev)
    fd = torch.from_numpy(first).to(dev)
    out = torch.full((int(first[-1]), 2), 0x11, dtype=torch.int32, device=dev)
    bad = torch.full((1,), 0x11, dtype=torch.int32, device=dev)
    k, s = ws.numel(), stream_ptr()

    def refused(status, name):
        assert status != 0
        msg = lib().ribca_last_error()
        assert msg and name in msg, msg

    assert ops.mask_rings_ws_bytes(0, w, n) == 0 and ops.mask_rings_ws_bytes(h, w, -1) == 0 and ops.mask_rings_ws_bytes(h, w, 2 ** 21 + 1) == 0
    assert ops.mask_rings_ws_bytes(46340, 46340, n) == 0 and ops.mask_rings_ws_bytes(46339, 46339, n) > 0      # (H + 1)(W + 1) < 2^31
    f = lib().ribca_mask_rings
    name = b"ribca_mask_rings"
    refused(f(None, h, w, ptr(td), L, n, R, ptr(rows), ptr(total), ptr(ws), k, s), name)
    refused(f(ptr(md), h, w, None, L, n, R, ptr(rows), ptr(total), ptr(ws), k, s), name)
    refused(f(ptr(md), h, w, ptr(td), L, n, R, None, ptr(total), ptr(ws), k, s), name)
    refused(f(ptr(md), h, w, ptr(td), L, n, R, ptr(rows), None, ptr(ws), k, s), name)
    refused(f(ptr(md), h, w, ptr(td), L, n, R, ptr(rows), ptr(total), None, k, s), name)
    refused(f(ptr(md), h, w, ptr(td), L, n, R, ptr(rows), ptr(total), ptr(ws), k - 1, s), name)
    refused(f(ptr(md), 0, w, ptr(td), L, n, R, ptr(rows), ptr(total), ptr(ws), k, s), name)
    refused(f(ptr(md), 46340, 46340, ptr(td), L, n, R, ptr(rows), ptr(total), ptr(ws), k, s), name)
    refused(f(ptr(md), h, w, ptr(td), 0, n, R, ptr(rows), ptr(total), ptr(ws), k, s), name)
    refused(f(ptr(md), h, w, ptr(td), L, -1, R, ptr(rows), ptr(total), ptr(ws), k, s), name)
    refused(f(ptr(md), h, w, ptr(td), L, 2 ** 21 + 1, R, ptr(rows), ptr(total), ptr(ws), k, s), name)
    refused(f(ptr(md), h, w, ptr(td), L, n, 0, ptr(rows), ptr(total), ptr(ws), k, s), name)
    refused(f(ptr(md), h, w, ptr(td), L, n, R, ptr(rows), ptr(rows), ptr(ws), k, s), name)      # total inside rings
    g = lib().ribca_mask_ring_vertices
    name = b"ribca_mask_ring_vertices"
    rd = torch.from_numpy(rings).to(dev)
    refused(g(None, h, w, ptr(td), L, n, ptr(rd), R, ptr(fd), ptr(out), ptr(bad), s), name)
    refused(g(ptr(md), h, w, None, L, n, ptr(rd), R, ptr(fd), ptr(out), ptr(bad), s), name)
    refused(g(ptr(md), h, w, ptr(td), L, n, None, R, ptr(fd), ptr(out), ptr(bad), s), name)
    refused(g(ptr(md), h, w, ptr(td), L, n, ptr(rd), R, None, ptr(out), ptr(bad), s), name)
    refused(g(ptr(md), h, w, ptr(td), L, n, ptr(rd), R, ptr(fd), None, ptr(bad), s), name)
    refused(g(ptr(md), h, w, ptr(td), L, n, ptr(rd), R, ptr(fd), ptr(out), None, s), name)
    refused(g(ptr(md), h, 0, ptr(td), L, n, ptr(rd), R, ptr(fd), ptr(out), ptr(bad), s), name)
    refused(g(ptr(md), h, w, ptr(td), L, 2 ** 21 + 1, ptr(rd), R, ptr(fd), ptr(out), ptr(bad), s), name)
    refused(g(ptr(md), h, w, ptr(td), L, n, ptr(rd), -1, ptr(fd), ptr(out), ptr(bad), s), name)
    refused(g(ptr(md), h, w, ptr(td), L, n, ptr(rd), R, ptr(fd), ptr(fd), ptr(bad), s), name)      # vertices inside first
    torch.cuda.synchronize()
    assert (rows == 0x11).all() and (total == 0x11).all() and (out == 0x11).all() and (bad == 0x11).all()      # nothing was launched
    # n = 0 and R = 0: total and bad are set, nothing is walked
    assert f(ptr(md), h, w, ptr(td), L, 0, R, ptr(rows), ptr(total), ptr(ws), k, s) == 0
    assert g(ptr(md), h, w, ptr(td), L, n, ptr(rd), 0, ptr(fd), ptr(out), ptr(bad), s) == 0
    torch.cuda.synchronize()
    assert int(total.item()) == 0 and (rows == -1).all() and int(bad.item()) == 0 and (out == 0x11).all()
    assert f(ptr(md), h, w, ptr(td), L, n, R, ptr(rows), ptr(total), ptr(ws), k, s) == 0
    torch.cuda.synchronize()
    assert int(total.item()) == R and _sorted(rows.cpu().numpy()).tobytes() == rings.tobytes()
