"""Connected components on the GPU: ribca_mask_components (csrc/components.hip) against tests/components_numpy.py for EQUALITY of the bytes of
``root`` and ``stats``, outputs and workspace junk-filled to exactly the queried size before every call and the input unchanged after it: a
mask that is no multiple of the pixel tile with discs, bars across every seam and cells on all four borders, thin and tiny masks, uniform
masks, the shapes whose components can be stated in words (diagonal contacts across a tile corner, a background pixel inside a diagonal ring,
neighbouring labels, one label in two blobs, a serpentine and a channel through 3 x 3 tiles, a comb), labels next to INT32_MAX, negative
pixels; then ribca_mask_relabel, ops.repair_labels against the restated repair, and the refusals."""
import numpy as np
import pytest
import torch

import components_numpy as CN
import expand_numpy as EN
from multiplexed_image_annotator_amd import _lib, ops, repair
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
T = ops.COMPONENTS_TILE


def _gpu(mask, junk=0x5A):
    """the entry point itself on junk-filled outputs and a junk-filled workspace of exactly the size the query asks for"""
    dev = _lib.require_gpu()
    mask = np.ascontiguousarray(mask, dtype=np.int32)
    md = torch.from_numpy(mask).to(dev)
    h, w = mask.shape
    root = torch.full((h, w), junk, dtype=torch.int32, device=dev)
    stats = torch.full((h * w, 4), junk, dtype=torch.int32, device=dev)
    ws = torch.full((ops.mask_components_ws_bytes(h, w),), junk, dtype=torch.uint8, device=dev)
    assert ws.numel() > 0
    status = lib().ribca_mask_components(ptr(md), h, w, ptr(root), ptr(stats), ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    assert np.array_equal(md.cpu().numpy(), mask)      # the input is read only
    return root.cpu().numpy(), stats.cpu().numpy()


def _equal_to_the_restatement(mask):
    want_root, want_stats = CN.components(mask)
    root, stats = _gpu(mask)
    assert root.dtype == np.int32 and stats.dtype == np.int32 and stats.shape == (mask.size, 4)
    assert root.tobytes() == want_root.tobytes(), (mask.shape, "root", int((root != want_root).sum()))
    assert stats.tobytes() == want_stats.tobytes(), (mask.shape, "stats", np.argwhere(stats != want_stats)[:5].tolist())
    return root, stats


@pytest.fixture(scope="module")
def discs():
    """67 x 131: 3 x 5 tiles of 32 with ragged last ones; damaged discs, some cut by each of the four borders, and bars across every seam"""
    assert T == 32
    mask = CN.damaged_discs(67, 131, 40, 11)
    mask[31:33, 40:60] = 41
    mask[5:20, 63:65] = 42
    mask[30:36, 128:131] = 43
    mask[63:66, 10:120] = 44      # across the four vertical seams
    mask[2:66, 95:98] = 45        # across the two horizontal seams
    assert mask[0].any() and mask[-1].any() and mask[:, 0].any() and mask[:, -1].any()
    return mask


@pytest.fixture(scope="module")
def disc_result(discs):
    return _gpu(discs)


def test_damaged_discs_across_tile_seams_and_image_borders(discs, disc_result):
    want_root, want_stats = CN.components(discs)
    root, stats = disc_result
    assert root.tobytes() == want_root.tobytes() and stats.tobytes() == want_stats.tobytes()
    roots = np.flatnonzero(stats[:, 0] > 0)
    assert stats[:, 0].sum() == discs.size and len(roots) > 40 and (stats[roots, 1] == 0).any() and (stats[roots, 2] != stats[roots, 3]).any()
    assert np.array_equal(np.unique(root), roots) and (root.reshape(-1)[roots] == roots).all()      # a partition whose names are first pixels


@pytest.mark.parametrize("shape", [(1, 50), (50, 1), (33, 33), (1, 1)])
def test_thin_masks_one_past_the_tile_and_one_pixel(shape):
    h, w = shape
    if min(shape) == 1:
        mask = np.zeros(50, dtype=np.int32)
        mask[[3, 4, 20, 49]] = (5, 5, 2, 5)
        mask = mask[-h * w:].reshape(shape)      # (1, 1): the last pixel alone, a label
    else:
        mask = EN.random_discs(h, w, 9, 5, rmax=4.0)
        mask[32, 32] = 77      # alone in its tile
    _equal_to_the_restatement(mask)


def test_uniform_masks():
    root, stats = _equal_to_the_restatement(np.zeros((40, 70), dtype=np.int32))
    assert not root.any() and stats[0].tolist() == [2800, 1, 0, 0] and not stats[1:].any()
    root, stats = _equal_to_the_restatement(np.full((40, 70), 9, dtype=np.int32))
    assert not root.any() and stats[0].tolist() == [2800, 1, 0, 0] and not stats[1:].any()
    root, stats = _equal_to_the_restatement(np.full((1, 1), -8, dtype=np.int32))
    assert root.tolist() == [[0]] and stats.tolist() == [[1, 1, 0, 0]]


@pytest.fixture(scope="module")
def special():
    masks = CN.special_masks(T)
    return {name: (m,) + _equal_to_the_restatement(m) for name, m in masks.items()}


def test_a_diagonal_contact_across_a_tile_corner_joins_foreground(special):
    for name, first in (("diagonal_down", (T - 1) * 2 * T + T - 1), ("diagonal_up", (T - 1) * 2 * T + T)):
        mask, root, stats = special[name]
        assert sorted(np.unique(root[mask == 5]).tolist()) == [first] and stats[first].tolist() == [2, 0, 0, 0]
        assert stats[0].tolist() == [mask.size - 2, 1, 5, 5]      # and the background around it is one component


def test_a_background_pixel_inside_a_diagonal_ring_does_not_leak(special):
    mask, root, stats = special["diagonal_ring"]
    p = T * 2 * T + T
    assert root[T, T] == p and stats[p].tolist() == [1, 0, 7, 7]
    assert len(np.unique(root[mask == 7])) == 1 and len(np.unique(root)) == 3


def test_neighbouring_labels_stay_apart_and_distant_blobs_stay_two(special):
    mask, root, stats = special["side_by_side"]
    a, b = root[4, T - 6], root[4, T]
    assert a != b and stats[a].tolist() == [48, 0, 9, 9] and stats[b].tolist() == [48, 0, 2, 2] and stats[0].tolist()[2:] == [2, 9]
    mask, root, stats = special["two_blobs"]
    assert len(np.unique(root[mask == 4])) == 2 and len(np.unique(root)) == 3


def test_long_chains_through_three_by_three_tiles(special):
    for name, value in (("serpentine", 6), ("channel", 0)):
        mask, root, stats = special[name]
        sel = mask == value
        assert len(np.unique(root[sel])) == 1 and root[sel][0] == 0 and stats[0, 0] == sel.sum() > 4 * 3 * T
    mask, root, stats = special["channel"]
    assert len(np.unique(root[mask == 6])) == 3 * T // 2      # the walls between the turns of the channel touch only diagonally: one each
    mask, root, stats = special["comb"]
    assert len(np.unique(root[mask == 3])) == 1 and root[0, 1] == 1 and root[0, 3 * T - 2] == 1


def test_labels_next_to_int32_max_and_negative_pixels(special):
    mask, root, stats = special["near_int32_max"]
    a, b = root[3, 3], root[3, 9]
    assert a != b and stats[a].tolist()[2:] == [INT32_MAX - 1, INT32_MAX - 1] and stats[b].tolist()[2:] == [INT32_MAX, INT32_MAX]
    assert len(np.unique(root[mask == INT32_MAX])) == 2 and stats[0].tolist()[2:] == [INT32_MAX - 1, INT32_MAX]
    mask, root, stats = special["negative"]
    zeroed = np.where(mask > 0, mask, 0).astype(np.int32)
    assert (mask < 0).sum() > 50 and mask[0, 0] == -(2 ** 31)
    again = _gpu(zeroed)
    assert again[0].tobytes() == root.tobytes() and again[1].tobytes() == stats.tobytes()      # negative is background, nothing else


def test_two_calls_give_equal_bytes(discs, disc_result, special):
    again = _gpu(discs, junk=0x33)
    assert again[0].tobytes() == disc_result[0].tobytes() and again[1].tobytes() == disc_result[1].tobytes()
    mask, root, stats = special["serpentine"]
    again = _gpu(mask, junk=0x33)
    assert again[0].tobytes() == root.tobytes() and again[1].tobytes() == stats.tobytes()


def test_relabel_and_the_wrappers(discs, disc_result):
    dev = _lib.require_gpu()
    md = torch.from_numpy(discs).to(dev)
    root, stats = ops.mask_components(md)
    assert root.is_cuda and root.dtype == torch.int32 and stats.shape == (discs.size, 4)
    assert np.array_equal(root.cpu().numpy(), disc_result[0]) and np.array_equal(stats.cpu().numpy(), disc_result[1])
    table = np.random.RandomState(3).randint(-5, INT32_MAX, discs.size).astype(np.int32)
    out = ops.relabel(root, torch.from_numpy(table).to(dev))
    assert out.dtype == torch.int32 and out.data_ptr() != root.data_ptr()
    assert np.array_equal(out.cpu().numpy(), table[disc_result[0]])
    assert np.array_equal(ops.relabel(root, md.reshape(-1)).cpu().numpy(), discs)      # every component takes the value at its first pixel
    for bad in (md.to(torch.int64), md.cpu(), md.reshape(-1), discs):
        with pytest.raises(ValueError):
            ops.mask_components(bad)
    with pytest.raises(ValueError):
        ops.relabel(root, torch.zeros(discs.size - 1, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("min_area", [1, 3, 10])
def test_repair_labels_is_the_restated_repair(discs, min_area):
    dev = _lib.require_gpu()
    want, text, counts = CN.repair(discs, min_area)
    out, rows, record = ops.repair_labels(torch.from_numpy(discs).to(dev), min_area)
    assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), want)
    assert repair.cells_csv(rows) == text
    assert {k: v for k, v in record.items() if k != "repair_ms"} == counts
    assert counts["components_split"] > 0 and counts["holes_filled"] > 0
    again, rows2, record2 = ops.repair_labels(out, min_area)
    assert torch.equal(again, out) and record2["components_split"] == record2["components_dropped"] == record2["holes_filled"] == 0


def test_a_binary_mask_comes_out_as_an_instance_labelling():
    dev = _lib.require_gpu()
    mask = np.zeros((40, 70), dtype=np.int32)
    mask[2:6, 2:6], mask[10:30, 20:50], mask[35:38, 60:66] = 255, 255, 255
    out, rows, record = ops.repair_labels(torch.from_numpy(mask).to(dev), 1)
    out = out.cpu().numpy()
    assert out[2, 2] == 256 and out[10, 20] == 255 and out[35, 60] == 257 and np.array_equal(out > 0, mask > 0)
    assert record["labels_in"] == 1 and record["labels_out"] == 3


def test_refused_arguments_return_a_status_and_leave_the_process_alive(discs, disc_result):
    dev = _lib.require_gpu()
    md = torch.from_numpy(discs).to(dev)
    h, w = discs.shape
    root = torch.full((h, w), 0x11, dtype=torch.int32, device=dev)
    stats = torch.full((h * w, 4), 0x11, dtype=torch.int32, device=dev)
    out = torch.full((h, w), 0x11, dtype=torch.int32, device=dev)
    ws = torch.zeros(ops.mask_components_ws_bytes(h, w), dtype=torch.uint8, device=dev)
    n, s = ws.numel(), stream_ptr()

    def refused(status, name):
        assert status != 0
        msg = lib().ribca_last_error()
        assert msg and name in msg, msg

    f = lib().ribca_mask_components
    assert ops.mask_components_ws_bytes(0, w) == 0 and ops.mask_components_ws_bytes(h, -1) == 0 and ops.mask_components_ws_bytes(65536, 32768) == 0
    refused(f(None, h, w, ptr(root), ptr(stats), ptr(ws), n, s), b"ribca_mask_components")
    refused(f(ptr(md), h, w, None, ptr(stats), ptr(ws), n, s), b"ribca_mask_components")
    refused(f(ptr(md), h, w, ptr(root), None, ptr(ws), n, s), b"ribca_mask_components")
    refused(f(ptr(md), h, w, ptr(root), ptr(stats), None, n, s), b"ribca_mask_components")
    refused(f(ptr(md), 0, w, ptr(root), ptr(stats), ptr(ws), n, s), b"ribca_mask_components")
    refused(f(ptr(md), 65536, 32768, ptr(root), ptr(stats), ptr(ws), n, s), b"ribca_mask_components")
    refused(f(ptr(md), h, w, ptr(md), ptr(stats), ptr(ws), n, s), b"ribca_mask_components")
    refused(f(ptr(md), h, w, ptr(root), ptr(stats), ptr(stats), n, s), b"ribca_mask_components")
    refused(f(ptr(md), h, w, ptr(stats), ptr(stats), ptr(ws), n, s), b"ribca_mask_components")
    refused(f(ptr(md), h, w, ptr(root), ptr(stats), ptr(ws), n - 1, s), b"ribca_mask_components")
    g = lib().ribca_mask_relabel
    refused(g(None, ptr(md), h, w, ptr(out), s), b"ribca_mask_relabel")
    refused(g(ptr(md), ptr(md), h, 0, ptr(out), s), b"ribca_mask_relabel")
    refused(g(ptr(out), ptr(md), h, w, ptr(out), s), b"ribca_mask_relabel")
    refused(g(ptr(md), ptr(out), h, w, ptr(out), s), b"ribca_mask_relabel")
    torch.cuda.synchronize()
    assert (root == 0x11).all() and (stats == 0x11).all() and (out == 0x11).all()      # nothing was launched
    assert f(ptr(md), h, w, ptr(root), ptr(stats), ptr(ws), n, s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(root.cpu().numpy(), disc_result[0])
