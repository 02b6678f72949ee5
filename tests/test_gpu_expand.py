"""Label expansion on the GPU: ribca_expand_labels (csrc/expand.hip) against tests/expand_numpy.py for EQUALITY of the bytes of ``out`` and
``dist2``, outputs and workspace junk-filled to exactly the queried size before every call: masks that are no multiple of the pixel tile with
cells across every seam and on all four image borders at every halo width of the kernel, masks thinner than the halo, a reach longer than the
image, the copy-through tiles, labels near INT32_MAX, negative pixels, the tie rule, a label just within and just beyond the halo of the next
tile; then the properties that hold whatever the mask, and the refusals."""
import numpy as np
import pytest
import torch

import expand_numpy as EN
from multiplexed_image_annotator_amd import _lib, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
DISTANCES = (1, 2, 5, 8, 16, 32)


def _gpu(mask, d, junk=0x5A, want_dist2=True):
    """the entry point itself on junk-filled outputs and a junk-filled workspace of exactly the size the query asks for"""
    dev = _lib.require_gpu()
    md = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.int32)).to(dev)
    h, w = mask.shape
    out = torch.full((h, w), junk, dtype=torch.int32, device=dev)
    dist2 = torch.full((h, w), junk, dtype=torch.int32, device=dev) if want_dist2 else None
    ws = torch.full((ops.expand_labels_ws_bytes(h, w, d),), junk, dtype=torch.uint8, device=dev)
    assert ws.numel() > 0
    status = lib().ribca_expand_labels(ptr(md), h, w, d, ptr(out), ptr(dist2), ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert status == 0, lib().ribca_last_error()
    assert np.array_equal(md.cpu().numpy(), mask)      # the input is read only
    return out.cpu().numpy(), None if dist2 is None else dist2.cpu().numpy()


def _equal_to_the_restatement(mask, d):
    want = EN.expand(mask, d)
    out, dist2 = _gpu(mask, d)
    assert out.dtype == np.int32 and dist2.dtype == np.int32
    assert out.tobytes() == want[0].tobytes(), (mask.shape, d, "out", int((out != want[0]).sum()))
    assert dist2.tobytes() == want[1].tobytes(), (mask.shape, d, "dist2", int((dist2 != want[1]).sum()))
    return want


@pytest.fixture(scope="module")
def discs():
    """67 x 131: 3 x 5 tiles of 32 with ragged last ones; 40 discs, some cut by each of the four borders, and two bars across the seams"""
    mask = EN.random_discs(67, 131, 40, 11)
    mask[31:33, 40:60] = 41
    mask[5:20, 63:65] = 42
    mask[30:36, 128:131] = 43
    assert mask[0].any() and mask[-1].any() and mask[:, 0].any() and mask[:, -1].any()
    return mask


@pytest.fixture(scope="module")
def disc_results(discs):
    """the GPU result at every distance, once"""
    return {d: _gpu(discs, d) for d in DISTANCES}


@pytest.mark.parametrize("d", DISTANCES)
def test_random_discs_across_tile_seams_and_image_borders(discs, disc_results, d):
    want = EN.expand(discs, d)
    out, dist2 = disc_results[d]
    assert out.tobytes() == want[0].tobytes() and dist2.tobytes() == want[1].tobytes()
    assert ((want[0] > 0) & (discs <= 0)).any() and want[2].any()      # something grew, and some pixels were ties
    if d <= 5:
        assert (want[1] == -1).any()


@pytest.mark.parametrize("shape", [(1, 50), (50, 1), (33, 33)])
@pytest.mark.parametrize("d", [1, 3, 8, 32])
def test_masks_thinner_than_the_halo_and_one_past_the_tile(shape, d):
    h, w = shape
    if min(shape) == 1:
        mask = np.zeros(h * w, dtype=np.int32)
        mask[[3, 4, 20, 49]] = (5, 5, 2, 9)
        mask = mask.reshape(shape)
    else:
        mask = EN.random_discs(h, w, 9, 5, rmax=4.0)
        mask[32, 32] = 77      # alone in its tile
    _equal_to_the_restatement(mask, d)


def test_a_reach_longer_than_the_image():
    mask = np.zeros((9, 9), dtype=np.int32)
    mask[0, 0], mask[8, 8], mask[4, 5] = 4, 2, 9
    want = _equal_to_the_restatement(mask, 32)
    assert (want[0] > 0).all()


def test_an_empty_mask_comes_back_unchanged():
    mask = np.zeros((40, 70), dtype=np.int32)
    out, dist2 = _gpu(mask, 7)
    assert not out.any() and (dist2 == -1).all()
    mask[:] = -3
    out, dist2 = _gpu(mask, 7)
    assert (out == -3).all() and (dist2 == -1).all()


def test_a_mask_without_background():
    mask = (1 + np.arange(40 * 70) % 13).astype(np.int32).reshape(40, 70)
    out, dist2 = _gpu(mask, 4)
    assert np.array_equal(out, mask) and not dist2.any()
    _equal_to_the_restatement(mask, 4)


def test_labels_near_int32_max_and_sparse_label_sets():
    mask = np.zeros((20, 45), dtype=np.int32)
    mask[10, 5], mask[10, 11], mask[4, 30], mask[10, 17] = INT32_MAX, 3, 1_000_000, INT32_MAX - 1
    want = _equal_to_the_restatement(mask, 8)
    assert set(np.unique(want[0])) == {0, 3, 1_000_000, INT32_MAX - 1, INT32_MAX}
    assert want[0][10, 8] == 3 and want[0][10, 14] == 3 and want[2][10, 8]      # tied with INT32_MAX at distance 3: the smaller label


def test_negative_pixels_are_grown_over_within_reach_and_pass_through_beyond():
    mask = np.zeros((12, 40), dtype=np.int32)
    mask[6, 6] = 8
    mask[6, 8], mask[6, 30], mask[0, 0] = -5, -7, -2
    want = _equal_to_the_restatement(mask, 3)
    assert want[0][6, 8] == 8 and want[0][6, 30] == -7 and want[0][0, 0] == -2 and want[1][6, 30] == -1


def test_the_tie_goes_to_the_smaller_label_whichever_way_the_mask_is_flipped():
    mask = np.zeros((1, 5), dtype=np.int32)
    mask[0, 0], mask[0, 4] = 7, 3
    for m in (mask, mask[:, ::-1].copy(), mask.T.copy(), mask.T[::-1].copy()):
        out, dist2 = _gpu(m, 2)
        assert out.reshape(-1)[2] == 3 and dist2.reshape(-1)[2] == 4
        assert sorted(out.reshape(-1).tolist()) == [3, 3, 3, 7, 7]


@pytest.mark.parametrize("d", [2, 4, 5, 16, 32])
def test_a_label_at_the_edge_of_the_next_tile_s_halo(d):
    """the pixel (40, 40) belongs to the tile at (32, 32); a label d rows above it reaches it with dist2 = d d, a label d + 1 rows above does not,
    and the same along the row -- d = 5 runs in the kernel form with a halo of 8, whose staged square holds the label that is out of reach"""
    t = ops.EXPAND_TILE
    assert t == 32
    for axis in (0, 1):
        for gap, reached in ((d, True), (d + 1, False)):
            mask = np.zeros((3 * t, 3 * t), dtype=np.int32)
            at = [40, 40]
            at[axis] -= gap
            mask[at[0], at[1]] = 6
            out, dist2 = _gpu(mask, d)
            assert (out[40, 40], dist2[40, 40]) == ((6, d * d) if reached else (0, -1)), (d, axis, gap)
            want = EN.expand(mask, d)
            assert np.array_equal(out, want[0]) and np.array_equal(dist2, want[1])


def test_distance_one_is_the_four_neighbour_formula(discs):
    out, dist2 = _gpu(discs, 1)
    lab = np.where(discs > 0, discs, 0).astype(np.int64)
    pad = np.pad(lab, 1)
    shifts = np.stack([pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]])
    smallest = np.where(shifts > 0, shifts, np.int64(1) << 40).min(axis=0)
    grown = (discs <= 0) & (shifts > 0).any(axis=0)
    assert np.array_equal(out, np.where(grown, smallest, discs))
    assert np.array_equal(dist2, np.where(discs > 0, 0, np.where(grown, 1, -1)))


def test_properties_that_hold_for_every_mask(discs, disc_results):
    ids = np.unique(discs[discs > 0])
    for d in DISTANCES:
        out, dist2 = disc_results[d]
        assert np.array_equal(out[discs > 0], discs[discs > 0]) and not dist2[discs > 0].any()      # every labelled pixel is unchanged
        assert np.array_equal(np.unique(out[out > 0]), ids)                                         # no label made, none lost
        assert np.array_equal(dist2 >= 0, out > 0) and dist2.max() <= d * d
    for d1, d2 in zip(DISTANCES[:-1], DISTANCES[1:]):
        (o1, q1), (o2, q2) = disc_results[d1], disc_results[d2]
        assert not ((o1 > 0) & ~(o2 > 0)).any()
        near = (q2 >= 0) & (q2 <= d1 * d1)
        assert np.array_equal(q1[near], q2[near]) and np.array_equal(o1[near], o2[near]) and np.array_equal(q1 >= 0, near)


def test_two_calls_give_equal_bytes_and_dist2_is_optional(discs, disc_results):
    for d in (2, 32):
        again = _gpu(discs, d, junk=0x33)
        assert again[0].tobytes() == disc_results[d][0].tobytes() and again[1].tobytes() == disc_results[d][1].tobytes()
        assert _gpu(discs, d, want_dist2=False)[0].tobytes() == disc_results[d][0].tobytes()


def test_the_wrapper(discs, disc_results):
    dev = _lib.require_gpu()
    md = torch.from_numpy(discs).to(dev)
    out = ops.expand_labels(md, 5)
    assert out.is_cuda and out.dtype == torch.int32 and out.data_ptr() != md.data_ptr()
    assert np.array_equal(out.cpu().numpy(), disc_results[5][0])
    out, dist2 = ops.expand_labels(md, np.int64(5), want_dist2=True)
    assert np.array_equal(out.cpu().numpy(), disc_results[5][0]) and np.array_equal(dist2.cpu().numpy(), disc_results[5][1])
    assert ops.EXPAND_MAX_DISTANCE == 32
    for bad in (0, 33, -1, True, 2.0, "3", None):
        with pytest.raises(ValueError):
            ops.expand_labels(md, bad)
    with pytest.raises(ValueError):
        ops.expand_labels(md.to(torch.int64), 3)


def test_refused_arguments_return_a_status_and_leave_the_process_alive(discs):
    dev = _lib.require_gpu()
    md = torch.from_numpy(discs).to(dev)
    h, w = discs.shape
    out = torch.full((h, w), 0x11, dtype=torch.int32, device=dev)
    ws = torch.zeros(max(ops.expand_labels_ws_bytes(h, w, 3), 1), dtype=torch.uint8, device=dev)

    def refused(status):
        assert status != 0
        msg = lib().ribca_last_error()
        assert msg and b"ribca_expand_labels" in msg, msg

    assert ops.expand_labels_ws_bytes(h, w, 0) == 0 and ops.expand_labels_ws_bytes(h, w, 33) == 0 and ops.expand_labels_ws_bytes(0, w, 3) == 0
    assert ops.expand_labels_ws_bytes(65536, 65536, 3) == 0
    refused(lib().ribca_expand_labels(ptr(md), h, w, 0, ptr(out), None, ptr(ws), ws.numel(), stream_ptr()))
    refused(lib().ribca_expand_labels(ptr(md), h, w, 33, ptr(out), None, ptr(ws), ws.numel(), stream_ptr()))
    refused(lib().ribca_expand_labels(ptr(md), h, w, 3, ptr(md), None, ptr(ws), ws.numel(), stream_ptr()))
    refused(lib().ribca_expand_labels(ptr(md), h, w, 3, ptr(out), ptr(out), ptr(ws), ws.numel(), stream_ptr()))
    refused(lib().ribca_expand_labels(ptr(md), h, w, 3, ptr(out), None, None, ws.numel(), stream_ptr()))
    refused(lib().ribca_expand_labels(ptr(md), h, w, 3, ptr(out), None, ptr(ws), ws.numel() - 1, stream_ptr()))
    refused(lib().ribca_expand_labels(None, h, w, 3, ptr(out), None, ptr(ws), ws.numel(), stream_ptr()))
    torch.cuda.synchronize()
    assert (out == 0x11).all()      # nothing was launched
    assert lib().ribca_expand_labels(ptr(md), h, w, 3, ptr(out), None, ptr(ws), ws.numel(), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), EN.expand(discs, 3)[0])
