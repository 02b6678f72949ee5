"""Marker colocalisation on the GPU: ribca_cell_coloc (csrc/colocalization.hip) through ops.cell_coloc against tests/coloc_numpy.py for
EQUALITY of the bytes of all five outputs.  One 96 x 128 image of six channels -- random fp32 in [-1, 1], about 3 % of every channel exactly at
its gate, so the strict comparison is checked -- with, in ONE launch, ids that are no cell, an empty box, a box outside the image, cells of 1,
2, 255, 256 and 257 pixels, a solid box of exactly ops.INTENSITY_SMALL_BOX pixels and one of one pixel more, a box that leaves out part of its
label, a label in two blobs, a cell cut by the image border.  A second 128 x 160 image with labels of ops.COLOC_RESIDENT, one more and 9000
pixels: the kernel's only form boundary, resident against streaming.  Both at K = 2, K = 3 and K = 6 as a permutation that is not monotone;
K = 32 on a 32-channel image.  Then: sums and the diagonal of cross are ops.cell_intensities' sum and ssd; one cell per chunk gives the same
bytes; a second call gives the same bytes; ``out=`` tensors are overwritten, every byte."""
import numpy as np
import pytest
import torch

import coloc_numpy as CN
from multiplexed_image_annotator_amd import _lib, ops

pytestmark = pytest.mark.gpu

NAMES = ("area", "both", "sums", "cross", "gated")


def _case(which):
    if which == "small":
        mask, ids, bbox = CN.small_cells(ops.INTENSITY_SMALL_BOX)
        return CN.generated_image(6, 96, 128, 41), mask, ids, bbox
    mask, ids, bbox = CN.large_cells(ops.COLOC_RESIDENT)
    return CN.generated_image(6, 128, 160, 42), mask, ids, bbox


def _gates(chan):
    return np.array([CN.GATES[c % len(CN.GATES)] for c in chan], dtype=np.float32)


def _device(image, mask):
    dev = _lib.require_gpu()
    return torch.from_numpy(image).to(dev), torch.from_numpy(mask).to(dev)


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, np.argwhere(g != w)[:6].tolist())


@pytest.fixture(scope="module")
def results():
    """every (image, selection) once: (inputs, the kernel's outputs, the restatement's)"""
    out = {}
    for which in ("small", "large"):
        image, mask, ids, bbox = _case(which)
        image_d, mask_d = _device(image, mask)
        for chan in CN.SELECTIONS:
            thr = _gates(chan)
            out[which, chan] = ((image, mask, ids, bbox, image_d, mask_d, thr), ops.cell_coloc(image_d, mask_d, ids, bbox, chan, thr),
                                CN.coloc(image, mask, ids, bbox, chan, thr))
    return out


@pytest.mark.parametrize("chan", CN.SELECTIONS)
@pytest.mark.parametrize("which", ["small", "large"])
def test_all_five_outputs_are_the_restatement_s_bytes(results, which, chan):
    (image, mask, ids, bbox, *_), got, want = results[which, chan]
    _same(got, want, (which, chan))
    area = want[0]
    if which == "small":
        assert area.tolist() == [1024, 1025, 256, 255, 257, 1, 2, 8 * 14, 6 * 8 + 7 * 10, 30, 80, 0, 0, 0, 0]
        assert not any(x[area == 0].any() for x in got)      # zeros everywhere for a cell without a pixel
        k = len(chan)
        diag = [j for j, (a, b) in enumerate(CN.pairs(k)) if a == b]
        at_gate = sum(int(((image[c] == t) & (mask > 0)).sum()) for c, t in zip(chan, _gates(chan)))
        assert at_gate > 20      # pixels exactly at their gate inside cells: a comparison that is not strict would count them
        assert (want[1][:, diag] <= area[:, None]).all() and (want[1][area > 100][:, diag] > 0).all()
    else:
        assert area.tolist() == [ops.COLOC_RESIDENT, ops.COLOC_RESIDENT + 1, 9000]


def test_k_32_on_a_32_channel_image():
    mask, ids, bbox = CN.wide_cells()
    image = CN.generated_image(32, 40, 40, 43)
    rng = np.random.default_rng(7)
    chan = rng.permutation(32).tolist()
    thr = _gates(chan)
    image_d, mask_d = _device(image, mask)
    got = ops.cell_coloc(image_d, mask_d, ids, bbox, chan, thr)
    want = CN.coloc(image, mask, ids, bbox, chan, thr)
    assert want[0].tolist() == [170, 550, 12] and want[1].shape == (3, 528) and want[4].shape == (3, 32, 32)
    _same(got, want, "K = 32")


@pytest.mark.parametrize("which", ["small", "large"])
def test_sums_and_the_diagonal_of_cross_are_cell_intensities_sum_and_ssd(results, which):
    chan = CN.SELECTIONS[2]
    (image, mask, ids, bbox, image_d, mask_d, thr), got, _ = results[which, chan]
    area, sums, _ = ops.cell_intensities(image_d, mask_d, ids, bbox)
    diag = [j for j, (a, b) in enumerate(CN.pairs(len(chan))) if a == b]
    assert got[0].tobytes() == area.tobytes()
    assert got[2].tobytes() == np.ascontiguousarray(sums[:, list(chan), 0]).tobytes()
    assert np.ascontiguousarray(got[3][:, diag]).tobytes() == np.ascontiguousarray(sums[:, list(chan), 1]).tobytes()


def test_a_constant_channel_gives_cross_of_exactly_zero_in_its_row_and_column():
    image, mask, ids, bbox = _case("small")
    image = image.copy()
    image[2] = np.float32(0.3)      # not a dyadic value: its sum over a pixels is exact in fp64 all the same
    image_d, mask_d = _device(image, mask)
    chan = (0, 2, 5)
    got = ops.cell_coloc(image_d, mask_d, ids, bbox, chan, _gates(chan))
    _same(got, CN.coloc(image, mask, ids, bbox, chan, _gates(chan)), "constant")
    with_2 = [j for j, (a, b) in enumerate(CN.pairs(3)) if 1 in (a, b)]
    assert not got[3][:, with_2].any() and got[3][got[0] > 2][:, [0, 5]].all()


@pytest.mark.parametrize("which", ["small", "large"])
def test_one_cell_per_chunk_and_a_second_call_give_the_same_bytes(results, which, monkeypatch):
    chan = CN.SELECTIONS[1]
    (image, mask, ids, bbox, image_d, mask_d, thr), got, _ = results[which, chan]
    _same(ops.cell_coloc(image_d, mask_d, ids, bbox, chan, thr), got, "second call")
    monkeypatch.setattr(ops, "COLOC_CHUNK_BYTES", 1)
    _same(ops.cell_coloc(image_d, mask_d, ids, bbox, chan, thr), got, "one cell per chunk")
    dev = image_d.device
    k, n = len(chan), len(ids)
    p = k * (k + 1) // 2
    out = (torch.full((n,), -1, dtype=torch.int32, device=dev), torch.full((n, p), -1, dtype=torch.int32, device=dev),
           torch.full((n, k), float("nan"), dtype=torch.float64, device=dev), torch.full((n, p), float("nan"), dtype=torch.float64, device=dev),
           torch.full((n, k, k), float("nan"), dtype=torch.float64, device=dev))
    assert ops.cell_coloc(image_d, mask_d, ids, bbox, chan, thr, out=out) is out      # chunked into the caller's tensors
    _same([x.cpu().numpy() for x in out], got, "out=, one cell per chunk")


def test_out_tensors_are_overwritten_every_byte(results):
    chan = CN.SELECTIONS[2]
    (image, mask, ids, bbox, image_d, mask_d, thr), got, _ = results["small", chan]
    dev = image_d.device
    k, n = len(chan), len(ids)
    p = k * (k + 1) // 2
    ids_d, bbox_d = torch.from_numpy(ids).to(dev), torch.from_numpy(bbox).to(dev)      # device tables, as ImageProcessor keeps them
    for poison in (0x5A, 0xFF):
        out = tuple(torch.full((size,), poison, dtype=torch.uint8, device=dev).view(dtype).view(shape)
                    for size, dtype, shape in ((4 * n, torch.int32, (n,)), (4 * n * p, torch.int32, (n, p)), (8 * n * k, torch.float64, (n, k)),
                                               (8 * n * p, torch.float64, (n, p)), (8 * n * k * k, torch.float64, (n, k, k))))
        back = ops.cell_coloc(image_d, mask_d, ids_d, bbox_d, chan, thr, out=out)
        assert all(b is o for b, o in zip(back, out))
        _same([x.cpu().numpy() for x in out], got, ("out=", poison))


def test_no_cells_and_wrong_arguments():
    image, mask, ids, bbox = _case("small")
    image_d, mask_d = _device(image, mask)
    empty = ops.cell_coloc(image_d, mask_d, ids[:0], bbox[:0], (0, 1), (0.0, 0.0))
    assert [x.shape for x in empty] == [(0,), (0, 3), (0, 2), (0, 3), (0, 2, 2)]
    with pytest.raises(ValueError, match="one gate per selected channel"):
        ops.cell_coloc(image_d, mask_d, ids, bbox, (0, 1), (0.0,))
    with pytest.raises(ValueError, match="one box"):
        ops.cell_coloc(image_d, mask_d, ids, bbox[:3], (0, 1), (0.0, 0.0))
    for chan, thr, text in (((0,), (0.0,), "2 <= K <= 32"), ((0, 0), (0.0, 0.0), "twice"), ((0, 6), (0.0, 0.0), "chan"),
                            ((0, 1), (0.0, float("nan")), "finite")):
        with pytest.raises(RuntimeError, match="ribca_cell_coloc") as err:
            ops.cell_coloc(image_d, mask_d, ids, bbox, chan, thr)
        assert text in str(err.value)
