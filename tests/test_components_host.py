"""Connected components without a GPU: the library's version, every refusal of the three entry points and of the workspace query -- a status
whose text names the entry point, raised before any HIP call, so host pointers do -- and the restatement tests/components_numpy.py against
scipy.ndimage.label: per label with the 3 x 3 structure, for ``mask <= 0`` with the cross, on damaged-disc masks and on the special shapes."""
import ctypes

import numpy as np
import pytest

import components_numpy as CN
from multiplexed_image_annotator_amd import _lib, ops

T = 32


def test_version():
    assert _lib.lib().ribca_version() >= 110
    assert ops.COMPONENTS_TILE == T


def test_every_refusal_names_its_entry_point_before_any_hip_call():
    lib = _lib.lib()
    h, w = 5, 7
    mask = np.zeros((h, w), dtype=np.int32)
    root = np.full((h, w), 0x11, dtype=np.int32)
    stats = np.full((h * w, 4), 0x11, dtype=np.int32)
    out = np.full((h, w), 0x11, dtype=np.int32)
    n = int(lib.ribca_mask_components_ws_bytes(h, w))
    assert n > 0
    ws = np.zeros(n, dtype=np.uint8)
    m, r, s, o, k = (a.ctypes.data for a in (mask, root, stats, out, ws))

    def refused(status, name):
        assert status != 0
        msg = lib.ribca_last_error()
        assert msg and name in msg, msg

    for bad in ((0, w), (h, 0), (-1, w), (h, -3), (65536, 32768), (2 ** 31 - 1, 2)):
        assert lib.ribca_mask_components_ws_bytes(*bad) == 0
        refused(lib.ribca_mask_components(m, bad[0], bad[1], r, s, k, n, None), b"ribca_mask_components")
        refused(lib.ribca_mask_relabel(r, m, bad[0], bad[1], o, None), b"ribca_mask_relabel")
    assert lib.ribca_mask_components_ws_bytes(46340, 46340) > 0      # H W < 2^31
    f = lib.ribca_mask_components
    refused(f(None, h, w, r, s, k, n, None), b"ribca_mask_components: NULL")
    refused(f(m, h, w, None, s, k, n, None), b"ribca_mask_components: NULL")
    refused(f(m, h, w, r, None, k, n, None), b"ribca_mask_components: NULL")
    refused(f(m, h, w, r, s, None, n, None), b"ribca_mask_components: NULL")
    refused(f(m, h, w, r, s, k, n - 1, None), b"ribca_mask_components: workspace too small")
    refused(f(m, h, w, r, s, k, 0, None), b"ribca_mask_components: workspace too small")
    refused(f(m, h, w, m, s, k, n, None), b"ribca_mask_components: mask, root, stats and ws must not overlap")
    refused(f(m, h, w, r, m, k, n, None), b"ribca_mask_components: mask, root")
    refused(f(m, h, w, s, s, k, n, None), b"ribca_mask_components: mask, root")
    refused(f(m, h, w, s + 4 * (h * w * 4 - 1), s, k, n, None), b"ribca_mask_components: mask, root")      # root begins in the last row of stats
    refused(f(m, h, w, r, s, r, n, None), b"ribca_mask_components: mask, root")
    refused(f(m, h, w, r, s, m + 4, n, None), b"ribca_mask_components: mask, root")
    g = lib.ribca_mask_relabel
    refused(g(None, m, h, w, o, None), b"ribca_mask_relabel: NULL")
    refused(g(r, None, h, w, o, None), b"ribca_mask_relabel: NULL")
    refused(g(r, m, h, w, None, None), b"ribca_mask_relabel: NULL")
    refused(g(o, m, h, w, o, None), b"ribca_mask_relabel: out must not overlap")
    refused(g(r, o + 4, h, w, o, None), b"ribca_mask_relabel: out must not overlap")
    assert (root == 0x11).all() and (stats == 0x11).all() and (out == 0x11).all() and not mask.any()
    assert isinstance(ctypes.c_void_p(m).value, int)


def _scipy_partition(mask):
    """every pixel -> (class, index of its component in scipy's labelling of that class)"""
    from scipy import ndimage
    part = np.zeros(mask.shape + (2,), dtype=np.int64)
    lab, n = ndimage.label(mask <= 0)      # the cross: 4-connectivity
    part[mask <= 0, 1] = lab[mask <= 0]
    for v in np.unique(mask[mask > 0]):
        lab, n = ndimage.label(mask == v, structure=np.ones((3, 3), dtype=int))
        part[mask == v, 0], part[mask == v, 1] = v, lab[mask == v]
    return part


def _same_partition(mask):
    root, stats = CN.components(mask)
    part = _scipy_partition(mask).reshape(-1, 2)
    flat = root.reshape(-1)
    names = {}
    for p, key in zip(flat.tolist(), map(tuple, part.tolist())):
        assert names.setdefault(key, p) == p      # one root per scipy component
    assert len(set(names.values())) == len(names)      # and one scipy component per root
    roots = np.flatnonzero(stats[:, 0] > 0)
    assert sorted(names.values()) == roots.tolist()
    for p in roots.tolist():
        members = np.flatnonzero(flat == p)
        assert members[0] == p and stats[p, 0] == len(members)      # named after its first pixel
    assert not stats[np.setdiff1d(np.arange(mask.size), roots)].any()
    return root, stats


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_the_restatement_against_scipy_on_damaged_discs(seed):
    mask = CN.damaged_discs(67, 131, 40, seed)
    root, stats = _same_partition(mask)
    ids = np.unique(mask[mask > 0])
    assert len(np.unique(root[mask > 0])) > len(ids)      # some label is torn
    # border, lo and hi by their definitions, over numpy shifts
    pad = np.pad(np.where(mask > 0, mask, 0).astype(np.int64), 1)
    cls = pad[1:-1, 1:-1]
    for p in np.flatnonzero(stats[:, 0] > 0).tolist():
        sel = root == p
        rr, cc = np.nonzero(sel)
        assert stats[p, 1] == int(rr.min() == 0 or cc.min() == 0 or rr.max() == mask.shape[0] - 1 or cc.max() == mask.shape[1] - 1)
        near = []
        for dr, dc in CN.N4:
            v = pad[1 + dr:pad.shape[0] - 1 + dr, 1 + dc:pad.shape[1] - 1 + dc][sel]
            near.append(v[(v > 0) & (v != cls[sel])])
        near = np.concatenate(near)
        assert stats[p, 2:].tolist() == ([int(near.min()), int(near.max())] if len(near) else [0, 0])


def test_the_restatement_against_scipy_on_the_special_masks():
    for name, mask in CN.special_masks(T).items():
        _same_partition(mask)
    _same_partition(np.zeros((3, 4), dtype=np.int32))
    _same_partition(np.full((3, 4), 9, dtype=np.int32))


def test_the_restatement_on_hand_written_cases():
    m = np.array([[1, 0, 1],
                  [0, 1, 0],
                  [2, 0, -3]], dtype=np.int32)
    root, stats = CN.components(m)
    assert root.tolist() == [[0, 1, 0], [3, 0, 5], [6, 5, 5]]      # label 1 joins over its diagonals, the background between does not
    assert stats[0].tolist() == [3, 1, 0, 0] and stats[1].tolist() == [1, 1, 1, 1] and stats[3].tolist() == [1, 1, 1, 2]
    assert stats[5].tolist() == [3, 1, 1, 2] and stats[6].tolist() == [1, 1, 0, 0]      # -3 is background like 0
    assert not stats[[2, 4, 7, 8]].any()
