"""The permutation nulls share ONE sigma (csrc/ribca_perm.h, csrc/perm.hip): for the same (seed, image, p0, P) the neighbourhood null over a
neighbour list and the edge null over the same pairs written out as a directed edge list give the same counts, bit for bit.  Every other test
compares one null with its own numpy restatement; this one compares two of them with each other."""
import numpy as np
import pytest
import torch

from multiplexed_image_annotator_amd import _lib, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

P0, PERMS, IMAGE = 40, 3, 2
# (n, m, T, labels outside [0, T)): the smallest list there is; a ragged second block of 256 cells; lists as long as the analyses use
CASES = [(2, 1, 2, False), (257, 3, 3, False), (300, 24, 5, True)]


def _nhood_entry_point(idx, labels, t, seed):
    """ribca_nhood_perm_counts itself: the library skips a label outside [0, T), ops.nhood_perm_counts refuses it before any launch"""
    n, m = idx.shape
    td = torch.from_numpy(labels).to(idx.device)
    out = torch.zeros((PERMS, t, t), dtype=torch.int64, device=idx.device)
    ws = torch.empty(max(ops.nhood_perm_counts_ws_bytes(n, PERMS), 1), dtype=torch.uint8, device=idx.device)
    _lib.check(lib().ribca_nhood_perm_counts(ptr(idx), ptr(td), n, m, t, seed, IMAGE, P0, PERMS, ptr(out), ptr(ws), ws.numel(), stream_ptr()),
               "ribca_nhood_perm_counts")
    return out


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 0x1234567])
@pytest.mark.parametrize("n,m,t,stray", CASES)
def test_neighbour_null_and_edge_null_shuffle_alike(n, m, t, stray, seed):
    dev = _lib.require_gpu()
    rng = np.random.default_rng(n)
    idx_host = ((np.arange(n)[:, None] + rng.integers(1, n, (n, m))) % n).astype(np.int32)      # m other cells each, repeats allowed
    labels = rng.integers(0, t, n).astype(np.int32)
    if stray:
        labels[rng.permutation(n)[:40]] = rng.choice([-1, t, t + 7, 255, 2 ** 31 - 1], 40)
    idx = torch.from_numpy(idx_host).to(dev)
    src, dst = np.repeat(np.arange(n, dtype=np.int32), m), idx_host.reshape(-1)
    edge = ops.edge_perm_counts(src, dst, labels, t, seed, IMAGE, P0, PERMS, device=dev)
    nhood = _nhood_entry_point(idx, labels, t, seed)
    assert edge.dtype == torch.int64 and edge.shape == (PERMS, t, t) and torch.equal(nhood, edge)
    totals = edge.sum(dim=(1, 2)).tolist()
    if stray:
        assert all(0 < v < n * m for v in totals)      # pairs with a stray end are skipped, by both, under every permutation
    else:
        assert totals == [n * m] * PERMS
        assert torch.equal(ops.nhood_perm_counts(idx, labels, t, seed, IMAGE, P0, PERMS), edge)
    if n > 2:
        assert not torch.equal(edge[0], edge[1]) and not torch.equal(edge[1], edge[2])      # the permutations differ: the equality above is not vacuous
