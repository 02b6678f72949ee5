"""The idioms the spatial analyses share (multiplexed_image_annotator_amd/analyses.py) on their own: file names, groups, selections and marker
names against literal values, the rank gate, the ranges of a permutation null, the packing of the tile-per-rank count all-reduce, and the
row exchange of cell_morphology / cell_intensities under a two-rank gloo group.  No GPU needed."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from batch_harness import free_port
from multiplexed_image_annotator_amd import analyses


class _Fake:
    """an Annotator with only the state a helper reads, without images or a GPU"""

    def __init__(self, **state):
        from multiplexed_image_annotator_amd.annotator import Annotator
        self.__class__ = type("FakeAnnotator", (Annotator,), {})
        self.__dict__.update(state)


def test_groups():
    assert analyses._groups(True, 3) == [[0, 1, 2]] and analyses._groups(False, 3) == [[0], [1], [2]]
    assert analyses._groups(True, 0) == [[]] and analyses._groups(False, 0) == []      # a rank without images still enters the integrated group


def test_group_stem():
    a = _Fake(batch_id="b7", preprocessor=SimpleNamespace(image_ids=[4, 9]))
    assert a._group_stem("contact", True, [0, 1]) == ("b7_integrated_contact", "")
    assert a._group_stem("contact", False, [1]) == ("b7_contact", "_9")
    assert a._group_stem("nearest_table", False, [0]) == ("b7_nearest_table", "_4")
    assert a._group_stem("morphology", True, []) == ("b7_integrated_morphology", "")      # no member is asked for its number
    assert "".join(a._group_stem("spatial_autocorr", False, [0])) == "b7_spatial_autocorr_4"


@pytest.mark.parametrize("world_size,tile_mode,rank,expected", [(1, False, 0, True), (2, False, 0, True), (2, False, 1, False), (2, True, 0, True),
                                                                  (2, True, 1, True)])
def test_computes_here(world_size, tile_mode, rank, expected):
    assert _Fake(world_size=world_size, tile_mode=tile_mode, rank=rank)._computes_here() is expected


def test_select_types():
    a = _Fake(cell_types=np.array(["B cell", "CD4 T cell", "Others"]))
    listed = "['B cell', 'CD4 T cell', 'Others']"
    assert a._select_types(None, "anchor") is None and a._select_types([], "anchor") == []
    assert a._select_types(["CD4 T cell", 0, np.int64(2), "B cell"], "target") == [1, 0, 2, 0]
    for bad, what, shown in (("T cell", "anchor", "'T cell'"), (True, "target", "True"), (3, "anchor", "3"), (-1, "target", "-1"), (1.0, "anchor", "1.0")):
        with pytest.raises(ValueError) as e:
            a._select_types(["Others", bad], what)
        assert str(e.value) == f"{what} {shown} is not one of the cell types {listed}"


def test_marker_names():
    a = _Fake(channel_parser=SimpleNamespace(markers=["CD3", "CD20", 7]))
    assert a._marker_names(5) == ["CD3", "CD20", "7", "channel 3", "channel 4"]      # fewer names than channels
    assert a._marker_names(3) == ["CD3", "CD20", "7"] and a._marker_names(2) == ["CD3", "CD20"] and a._marker_names(0) == []


def test_check_exact():
    a = _Fake(tile_mode=False, preprocessor=SimpleNamespace(_n_images=4))
    a._check_exact("who", "cells", [2 ** 52, 2 ** 52 - 1], 2 ** 60, True)      # the sum of a single-rank group: 2^53 - 1 passes
    a._check_exact("who", "cells", [2 ** 53 - 1, 2 ** 53 - 1], 2 ** 60, False)      # per image: the largest one
    a._check_exact("who", "cells", [], 2 ** 60, False)
    with pytest.raises(ValueError) as e:
        a._check_exact("contact_analysis", "pixel pairs", [2 ** 52, 2 ** 52], 1, True)
    assert str(e.value) == f"contact_analysis: a group of up to {2 ** 53} pixel pairs does not count exactly in fp64 (2^53)"
    a.tile_mode = True      # the integrated group of a tile-per-rank run: images of the batch x the bound, the same on every rank
    a._check_exact("who", "cells", [2 ** 60], 2 ** 51 - 1, True)
    with pytest.raises(ValueError, match=f"who: a group of up to {2 ** 53} cells does not count"):
        a._check_exact("who", "cells", [1], 2 ** 51, True)
    with pytest.raises(ValueError, match=f"up to {2 ** 60} cells"):
        a._check_exact("who", "cells", [2 ** 60], 1, False)      # per image, a tile-per-rank run judges its own


@pytest.mark.parametrize("p", [0, 1, 4, 5, 13])
def test_null_in_ranges(p):
    a = _Fake(NULL_BYTES=64)
    per_call = 4      # 64 bytes / 16 bytes per permutation
    ranges = list(a._null_in_ranges(p, 16))
    assert [q0 for q0, _ in ranges] == list(range(0, p, per_call))      # contiguous from 0
    assert all(1 <= q <= per_call for _, q in ranges) and sum(q for _, q in ranges) == p
    assert all(q0 + q == nxt for (q0, q), (nxt, _) in zip(ranges, ranges[1:]))
    assert list(a._null_in_ranges(3, 1000)) == [(0, 1), (1, 1), (2, 1)]      # a permutation larger than the budget still goes, alone
    from multiplexed_image_annotator_amd.annotator import Annotator
    assert Annotator.NULL_BYTES == 64 << 20


def _count_arrays():
    rng = np.random.RandomState(5)
    top = 2 ** 52 - 1      # twice this is still below 2^53
    arrays = [rng.randint(0, 1000, size=(3, 3)).astype(np.int64), np.zeros((0, 3, 3), dtype=np.int64),
              rng.randint(0, top, size=(2, 4, 3, 3)).astype(np.int64), np.array([0, top, 1, top - 1, 5], dtype=np.int64)]
    return arrays, [7, top, 0]


def test_all_reduce_counts_world_of_one():
    arrays, scalars = _count_arrays()
    arrays[0][0, 0], scalars[0] = 2 ** 53 - 1, 2 ** 53 - 1      # the largest count the callers admit survives the fp64 buffer
    kept = [a.copy() for a in arrays]
    out, back = analyses._all_reduce_counts(arrays, scalars)
    assert back == scalars and all(type(v) is int for v in back)
    assert len(out) == len(arrays)
    for got, want in zip(out, kept):
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    assert all(np.array_equal(a, k) for a, k in zip(arrays, kept))      # the arguments are not modified


def test_all_reduce_counts_splits_a_summed_buffer(monkeypatch):
    """a collective that doubles: every array and scalar has to come back from its own stretch of the buffer"""
    arrays, scalars = _count_arrays()
    seen = []
    def doubled(buf):
        seen.append(buf)
        return 2 * buf
    monkeypatch.setattr(analyses.dist, "all_reduce_sum", doubled)
    out, back = analyses._all_reduce_counts(arrays, scalars)
    assert len(seen) == 1 and seen[0].dtype == torch.float64 and seen[0].shape == (sum(a.size for a in arrays) + len(scalars),)      # ONE all-reduce
    assert back == [2 * s for s in scalars]
    for got, want in zip(out, arrays):
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, 2 * want)


def _row_cases():
    """(name, cells per image) with image i on rank i % 2, as tile-per-rank mode deals them"""
    return [("unequal", [5, 3, 2]), ("one rank without rows", [4, 0, 6]), ("all empty", [0, 0, 0])]


def _rows(cells_per_image, width=5):
    """the single-rank table: image number, cell id (ascending, with gaps), three columns of thirds"""
    rng = np.random.RandomState(11)
    out = []
    for number, n in enumerate(cells_per_image):
        ids = np.sort(rng.choice(np.arange(1, 50), size=n, replace=False)).astype(np.float64)
        out.append(np.concatenate([np.full((n, 1), float(number)), ids.reshape(n, 1), rng.randint(-9, 9, size=(n, width - 2)) / 3.0], axis=1))
    return np.concatenate(out, axis=0) if out else np.zeros((0, width))


def _gather_worker(rank, world, port, out):
    import torch.distributed as td
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    a = _Fake(rank=rank, world_size=world)
    ok = []
    for name, cells in _row_cases():
        single = _rows(cells)
        mine = single[single[:, 0].astype(np.int64) % world == rank]
        got, extra = a._gather_rows(mine, extra=(rank + 3, 10 * rank))
        ok.append(got.dtype == np.float64 and got.shape == single.shape and np.array_equal(got, single) and extra == [3 + 4, 10])
        got, extra = a._gather_rows(mine[::-1].copy())      # whatever order a rank holds them in; no extra
        ok.append(np.array_equal(got, single) and extra == [])
    out[rank] = ok
    td.destroy_process_group()


def test_gather_rows_gloo_world2():
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_gather_worker, args=(2, free_port(), out), nprocs=2, join=True)
    assert dict(out) == {0: [True] * 6, 1: [True] * 6}


def test_gather_rows_world_of_one():
    a = _Fake(rank=0, world_size=1)
    single = _rows([3, 0, 4])
    got, extra = a._gather_rows(single[::-1].copy(), extra=(2,))
    assert np.array_equal(got, single) and extra == [2]
    got, extra = a._gather_rows(np.zeros((0, 5)))
    assert got.shape == (0, 5) and extra == []


def test_centroids():
    tab = np.array([[0, 0, 0, 0, 10, 30, 4], [0, 0, 0, 0, 7, 1, 3]], dtype=np.int64)      # ..., sum of rows, sum of columns, area
    x, y = _Fake(preprocessor=SimpleNamespace(cell_tables=[tab]))._centroids(0)
    assert x.dtype == np.float64 and y.dtype == np.float64
    assert np.array_equal(x, [7.5, 1.0 / 3.0]) and np.array_equal(y, [2.5, 7.0 / 3.0])
