"""The host-side helpers the ops wrappers share: the label -> cell table, the squared radii and the seed as the ABI's uint64_t.  No GPU."""
import numpy as np

from multiplexed_image_annotator_amd import ops


def test_cell_table_maps_labels_to_cells_and_nothing_else():
    table = ops._cell_table([2, 5])
    assert table.dtype == np.int32 and table.tolist() == [-1, -1, 0, -1, -1, 1]
    assert ops._cell_table(np.array([1, 2, 3], dtype=np.int32)).tolist() == [-1, 0, 1, 2]
    assert ops._cell_table([0, 3]).tolist() == [-1, -1, -1, 1]      # label 0 is the background whatever the list says


def test_cell_table_of_no_ids_is_one_entry_that_is_no_cell():
    for ids in ([], np.zeros(0, np.int64), np.zeros((0, 1), np.int32)):
        table = ops._cell_table(ids)
        assert table.dtype == np.int32 and table.tolist() == [-1]


def test_radii2_is_the_exact_fp64_square_as_a_contiguous_vector():
    radii = [0.0, 0.1, 30.0, 1e-160, 3.0000000000000004, 2.0 ** 500]
    r2 = ops._radii2(radii)
    assert r2.dtype == np.float64 and r2.ndim == 1 and r2.flags["C_CONTIGUOUS"]
    assert r2.tobytes() == np.array([r * r for r in radii], dtype=np.float64).tobytes()      # Python floats: one IEEE multiplication each
    wide = ops._radii2(np.array([[1, 2], [3, 4]], dtype=np.float32)[:, ::-1])      # any layout and real dtype, flattened in index order
    assert wide.dtype == np.float64 and wide.flags["C_CONTIGUOUS"] and wide.tolist() == [4.0, 1.0, 16.0, 9.0]
    assert ops._radii2([]).shape == (0,)


def test_u64_wraps_a_python_int():
    assert ops._u64(0) == 0 and ops._u64(2 ** 64 - 1) == 2 ** 64 - 1 and ops._u64(2 ** 63 + 5) == 2 ** 63 + 5
    assert ops._u64(-1) == 2 ** 64 - 1
    assert ops._u64(2 ** 64 + 3) == 3
    assert ops._u64(np.int64(-2)) == 2 ** 64 - 2 and isinstance(ops._u64(np.int64(7)), int)
