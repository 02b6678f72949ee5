"""outlines.hip keeps a walker's state -- vertex, direction, the running edge, vertex, area and saddle counts -- in scalars and the staged tile
and the candidates of a tile in LDS: no array is indexed by a direction or a pixel in registers, so the compile-only check of
tests/test_kernel_resources.py (no GPU needed) must report no spill and no scratch for every kernel of the file."""
import test_kernel_resources as R


def test_no_spills_no_scratch(tmp_path):
    R.test_no_spills_no_scratch("outlines.hip", tmp_path)
