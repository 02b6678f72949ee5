"""components.hip keeps the parent array of a tile, the staged labels and the per-root table of the statistics in LDS and a pixel's chain walk in
scalars: no array is indexed by a pixel or a label in registers, so the compile-only check of tests/test_kernel_resources.py (no GPU needed)
must report no spill and no scratch for every kernel of the file."""
import test_kernel_resources as R


def test_no_spills_no_scratch(tmp_path):
    R.test_no_spills_no_scratch("components.hip", tmp_path)
