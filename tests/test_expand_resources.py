"""expand.hip keeps the staged labels and the column minima in LDS and the running minimum of a pixel in scalars: no array is indexed by a
pixel or a label in registers, so the compile-only check of tests/test_kernel_resources.py (no GPU needed) must report no spill and no scratch
for every halo width of its kernel."""
import test_kernel_resources as R


def test_no_spills_no_scratch(tmp_path):
    R.test_no_spills_no_scratch("expand.hip", tmp_path)
