"""intensities.hip keeps the offsets, one channel's keys, the histograms and the partials of a cell in LDS and everything else in scalars: no
array is indexed by a label, a pixel or a rank outside LDS, so the compile-only check of tests/test_kernel_resources.py (no GPU needed) must
report no spill and no scratch for its kernel."""
import test_kernel_resources as R


def test_no_spills_no_scratch(tmp_path):
    R.test_no_spills_no_scratch("intensities.hip", tmp_path)
