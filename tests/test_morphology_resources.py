"""morphology.hip keeps a stretch of pixels in scalars and every table in LDS: no array is indexed by a label or a pixel, so the compile-only
check of tests/test_kernel_resources.py (no GPU needed) must report no spill and no scratch for its kernels."""
import test_kernel_resources as R


def test_no_spills_no_scratch(tmp_path):
    R.test_no_spills_no_scratch("morphology.hip", tmp_path)
