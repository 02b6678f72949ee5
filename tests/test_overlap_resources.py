"""overlap.hip keeps a thread's four labels and its running (cell, object, count) in scalars and the workgroup's pair table in LDS: no array is
indexed by a pixel in registers, so the compile-only check of tests/test_kernel_resources.py (no GPU needed) must report no spill and no scratch
for every kernel of the file, the shared row-table kernels of csrc/ribca_rowtable.h included."""
import test_kernel_resources as R


def test_no_spills_no_scratch(tmp_path):
    R.test_no_spills_no_scratch("overlap.hip", tmp_path)
