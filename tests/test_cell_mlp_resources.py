"""cell_mlp.hip fills registers with inline-asm ds_read behind counted waits and refills a three-slot LDS ring behind its stage barriers:
the two compile-only checks of tests/test_kernel_resources.py (no GPU needed) hold for it as for the GEMM family -- no spill and no
scratch (256 registers, two workgroups per CU), and no ds_read in flight across a barrier behind which a slot is refilled."""
import test_kernel_resources as R


def test_no_spills_no_scratch(tmp_path):
    R.test_no_spills_no_scratch("cell_mlp.hip", tmp_path)


def test_no_lds_read_in_flight_across_a_ring_barrier(tmp_path):
    R.test_no_lds_read_in_flight_across_a_ring_barrier("cell_mlp.hip", tmp_path)
