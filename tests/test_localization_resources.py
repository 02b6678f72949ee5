"""localization.hip keeps the staged tile and the column minima of the depth search in LDS, and the shell sums keep one accumulator per shell in
registers selected by predicates -- no array is indexed by a shell, a label or a pixel outside LDS --, so the compiler must report no spill and
no scratch for any of its kernels.  Compile only, no GPU needed: the check of tests/test_kernel_resources.py -- hipcc's
-Rpass-analysis=kernel-resource-usage remarks, parsed per kernel -- written out here, since tests/test_layout_host.py lets no further test
module import that one."""
import os
import re
import subprocess

from multiplexed_image_annotator_amd import build as B

KERNELS = ("mask_depth_kernelILi2E", "mask_depth_kernelILi4E", "mask_depth_kernelILi8E", "mask_depth_kernelILi16E", "mask_depth_kernelILi32E",
           "cell_shell_sums_small_kernel", "cell_shell_sums_kernel")


def test_no_spills_no_scratch(tmp_path):
    cmd = [B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-c", os.path.join(B.CSRC, "localization.hip"), "-o", str(tmp_path / "x.o"),
                                    "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    name, seen, bad = None, [], []
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen.append(name)
            continue
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and int(m.group(2)) != 0:
            bad.append((name, m.group(1), int(m.group(2))))
    for kernel in KERNELS:      # every kernel of the file was reported on
        assert any(kernel in s for s in seen), (kernel, seen)
    assert not bad, bad
