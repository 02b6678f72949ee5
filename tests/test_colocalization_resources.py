"""colocalization.hip keeps a block's 16 accumulators for each of a lane's four partials in registers chosen by compile-time indices, and the
offsets, the gate words, the stage and the selected channel numbers in LDS -- no array is indexed by a label, a pixel or a runtime channel
number outside LDS --, so the compiler must report no spill and no scratch for its kernel, and an LDS size at or under 64 KB, which keeps two
workgroups or more on a CU.  Compile only, no GPU needed: the check of tests/test_kernel_resources.py -- hipcc's
-Rpass-analysis=kernel-resource-usage remarks, parsed per kernel -- written out here, since tests/test_layout_host.py lets no further test
module import that one."""
import os
import re
import subprocess

from multiplexed_image_annotator_amd import build as B

KERNELS = ("cell_coloc_kernel",)


def test_no_spills_no_scratch_and_lds_within_64_kb(tmp_path):
    cmd = [B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-c", os.path.join(B.CSRC, "colocalization.hip"), "-o", str(tmp_path / "x.o"),
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
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and int(m.group(1)) > 64 * 1024:
            bad.append((name, "LDS", int(m.group(1))))
        m = re.search(r"\bVGPRs: (\d+)", line)
        if m and int(m.group(1)) > 256:      # two waves per SIMD: the two workgroups the LDS allows
            bad.append((name, "VGPRs", int(m.group(1))))
    for kernel in KERNELS:      # every kernel of the file was reported on
        assert any(kernel in s for s in seen), (kernel, seen)
    assert len(seen) == len(KERNELS), seen
    assert not bad, bad
