"""cell_attention_mx.hip refills a three-slot LDS ring behind its step barriers and holds a cell's token rows, their fp8 / fp6 images and twelve
accumulator tiles in registers for the whole kernel.  Compile-only (no GPU needed): the kernel's own budget, at most 256 vector registers
(two waves per SIMD at 512 threads) and at most 160 KB of LDS, static plus the dynamic size its launcher asks for.  No spill, no scratch and
no ds_read in flight across a barrier behind which a slot is refilled: tests/test_kernel_resources.py, which lists this file beside the
fp16x3 kernel's."""
import os
import re
import subprocess

import pytest

from multiplexed_image_annotator_amd import build as B

SRC = os.path.join(B.CSRC, "cell_attention_mx.hip")
LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """the compiler's kernel-resource-usage remarks of the file: {kernel name: {field: value}}"""
    out = tmp_path_factory.mktemp("cam") / "x.o"
    cmd = [B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-c", SRC, "-o", str(out), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    name, seen = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
            continue
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|VGPRs|AGPRs|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            seen[name][m.group(1)] = int(m.group(2))
    assert seen, "no kernel-resource-usage remarks in the compiler output"
    return seen


def _dynamic_lds():
    """the LDS map of CellMxGeom<384, 32>, restated from the constants of the source: ring of 3 stages, two K images, the V image, column sums and bias"""
    d, gd, ntp, tp, vrows = 384, 64, 4, 112, 128
    stage = ntp * 4096 + ntp * 1024 + ntp * 512 + 1024
    vimg = vrows * 4 * gd + 64
    return 3 * stage + (gd // 32) * tp * 128 + (vimg + 15) // 16 * 16 + 2 * 3 * d * 4


def test_registers_and_lds(usage):
    kern = [k for k in usage if "cell_qkv_attention_mx_kernel" in k]
    assert len(kern) == 1, list(usage)
    res = usage[kern[0]]
    dyn = _dynamic_lds()
    print("[measured]", kern[0], res, "dynamic LDS", dyn)
    assert res["VGPRs"] + res.get("AGPRs", 0) <= 256, res
    assert "static_assert(LDS <= 160 * 1024" in open(SRC).read()      # the source checks its own map; this restatement gives the figure
    assert res["LDS Size [bytes/block]"] + dyn <= LDS_CU, (res, dyn)
