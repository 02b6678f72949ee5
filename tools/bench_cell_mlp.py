#!/usr/bin/env python3
"""Times the one-kernel second half of a 144-wide block (cell_mlp.hip) against the launches it replaces -- proj (residual GEMM on the
two-workgroups kernel + finaliser), fc1 (folded GELU GEMM), fc2 (residual GEMM + finaliser) -- on the same rows, through the hooks.
usage: python tools/bench_cell_mlp.py [rows]   (default 103424 = 1024 cells: one chunk of the bench workload)
The replaced sequence as timed here carries two launch_pack_wf launches the forward does not make (the duo hook packs its weight per
call: 2 x ~3 us); tools/bench_block.py nerve under RIBCA_CELL_MLP=0 / 1 is the in-forward comparison."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from multiplexed_image_annotator_amd import _lib
from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr

dev = _lib.require_gpu()
M = int(sys.argv[1]) if len(sys.argv) > 1 else 103424
D, DP, H4 = 144, 160, 576
g = torch.Generator().manual_seed(0)


def ps(rows, cols2, scale):
    return (torch.randn((rows, cols2), generator=g) * scale).to(torch.float16).view(torch.int16).to(dev)


xa, z0 = ps(M, 2 * DP, 0.5), ps(M, 2 * DP, 0.5)
npd, n1p = lib().ribca_gemm_padded_n(D), lib().ribca_gemm_padded_n(H4)
wp, w1, w2 = ps(npd, 2 * DP, 0.05), ps(n1p, 2 * DP, 0.05), ps(npd, 2 * H4, 0.03)
bp, b2 = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
c1, b1 = torch.zeros(H4, device=dev), torch.zeros(H4, device=dev)
rs0 = torch.cat([torch.ones((M, 1)), torch.zeros((M, 1))], 1).to(dev)
z, rs, rs2 = z0.clone(), rs0.clone(), rs0.clone()
img = torch.zeros(lib().ribca_test_cell_mlp_image_bytes(D) // 2, dtype=torch.int16, device=dev)
h = torch.zeros((M, 2 * H4), dtype=torch.int16, device=dev)
part = torch.zeros((lib().ribca_test_resid_part_rows(D), M, 2), device=dev)
wfp, wf1, wf2 = torch.zeros_like(wp), torch.zeros_like(w1), torch.zeros_like(w2)
packed = [0]


def fused():
    check(lib().ribca_test_cell_mlp(ptr(xa), 2 * DP, ptr(wp), ptr(w1), ptr(w2), ptr(bp), ptr(c1), ptr(b1), ptr(b2), ptr(img), 1 - packed[0], ptr(z),
                                    2 * DP, ptr(rs), M, D, stream_ptr()), "cell_mlp")
    packed[0] = 1


def replaced():
    check(lib().ribca_test_gemm_resid_ps_duo(ptr(xa), 2 * DP, ptr(wp), 2 * DP, M, D, DP, ptr(bp), ptr(wfp), ptr(z), 2 * DP, ptr(part), ptr(rs2), ptr(rs),
                                             stream_ptr()), "proj")
    check(lib().ribca_test_gemm_duo_gelu(ptr(z), 2 * DP, ptr(w1), 2 * DP, M, H4, DP, ptr(b1), ptr(c1), ptr(rs2), ptr(wf1), ptr(h), 2 * H4, stream_ptr()),
          "fc1")
    check(lib().ribca_test_gemm_resid_ps_duo(ptr(h), 2 * H4, ptr(w2), 2 * H4, M, D, H4, ptr(b2), ptr(wf2), ptr(z), 2 * DP, ptr(part), ptr(rs), ptr(rs2),
                                             stream_ptr()), "fc2")


res = {}
for name, fn in (("cell_mlp (one launch)", fused), ("proj + fc1 + fc2 + two finalisers", replaced)):
    runs = []
    for rep in range(5):
        z.copy_(z0)
        rs.copy_(rs0)
        fn()                                         # warm
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / 5 * 1e3)
    res[name] = runs
    print(f"M={M} {name}: best {min(runs):.1f} us, runs " + " ".join(f"{r:.1f}" for r in runs), flush=True)
a, b = res["cell_mlp (one launch)"], res["proj + fc1 + fc2 + two finalisers"]
print(f"ratio of the bests {min(a) / min(b):.3f}; spread of repeated runs: {max(a) - min(a):.1f} us / {max(b) - min(b):.1f} us", flush=True)
