#!/usr/bin/env python3
"""Fingerprint of what the transformer forwards compute and launch, for comparing two builds of the library bit for bit: one JSON line
per case with the sha256 of the output bytes, the workspace sizes the library asks for, and the per-class launch counts of ribca_prof_read.

    python tools/forward_bits.py                                     > new.jsonl        (this tree's library)
    RIBCA_LIB=libribca_ab_old.so python tools/forward_bits.py        > old.jsonl        (python tools/build_ab_lib.py old <rev>)
    RIBCA_MAE_FOLD=0 python tools/forward_bits.py --imputer-only                        (the imputer's fp16x3 path)

The process switches (RIBCA_MX, RIBCA_MXZ, RIBCA_CELL_ATTN) are read once per process: one run per setting, the two files of a setting must
be byte-identical.  Cases: the five classifiers at depth 2 and depth 1, 19 cells in chunks of 8, through ribca_vit_forward and
ribca_vit_forward_precise; the imputer of the three panels at depth 2 + 2, 11 cells in chunks of 4, last marker missing.  The load-time
probes choose between these paths and are switched off here: the paths themselves are what is compared."""
import hashlib
import json
import os
import sys

os.environ["RIBCA_MARGIN_PROBE"] = "0"
os.environ["RIBCA_CHUNK_SCALE"] = "1"      # the chunk asked for, not the width's scaled one
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from multiplexed_image_annotator_amd import _lib, ops, synth

dev = _lib.require_gpu()
lib = _lib.lib()


def report(case, out, workspace_bytes):
    torch.cuda.synchronize()
    counts = {name: n for name, (_, n) in ops.prof_read().items()}
    sha = hashlib.sha256(out.cpu().contiguous().numpy().tobytes()).hexdigest()
    print(json.dumps({"case": case, "sha256": sha, "workspace_bytes": workspace_bytes, "launches": counts}, sort_keys=True), flush=True)


def classifiers():
    for name, (d, c, k) in synth.VIT_CONFIGS.items():
        g = torch.Generator().manual_seed(19 + d)
        patches = (torch.rand((19, c, 40, 40), generator=g) * 2 - 1).to(dev)
        for depth in (2, 1):
            model = ops.VitModel(synth.make_vit_state_dict(name, synth.SEED_BASE + 3, depth=depth), dev)
            ws = [int(lib.ribca_vit_workspace_bytes(model._h, n)) for n in (8, 1024)]
            for entry, kw in (("forward", {"force_fast": True}), ("forward_precise", {"precise": True})):
                ops.prof_enable(True)
                probs = model._forward(patches, list(range(c)), chunk_cells=8, **kw)
                report(f"vit {name} depth {depth} {entry}", probs, ws)
                ops.prof_enable(False)


def imputers():
    for panel, L in synth.MAE_PANELS.items():
        model = ops.MaeModel(synth.make_mae_state_dict(panel, synth.SEED_BASE + 5, enc_depth=2, dec_depth=2), dev)
        g = torch.Generator().manual_seed(11 + L)
        x = (torch.rand((11, L, 40, 40), generator=g) * 2 - 1).to(dev)
        ws = [int(lib.ribca_mae_workspace_bytes(model._h, n, L - 1)) for n in (4, 1024)]
        ops.prof_enable(True)
        model.impute(x, list(range(L - 1)), chunk_cells=4)
        report(f"mae {panel} depth 2+2", x, ws)
        ops.prof_enable(False)


if "--imputer-only" not in sys.argv:
    classifiers()
imputers()
