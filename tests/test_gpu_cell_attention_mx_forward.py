"""The classifiers' forward with and without the per-cell kernel's MX products (process switch RIBCA_CELL_ATTN_MX, read once per process:
one child process per setting -- the switch is what this test is about).  On 8 cells per classifier:

* the fast forwards of the two processes differ by no more than the load-time probe's own acceptance, predicted worst |dp| <=
  RECHECK_MARGIN / PROBE_DIVISOR (ops.VitModel._calibrate_margin): what the margin-gated re-evaluation of Annotator.predict rests on;
* the precise forward (ribca_vit_forward_precise) is bit-identical in both: precise() clears the flag, the fp16x3 kernel is untouched, and
  RIBCA_CELL_ATTN_MX=0 is the path of the tree before this kernel existed;
* classifiers without a per-cell MX kernel (every width but 384) have bit-identical fast forwards as well, and report fast level 1;
* the level switch is stateless (ribca_vit_set_fast_level on the RIBCA_CELL_ATTN_MX=1 handles, after their forwards): at level 1 the fast
  forward of the 384-wide handle has the bits of the RIBCA_CELL_ATTN_MX=0 process -- the forward of the tree before the per-cell MX kernel --
  back at level 2 it has the bits of the first level-2 forward, and the precise forward has the same bits at either level.

Measured on MI355X: the 384-wide model ends at level 2 (predicted worst |dp| 3.1e-4; 2.5e-4 at level 1 in the other process), its fast
forwards under the two switches differ by 6.0e-6 on the 8 cells, every other width by 0."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
import torch
from multiplexed_image_annotator_amd import _lib, ops, synth
dev = _lib.require_gpu()
out = {}
for name, (d, c, k) in synth.VIT_CONFIGS.items():
    g = torch.Generator().manual_seed(8 + d)
    u = torch.rand((8, c, 40, 40), generator=g) * 2 - 1
    x = torch.where(u > 0.1, u, torch.full_like(u, -1.0)).to(dev)
    model = ops.VitModel(synth.make_vit_state_dict(name, synth.SEED_BASE + 3), dev)
    fast = model._forward(x, list(range(c)), chunk_cells=8, precise=False).cpu()
    full = model._forward(x, list(range(c)), chunk_cells=8, precise=True).cpu()
    out[name] = {"D": d, "fast": fast.double().tolist(), "fast_sha": hashlib.sha256(fast.numpy().tobytes()).hexdigest(),
                 "precise_sha": hashlib.sha256(full.numpy().tobytes()).hexdigest(), "fast_level": model.fast_level, "uses_mx": model.uses_mx,
                 "probe_level_dp": model.probe_level_dp, "bar": float(ops.VitModel.RECHECK_MARGIN) / ops.VitModel.PROBE_DIVISOR}
    if model.fast_level == 2:      # the switch, after the forwards: down to level 1, up again
        sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
        out[name]["down"] = model._set_fast_level(1)
        out[name]["fast_sha_level1"] = sha(model._forward(x, list(range(c)), chunk_cells=8, precise=False))
        out[name]["precise_sha_level1"] = sha(model._forward(x, list(range(c)), chunk_cells=8, precise=True))
        out[name]["up"] = model._set_fast_level(2)
        out[name]["fast_sha_level2_again"] = sha(model._forward(x, list(range(c)), chunk_cells=8, precise=False))
        out[name]["precise_sha_level2_again"] = sha(model._forward(x, list(range(c)), chunk_cells=8, precise=True))
print("RESULT " + json.dumps(out))
""" % ROOT


def _child(setting):
    env = dict(os.environ, RIBCA_CELL_ATTN_MX=setting)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][7:])


def test_forward_with_and_without_the_per_cell_mx_products():
    off, on = _child("0"), _child("1")
    assert set(off) == set(on) and len(on) == 5
    for name in on:
        a, b = off[name], on[name]
        assert a["precise_sha"] == b["precise_sha"], name
        assert a["fast_level"] <= 1, (name, a["fast_level"])                  # the switch at 0: no handle has the per-cell MX kernel
        dp = max(abs(p - q) for ra, rb in zip(a["fast"], b["fast"]) for p, q in zip(ra, rb))
        print(f"[measured] {name} D={b['D']}: fast level {a['fast_level']} / {b['fast_level']}, max |dp| between the switches {dp:.3e} "
              f"(bar {b['bar']:.1e}); probe predicted worst |dp| per level {a['probe_level_dp']} / {b['probe_level_dp']}")
        assert dp <= b["bar"], (name, dp, b["bar"])
        if b["D"] != 384:
            assert b["fast_level"] <= 1 and a["fast_sha"] == b["fast_sha"], name
        else:
            assert b["uses_mx"] and b["fast_level"] == 2, (name, b["fast_level"], b["probe_level_dp"])
            assert (b["down"], b["up"]) == (1, 2), name
            assert b["fast_sha"] != a["fast_sha"], name                       # (the two levels differ on these cells: the next lines say something)
            assert b["fast_sha_level1"] == a["fast_sha"], name                # level 1 on a level-2 handle: the pre-MX forward, bit for bit
            assert b["fast_sha_level2_again"] == b["fast_sha"], name          # and back: no state left behind
            assert b["precise_sha_level1"] == b["precise_sha"] == b["precise_sha_level2_again"], name
