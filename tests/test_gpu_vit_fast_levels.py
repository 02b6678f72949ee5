"""The two fast levels of a classifier handle (ribca_vit_set_fast_level: 2 = with the per-cell kernel's MX products, 1 = that kernel at three
fp16 passes and every other MX product as before) and the load-time probe that chooses between them (ops.VitModel._calibrate_margin).

Entry point (handles created with RIBCA_MARGIN_PROBE=0: no probe forwards): the level returned per request on a 384-wide handle (2, 1) and
on a 288-wide one (1 whatever is asked); levels 0 and 3 and a NULL handle are refused with -1 and a message that names the entry point, and
the level in effect -- seen through the bits of the fast forward -- is what it was; the workspace size does not depend on the level.

Fallback: a 384-wide model that FAILS level 2 and KEEPS level 1, the case the entry point exists for.  Candidates are
synth.make_vit_state_dict_heavy(.., SEED_BASE + s, head_gain=4.0), s = 7, 3, 11, 13, each loaded once under a bar nothing passes
(RECHECK_MARGIN = 1e-12: both levels probed and refused, the fast forward IS the precise one); a = predicted worst |dp| at level 2, b = at
level 1; the first candidate with a > 1.05 b is reloaded under a bar of sqrt(a b) (level 2 refused, level 1 kept: the same a and b
exactly, the fast forward bit-equal to that of a handle switched to level 1 by hand, |fast - precise| of 8 cells within the bar) and under a
bar of 2 a (level 2 kept, level 1 never probed).  No value of a or b is assumed: every bar is built from what was measured, and each
(a, b) is appended to profiles/cell_attn_mx/gpu_tests_measured.log.

Measured on MI355X: the first candidate (SEED_BASE + 7) separates the levels, a = 8.354e-4 at level 2 and b = 6.995e-4 at level 1 (a / b =
1.19; the product's bar, 4e-4, refuses both, which is why the bars here are built from a and b); under the bar sqrt(a b) = 7.644e-4 the
model keeps level 1 and its 8 cells differ from the precise forward by 2.4e-5."""
import math
import os

import pytest
import torch

from multiplexed_image_annotator_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "cell_attn_mx", "gpu_tests_measured.log")
WIDE, NARROW = "immune_extended", "immune_base"      # 384 wide: the per-cell MX kernel; 288 wide: none
CANDIDATES = [7, 3, 11, 13]


@pytest.fixture(scope="module")
def dev():
    from multiplexed_image_annotator_amd import _lib
    return _lib.require_gpu()


def _log(line):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")
    print("[measured] " + line)


def _cells(name, dev, n=8):
    """the cells of tests/test_gpu_cell_attention_mx_forward.py"""
    d, c, _ = synth.VIT_CONFIGS[name]
    g = torch.Generator().manual_seed(8 + d)
    u = torch.rand((n, c, 40, 40), generator=g) * 2 - 1
    return torch.where(u > 0.1, u, torch.full_like(u, -1.0)).to(dev), list(range(c))


def test_set_fast_level_entry_point(dev, monkeypatch):
    from multiplexed_image_annotator_amd import ops
    from multiplexed_image_annotator_amd._lib import lib
    monkeypatch.setenv("RIBCA_MARGIN_PROBE", "0")      # handles only: no probe forwards at load
    set_level, last_error, ws_bytes = lib().ribca_vit_set_fast_level, lib().ribca_last_error, lib().ribca_vit_workspace_bytes
    wide = ops.VitModel(synth.make_vit_state_dict(WIDE, synth.SEED_BASE + 7, depth=2), dev)
    narrow = ops.VitModel(synth.make_vit_state_dict(NARROW, synth.SEED_BASE + 7, depth=2), dev)
    assert wide.fast_level == 2 and narrow.fast_level == 1                      # what create leaves
    x, src = _cells(WIDE, dev)

    def fast():
        y = wide._forward(x, src, chunk_cells=8, precise=False)
        torch.cuda.synchronize()
        return y

    def refusals(want):
        """every refused request: -1, a message that names the entry point, and the fast forward keeps the bits it had"""
        for handle, level in ((wide._h, 0), (wide._h, 3), (wide._h, -1), (None, 2), (None, 1)):
            assert set_level(handle, level) == -1, (handle, level)
            assert b"ribca_vit_set_fast_level" in last_error(), (handle, level)
            assert torch.equal(fast(), want), f"a refused request (level {level}) changed the level in effect"

    assert set_level(wide._h, 2) == 2
    sizes = {2: [int(ws_bytes(wide._h, n)) for n in (1, 8, 64)]}
    y2 = fast()
    refusals(y2)
    assert set_level(wide._h, 1) == 1
    sizes[1] = [int(ws_bytes(wide._h, n)) for n in (1, 8, 64)]
    y1 = fast()
    assert not torch.equal(y1, y2)                                              # the levels are two arithmetics: the checks above can fail
    refusals(y1)
    assert sizes[1] == sizes[2] and min(sizes[1]) > 0
    assert set_level(wide._h, 2) == 2 and torch.equal(fast(), y2)
    for level in (2, 1, 2):
        assert set_level(narrow._h, level) == 1                                 # no per-cell MX kernel to switch
    assert set_level(narrow._h, 0) == -1 and b"ribca_vit_set_fast_level" in last_error()


def test_probe_falls_back_to_level_1(dev, monkeypatch):
    from multiplexed_image_annotator_amd import ops
    monkeypatch.delenv("RIBCA_MARGIN_PROBE", raising=False)      # the probe is what this test is about
    x, src = _cells(WIDE, dev)

    def load(sd, margin):
        monkeypatch.setattr(ops.VitModel, "RECHECK_MARGIN", margin)
        return ops.VitModel(sd, dev)

    def forwards(model):
        fast = model._forward(x, src, chunk_cells=8, precise=False)
        full = model._forward(x, src, chunk_cells=8, precise=True)
        torch.cuda.synchronize()
        return fast, full

    chosen = None
    for s in CANDIDATES:
        sd = synth.make_vit_state_dict_heavy(WIDE, synth.SEED_BASE + s, head_gain=4.0)
        model = load(sd, 1e-12)                                                 # a bar nothing passes: both levels probed, both refused
        assert model.fast_level == 0 and not model.fast_ok and not model.uses_mx
        assert set(model.probe_level_dp) == {2, 1}
        fast, full = forwards(model)
        assert torch.equal(fast, full), "a refused model's fast forward is not the precise one"
        a, b = model.probe_level_dp[2], model.probe_level_dp[1]
        _log(f"fallback candidate heavy SEED_BASE+{s} head_gain 4: predicted worst |dp| level 2 a = {a:.6e}  level 1 b = {b:.6e}  a / b = "
             f"{a / b if b > 0 else float('inf'):.3f}")
        if a > 1.05 * b:
            chosen = (s, sd, a, b, full)
            break
    assert chosen is not None, "no candidate separates the levels (a > 1.05 b): the test means nothing"
    s, sd, a, b, full = chosen

    # ---- a bar between the two: level 2 fails, level 1 is kept
    bar = math.sqrt(a * b)
    model = load(sd, bar * ops.VitModel.PROBE_DIVISOR)
    assert model.fast_level == 1 and model.fast_ok and model.uses_mx
    assert model.probe_level_dp == {2: a, 1: b}
    fast, full_b = forwards(model)
    assert torch.equal(full_b, full)
    monkeypatch.setenv("RIBCA_MARGIN_PROBE", "0")                # a handle as create leaves it
    by_hand = ops.VitModel(sd, dev)
    monkeypatch.delenv("RIBCA_MARGIN_PROBE")
    assert by_hand.fast_level == 2 and by_hand.probe_level_dp == {}
    at2, _ = forwards(by_hand)
    assert by_hand._set_fast_level(1) == 1
    at1, _ = forwards(by_hand)
    assert torch.equal(fast, at1), "the probe's fallback is not the handle at level 1"
    assert not torch.equal(at1, at2)
    dp = (fast.double() - full.double()).abs().max().item()
    _log(f"fallback model heavy SEED_BASE+{s}: bar sqrt(a b) = {bar:.6e} keeps level 1; max |fast - precise| of 8 cells {dp:.3e}")
    assert dp <= bar, (dp, bar)

    # ---- a bar above both: level 2 is kept and level 1 never probed
    model = load(sd, 2.0 * a * ops.VitModel.PROBE_DIVISOR)
    assert model.fast_level == 2 and model.fast_ok and model.uses_mx
    assert set(model.probe_level_dp) == {2} and model.probe_level_dp[2] == a
    fast2, _ = forwards(model)
    assert torch.equal(fast2, at2)
