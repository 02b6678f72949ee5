"""cls_attention.hip: the attention output of the CLS row without the K / V product, through its hook and in the forward.

Accuracy: the reference is fp64 torch on the same rounded inputs (decoded packed-split rows, decoded folded weight, the fp32 bias); the
yardstick is the arithmetic the kernels replace -- folded qkv GEMM + attention kernel through ribca_test_qkv_attention_fold, row 0 of every
cell -- on the same inputs.  Per width, input family and cell count the new path's largest error may be at most TWICE the replaced path's
(the rule of tests/test_gpu_cell_mlp.py); no absolute number enters.  Every measured pair is appended to
profiles/cls_attn/gpu_tests_measured.log.

Input families (T = 101, cells = 1, 3, tile - 1, tile + 1 of the per-head kernels' cell tile):
    uniform   rows of mean 0.5 / spread 1, gains 1 +- 0.1
    heavy     one token row of every cell 50 times larger, LayerNorm gains 0.2 .. 5
    kbias     a k bias of +30: constant over the keys, so it drops out of the new form and only costs the replaced one bits
    wk0       W_k = 0: p is uniform and o = W'_v mean_j(y_j) + b'_v
    spike     W_k = 400 W_q, q bias 0: the CLS key's own score exceeds every other key's by more than 100 in at least one head of every
              cell; the other exponentials underflow and the output is finite

Contract: only columns 0 .. D - 1 of token row 0 of every cell are written (the rest of `out` keeps its 0x7E00 prefill), guard bands around
every buffer stay intact, two runs agree bit for bit, the bits do not depend on what the g / ybar scratch held, nor on the cell's place in
the tile or the call.

Forward: every classifier at depth 2, 19 cells, in this process and in a child with RIBCA_CLS_ATTN=0 (the switch is read once per process),
both against the oracle forward in fp64: at most twice the replaced path's error."""
import math
import os
import subprocess
import sys

import pytest
import torch

from multiplexed_image_annotator_amd import synth
from kernel_harness import Arena, fold_weight, ln_case, ps_decode, ps_encode, rnd, row_stats

pytestmark = pytest.mark.gpu

HEADS, T = 12, 101
WIDTHS = [144, 288, 384, 576]
FAMILIES = ["uniform", "heavy", "kbias", "wk0", "spike"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "cls_attn", "gpu_tests_measured.log")
PREFILL = 0x7E00      # an fp16 NaN in both halves of `out`


@pytest.fixture(scope="module")
def dev():
    from multiplexed_image_annotator_amd import _lib
    return _lib.require_gpu()


def _api():
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    return check, lib(), ptr, stream_ptr


def _log(line):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")
    print("[measured] " + line)


def _ratio(a, b):
    """a / b for the log; a replaced path that is exact has no ratio"""
    return f"{a / b:.2f}" if b > 0 else "n/a"


def _cell_counts():
    tile = _api()[1].ribca_test_cls_attention_cell_tile()
    assert tile > 1
    return [1, 3, tile - 1, tile + 1]


def _case(d, family, dev):
    """everything the kernels read for max(cells) cells of one (width, family), and the fp64 attention output of token 0 of every cell"""
    cells = max(_cell_counts())
    m = cells * T
    hd = d // HEADS
    z_ps, zq, g, b, dp = ln_case(m, d, 300 + d, dev, 0.5, 1.0)
    w = rnd((3 * d, d), 303 + d, dev, 1.0 / math.sqrt(d))
    bias = rnd((3 * d,), 304 + d, dev, 0.1)
    if family == "heavy":
        z = zq.to(torch.float32).contiguous()
        z.view(cells, T, d)[:, 37] *= 50.0
        z_ps = ps_encode(z, dp)
        zq = ps_decode(z_ps, d)
        u = synth.uniform(synth.stream_key(305, "cls_attn/gamma"), d).to(dev)
        g = torch.exp((2.0 * u - 1.0) * math.log(5.0)).to(torch.float32)
    elif family == "kbias":
        bias[d:2 * d] += 30.0
    elif family == "wk0":
        w[d:2 * d] = 0.0
    elif family == "spike":
        w[d:2 * d] = 400.0 * w[:d]
        bias[:d] = 0.0
    w_ps, csum, bias2 = fold_weight(w, g, b, bias, dp, dev)
    rs = row_stats(z_ps, dp, m, d, dev)
    # ---- fp64 on the rounded inputs: y = LayerNorm without gain / shift, the folded weight as the kernels hold it
    y = torch.nn.functional.layer_norm(zq, (d,), None, None, 1e-6).reshape(cells, T, d)
    wq = ps_decode(w_ps, d)[:3 * d]
    qkv = (y @ wq.t() + bias2.double()).reshape(cells, T, 3, HEADS, hd).permute(2, 0, 3, 1, 4)
    score = (qkv[0][:, :, :1] * hd ** -0.5) @ qkv[1].transpose(-1, -2)                # [cells][heads][1][T]
    ref = (torch.softmax(score, dim=-1) @ qkv[2]).permute(0, 2, 1, 3).reshape(cells, d)
    if family == "wk0":
        flat = y.mean(1) @ wq[2 * d:].t() + bias2[2 * d:].double()
        assert (flat - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    if family == "spike":
        top2 = score[:, :, 0].topk(2, dim=-1).values
        gap = (top2[..., 0] - top2[..., 1]).max(dim=1).values      # per cell: the clearest head
        assert gap.min().item() > 100.0, gap.min().item()
    torch.cuda.synchronize()
    return {"d": d, "dp": dp, "cells": cells, "z": z_ps, "w": w_ps, "csum": csum, "bias2": bias2, "rs": rs, "ref": ref}


@pytest.fixture(scope="module")
def cases(dev):
    cache = {}

    def get(d, family):
        if (d, family) not in cache:
            cache[(d, family)] = _case(d, family, dev)
        return cache[(d, family)]
    return get


def _run_new(f, cells, dev, band=0x00, scratch=0x00, first=0):
    """the hook on cells [first, first + cells) inside guard bands of `band` bytes: (arena, out rows [cells * T][2 dp])"""
    check, lib, ptr, stream_ptr = _api()
    d, dp = f["d"], f["dp"]
    rows = slice(first * T, (first + cells) * T)
    ar = Arena(dev, band, capacity=24 << 20)
    z, w, bias2, rs = ar.put(f["z"][rows]), ar.put(f["w"]), ar.put(f["bias2"]), ar.put(f["rs"][rows])
    g = ar.empty((cells * HEADS * d * 4,), torch.uint8)
    yb = ar.empty((cells * HEADS * d * 4,), torch.uint8)
    g.fill_(scratch)
    yb.fill_(scratch)
    out = ar.empty((cells * T, 2 * dp), torch.int16)
    out.fill_(PREFILL)
    check(lib.ribca_test_cls_attention(ptr(z), 2 * dp, ptr(w), 2 * dp, ptr(bias2), ptr(rs), cells, d, ptr(g), ptr(yb), ptr(out), 2 * dp,
                                       stream_ptr()), "cls attention")
    torch.cuda.synchronize()
    assert torch.equal(z, f["z"][rows]) and torch.equal(w, f["w"]) and torch.equal(rs, f["rs"][rows])      # inputs are read only
    return ar, out


def _run_old(f, cells, dev):
    """the replaced arithmetic: folded qkv GEMM + attention kernel; row 0 of every cell of its output"""
    check, lib, ptr, stream_ptr = _api()
    d, dp = f["d"], f["dp"]
    hdq = (d // HEADS + 7) // 8 * 8
    q = torch.zeros((cells, HEADS, 112, 2 * hdq), dtype=torch.int16, device=dev)
    k, vt = torch.zeros_like(q), torch.zeros_like(q)
    out = torch.zeros((cells * T, 2 * dp), dtype=torch.int16, device=dev)
    check(lib.ribca_test_qkv_attention_fold(ptr(f["z"]), 2 * dp, ptr(f["w"]), 2 * dp, cells, d, dp, ptr(f["bias2"]), ptr(f["csum"]), ptr(f["rs"]),
                                            ptr(q), ptr(k), ptr(vt), ptr(out), 2 * dp, stream_ptr()), "qkv fold + attention")
    torch.cuda.synchronize()
    return out


def _cls_rows(out, cells, k):
    return ps_decode(out.view(cells, T, -1)[:, 0].contiguous(), k)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", WIDTHS)
def test_cls_attention_accuracy_and_contract(dev, cases, d, family):
    f = cases(d, family)
    dp = f["dp"]
    whole = None
    for cells in sorted(_cell_counts(), reverse=True):
        ar, out = _run_new(f, cells, dev)
        got = _cls_rows(out, cells, d)
        old = _cls_rows(_run_old(f, cells, dev), cells, d)
        ref = f["ref"][:cells]
        e_new, e_old = (got - ref).abs().max().item(), (old - ref).abs().max().item()
        _log(f"{family} D={d} cells={cells}: new {e_new:.3e} replaced {e_old:.3e} (ratio {_ratio(e_new, e_old)}; largest |o| {ref.abs().max().item():.2f})")
        # ---- contract
        assert ar.bands_intact(), "a kernel wrote outside its operands"
        assert torch.isfinite(got).all()
        o3 = out.view(cells, T, 2 * dp)
        assert torch.all(o3[:, 1:] == PREFILL), "token rows 1 .. 100 of out were written"
        assert torch.all(o3[:, 0, 2 * d:] == PREFILL), "the pad columns D .. Dp of row 0 were written"
        # two runs, junk in the g / ybar scratch, NaN-pattern bands: the same bits
        for band, scratch in ((0x00, 0x00), (0x7C, 0xFF)):
            ar2, out2 = _run_new(f, cells, dev, band=band, scratch=scratch)
            assert ar2.bands_intact() and torch.equal(out2, out), (hex(band), hex(scratch))
        # a cell's bits do not depend on the call it is in
        if whole is None:
            whole = out.view(cells, T, 2 * dp)[:, 0].clone()
        else:
            assert torch.equal(o3[:, 0], whole[:cells]), f"cells 0 .. {cells - 1} alone differ from the same cells in the larger call"
        # ---- accuracy: at most twice the replaced path's error
        assert e_new <= 2.0 * e_old, (cells, e_new, e_old)
    # ... nor on its place in a tile: cells 5 .. 7 as cells 0 .. 2 of a call of their own
    _, win = _run_new(f, 3, dev, first=5)
    assert torch.equal(win.view(3, T, 2 * dp)[:, 0], whole[5:8])


def test_cls_attention_refuses_other_widths(dev):
    check, lib, ptr, stream_ptr = _api()
    t = torch.zeros(4096, dtype=torch.int16, device=dev)
    assert lib.ribca_test_cls_attention(ptr(t), 2 * 192, ptr(t), 2 * 192, ptr(t), ptr(t), 1, 192, ptr(t), ptr(t), ptr(t), 2 * 192, stream_ptr()) != 0
    assert b"ribca_test_cls_attention" in lib.ribca_last_error()


# ---------------------------------------------------------------------------------------------------------------- forward level
N_FWD = 19


def _fwd_inputs(name):
    d, c, k = synth.VIT_CONFIGS[name]
    u = synth.uniform(synth.stream_key(5, "cls_attn/fwd/" + name), N_FWD * c * 1600).reshape(N_FWD, c, 40, 40).to(torch.float32)
    return torch.where(u * 2 - 1 > 0.1, u * 2 - 1, torch.full_like(u, -1.0))


def _fwd_all(dev):
    """ribca_vit_forward of every classifier at depth 2 on the 19 cells, under whatever switches this process was started with"""
    from multiplexed_image_annotator_amd import ops
    res = {}
    for name in synth.VIT_CONFIGS:
        c = synth.VIT_CONFIGS[name][1]
        model = ops.VitModel(synth.make_vit_state_dict(name, synth.SEED_BASE + 7, depth=2), dev)
        res[name] = model._forward(_fwd_inputs(name).to(dev), list(range(c)), chunk_cells=8).cpu()
    return res


CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["RIBCA_ROOT"])
sys.path.insert(0, os.path.join(os.environ["RIBCA_ROOT"], "tests"))
import torch
from multiplexed_image_annotator_amd import _lib
import test_gpu_cls_attention as t
torch.save(t._fwd_all(_lib.require_gpu()), sys.argv[1])
"""


@pytest.fixture(scope="module")
def forwards(dev, tmp_path_factory):
    """(new path in this process, replaced path from a fresh child with RIBCA_CLS_ATTN=0)"""
    saved = os.environ.get("RIBCA_MARGIN_PROBE")
    os.environ["RIBCA_MARGIN_PROBE"] = "0"
    try:
        new = _fwd_all(dev)
        path = str(tmp_path_factory.mktemp("cls_attn") / "old.pt")
        env = dict(os.environ, RIBCA_CLS_ATTN="0", RIBCA_ROOT=ROOT)
        r = subprocess.run([sys.executable, "-c", CHILD, path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return new, torch.load(path)
    finally:
        if saved is None:
            del os.environ["RIBCA_MARGIN_PROBE"]
        else:
            os.environ["RIBCA_MARGIN_PROBE"] = saved


@pytest.mark.parametrize("name", list(synth.VIT_CONFIGS))
def test_vit_forward_new_against_replaced_path(forwards, name):
    from oracle import ref_vit
    new, old = forwards
    sd = {k: v.double() for k, v in synth.make_vit_state_dict(name, synth.SEED_BASE + 7, depth=2).items()}
    with torch.no_grad():
        ref = torch.softmax(ref_vit.logits(sd, _fwd_inputs(name).double()), dim=1)
    e_new, e_old = (new[name].double() - ref).abs().max().item(), (old[name].double() - ref).abs().max().item()
    _log(f"forward {name} depth 2, {N_FWD} cells: new {e_new:.3e} replaced {e_old:.3e} (ratio {_ratio(e_new, e_old)})")
    assert torch.isfinite(new[name]).all()
    assert e_new <= 2.0 * e_old, (e_new, e_old)
