"""cell_attention_mx.hip through its hooks: the per-cell norm1 -> qkv -> attention kernel with the QKV phase as fp16 hi * hi plus two
block-scaled products (D = 384; T = 101 is fixed by the kernel).

Accuracy: the reference is fp64 torch on the SAME rounded inputs (the packed-split rows, the packed-split folded weight, the column sums, the
folded bias and the row statistics the kernels read).  The yardstick is the unfused MX pair the repository already has at this width
(launch_gemm_mx_qkv_ln + attention kernel, hook ribca_test_qkv_attention_mx) on the same inputs against the same reference: both form the same
three products per 128 k from operands rounded by the same rules and differ in how k is grouped into 32-element scale blocks (here a block is
one lane's k = 32 s + 8 g + j, there 32 consecutive k) and in summation order, so per case the new kernel's error (max |out - ref|) may be at
most TWICE the pair's -- the margin tests/test_gpu_cell_mlp.py gives a re-ordered summation.  Families: "uniform" (weights N(0, 1 / D), gains
1 +- 0.1) and "heavy" (LayerNorm gains log-uniform in 0.2 .. 5, i.e. k columns of gamma o W a factor 25 apart inside one scale block, and one
row of W -- output column 2 D + 7, a v column, so that the softmax stays comparable -- multiplied by 50).  Cells 1, 3, 17: slices of one
17-cell case per family, whose reference is computed once.
Every measured pair is appended to profiles/cell_attn_mx/gpu_tests_measured.log.

Measured on MI355X (new / unfused MX pair): uniform 5.5e-5 / 5.6e-5 at 1 and 3 cells, 5.9e-5 / 6.0e-5 at 17; heavy 1.34e-2 / 0.91e-2 at 1
cell (ratio 1.46, the closest), 1.34e-2 / 1.19e-2 at 3, 1.34e-2 / 1.20e-2 at 17 (the v column scaled by 50 carries outputs of that size).

Contract: the weight image equals a numpy emulation written from tests/mx_emulation.py bit for bit (every byte of the image is written); two
launches agree bit for bit; a cell computed alone has the bits it has among 17; with every buffer carved out of an arena of 0xFF bytes and
the output prefilled with 0xFF the results are unchanged and every band between the buffers is intact.

Row families beside those two (tests/cell_mx_families.py; the weights of "uniform"): "mean30" (|mean| / std = 30: the folded-LayerNorm epilogue
under cancellation) and "edge_rows" (row scales over three decades shuffled so that the 16 tokens of a wave differ, outlier columns x 4096 --
some saturating fp16 --, an all-zero 128-k step, fp16-subnormal rows; rows 0 and T - 1 of cell 0, the token the pad rows copy, untouched).
For rows whose 32-value blocks are not of one exponent the pair is no fair yardstick against the EXACT reference (its blocks are other
blocks), so all four families are also held against fp64 on each kernel's OWN quantised operands -- mx_emulation.cell_gemm for this kernel,
mx_emulation.gemm for the pair, then the folded LayerNorm and the attention in fp64: only fp32 arithmetic separates a kernel from that --
and the new kernel's distance may be at most twice the pair's (cells 1 and 3).  The exact-reference criterion is kept for "mean30" with the
absolute bar the pair itself is held to, (4e-5 + 2e-4) (1 + 30) (tests/test_gpu_mx.py::test_qkv_attention_mx); for "edge_rows" the exact-
reference errors are logged only.  300 cells of "uniform" (more workgroups than the 256 CUs): arena contract, exact-reference criterion,
cells 0, 255, 256 and 299 alone.

Measured on MI355X, against the emulated operands (new / pair): uniform 8.5e-7 / 8.6e-7 at 1 cell, 9.0e-7 / 9.4e-7 at 3; edge_rows 8.0e-7 /
8.9e-7 and 9.8e-7 / 1.04e-6; mean30 1.43e-5 / 1.22e-5 and 1.60e-5 / 1.24e-5 (ratio 1.28, the closest: everything is 31 times larger there);
heavy 1.86e-4 / 1.60e-4 and 2.23e-4 / 2.86e-4 (fp32 arithmetic on the v column scaled by 50).  Against the exact reference: mean30 1.614e-3 /
1.603e-3 at 1 and 3 cells (bar 7.44e-3); edge_rows 3.31e-5 / 3.08e-5 and 3.84e-5 / 3.79e-5; uniform at 300 cells 6.9e-5 / 6.7e-5.  No
defect was found."""
import math
import os

import numpy as np
import pytest
import torch

import cell_mx_families as cf
import mx_emulation as mx
from kernel_harness import Arena, fold_weight, ln_case, ps_decode, rnd, row_stats
from kernel_harness import ps_encode
from multiplexed_image_annotator_amd import synth

pytestmark = pytest.mark.gpu

D, DP, HEADS, T, HD = 384, 384, 12, 101, 32
CELLS = [1, 3, 17]
CMAX = max(CELLS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "cell_attn_mx", "gpu_tests_measured.log")
# the stage image of cell_attention_mx.hip (CellMxGeom<384, 32>)
GD, NTP, NS = 64, 4, 3
SPG, GROUPS = 3 * NS, D // GD
OFF_L6A, OFF_L6B, OFF_SC = NTP * 4096, NTP * 4096 + NTP * 1024, NTP * 4096 + NTP * 1024 + NTP * 512
WSTAGE = OFF_SC + 1024


@pytest.fixture(scope="module")
def dev():
    from multiplexed_image_annotator_amd import _lib
    return _lib.require_gpu()


def _api():
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    return check, lib(), ptr, stream_ptr


def _family(name, dev):
    m = CMAX * T
    if name == "uniform":
        z_ps, zq, g, b, dp = ln_case(m, D, 90, dev, 0.5, 1.0)
        w = rnd((3 * D, D), 93, dev, 1.0 / math.sqrt(D))
    else:
        z_ps, zq, g, b, dp = ln_case(m, D, 95, dev, 0.5, 1.0)
        u = synth.uniform(synth.stream_key(97, "cell_attn_mx/gamma"), D)
        g = torch.exp((2.0 * u - 1.0) * math.log(5.0)).to(torch.float32).to(dev)
        w = rnd((3 * D, D), 98, dev, 1.0 / math.sqrt(D))
        w[2 * D + 7] *= 50.0
    assert dp == DP
    bias = rnd((3 * D,), 94, dev, 0.1)
    w_ps, csum, bias2 = fold_weight(w, g, b, bias, DP, dev)
    rs = row_stats(z_ps, DP, m, D, dev)
    # ---- fp64 on the rounded inputs: x = rstd (z (gamma o W)^T) - rstd mean csum + bias2, then softmax attention per head
    wq = ps_decode(w_ps, D)[:3 * D]
    rstd, mean = rs[:, 0:1].double(), rs[:, 1:2].double()
    x = rstd * (zq @ wq.t()) - rstd * mean * csum.double() + bias2.double()
    qkv = x.reshape(CMAX, T, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * HD ** -0.5, dim=-1) @ qkv[2]
    ref = att.permute(0, 2, 1, 3).reshape(m, D)
    torch.cuda.synchronize()
    return {"z": z_ps, "w": w_ps, "csum": csum, "bias2": bias2, "rs": rs, "ref": ref}


@pytest.fixture(scope="module")
def families(dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _family(name, dev)
        return cache[name]
    return get


def _run_new(f, cells, dev, first=0, capacity=24 << 20):
    """the pack hook and the kernel hook on cells [first, first + cells) of the family, every buffer inside an arena of 0xFF bytes and the
    image and the output prefilled with 0xFF: (arena, image, output)"""
    check, lib, ptr, stream_ptr = _api()
    a = Arena(dev, 0xFF, capacity=capacity)
    rows = slice(first * T, (first + cells) * T)
    z, w = a.put(f["z"][rows]), a.put(f["w"])
    csum, bias2, rs = a.put(f["csum"]), a.put(f["bias2"]), a.put(f["rs"][rows])
    img = a.empty((lib.ribca_test_cell_attention_mx_image_bytes(D),), torch.uint8)
    out = a.empty((cells * T, 2 * DP), torch.int16)
    check(lib.ribca_test_cell_attention_mx_pack(ptr(w), 2 * DP, D, ptr(img), stream_ptr()), "pack")
    check(lib.ribca_test_cell_attention_mx(ptr(z), 2 * DP, ptr(img), cells, D, ptr(bias2), ptr(csum), ptr(rs), ptr(out), 2 * DP, stream_ptr()),
          "cell attention mx")
    torch.cuda.synchronize()
    assert torch.equal(z, f["z"][rows]) and torch.equal(w, f["w"]) and torch.equal(rs, f["rs"][rows])      # inputs are read only
    return a, img, out


def _run_pair(f, cells, dev):
    """the unfused MX pair on the same inputs: MX3 planes of the rows, the MX weight image, the qkv GEMM on the MX kernel, the attention kernel"""
    check, lib, ptr, stream_ptr = _api()
    m = cells * T
    a_hi = torch.zeros((m, DP), dtype=torch.int16, device=dev)
    a_l8 = torch.zeros((m, DP), dtype=torch.uint8, device=dev)
    a_sc = torch.zeros((m, DP // 32), dtype=torch.uint8, device=dev)
    wh = torch.zeros(lib.ribca_test_mx_weight_bytes(3 * D, DP, 0), dtype=torch.uint8, device=dev)
    wx = torch.zeros(lib.ribca_test_mx_weight_bytes(3 * D, DP, 1), dtype=torch.uint8, device=dev)
    q = torch.zeros((cells, HEADS, 112, 2 * HD), dtype=torch.int16, device=dev)
    k, vt = torch.zeros_like(q), torch.zeros_like(q)
    out = torch.zeros((m, 2 * DP), dtype=torch.int16, device=dev)
    check(lib.ribca_test_qkv_attention_mx(ptr(f["z"]), 2 * DP, ptr(f["w"]), 2 * DP, cells, D, DP, ptr(f["bias2"]), ptr(f["csum"]), ptr(f["rs"]),
                                          ptr(a_hi), ptr(a_l8), ptr(a_sc), ptr(wh), ptr(wx), ptr(q), ptr(k), ptr(vt), ptr(out), 2 * DP, stream_ptr()),
          "unfused mx pair")
    torch.cuda.synchronize()
    return out


def _err(f, cells, out):
    return (ps_decode(out, D) - f["ref"][:cells * T]).abs().max().item()


@pytest.mark.parametrize("family", ["uniform", "heavy"])
@pytest.mark.parametrize("cells", CELLS)
def test_accuracy_and_contract(dev, families, family, cells):
    f = families(family)
    a, img, out = _run_new(f, cells, dev)
    new, old = _err(f, cells, out), _err(f, cells, _run_pair(f, cells, dev))
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as log:
        log.write(f"D={D} {family} cells={cells}: max |out - fp64| new {new:.3e}  unfused MX pair {old:.3e}  bound {2.0 * old:.3e}\n")
    print(f"[measured] cell_attention_mx {family} cells={cells}: new {new:.3e} pair {old:.3e}")
    assert a.bands_intact()
    assert torch.isfinite(ps_decode(out, D)).all()
    # ---- two identical launches: identical bits (of the image as well)
    _, img_b, out_b = _run_new(f, cells, dev)
    assert torch.equal(img_b, img) and torch.equal(out_b, out)
    # ---- accuracy: at most twice the error of the unfused MX pair on the same inputs against the same reference
    assert new <= 2.0 * old, (new, old)


@pytest.mark.parametrize("family", ["uniform", "heavy"])
def test_a_cell_alone_has_the_bits_it_has_among_17(dev, families, family):
    f = families(family)
    _, _, out_all = _run_new(f, CMAX, dev)
    for c in (0, 5, CMAX - 1):
        _, _, out_one = _run_new(f, 1, dev, first=c)
        assert torch.equal(out_one, out_all[c * T:(c + 1) * T]), c
    _, _, out_3 = _run_new(f, 3, dev)
    assert torch.equal(out_3, out_all[:3 * T])


# ------------------------------------------------------------------------------- row families, the kernel's own operands as the reference
EMU_CELLS = [1, 3]
EMU_CMAX = max(EMU_CELLS)
MANY = 300            # more workgroups than the 256 CUs


def _ps_halves(buf, k):
    """packed-split [R, 2 Kp] int16 -> (hi, lo) float16 arrays [R, k] on the host"""
    r = buf.shape[0]
    h = buf.view(torch.float16).view(r, -1, 2, 8)
    return h[:, :, 0, :].reshape(r, -1)[:, :k].cpu().numpy(), h[:, :, 1, :].reshape(r, -1)[:, :k].cpu().numpy()


def _rows_family(name, cells, dev):
    """a row family of tests/cell_mx_families.py with the weights, gains and biases of `uniform`; the same record as _family's"""
    m = cells * T
    if name == "mean30":
        z_ps, zq, g, b, dp = ln_case(m, D, 90, dev, 30.0, 1.0)
    else:
        _, _, g, b, dp = ln_case(1, D, 90, dev, 0.5, 1.0)        # (gains and shifts do not depend on the row count)
        z_ps = ps_encode(cf.rows_f32(name, m).to(dev), dp)
        zq = ps_decode(z_ps, D)
    assert dp == DP
    w = rnd((3 * D, D), 93, dev, 1.0 / math.sqrt(D))
    bias = rnd((3 * D,), 94, dev, 0.1)
    w_ps, csum, bias2 = fold_weight(w, g, b, bias, DP, dev)
    rs = row_stats(z_ps, DP, m, D, dev)
    wq = ps_decode(w_ps, D)[:3 * D]
    rstd, mean = rs[:, 0:1].double(), rs[:, 1:2].double()
    x = rstd * (zq @ wq.t()) - rstd * mean * csum.double() + bias2.double()
    qkv = x.reshape(cells, T, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * HD ** -0.5, dim=-1) @ qkv[2]
    ref = att.permute(0, 2, 1, 3).reshape(m, D)
    torch.cuda.synchronize()
    return {"z": z_ps, "w": w_ps, "csum": csum, "bias2": bias2, "rs": rs, "ref": ref}


@pytest.fixture(scope="module")
def emulated(dev, families):
    """per family: (the record of the inputs, fp64 attention on the per-cell kernel's emulated product, the same on the unfused pair's)
    for EMU_CMAX cells; a cell's rows depend on that cell alone, so the first cells * T rows serve every smaller case"""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        f = families(name) if name in ("uniform", "heavy") else _rows_family(name, EMU_CMAX, dev)
        m = EMU_CMAX * T
        z_hi, z_lo = _ps_halves(f["z"][:m], D)
        # the rows the kernels read are the rows tests/test_mx_format.py examined on the host
        h_hi, h_lo = cf.split_host(cf.rows_f32(name, m).numpy())
        assert np.array_equal(z_hi.view(np.uint16), h_hi.view(np.uint16)) and np.array_equal(z_lo.view(np.uint16), h_lo.view(np.uint16))
        w_hi, w_lo = _ps_halves(f["w"][:3 * D], D)
        rstd, mean = f["rs"][:m, 0:1].double(), f["rs"][:m, 1:2].double()
        refs = []
        for prod in cf.qkv_products(z_hi, z_lo, w_hi, w_lo):
            x = rstd * torch.from_numpy(prod).to(dev) - rstd * mean * f["csum"].double() + f["bias2"].double()
            qkv = x.reshape(EMU_CMAX, T, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
            att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * HD ** -0.5, dim=-1) @ qkv[2]
            refs.append(att.permute(0, 2, 1, 3).reshape(m, D))
        cache[name] = (f, refs[0], refs[1])
        return cache[name]
    return get


def _log(line):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as log:
        log.write(line + "\n")
    print("[measured] cell_attention_mx " + line)


@pytest.mark.parametrize("family", cf.ROW_FAMILIES)
@pytest.mark.parametrize("cells", EMU_CELLS)
def test_against_the_emulated_operands(dev, emulated, family, cells):
    """either kernel against fp64 on ITS OWN quantised operands (fp32 arithmetic is all that separates them): the new kernel's distance may
    be at most twice the unfused pair's; against the exact reference: the pair's criterion for mean30 (and the pair's own absolute bar),
    figures only for edge_rows"""
    f, ref_new, ref_pair = emulated(family)
    m = cells * T
    a, _, out = _run_new(f, cells, dev)
    got, old = ps_decode(out, D), ps_decode(_run_pair(f, cells, dev), D)
    assert a.bands_intact()
    assert torch.isfinite(got).all()
    e_new_emu, e_pair_emu = (got - ref_new[:m]).abs().max().item(), (old - ref_pair[:m]).abs().max().item()
    e_new, e_pair = (got - f["ref"][:m]).abs().max().item(), (old - f["ref"][:m]).abs().max().item()
    _log(f"D={D} {family} cells={cells}: max |out - fp64 of its own emulated operands| new {e_new_emu:.3e}  unfused MX pair {e_pair_emu:.3e}  "
         f"bound {2.0 * e_pair_emu:.3e};  max |out - fp64| new {e_new:.3e}  unfused MX pair {e_pair:.3e}")
    assert e_new_emu <= 2.0 * e_pair_emu, (e_new_emu, e_pair_emu)
    if family == "mean30":
        assert e_new <= 2.0 * e_pair, (e_new, e_pair)
        assert e_new < (4e-5 + 2e-4) * (1.0 + 30.0), e_new      # the bar of tests/test_gpu_mx.py::test_qkv_attention_mx at |mean| / std = 30


def test_more_workgroups_than_cus(dev):
    """300 cells of `uniform`: the arena contract, the exact-reference criterion against the pair, and four cells alone"""
    f = _rows_family("uniform", MANY, dev)
    a, _, out = _run_new(f, MANY, dev, capacity=128 << 20)
    assert a.bands_intact()
    assert torch.isfinite(ps_decode(out, D)).all()
    new, old = _err(f, MANY, out), _err(f, MANY, _run_pair(f, MANY, dev))
    _log(f"D={D} uniform cells={MANY}: max |out - fp64| new {new:.3e}  unfused MX pair {old:.3e}  bound {2.0 * old:.3e}")
    for c in (0, 255, 256, MANY - 1):
        _, _, out_one = _run_new(f, 1, dev, first=c)
        assert torch.equal(out_one, out[c * T:(c + 1) * T]), c
    assert new <= 2.0 * old, (new, old)


def _fp6_codes(v, negative):
    """e2m3 codes (sign | 2 exponent bits | 3 mantissa bits) of values already on the e2m3 grid; the sign bit is the source's, zero included"""
    a = np.abs(v)
    e = np.where(a >= 1.0, np.floor(np.log2(np.maximum(a, 1.0))) + 1, 0).astype(np.int64)
    mant = np.where(e == 0, a * 8.0, (a / 2.0 ** np.maximum(e - 1, 0) - 1.0) * 8.0)
    assert np.array_equal(mant, np.rint(mant)) and mant.max() <= 7 and e.max() <= 3
    return (negative.astype(np.int64) << 5) | (e << 3) | mant.astype(np.int64)


def _emulate_image(w_ps):
    """the stage image from the packed-split weight [>= 3 D][2 DP] (host), with the rules of tests/mx_emulation.py: block = the 32 values
    k = 128 S + 32 s + 8 g + j of one row; hi fragments copied, lo as e2m3 under its own exponent (largest magnitude in [4, 8)), scale
    bytes sl, sh = max(exponent field, 1) + 110"""
    f16 = w_ps.cpu().numpy().view(np.float16).reshape(w_ps.shape[0], -1, 2, 8)
    hi = np.ascontiguousarray(f16[:, :, 0, :]).reshape(w_ps.shape[0], -1)[:, :D]      # [n, k]
    lo = np.ascontiguousarray(f16[:, :, 1, :]).reshape(w_ps.shape[0], -1)[:, :D]
    img = np.zeros((GROUPS * SPG, WSTAGE), np.uint8)
    lane = np.arange(64)
    r16, g = lane & 15, lane >> 4
    for stage in range(GROUPS * SPG):
        hg, rem = divmod(stage, SPG)
        S, part = divmod(rem, 3)
        st = img[stage]
        for jt in range(NTP):
            n = part * D + hg * GD + 16 * jt + r16                                      # [64]
            k = 128 * S + 32 * np.arange(4)[None, :, None] + 8 * g[:, None, None] + np.arange(8)[None, None, :]      # [64, 4, 8]
            bh, bl = hi[n[:, None, None], k], lo[n[:, None, None], k]                      # float16 [64, 4, 8]
            for t in range(4):
                st[(jt * 4 + t) * 1024:(jt * 4 + t + 1) * 1024] = np.ascontiguousarray(bh[:, t, :]).view(np.uint8).reshape(-1)
            l32 = bl.reshape(64, 32)
            deq = mx.fp6_image(l32)                                                        # dequantised float64
            el = np.maximum(mx.f16_exp_field(np.abs(l32)).max(axis=1), 1)
            eh = np.maximum(mx.f16_exp_field(np.abs(bh.reshape(64, 32))).max(axis=1), 1)
            codes = _fp6_codes(deq / 2.0 ** (el.astype(np.float64) - 17)[:, None], np.signbit(l32))
            bits = np.zeros(64, dtype=object)
            for i in range(32):
                bits = bits | (codes[:, i].astype(object) << (6 * i))                      # element i at bits 6 i .. 6 i + 5 of 192
            by = np.array([[(int(b) >> (8 * q)) & 0xFF for q in range(24)] for b in bits], np.uint8)
            st[OFF_L6A + jt * 1024:OFF_L6A + (jt + 1) * 1024] = by[:, :16].reshape(-1)
            st[OFF_L6B + jt * 512:OFF_L6B + (jt + 1) * 512] = by[:, 16:].reshape(-1)
            st[OFF_SC + lane * 16 + 2 * jt] = (el + 110).astype(np.uint8)
            st[OFF_SC + lane * 16 + 2 * jt + 1] = (eh + 110).astype(np.uint8)
    return img.reshape(-1)


@pytest.mark.parametrize("family", ["uniform", "heavy"])
def test_weight_image_bit_for_bit(dev, families, family):
    check, lib, ptr, stream_ptr = _api()
    f = families(family)
    assert lib.ribca_test_cell_attention_mx_image_bytes(D) == GROUPS * SPG * WSTAGE
    _, img, _ = _run_new(f, 1, dev)
    got, want = img.cpu().numpy(), _emulate_image(f["w"])
    diff = np.flatnonzero(got != want)
    print(f"[measured] cell_attention_mx image {family}: {diff.size} of {got.size} bytes differ",
          [(int(i) // WSTAGE, int(i) % WSTAGE, int(got[i]), int(want[i])) for i in diff[:8]])
    assert diff.size == 0


def test_refuses_other_widths(dev):
    check, lib, ptr, stream_ptr = _api()
    t = torch.zeros(4096, dtype=torch.int16, device=dev)
    for d in (144, 288, 576):
        assert lib.ribca_test_cell_attention_mx_image_bytes(d) == 0
        assert lib.ribca_test_cell_attention_mx_pack(ptr(t), 2 * d, d, ptr(t), stream_ptr()) != 0
        assert lib.ribca_test_cell_attention_mx(ptr(t), 2 * d, ptr(t), 1, d, ptr(t), ptr(t), ptr(t), ptr(t), 2 * d, stream_ptr()) != 0
