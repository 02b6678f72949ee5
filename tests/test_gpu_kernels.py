"""GPU parity tests, kernel by kernel, through the C ABI (ctypes).  Floating-point kernels are compared with a plain
torch fp64/fp32 statement of the same op (tolerances written at each assert); integer / byte work with the golden
fixtures (bit-exact)."""
import json
import os

import numpy as np
import pytest
import torch

from batch_harness import neighborhood_inputs
from kernel_harness import fold_weight, ln_case, note_err, ps_decode, ps_encode, rnd, row_stats, stats_err
from multiplexed_image_annotator_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from multiplexed_image_annotator_amd import _lib
    return _lib.require_gpu()


def _ops():
    from multiplexed_image_annotator_amd import ops
    return ops


def test_pack_roundtrip(dev):
    x = rnd((37, 100), 1, dev)
    buf = ps_encode(x, 128, 48)
    y = ps_decode(buf, 100)
    # hi = fp16(x) (11 bits), lo = fp16(x - hi): |x - hi - lo| <= 2^-11 |lo| <= 2^-23 |x| while lo is a normal fp16; below 2^-14 lo
    # is subnormal with quantum 2^-24, i.e. an absolute error of at most 2^-25
    assert torch.all((y[:37] - x.double()).abs() <= x.double().abs() * 2.0 ** -23 + 2.0 ** -25)
    assert torch.all(y[37:] == 0) and torch.all(ps_decode(buf, 128)[:, 100:] == 0)


@pytest.mark.parametrize("d", [144, 288, 384, 576])
def test_layernorm(dev, d):
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    m = 203
    z = rnd((m, d), 2, dev, 3.0) + 0.5
    g = rnd((d,), 3, dev, 0.1) + 1.0
    b = rnd((d,), 4, dev, 0.1)
    dp = (d + 31) // 32 * 32
    out = torch.zeros((m, 2 * dp), dtype=torch.int16, device=dev)
    check(lib().ribca_test_layernorm(ptr(z), d, ptr(g), ptr(b), ptr(out), 2 * dp, m, d, stream_ptr()), "ln")
    ref = torch.nn.functional.layer_norm(z.double(), (d,), g.double(), b.double(), 1e-6)
    got = ps_decode(out, d)
    err = (got - ref).abs().max().item()
    note_err(f"layernorm d={d}", err)
    # fp32 mean / variance / affine: a handful of roundings at |y| <~ 6 (ulp 4.8e-7), then the hi+lo split (2^-23 relative)
    assert err < 3e-6, err
    assert torch.all(ps_decode(out, dp)[:, d:] == 0)


GEMM_SHAPES = [(1, 288, 288), (100, 864, 288), (128, 1152, 288), (300, 288, 1152), (257, 144, 144), (130, 432, 144),
               (77, 576, 2304), (200, 1728, 576), (129, 384, 384), (64, 64, 64),
               # >= 256 tiles of 256 x 96: the persistent streaming kernel (1 and 2 epilogue sub-tiles per K step), ragged last m-tile
               (11100, 576, 576), (22100, 288, 288), (11011, 576, 2304), (16500, 384, 384), (40000, 576, 576), (70001, 288, 288)]


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_residual(dev, m, n, k):
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    kp = (k + 31) // 32 * 32
    a = rnd((m, k), 5, dev)
    w = rnd((n, k), 6, dev, 1.0 / np.sqrt(k))
    bias = rnd((n,), 7, dev, 0.1)
    z0 = rnd((m, n), 8, dev)
    a_ps = ps_encode(a, kp)
    w_ps = ps_encode(w, kp, lib().ribca_gemm_padded_n(n))
    z = z0.clone()
    check(lib().ribca_test_gemm(0, ptr(a_ps), 2 * kp, ptr(w_ps), 2 * kp, m, n, kp, ptr(bias), ptr(z), n, stream_ptr()), "gemm")
    ref = z0.double() + a.double() @ w.double().t() + bias.double()
    err = (z.double() - ref).abs().max().item()
    note_err(f"gemm_residual {m}x{n}x{k}", err)
    # Operands enter at 2^-23 relative (hi+lo fp16), so what is left is the fp32 accumulation of K products of O(K^-1/2) terms
    # plus the residual add at |z| <~ 5: std ~ sqrt(K) 2^-24 |partial sum| ~ 3e-6 at K = 2304; 7 sigma over <= 2e7 outputs.
    # Measured on MI355X (RIBCA_TEST_REPORT=1): 0.8e-6 (K = 64) ... 7.8e-6 (K = 2304).
    assert err < 2e-5, err


@pytest.mark.parametrize("m,n,k", [(150, 1152, 288), (101, 576, 144), (260, 2304, 576), (7001, 1152, 288), (3000, 2304, 576), (20000, 1152, 288), (12000, 2304, 576)])
def test_gemm_gelu(dev, m, n, k):
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    kp = (k + 31) // 32 * 32
    a = rnd((m, k), 9, dev)
    w = rnd((n, k), 10, dev, 2.0 / np.sqrt(k))
    bias = rnd((n,), 11, dev, 0.1)
    a_ps = ps_encode(a, kp)
    w_ps = ps_encode(w, kp, lib().ribca_gemm_padded_n(n))
    out = torch.zeros((m, 2 * n), dtype=torch.int16, device=dev)
    check(lib().ribca_test_gemm(1, ptr(a_ps), 2 * kp, ptr(w_ps), 2 * kp, m, n, kp, ptr(bias), ptr(out), 2 * n, stream_ptr()), "gemm")
    ref = torch.nn.functional.gelu(a.double() @ w.double().t() + bias.double())
    err = (ps_decode(out, n) - ref).abs().max().item()
    note_err(f"gemm_gelu {m}x{n}x{k}", err)
    # as test_gemm_residual (pre-activations ~ N(0, 4)), GELU slope <= 1.13, erf_fast 6e-7 absolute x |x| / 2; measured 3.6e-6 ... 6.6e-6
    assert err < 2e-5, err


def test_split_operand_range(dev):
    """the fp16 hi+lo split has a range the bf16 split did not.  (a) activations of 1e3 ... 3e4 against small weights and
    (b) weights of 1e-5 (lo subnormal: absolute 2^-25 error per operand) still match fp64 to the documented precision;
    (c) an operand beyond 65504 saturates SILENTLY at +-65504 (finite, wrong by construction) -- pinned so that a change is noticed."""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    m, n, k = 300, 288, 288
    kp = k
    for tag, a_scale, w_scale in (("large activations", 1.0e4, 1e-3), ("tiny weights", 1.0, 1e-5)):
        a = rnd((m, k), 70, dev, a_scale)
        w = rnd((n, k), 71, dev, w_scale)
        bias = torch.zeros(n, device=dev)
        z = torch.zeros((m, n), device=dev)
        a_ps, w_ps = ps_encode(a, kp), ps_encode(w, kp, lib().ribca_gemm_padded_n(n))      # named: they must outlive the launch
        check(lib().ribca_test_gemm(0, ptr(a_ps), 2 * kp, ptr(w_ps), 2 * kp, m, n, kp, ptr(bias), ptr(z), n, stream_ptr()), "gemm")
        ref = a.double() @ w.double().t()
        mag = a.double().abs() @ w.double().abs().t()
        # per product: 2^-22 relative (dropped lo*lo) + the operands' split error: relative 2^-23 where lo is normal, absolute 2^-25 below
        bound = mag * 2.0 ** -20 + (a.double().abs().sum(1, keepdim=True) * 2.0 ** -25 + 2.0 ** -25 * w.double().abs().sum(1)[None, :]) + 1e-12
        err = ((z.double() - ref).abs() / bound).max().item()
        note_err(f"split operand range: {tag} (error / bound)", err)
        assert err < 1.0, (tag, err)
    a = rnd((m, k), 72, dev, 1.0)
    a[:, 0] = 1.0e6                                  # beyond fp16: clamps to 65504
    w = rnd((n, k), 73, dev, 0.05)
    bias = torch.zeros(n, device=dev)
    z = torch.zeros((m, n), device=dev)
    a_ps, w_ps = ps_encode(a, kp), ps_encode(w, kp, lib().ribca_gemm_padded_n(n))
    check(lib().ribca_test_gemm(0, ptr(a_ps), 2 * kp, ptr(w_ps), 2 * kp, m, n, kp, ptr(bias), ptr(z), n, stream_ptr()), "gemm")
    assert torch.isfinite(z).all()
    a_sat = a.clone()
    a_sat[:, 0] = 65504.0
    ref = a_sat.double() @ w.double().t()
    # the saturated operand meets weights of ~0.05 whose lo halves are subnormal (absolute 2^-25): 65504 x 2^-25 = 2e-3 per product
    assert (z.double() - ref).abs().max().item() < 65504 * 2.0 ** -23


@pytest.mark.parametrize("n,k", [(432, 144), (1152, 288), (1536, 384), (2304, 576)])
def test_fold_weight(dev, n, k):
    """gamma o W packed, csum = row sums of the PACKED values (what the MFMAs multiply the row mean with), bias2 = b + W beta"""
    kp = (k + 31) // 32 * 32
    w = rnd((n, k), 40, dev, 1.0 / np.sqrt(k))
    g = rnd((k,), 41, dev, 0.1) + 1.0
    b = rnd((k,), 42, dev, 0.1)
    bias = rnd((n,), 43, dev, 0.1)
    w_ps, csum, bias2 = fold_weight(w, g, b, bias, kp, dev)
    wq = ps_decode(w_ps, kp)
    ref = (g * w).double()                                           # the kernel rounds gamma * w to fp32 once, then splits
    assert torch.all((wq[:n, :k] - ref).abs() <= ref.abs() * 2.0 ** -23 + 2.0 ** -25)
    assert torch.all(wq[n:] == 0) and torch.all(wq[:, k:] == 0)
    # fp64 sums rounded once to fp32
    assert torch.all((csum.double() - wq[:n].sum(1)).abs() <= wq[:n].sum(1).abs() * 2.0 ** -23 + 1e-12)
    ref_b = bias.double() + w.double() @ b.double()
    assert torch.all((bias2.double() - ref_b).abs() <= ref_b.abs() * 2.0 ** -23 + 1e-9)


@pytest.mark.parametrize("d", [144, 288, 384, 576, 768])
@pytest.mark.parametrize("mean,std", [(0.5, 3.0), (30.0, 1.0), (-300.0, 2.0)])
def test_row_stats(dev, d, mean, std):
    m = 203
    z_ps, zq, _, _, dp = ln_case(m, d, 44, dev, mean, std, row_scale=(mean == 0.5))
    rs = row_stats(z_ps, dp, m, d, dev)
    # two-pass fp32 statistics of exactly representable inputs: the mean carries 2^-24 |mu| (relative to the spread: x |mu| / sigma),
    # the centred squares then see that error twice
    e1, e2 = stats_err(rs, zq)
    note_err(f"row_stats d={d} mean {mean}", max(e1, e2))
    assert e1 < 4e-7 and e2 < 4e-7, (e1, e2)
    assert torch.equal(ps_decode(z_ps, d), zq)                      # untouched
    # re-centred: the rows are rewritten as z - mean (|stored mean| << spread) and the statistics are those of what is stored
    rs2 = row_stats(z_ps, dp, m, d, dev, recentre=True)
    z2 = ps_decode(z_ps, d)
    e1, e2 = stats_err(rs2, z2)
    assert e1 < 4e-7 and e2 < 4e-7, (e1, e2)
    sig = zq.std(1, unbiased=False)
    assert torch.all(z2.mean(1).abs() <= 1e-6 * sig + 2.0 ** -21 * zq.mean(1).abs())      # the fp32 mean itself: a few ulps of |mean|
    # the same LayerNorm input: fp32 z - mean of nearby numbers is (nearly) exact, the re-split costs 2^-23 of the CENTRED value
    ln1 = torch.nn.functional.layer_norm(zq, (d,), None, None, 1e-6)
    ln2 = torch.nn.functional.layer_norm(z2, (d,), None, None, 1e-6)
    assert (ln1 - ln2).abs().max().item() < 5e-6
    assert torch.all(ps_decode(z_ps, dp)[:, d:] == 0)


RESID_PS_SHAPES = [(1, 288, 288), (300, 288, 1152), (257, 144, 144), (130, 144, 576), (77, 576, 2304), (129, 384, 384), (515, 768, 768),
                   (11100, 576, 576), (22100, 288, 288), (16500, 384, 1536), (40000, 144, 144)]
# the two-workgroups-per-CU form with the residual tile riding the A ring (what the full blocks run where it is faster): every tile width
# (96 / 128 / 64, and 128 x 192 tiles where N % 192 == 0), a single row, ragged last row tiles, a last column tile half behind N (144, 240), short and long K, one K step
RESID_ZK_SHAPES = [(1, 288, 288), (300, 144, 576), (909, 576, 576), (193, 384, 384), (4100, 256, 512), (129, 192, 64), (11100, 576, 576), (22100, 288, 288), (16500, 384, 1536), (40000, 144, 144), (4100, 144, 576), (5000, 768, 768),
                   (4097, 64, 64), (4200, 192, 96), (4300, 240, 32), (6000, 576, 2304), (4096, 288, 1152)]


@pytest.mark.parametrize("m,n,k,duo", [s + (False,) for s in RESID_PS_SHAPES] + [s + (True,) for s in RESID_ZK_SHAPES])
@pytest.mark.parametrize("mean,recentre", [(0.3, False), (40.0, False), (40.0, True)])
def test_gemm_resid_ps(dev, m, n, k, duo, mean, recentre):
    """proj / fc2 of the classifiers: z (packed-split) += A W^T + b in place, plus (rstd, -mean rstd) of the NEW rows out of the
    epilogue's per-tile pairs (2 ... 6 column tiles; duo: 3 ... 24 wave column blocks), also for rows whose mean dwarfs their spread"""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    kp = (k + 31) // 32 * 32
    a = rnd((m, k), 5, dev)
    w = rnd((n, k), 6, dev, 1.0 / np.sqrt(k))
    bias = rnd((n,), 7, dev, 0.1)
    npd = (n + 31) // 32 * 32
    z0 = rnd((m, n), 8, dev) + mean
    a_ps = ps_encode(a, kp)
    w_ps = ps_encode(w, kp, lib().ribca_gemm_padded_n(n))
    z_ps = ps_encode(z0, npd)
    z0q = ps_decode(z_ps, n)
    aq, wq = ps_decode(a_ps, k), ps_decode(w_ps, k)[:n]
    tiles = lib().ribca_test_resid_part_rows(n) if duo else lib().ribca_test_resid_tiles(n)
    part = torch.zeros((tiles, m, 2), dtype=torch.float32, device=dev)
    rs = torch.zeros((m, 2), dtype=torch.float32, device=dev)
    # the forward hands the epilogue the (rstd, mean) the stored rows had: it subtracts that mean (re-centring)
    prev = row_stats(z_ps, npd, m, n, dev) if recentre else None
    if duo:
        wf = torch.zeros_like(w_ps)
        check(lib().ribca_test_gemm_resid_ps_duo(ptr(a_ps), 2 * kp, ptr(w_ps), 2 * kp, m, n, kp, ptr(bias), ptr(wf), ptr(z_ps), 2 * npd, ptr(part),
                                                 ptr(rs), ptr(prev) if recentre else None, stream_ptr()), "resid_ps duo")
    else:
        check(lib().ribca_test_gemm_resid_ps(ptr(a_ps), 2 * kp, ptr(w_ps), 2 * kp, m, n, kp, ptr(bias), ptr(z_ps), 2 * npd, ptr(part), ptr(rs),
                                             ptr(prev) if recentre else None, stream_ptr()), "resid_ps")
    ref = z0q + aq @ wq.t() + bias.double()
    if recentre:
        ref = ref - prev[:, 1:2].double()
    got = ps_decode(z_ps, n)
    err = ((got - ref).abs() / (1.0 + ref.abs())).max().item()
    note_err(f"gemm_resid_ps {m}x{n}x{k} mean {mean} recentre {recentre} duo {duo}", err)
    # as test_gemm_residual, plus the re-split of the new row (2^-23 relative); re-centred rows: z - mean is one more fp32 rounding
    # at |z| <= 45 (2^-24 x 45 = 2.7e-6 absolute)
    assert err < 2e-5, err
    assert torch.all(ps_decode(z_ps, npd)[:, n:] == 0)
    if recentre:
        assert got.mean(1).abs().max().item() < 1.0        # the offset is gone: what is left is the mean of the update itself
    # the statistics describe the rows that were STORED
    e1, e2 = stats_err(rs, got)
    note_err(f"resid_ps stats {m}x{n}x{k} mean {mean}", max(e1, e2))
    assert e1 < 1e-6 and e2 < 1e-6, (e1, e2)


@pytest.mark.parametrize("m,d", [(150, 288), (101, 144), (260, 576), (7001, 288), (5000, 576), (20000, 288), (12000, 384), (9000, 144)])
@pytest.mark.parametrize("mean,std", [(0.5, 3.0), (30.0, 1.0)])
def test_gemm_fold_gelu(dev, m, d, mean, std):
    """norm2 -> mlp.fc1 folded: gelu(LN(z) W^T + b) from the packed-split z, the folded weight and the row statistics; the
    two-workgroups-per-CU kernel the forward uses for M >= 4096 must give the same bits as the one-workgroup kernel"""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    n = 4 * d
    z_ps, zq, g, b, dp = ln_case(m, d, 50, dev, mean, std, row_scale=(mean == 0.5))
    w = rnd((n, d), 53, dev, 2.0 / np.sqrt(d))
    bias = rnd((n,), 54, dev, 0.1)
    w_ps, csum, bias2 = fold_weight(w, g, b, bias, dp, dev)
    rs = row_stats(z_ps, dp, m, d, dev)
    out = torch.zeros((m, 2 * n), dtype=torch.int16, device=dev)
    check(lib().ribca_test_gemm_fold(1, ptr(z_ps), 2 * dp, ptr(w_ps), 2 * dp, m, n, dp, ptr(bias2), ptr(csum), ptr(rs), ptr(out), 2 * n,
                                     stream_ptr()), "gemm_fold")
    ln = torch.nn.functional.layer_norm(zq, (d,), g.double(), b.double(), 1e-6)
    ref = torch.nn.functional.gelu(ln @ w.double().t() + bias.double())
    err = (ps_decode(out, n) - ref).abs().max().item()
    note_err(f"gemm_fold_gelu {m}x{n}x{d} mean {mean}", err)
    # test_gemm_gelu's bound (2e-5) times the amplification of the cancellation rstd (acc - mean c): products carry 2^-24 relative
    # to |z| ~ |mean|, the LayerNorm output lives on the scale sigma
    assert err < 2e-5 * (1.0 + abs(mean) / std), err
    if m >= 4096:
        wf = torch.zeros_like(w_ps)
        out2 = torch.zeros_like(out)
        check(lib().ribca_test_gemm_duo_gelu(ptr(z_ps), 2 * dp, ptr(w_ps), 2 * dp, m, n, dp, ptr(bias2), ptr(csum), ptr(rs), ptr(wf), ptr(out2),
                                             2 * n, stream_ptr()), "duo fold")
        assert torch.equal(out, out2)


def test_gemm_duo_bit_identical(dev):
    """gemm_duo.hip (two workgroups per CU, weights in fragment order straight to registers; the forward's mlp.fc1 kernel for
    M >= 4096) accumulates every output element in the one-workgroup kernel's order: GELU outputs must be equal bit for bit,
    ragged M and every column-tile width included."""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    for m, n, k in [(4096, 576, 144), (5000, 1152, 288), (7001, 1536, 384), (11100, 2304, 576), (4100, 64, 64), (6000, 192, 96)]:
        kp = (k + 31) // 32 * 32
        a = rnd((m, k), 9, dev)
        w = rnd((n, k), 10, dev, 2.0 / np.sqrt(k))
        bias = rnd((n,), 11, dev, 0.1)
        a_ps = ps_encode(a, kp)
        w_ps = ps_encode(w, kp, lib().ribca_gemm_padded_n(n))
        o1 = torch.zeros((m, 2 * n), dtype=torch.int16, device=dev)
        o2 = torch.zeros_like(o1)
        wf = torch.zeros_like(w_ps)
        check(lib().ribca_test_gemm(1, ptr(a_ps), 2 * kp, ptr(w_ps), 2 * kp, m, n, kp, ptr(bias), ptr(o1), 2 * n, stream_ptr()), "gemm")
        check(lib().ribca_test_gemm_duo_gelu(ptr(a_ps), 2 * kp, ptr(w_ps), 2 * kp, m, n, kp, ptr(bias), None, None, ptr(wf), ptr(o2), 2 * n,
                                             stream_ptr()), "duo")
        assert torch.equal(o1, o2), (m, n, k)


@pytest.mark.parametrize("d,cells", [(144, 3), (288, 3), (384, 3), (576, 3), (288, 130), (384, 70), (576, 131)])
@pytest.mark.parametrize("mean,std", [(0.5, 1.0), (30.0, 1.0)])
def test_qkv_attention_fold(dev, d, cells, mean, std):
    """norm1 -> attn.qkv folded + attention: against LayerNorm + qkv + softmax attention in fp64"""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    heads, ntok = 12, 101
    hd = d // heads
    hdp, hdv = (hd + 7) // 8 * 8, (hd + 15) // 16 * 16
    m = cells * ntok
    z_ps, zq, g, b, dp = ln_case(m, d, 60, dev, mean, std)
    w = rnd((3 * d, d), 63, dev, 1.0 / np.sqrt(d))
    bias = rnd((3 * d,), 64, dev, 0.1)
    w_ps, csum, bias2 = fold_weight(w, g, b, bias, dp, dev)
    rs = row_stats(z_ps, dp, m, d, dev)
    q = torch.zeros((cells, heads, 112, 2 * hdp), dtype=torch.int16, device=dev)
    k = torch.zeros_like(q)
    vt = torch.zeros_like(q)
    out = torch.zeros((m, 2 * dp), dtype=torch.int16, device=dev)
    check(lib().ribca_test_qkv_attention_fold(ptr(z_ps), 2 * dp, ptr(w_ps), 2 * dp, cells, d, dp, ptr(bias2), ptr(csum), ptr(rs), ptr(q), ptr(k),
                                              ptr(vt), ptr(out), 2 * dp, stream_ptr()), "qkv fold")
    ln = torch.nn.functional.layer_norm(zq, (d,), g.double(), b.double(), 1e-6)
    qkv = (ln @ w.double().t() + bias.double()).reshape(cells, ntok, 3, heads, hd).permute(2, 0, 3, 1, 4)
    qq, kk, vv = qkv[0], qkv[1], qkv[2]
    qd = ps_decode(q.reshape(-1, 2 * hdp), hdp).reshape(cells, heads, 112, hdp)
    kd = ps_decode(k.reshape(-1, 2 * hdp), hdp).reshape(cells, heads, 112, hdp)
    amp = 1.0 + abs(mean) / std
    assert torch.all((qd[:, :, :ntok, :hd] - qq * hd ** -0.5).abs() <= (qq.abs() + 1.0) * 1e-5 * amp)
    assert torch.all((kd[:, :, :ntok, :hd] - kk).abs() <= (kk.abs() + 1.0) * 1e-5 * amp)
    att = torch.softmax(qq @ kk.transpose(-1, -2) * hd ** -0.5, dim=-1) @ vv
    ref = att.permute(0, 2, 1, 3).reshape(m, d)
    err = (ps_decode(out, d) - ref).abs().max().item()
    note_err(f"qkv_attention_fold d={d} cells={cells} mean {mean}", err)
    assert err < 4e-5 * amp, err


@pytest.mark.parametrize("d,cells", [(144, 1), (288, 1), (384, 1), (144, 37), (288, 130), (384, 70), (288, 600)])
@pytest.mark.parametrize("mean,std", [(0.5, 1.0), (30.0, 1.0)])
def test_cell_attention_fused(dev, d, cells, mean, std):
    """cell_attention.hip: norm1 -> qkv -> attention of one cell per workgroup (q, k, v stay on chip) against LayerNorm + qkv + softmax
    attention in fp64 and against the unfused kernels on the same inputs"""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    heads, ntok = 12, 101
    hd = d // heads
    hdp = (hd + 7) // 8 * 8
    m = cells * ntok
    z_ps, zq, g, b, dp = ln_case(m, d, 80, dev, mean, std)
    w = rnd((3 * d, d), 83, dev, 1.0 / np.sqrt(d))
    bias = rnd((3 * d,), 84, dev, 0.1)
    w_ps, csum, bias2 = fold_weight(w, g, b, bias, dp, dev)
    rs = row_stats(z_ps, dp, m, d, dev)
    out = torch.zeros((m, 2 * dp), dtype=torch.int16, device=dev)
    check(lib().ribca_test_cell_attention(ptr(z_ps), 2 * dp, ptr(w_ps), 2 * dp, cells, d, ptr(bias2), ptr(csum), ptr(rs), ptr(out), 2 * dp, stream_ptr()),
          "cell attention")
    ln = torch.nn.functional.layer_norm(zq, (d,), g.double(), b.double(), 1e-6)
    qkv = (ln @ w.double().t() + bias.double()).reshape(cells, ntok, 3, heads, hd).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * hd ** -0.5, dim=-1) @ qkv[2]
    ref = att.permute(0, 2, 1, 3).reshape(m, d)
    got = ps_decode(out, d)
    err = (got - ref).abs().max().item()
    note_err(f"cell_attention_fused d={d} cells={cells} mean {mean}", err)
    assert err < 4e-5 * (1.0 + abs(mean) / std), err           # test_qkv_attention_fold's bound
    assert torch.all(ps_decode(out, dp)[:, d:] == 0)
    # the unfused pair on the same inputs: the same arithmetic up to the order of two roundings (q, k are split before / after the
    # head permutation, identical values) -- far inside the bound above
    q = torch.zeros((cells, heads, 112, 2 * hdp), dtype=torch.int16, device=dev)
    k, vt = torch.zeros_like(q), torch.zeros_like(q)
    out2 = torch.zeros_like(out)
    check(lib().ribca_test_qkv_attention_fold(ptr(z_ps), 2 * dp, ptr(w_ps), 2 * dp, cells, d, dp, ptr(bias2), ptr(csum), ptr(rs), ptr(q), ptr(k), ptr(vt),
                                              ptr(out2), 2 * dp, stream_ptr()), "unfused")
    d2 = (got - ps_decode(out2, d)).abs().max().item()
    note_err(f"cell_attention_fused vs unfused d={d}", d2)
    assert d2 < 1e-5 * (1.0 + abs(mean) / std), d2


@pytest.mark.parametrize("d,cells", [(144, 3), (288, 3), (384, 3), (576, 3), (288, 130), (384, 130), (576, 131), (288, 400)])
def test_qkv_attention(dev, d, cells):
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    heads, ntok = 12, 101
    hd = d // heads
    hdp, hdv = (hd + 7) // 8 * 8, (hd + 15) // 16 * 16       # Q/K rows are stored compactly: whole PS groups of 8 dims only
    m = cells * ntok
    dp = (d + 31) // 32 * 32
    y = rnd((m, d), 12, dev)
    w = rnd((3 * d, d), 13, dev, 1.0 / np.sqrt(d))   # q, k ~ N(0,1): scores O(1) like a trained ViT
    bias = rnd((3 * d,), 14, dev, 0.1)
    y_ps = ps_encode(y, dp)
    w_ps = ps_encode(w, dp, lib().ribca_gemm_padded_n(3 * d))
    q = torch.zeros((cells, heads, 112, 2 * hdp), dtype=torch.int16, device=dev)
    k = torch.zeros_like(q)
    vt = torch.zeros_like(q)
    out = torch.zeros((m, 2 * dp), dtype=torch.int16, device=dev)
    check(lib().ribca_test_qkv_attention(ptr(y_ps), 2 * dp, ptr(w_ps), 2 * dp, cells, d, dp, ptr(bias), ptr(q), ptr(k), ptr(vt),
                                         ptr(out), 2 * dp, stream_ptr()), "qkv+attention")
    qkv = (y.double() @ w.double().t() + bias.double()).reshape(cells, ntok, 3, heads, hd).permute(2, 0, 3, 1, 4)
    qq, kk, vv = qkv[0], qkv[1], qkv[2]
    # intermediate layouts first (localises a failure): Q rows pre-scaled, K rows, V rows
    qd = ps_decode(q.reshape(-1, 2 * hdp), hdp).reshape(cells, heads, 112, hdp)
    kd = ps_decode(k.reshape(-1, 2 * hdp), hdp).reshape(cells, heads, 112, hdp)
    def close(got, ref):   # stored as hi+lo fp16 (2^-23 relative) + fp32 accumulation of K <= 576 products (measured <= 2.6e-6 relative to 1 + |ref|)
        return bool(torch.all((got - ref).abs() <= (ref.abs() + 1.0) * 1e-5))
    assert close(qd[:, :, :ntok, :hd], qq * hd ** -0.5)
    assert close(kd[:, :, :ntok, :hd], kk)
    assert torch.all(qd[:, :, ntok:] == 0) and torch.all(qd[..., hd:] == 0)
    # V is stored row-major like K (the attention kernel transposes it out of LDS); pad rows / dims stay zero
    vd = ps_decode(vt.reshape(-1, 2 * hdp), hdp).reshape(cells, heads, 112, hdp)
    assert close(vd[:, :, :ntok, :hd], vv)
    assert torch.all(vd[:, :, ntok:] == 0) and torch.all(vd[..., hd:] == 0)
    att = torch.softmax((qq * hd ** -0.5) @ kk.transpose(-1, -2), dim=-1)
    ref = (att @ vv).transpose(1, 2).reshape(m, d)
    err = (ps_decode(out, d) - ref).abs().max().item()
    note_err(f"qkv_attention d={d} cells={cells}", err)
    note_err(f"qkv_attention d={d} q/k/v rel", max(((qd[:, :, :ntok, :hd] - qq * hd ** -0.5).abs() / ((qq * hd ** -0.5).abs() + 1)).max().item(),
                                                    ((kd[:, :, :ntok, :hd] - kk).abs() / (kk.abs() + 1)).max().item()))
    # Derived, not fitted: q, k, v reach the attention kernel with delta <= 2.6e-6 (1 + |x|) (asserted above).  A score is a sum of
    # hd <= 48 products, so |ds| <~ sqrt(hd) * 2 delta |q||k| ~ 7 * 5e-6 * 3 = 1e-4 worst case, ~1e-5 typical; softmax turns it into
    # a relative error ds on every P, and o = sum P v inherits |do| <= max|ds| * max|v - o| <~ 1e-5 * 4.  Bound 4e-5; measured
    # 1.1e-6 ... 3.1e-6 on MI355X (the round-1 bf16 split needed 2e-4 here).
    assert err < 4e-5, err
    assert torch.all(ps_decode(out, dp)[:, d:] == 0)


@pytest.mark.parametrize("name", list(synth.VIT_CONFIGS))
def test_vit_forward_vs_oracle(dev, name):
    from oracle import ref_vit
    ops = _ops()
    d, c, k = synth.VIT_CONFIGS[name]
    sd = synth.make_vit_state_dict(name, synth.SEED_BASE + 7)
    n = 21
    u = synth.uniform(synth.stream_key(5, "vitx/" + name), n * c * 1600).reshape(n, c, 40, 40).to(torch.float32)
    x = torch.where(u * 2 - 1 > 0.1, u * 2 - 1, torch.full_like(u, -1.0))
    ref = ref_vit.predict_proba(sd, x, 8)
    model = ops.VitModel(sd, dev)
    got = model.predict_proba(x.to(dev), list(range(c)), chunk_cells=8).cpu()   # 3 chunks, last one ragged
    err = (got - ref).abs().max().item()
    note_err(f"vit_forward {name}", err)
    # north-star tolerance is 1e-3 on confidences; the fp16 hi+lo split holds 2e-5 through 12 blocks (emulated on the oracle:
    # tests/precision_study.py f16x3 3.7e-6 ... 5.4e-6 over 256 cells; measured here 1.2e-6 ... 3.4e-6).  Widths whose products run as
    # fp16 hi * hi + block-scaled corrections (csrc/gemm_mx.hip: 4 D % 128 == 0) carry the 2^-16-class operand error of that scheme
    # through 12 blocks: emulated 4.3e-5 ... 9.6e-5 with EVERY product in that form (same study, rows "MX-fp8 / MX-fp6 corrections")
    assert err < (2e-5 if (4 * d) % 128 else 1.5e-4), err
    assert torch.equal(got.argmax(1), ref.argmax(1))
    got2 = model.predict_proba(x.to(dev), list(range(c)), chunk_cells=64).cpu()
    assert torch.equal(got, got2)     # chunking does not change results
    # the full-precision forward (what cells near a decision boundary are re-evaluated with): three fp16 passes whatever the width
    prec = model._forward(x.to(dev), list(range(c)), chunk_cells=8, precise=True).cpu()
    assert (prec - ref).abs().max().item() < 2e-5
    if (4 * d) % 128:
        assert torch.equal(prec, got)      # no MX pair at this width: the same kernels
    # ... and the re-evaluation itself: with a margin of 2 (every cell "near a boundary") the result is the full-precision one, bit for bit
    saved = type(model).RECHECK_MARGIN
    try:
        type(model).RECHECK_MARGIN = 2.0
        allc = model.predict_proba(x.to(dev), list(range(c)), chunk_cells=8, recheck=[]).cpu()
    finally:
        type(model).RECHECK_MARGIN = saved
    assert torch.equal(allc, prec)
    some = model.predict_proba(x.to(dev), list(range(c)), chunk_cells=8, recheck=[0.5]).cpu()
    top = ref.sort(dim=1, descending=True).values
    far = ((top[:, 0] - top[:, 1]) > 2e-3) & ((top[:, 0] - 0.5).abs() > 2e-3)
    assert torch.equal(some[far], got[far])      # cells far from every boundary keep the fast result


@pytest.mark.parametrize("name", list(synth.VIT_CONFIGS))
def test_vit_forward_heavy_tailed_weights(dev, name):
    """the precision machinery had only seen the uniform weight family.  synth.make_vit_state_dict_heavy has what
    trained ViTs have (the stand-in for reference model.py:188-239's checkpoints, which cannot be downloaded here): Student-t(3) linear
    weights, LayerNorm gains over two decades, four residual channels 50 x the rest (an |x| >> its neighbours inside the 32-wide MX blocks
    of both operands).  What must hold: confidences within the north-star 1e-3 of the fp32 oracle; labels identical wherever the
    reference's own top-2 margin exceeds twice the measured error; the full-precision forward in the fp32 reference's own class of error;
    and the premise of the margin-gated re-evaluation, |fast - full precision| <= RECHECK_MARGIN / 2.5, for the forward the model really
    uses -- a model whose load-time probe refuses its weights (ops.VitModel._calibrate_margin) runs every product at three fp16 passes, and
    the raw MX forward it was protected from is measured beside it (force_fast)."""
    from oracle import ref_vit
    ops = _ops()
    d, c, k = synth.VIT_CONFIGS[name]
    sd = synth.make_vit_state_dict_heavy(name, synth.SEED_BASE + 7, head_gain=1.5)
    n = 48
    u = synth.uniform(synth.stream_key(5, "vitx/" + name), n * c * 1600).reshape(n, c, 40, 40).to(torch.float32)
    x = torch.where(u * 2 - 1 > 0.1, u * 2 - 1, torch.full_like(u, -1.0))
    with torch.no_grad():
        sd["head.bias"] = synth.calibrate_head_bias(sd, ref_vit.forward_features(sd, x))      # every class in use: labels have teeth
    ref = ref_vit.predict_proba(sd, x, 8)
    sd64 = {key: v.double() for key, v in sd.items()}
    with torch.no_grad():
        p64 = torch.softmax(ref_vit.logits(sd64, x.double()), dim=1)
    err32 = (ref.double() - p64).abs().max().item()
    model = ops.VitModel(sd, dev)
    src = list(range(c))
    raw_mx = model._forward(x.to(dev), src, chunk_cells=16, precise=False, force_fast=True).cpu()
    fast = model._forward(x.to(dev), src, chunk_cells=16, precise=False).cpu()
    full = model._forward(x.to(dev), src, chunk_cells=16, precise=True).cpu()
    got = model.predict_proba(x.to(dev), src, chunk_cells=16, recheck=[]).cpu()
    err, err_full = (got - ref).abs().max().item(), (full - ref).abs().max().item()
    moved, moved_raw = (fast - full).abs().max().item(), (raw_mx - full).abs().max().item()
    note_err(f"vit_forward heavy-tailed {name} (fp32 vs fp64 {err32:.1e}; full precision {err_full:.1e}; probe delta {model.probe_logit_delta:.1e} (predicted worst |dp| {model.probe_predicted_dp:.1e}) -> "
             f"MX {'in use' if model.uses_mx else 'refused' if (4 * d) % 128 == 0 else 'n/a'}; |raw MX - full| {moved_raw:.1e})", err)
    assert err < 1e-3, err                                  # north star
    assert err_full < max(1e-4, 6.0 * err32), (err_full, err32)      # three fp16 passes: the fp32 reference's own class of error
    assert moved <= model.recheck_margin / 2.5, (moved, model.recheck_margin)
    if not model.fast_ok:
        assert torch.equal(fast, full)                      # a refused model runs the precise forward for every cell
    srt = ref.sort(dim=1, descending=True).values
    decided = (srt[:, 0] - srt[:, 1]) > 2.0 * err
    assert torch.equal(got.argmax(1)[decided], ref.argmax(1)[decided])
    assert len(torch.unique(ref.argmax(1))) >= 2             # not a saturated net: the outputs depend on the cell


def _large_mean_state_dict(name, c0=125.0, c1=30.0):
    """adversarial statistics for the folded LayerNorm: a shared offset on every residual row (pos_embed + c0, and + c1 from every
    attn.proj / mlp.fc2 bias so that it keeps pace with the growing spread): |row mean| / row std >= 30 at the input of every block"""
    sd = synth.make_vit_state_dict(name, synth.SEED_BASE + 7)
    sd["pos_embed"] = sd["pos_embed"] + c0
    for i in range(12):
        sd[f"blocks.{i}.attn.proj.bias"] = sd[f"blocks.{i}.attn.proj.bias"] + c1
        sd[f"blocks.{i}.mlp.fc2.bias"] = sd[f"blocks.{i}.mlp.fc2.bias"] + c1
    return sd


@pytest.mark.parametrize("name", ["nerve", "immune_base", "immune_full"])
def test_vit_forward_large_row_mean(dev, name):
    """the LayerNorm fold computes rstd (z (gamma o W)^T - mean c), whose cancellation grows with |mean| / std of
    the residual rows.  Weights with a large shared offset put every row at |mean| / std = 30 ... 65 (checked below on the fp64
    oracle); the fp32 reference itself then sits 4e-5 ... 2.4e-4 from the fp64 forward (x - mean in fp32 loses log2(|mean| / std)
    bits).  Bound: the end-to-end tolerance of the golden / config tests (E2E_TOL = 2e-4 in test_gpu_e2e.py) against the fp64
    forward, or 3x the fp32 reference's own distance from it where that is larger; always inside the north-star 1e-3; labels identical."""
    from oracle import ref_vit
    ops = _ops()
    d, c, k = synth.VIT_CONFIGS[name]
    sd = _large_mean_state_dict(name)
    n = 24
    u = synth.uniform(synth.stream_key(5, "vitx/" + name), n * c * 1600).reshape(n, c, 40, 40).to(torch.float32)
    x = torch.where(u * 2 - 1 > 0.1, u * 2 - 1, torch.full_like(u, -1.0))
    sd64 = {key: v.double() for key, v in sd.items()}
    with torch.no_grad():
        z = torch.cat((sd64["cls_token"].expand(n, -1, -1), ref_vit.patch_embed(sd64, x.double())), dim=1) + sd64["pos_embed"]
        for i in range(12):
            ratio = z.mean(-1).abs() / z.std(-1, unbiased=False)
            assert ratio.min().item() >= 30.0, (i, ratio.min().item())
            z = ref_vit.block(sd64, i, z)
        p64 = torch.softmax(ref_vit.logits(sd64, x.double()), dim=1)
    p32 = ref_vit.predict_proba(sd, x, 8)
    got = ops.VitModel(sd, dev).predict_proba(x.to(dev), list(range(c)), chunk_cells=16).cpu()
    err = (got.double() - p64).abs().max().item()
    err32 = (p32.double() - p64).abs().max().item()
    note_err(f"vit_forward large row mean {name} (fp32 reference vs fp64: {err32:.2e})", err)
    assert err < max(2e-4, 3.0 * err32) and err < 1e-3, (err, err32)
    assert torch.equal(got.argmax(1), p64.argmax(1))


def test_vit_golden_logits(dev, golden_dir):
    ops = _ops()
    g = np.load(os.path.join(golden_dir, "vit_logits.npz"))
    for name, (d, c, k) in synth.VIT_CONFIGS.items():
        sd = synth.make_vit_state_dict(name, synth.SEED_BASE + 7)
        u = synth.uniform(synth.stream_key(synth.SEED_BASE + 7, "vitx/" + name), 8 * c * 1600).reshape(8, c, 40, 40).to(torch.float32)
        x = torch.where(u * 2 - 1 > 0.1, u * 2 - 1, torch.full_like(u, -1.0))
        got = ops.VitModel(sd, dev).predict_proba(x.to(dev), list(range(c))).cpu().numpy()
        assert np.abs(got - g[name + "_probs"]).max() < 1e-4
        assert (got.argmax(1) == g[name + "_probs"].argmax(1)).all()


def test_blank_and_aliased_channels(dev):
    from oracle import ref_vit, ref_preprocess
    ops = _ops()
    name = "immune_base"
    d, c, k = synth.VIT_CONFIGS[name]
    sd = synth.make_vit_state_dict(name, 3)
    n, c_img = 5, 9
    full = (synth.uniform(synth.stream_key(6, "full"), n * c_img * 1600).reshape(n, c_img, 40, 40) * 2 - 1).to(torch.float32)
    index = [3, -1, 0, 8, -1, 2, 5]                      # first -1 blank, second -1 -> last image channel
    sel = np.stack([ref_preprocess.select_channels(full[i].numpy(), index) for i in range(n)])
    ref = ref_vit.predict_proba(sd, torch.from_numpy(sel.astype(np.float32)))
    got = ops.VitModel(sd, dev).predict_proba(full.to(dev), ops.resolve_channels(index, c_img)).cpu()
    assert (got - ref).abs().max().item() < 1e-4


# ------------------------------------------------------------------------------------------- integer / byte work
def test_label_table_golden(dev, golden_dir):
    ops = _ops()
    g = np.load(os.path.join(golden_dir, "cellpos.npz"))
    for key, mask in (("odd", g["odd_mask"]), ("example2", g["example2_mask"].astype(np.int32)),
                      ("example1", g["example1_mask"].astype(np.int32))):       # example1 = BASELINE config 1's mask (1850 cells)
        ids, tab = ops.label_table(torch.from_numpy(mask.astype(np.int32)).to(dev))
        np.testing.assert_array_equal(ids, g[key + "_ids"])
        np.testing.assert_array_equal(tab, g[key + "_table"])
    ms, _ = synth.make_mask_and_image(160, 200, 60, 1, synth.SEED_BASE + 111, want_image=False)
    ids, tab = ops.label_table(ms.to(dev))
    np.testing.assert_array_equal(ids, g["synth_ids"])
    np.testing.assert_array_equal(tab, g["synth_table"])


def test_label_table_edge_cases(dev):
    ops = _ops()
    ids, tab = ops.label_table(torch.zeros((7, 13), dtype=torch.int32, device=dev))
    assert ids.shape == (0,) and tab.shape == (0, 7)
    one = torch.zeros((3, 5), dtype=torch.int32)
    one[2, 4] = 7
    ids, tab = ops.label_table(one.to(dev))
    assert ids.tolist() == [7] and tab.tolist() == [[2, 2, 4, 4, 2, 4, 1]]
    with pytest.raises(ValueError):
        ops.label_table(torch.full((2, 2), -1, dtype=torch.int32, device=dev))


def test_label_table_matches_oracle_large(dev):
    from oracle import ref_preprocess
    ops = _ops()
    ms, _ = synth.make_mask_and_image(1000, 1001, 3000, 1, 99, want_image=False)   # W not a multiple of 8
    ids, tab = ops.label_table(ms.to(dev))
    rids, rtab = ref_preprocess.cell_table(ms.numpy())
    np.testing.assert_array_equal(ids, rids)
    np.testing.assert_array_equal(tab, rtab)


def test_channel_min(dev):
    ops = _ops()
    x = rnd((5, 97, 131), 20, dev)
    x[3] = x[3].abs() + 0.25
    np.testing.assert_array_equal(ops.channel_min(x).cpu().numpy(), x.amin(dim=(1, 2)).cpu().numpy())


def test_patches_golden(dev, golden_dir):
    ops = _ops()
    g = np.load(os.path.join(golden_dir, "patches.npz"))
    img = torch.from_numpy(g["A_image"]).to(dev)
    mask = torch.from_numpy(g["A_mask"]).to(dev)
    ids, tab = ops.label_table(mask)
    cmin = ops.channel_min(img)
    patches, avg = ops.extract_patches(img, mask, cmin, torch.from_numpy(ids.astype(np.int32)).to(dev),
                                       torch.from_numpy(tab[:, :4].astype(np.int32)).to(dev), want_avg=True)
    got = patches.cpu().numpy()
    np.testing.assert_array_equal(got, g["A_all7_patches"])             # same arithmetic, operation for operation
    inten = (avg.cpu().numpy() + 1) / 2
    np.testing.assert_allclose(inten, g["A_all7_intensity"], rtol=1e-12, atol=1e-14)   # summation order differs only
    for name in ("perm", "one_missing", "two_missing", "three"):
        idx = ops.resolve_channels(g[f"A_{name}_index"].tolist(), 7)
        sel = np.stack([got[:, s] if s >= 0 else np.full_like(got[:, 0], -1.0) for s in idx], axis=1)
        np.testing.assert_array_equal(sel, g[f"A_{name}_patches"])


def test_patches_unnormalised_golden(dev, golden_dir):
    ops = _ops()
    g = np.load(os.path.join(golden_dir, "patches.npz"))
    img = torch.from_numpy(g["B_raw"].astype(np.float32)).to(dev)      # uint16 -> fp32 is exact
    mask = torch.from_numpy(g["B_mask"]).to(dev)
    ids, tab = ops.label_table(mask)
    patches, avg = ops.extract_patches(img, mask, ops.channel_min(img), torch.from_numpy(ids.astype(np.int32)).to(dev),
                                       torch.from_numpy(tab[:, :4].astype(np.int32)).to(dev), want_avg=True)
    got = patches.cpu().numpy()[:, [2, 0, 1]]
    np.testing.assert_array_equal(got, g["B_patches"])
    np.testing.assert_allclose((avg.cpu().numpy() + 1) / 2, g["B_intensity"], rtol=1e-12)


def test_vote_golden(dev, golden_dir):
    from oracle import ref_vote
    ops = _ops()
    meta = json.load(open(os.path.join(golden_dir, "vote_cases.json")))
    arrs = np.load(os.path.join(golden_dir, "vote_cases.npz"))
    gid = {n: i for i, n in enumerate(ops.GLOBAL_NAMES)}
    n_checked = 0
    for key, m in meta.items():
        if key == "branch1":
            continue
        cname = key.split("__")[0]
        tables = []
        if m["immune"]:
            tables.append((m["immune"], arrs[f"{cname}__p_{m['immune']}"]))
        if m["struct"]:
            tables.append(("struct", arrs[f"{cname}__p_struct"]))
        if m["nerve"] and len(tables) < 2:
            tables.append(("nerve", arrs[f"{cname}__p_nerve"]))
        tc = m["type_conf"] or {n: -1 for n in ops.GLOBAL_NAMES}
        tcv = [tc[n] for n in ops.GLOBAL_NAMES]
        (ma, pa) = tables[0]
        pb = torch.from_numpy(tables[1][1]).to(dev) if len(tables) > 1 else None
        mb = [gid[c] for c in ref_vote.CLASS_NAMES[tables[1][0]]] if len(tables) > 1 else None
        lab, conf = ops.vote(torch.from_numpy(pa).to(dev), [gid[c] for c in ref_vote.CLASS_NAMES[ma]], pb, mb, tcv, m["conf"])
        labels = [ops.GLOBAL_NAMES[i] for i in lab.cpu().tolist()]
        assert labels == m["labels"], key
        np.testing.assert_array_equal(conf.cpu().numpy(), arrs[key + "__conf"])
        n_checked += 1
    assert n_checked == 44


# ------------------------------------------------------------------------------------------- whole-image normalisation
@pytest.mark.parametrize("key,src,blur,amax", [
    ("a_out_blur0", "a_in", 0, 99.8), ("a_out_blur0.3", "a_in", 0.3, 99.8), ("a_out_blur0.5", "a_in", 0.5, 99.8),
    ("a_out_blur1", "a_in", 1, 99.8), ("a_out_amax100", "a_in", 0, 100), ("b_out_blur0.3", "b_in", 0.3, 99.8),
    ("c_out_blur0", "c_in", 0, 99.8)])
def test_normalize_golden(dev, golden_dir, key, src, blur, amax):
    ops = _ops()
    g = np.load(os.path.join(golden_dir, "normalize.npz"))
    got = ops.normalize_image(g[src], blur=blur, amax=amax).cpu().numpy()
    np.testing.assert_array_equal(got, g[key])      # same operations in the same order and precision as scipy / numpy


def test_gaussian_filter_matches_scipy(dev):
    from scipy.ndimage import gaussian_filter
    ops = _ops()
    x = (rnd((2, 70, 45), 31, dev).abs() * 100).contiguous()
    for sigma, mode in ((20, "reflect"), (0.3, "reflect"), (2, "nearest"), (1, "reflect")):
        got = ops.gaussian_filter_f32(x, sigma, mode=mode).cpu().numpy()
        ref = np.stack([gaussian_filter(p, sigma, mode=mode) for p in x.cpu().numpy()])
        np.testing.assert_array_equal(got, ref)


def test_order_statistics_exact(dev):
    ops = _ops()
    x = (rnd((3, 211, 97), 32, dev).abs() * 1000).contiguous()
    x[1] = torch.floor(x[1] / 100)            # many ties
    x[2, :100] = 0
    n = 211 * 97
    xs = np.sort(x.cpu().numpy().reshape(3, -1), axis=1)
    for rank in (0, 1, n // 2, n - 2, n - 1, 12345):
        got = ops._order_statistics(x, np.full(3, rank))
        np.testing.assert_array_equal(got, xs[:, rank])


def test_normalize_large_matches_oracle(dev):
    from oracle import ref_preprocess
    ops = _ops()
    _, img = synth.make_mask_and_image(700, 900, 2500, 3, 77)
    raw = img.numpy().astype(np.uint16)
    got = ops.normalize_image(raw, blur=0.3, amax=99.8).cpu().numpy()
    np.testing.assert_array_equal(got, ref_preprocess.normalize_image(raw, blur=0.3, amax=99.8))


def test_normalize_threshold_branches_match_oracle(dev):
    """the three per-plane scalars of the finalise kernel (mode, clip, denom) must reach it un-aliased.  Planes chosen so
    that every branch of preprocess.py:228-239 differs between them: the amax percentile lies in (20, 25) (clip at t, divide by 25),
    no positive pixel at all (plane of -1), t > 25 (clip at t, divide by t), and t <= 20 (no clip, divide by max(25, max)).  The
    oracle is bit-exact against the reference's own _normalize (tests/golden/normalize.npz)."""
    from oracle import ref_preprocess
    ops = _ops()
    h, w = 256, 320
    rng = np.random.default_rng(5)
    flat = rng.integers(40, 60, (h, w)).astype(np.float64)               # background ~50, removed by the sigma-20 filter
    def plane(peak, frac):
        x = flat.copy()
        m = rng.random((h, w)) < frac
        x[m] += peak * rng.random(int(m.sum()))
        return x
    raw = np.stack([plane(24, 0.02),        # t in (20, 25): 23.2, plane maximum 32
                    np.zeros((h, w)),        # nothing positive -> -1
                    plane(4000, 0.05),       # t > 25
                    plane(8, 0.01)]          # t <= 20
                   ).astype(np.uint16)
    ref = ref_preprocess.normalize_image(raw, blur=0, amax=99.8)
    # the planes really take four different branches
    x = raw.astype(np.float32)
    from scipy.ndimage import gaussian_filter
    ts = []
    for c in range(4):
        v = np.clip(x[c] - np.minimum(gaussian_filter(x[c], 20), 125), 0, None)
        ts.append(float(np.percentile(v, 99.8)) if (v > 0).any() else None)
    assert 20 < ts[0] < 25 and ts[1] is None and ts[2] > 25 and ts[3] <= 20, ts
    got = ops.normalize_image(raw, blur=0, amax=99.8).cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    assert (got[1] == -1).all()


# ------------------------------------------------------------------------------------------- marker imputer
def _mae_inputs(panel, n, seed):
    L = synth.MAE_PANELS[panel]
    u = synth.uniform(synth.stream_key(seed, "maex/" + panel), n * L * 1600).reshape(n, L, 40, 40).to(torch.float32)
    x = u * 2 - 1
    return torch.where(x > 0.0, x, torch.full_like(x, -1.0))


@pytest.mark.parametrize("panel", ["immune_base", "immune_full"])
def test_mae_golden(dev, golden_dir, panel):
    """HIP imputer vs the reference's own MarkerImputer.impute (full-depth seeded weights)."""
    ops = _ops()
    g = np.load(os.path.join(golden_dir, "mae.npz"))
    present = g[panel + "_present"].tolist()
    seed = synth.SEED_BASE + 301
    model = ops.MaeModel(synth.make_mae_state_dict(panel, seed), dev)
    x = _mae_inputs(panel, 6, seed)
    missing = [c for c in range(x.shape[1]) if c not in present]
    x[:, missing] = -1.0
    y = model.impute(x.to(dev).contiguous(), present, chunk_cells=4).cpu()      # 2 chunks, ragged tail
    assert torch.equal(y[:, present], x[:, present])                              # kept channels bit-for-bit untouched
    err = np.abs(y[:, missing].numpy() - g[panel + "_pred"]).max()
    note_err(f"mae golden {panel} (imputed planes vs the reference's MarkerImputer)", err)
    assert err < 5e-4, err          # pixel values in [-1, 1] feed a classifier whose 1e-3 budget is on probabilities


@pytest.mark.parametrize("panel,present", [("immune_extended", [0, 1, 2, 3, 5, 6, 7, 9]), ("immune_base", [1, 2, 3, 4, 5, 6]),
                                           ("immune_full", list(range(14)))])
def test_mae_vs_oracle(dev, panel, present):
    from oracle import ref_mae
    ops = _ops()
    sd = synth.make_mae_state_dict(panel, 17, enc_depth=3, dec_depth=2)
    x = _mae_inputs(panel, 37, 18)
    ref = ref_mae.impute(sd, x, present)
    got = ops.MaeModel(sd, dev).impute(x.to(dev).contiguous(), present, chunk_cells=16).cpu()
    assert torch.equal(got[:, present], x[:, present])
    err = (got - ref).abs().max().item()
    note_err(f"mae vs oracle {panel} ({len(present)} present)", err)
    assert err < 5e-4, err


@pytest.mark.gpu
def test_vit_segment_streams_identical():
    """Splitting the cells over several HIP streams (ops.VitModel.predict_proba(streams=...)) must not change a single bit."""
    import torch
    from multiplexed_image_annotator_amd import ops, synth
    dev = torch.device("cuda:0")
    sd = synth.make_vit_state_dict("immune_base", seed=5, depth=2)
    model = ops.VitModel(sd, dev)
    g = torch.Generator().manual_seed(3)
    patches = (torch.rand((700, 9, 40, 40), generator=g) * 2 - 1).to(dev)
    src = [0, 1, 2, -1, 4, 5, 8]
    a = model.predict_proba(patches, src, chunk_cells=64, streams=1)
    b = model.predict_proba(patches, src, chunk_cells=64, streams=3)
    c = model.predict_proba(patches, src, chunk_cells=64, streams=16)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("cell_size", [20, 34, 45, 60, 67])
def test_patches_scaled_match_oracle(dev, cell_size):
    """cell_size != 30 (reference preprocess.py:78,106): crop window int(40 * cell_size / 30), soft mask on that window,
    anti-aliased nearest-neighbour resize to 40 x 40.  Bit-exact against the oracle restatement (scipy primitives)."""
    from oracle import ref_preprocess as rp
    ops = _ops()
    mask_t, raw_t = synth.make_mask_and_image(200, 230, 60, 4, seed=77, device=torch.device("cpu"))
    mask = mask_t.numpy().astype(np.int32)
    image = rp.normalize_image(raw_t.numpy(), blur=0.3, amax=99.8)
    ids, table = rp.cell_table(mask)
    sel = np.arange(len(ids))[:40]
    exp, exp_int = rp.patches_for_panel(image, mask, [0, 1, 2, 3], ids[sel], table[sel], scale=cell_size / 30.0)
    img_d = torch.from_numpy(image).to(dev)
    mask_d = torch.from_numpy(mask).to(dev)
    got, avg = ops.extract_patches(img_d, mask_d, ops.channel_min(img_d), torch.from_numpy(ids[sel].astype(np.int32)).to(dev),
                                   torch.from_numpy(table[sel, :4].astype(np.int32)).to(dev), want_avg=True,
                                   patch_size=int(40 * (cell_size / 30.0)))
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    np.testing.assert_allclose((avg.cpu().numpy() + 1) / 2, exp_int, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("cell_size", [20, 34, 45, 60])
def test_patches_scaled_golden(dev, golden_dir, cell_size):
    """Same through the C ABI against vectors produced by the reference's own _img2patches (tests/golden/make_golden.py)."""
    ops = _ops()
    g = np.load(os.path.join(golden_dir, "patches_scaled.npz"))
    img = torch.from_numpy(g["image"]).to(dev)
    mask = torch.from_numpy(g["mask"]).to(dev)
    ids, tab = ops.label_table(mask)
    patches, avg = ops.extract_patches(img, mask, ops.channel_min(img), torch.from_numpy(ids.astype(np.int32)).to(dev),
                                       torch.from_numpy(tab[:, :4].astype(np.int32)).to(dev), want_avg=True,
                                       patch_size=int(40 * (cell_size / 30.0)))
    np.testing.assert_array_equal(patches.cpu().numpy()[:, [2, 0, 1]], g[f"s{cell_size}_patches"])
    # the intensity table is per IMAGE channel (crop_cell averages every channel), not per panel channel
    np.testing.assert_allclose((avg.cpu().numpy() + 1) / 2, g[f"s{cell_size}_intensity"], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("name", ["basic", "two_model"])
def test_colorize_golden(dev, golden_dir, name):
    """ribca_colorize against the three label paintings the reference's Annotator.colorize produced (model.py:806-858)."""
    from multiplexed_image_annotator_amd import colors
    ops = _ops()
    meta = json.load(open(os.path.join(golden_dir, "e2e.json")))[name]
    conf = np.load(os.path.join(golden_dir, "e2e.npz"))[f"{name}__conf"]
    g = np.load(os.path.join(golden_dir, "colorize.npz"))
    mask, _ = synth.make_mask_and_image(meta["h"], meta["w"], meta["cells"], len(meta["markers"]), meta["seed"], want_image=False)
    mask_d = mask.to(torch.int32).to(dev)
    ids, _ = ops.label_table(mask_d)
    tidx = np.array([meta["cell_types"].index(l) for l in meta["labels"]], np.int64)
    palette = np.array(colors.get_colors(len(meta["cell_types"])), np.uint8)
    t, c, i = ops.colorize(mask_d, ids, palette[tidx], colors.confidence_colors(conf), (tidx + 1).astype(np.uint8))
    np.testing.assert_array_equal(t.cpu().numpy(), g[f"{name}__type_rgb"])
    np.testing.assert_array_equal(c.cpu().numpy(), g[f"{name}__conf_rgb"])
    np.testing.assert_array_equal(i.cpu().numpy(), g[f"{name}__type_idx"])
    # odd pixel count (tail path of the 4-pixel groups)
    sub = mask_d[:7, :9].contiguous()
    t2, c2, i2 = ops.colorize(sub, ids, palette[tidx], colors.confidence_colors(conf), (tidx + 1).astype(np.uint8))
    np.testing.assert_array_equal(t2.cpu().numpy(), g[f"{name}__type_rgb"][:7, :9])
    np.testing.assert_array_equal(i2.cpu().numpy(), g[f"{name}__type_idx"][:7, :9])


@pytest.mark.parametrize("cname", ["basic", "two_model", "big"])
def test_knn_cooccurrence_golden(dev, golden_dir, cname):
    """ribca_knn_cooccurrence vs the CSVs the reference's neighborhood_analysis wrote (scikit-learn ball tree, spatial_methods.py:13-130)."""
    from oracle import ref_spatial
    ops = _ops()
    g, x, y, types, names = neighborhood_inputs(golden_dir, cname)
    for k in (10, 25):
        m = ops.knn_cooccurrence(x, y, types, len(names), k).cpu().numpy().astype(np.float64)
        assert ref_spatial.csv_text(ref_spatial.normalize_rows(m), names) == g[f"{cname}__k{k}"]
        assert m.sum() == len(x) * (k - 1)
    if cname == "big":
        raw = ops.knn_cooccurrence(x, y, types, len(names), 10).cpu().numpy().astype(np.float64)
        assert ref_spatial.csv_text(raw, names) == g["big_raw_k10"]
        acc = ops.knn_cooccurrence(x, y, types, len(names), 25)
        acc = ops.knn_cooccurrence(x[:700], y[:700], types[:700], len(names), 25, out=acc)
        assert ref_spatial.csv_text(ref_spatial.normalize_rows(acc.cpu().numpy().astype(np.float64)), names) == g["big_integrated_k25"]
        with pytest.raises(ValueError):
            ops.knn_cooccurrence(x[:5], y[:5], types[:5], len(names), 10)


def test_tissue_compositions_golden(dev, golden_dir):
    """ribca_knn_compositions (k = 201 via an LDS candidate buffer) vs the compositions matrix of the reference's tissue_region_partition."""
    ops = _ops()
    g = np.load(os.path.join(golden_dir, "tissue.npz"))
    _, x, y, types, _ = neighborhood_inputs(golden_dir, "big")
    got = ops.knn_compositions(x, y, types, int(types.max()) + 1)
    np.testing.assert_array_equal(got, g["compositions"])
    # small neighbourhoods agree with the register-list kernel
    c10 = ops.knn_compositions(x, y, types, 6, sizes=(9,))
    m = np.zeros((6, 6))
    np.add.at(m, (np.repeat(types, 6), np.tile(np.arange(6), len(types))), (c10 * 9).reshape(-1))
    np.testing.assert_allclose(m, ops.knn_cooccurrence(x, y, types, 6, 10).cpu().numpy(), atol=1e-6)
    with pytest.raises(ValueError):
        ops.knn_compositions(x[:100], y[:100], types[:100], 6)
    # many rounds of the candidate buffer without a re-sort in between (the path a small tile never takes)
    rng = np.random.default_rng(5)
    n = 9000
    px, py, pt = rng.random(n) * 1000, rng.random(n) * 800, rng.integers(0, 7, n)
    big = ops.knn_compositions(px, py, pt, 7)
    for j in rng.integers(0, n, 150):
        d = (px - px[j]) ** 2 + (py - py[j]) ** 2
        order = np.lexsort((np.arange(n), d))[1:201]
        row = np.concatenate([np.bincount(pt[order[:s]], minlength=7) / float(s) for s in ops.TISSUE_NEIGHBOURHOODS])
        np.testing.assert_array_equal(big[j], row)
