"""CPU tests of the MX3 operand format and of the MX product's arithmetic as tests/mx_emulation.py states them (the GPU tests compare the
kernels bit for bit with that module; these tests pin the module itself: the formats against exhaustive code tables, the format's
invariants, and the scheme's error against the exact product -- the bound the GPU test asserts, derived here without a GPU)."""
import numpy as np
import pytest

import cell_mx_families as cf
import mx_emulation as mx


def _e4m3_table():
    codes = np.arange(256, dtype=np.uint8)
    vals = mx.e4m3_decode(codes)
    keep = (codes & 0x7f) != 0x7f                     # 0x7f / 0xff are the NaN codes
    return np.unique(vals[keep])


def _e2m3_table():
    out = []
    for s in (1.0, -1.0):
        for e in range(4):
            for m in range(8):
                out.append(s * (m / 8.0 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1)))
    return np.unique(np.array(out))


def test_e4m3_round_is_nearest_even_on_the_code_table():
    """every representable value is a fixed point; between two neighbours the nearer one wins and the midpoint goes to the even code"""
    t = _e4m3_table()
    assert t.max() == 448.0 and t.min() == -448.0 and 2.0 ** -9 in t
    np.testing.assert_array_equal(mx.e4m3_round(t), t)
    pos = t[t >= 0]
    lo, hi = pos[:-1], pos[1:]
    np.testing.assert_array_equal(mx.e4m3_round(lo + 0.25 * (hi - lo)), lo)
    np.testing.assert_array_equal(mx.e4m3_round(lo + 0.75 * (hi - lo)), hi)
    mid = mx.e4m3_round(0.5 * (lo + hi))
    # index parity in the sorted non-negative table = parity of the code's mantissa LSB
    even = np.where(np.arange(len(lo)) % 2 == 0, lo, hi)
    np.testing.assert_array_equal(mid, even)


def test_e2m3_round_saturates_and_matches_the_code_table():
    t = _e2m3_table()
    assert t.max() == 7.5 and 0.125 in t
    np.testing.assert_array_equal(mx.e2m3_round(t), t)
    assert mx.e2m3_round(np.array([7.8, 100.0, -1e6])).tolist() == [7.5, 7.5, -7.5]
    x = np.linspace(-7.5, 7.5, 4001)
    r = mx.e2m3_round(x)
    assert np.all(np.isin(r, t))
    nearest = t[np.abs(x[:, None] - t[None, :]).argmin(axis=1)]
    ties = np.isclose(np.abs(x[:, None] - t[None, :]).min(axis=1) * 2, np.diff(t).min()) | (np.abs(r - x) == np.abs(nearest - x))
    assert np.all((r == nearest) | ties)


def test_hi_plane_permutation():
    """column c = 32 g + 8 s + j of a 128-column group sits at 32 s + 8 g + j: a permutation of every group, identity across groups"""
    c = np.arange(640)
    p = mx.hi_pos(c)
    assert np.array_equal(np.sort(p), c)
    assert np.array_equal(p // 128, c // 128)
    g, s, j = (c % 128) // 32, (c % 32) // 8, c % 8
    assert np.array_equal(p % 128, 32 * s + 8 * g + j)
    # what the layout is for: lane group g of sub-step s reads 8 contiguous elements, a lane's four sub-steps are 32 consecutive columns
    for grp in range(4):
        cols = np.concatenate([np.where((p % 128 >= 32 * sub + 8 * grp) & (p % 128 < 32 * sub + 8 * grp + 8) & (c < 128))[0] for sub in range(4)])
        assert np.array_equal(cols, np.arange(32 * grp, 32 * grp + 32))


@pytest.mark.parametrize("spread", [1.0, 1e-3, 3e3])
def test_pack_act_invariants(spread):
    """scale rule (lo / scale never reaches the e4m3 range limit: the hardware conversion does not saturate), reconstruction error of
    hi + lo' against x (2^-4 of |lo| <= 2^-16 of the block's largest magnitude), zero and subnormal blocks"""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((64, 256)) * spread * np.exp(rng.standard_normal((64, 1)))).astype(np.float32)
    x[1, :32] = 0.0
    x[2] *= 1e-7 / spread
    x = np.clip(x, -65504, 65504)
    hi = x.astype(np.float16)
    lo = x.astype(np.float64) - hi.astype(np.float64)
    plane, lo_q, q, sl = mx.pack_act(hi, lo)
    assert np.abs(q).max() <= 256.0
    assert sl.min() >= 94 and sl.max() <= 124
    assert np.array_equal(plane[:, mx.hi_pos(np.arange(256))], hi)
    blockmax = np.abs(hi.astype(np.float64)).reshape(64, 8, 32).max(axis=2)
    err = np.abs(hi.astype(np.float64) + lo_q - x.astype(np.float64)).reshape(64, 8, 32).max(axis=2)
    # lo <= half an ulp of hi <= 2^-11 blockmax; e4m3 keeps 4 significant bits (relative 2^-4); subnormal e4m3 step 2^-9 of the scale
    scale = 2.0 ** (sl.astype(np.float64) - 127)
    assert np.all(err <= 2.0 ** -15 * np.maximum(blockmax, 2.0 ** -14) + scale * 2.0 ** -10)


@pytest.mark.parametrize("m,n,k", [(24, 48, 128), (16, 96, 640), (8, 48, 2304)])
def test_scheme_error_against_exact_product(m, n, k):
    """fp16 hi * hi + (A lo as e4m3) x (W hi as e2m3) + (A hi as e2m3) x (W lo as e2m3), every primed operand block-scaled per 32 k:
    each correction operand keeps 4 significant bits (relative error <= 2^-4) and multiplies a factor <= 2^-11 of the product, and the
    lo * lo term (2^-22) is dropped: |error| <= sum_k |a w| * (2 * 2^-15 + 2^-22) in the worst case -- the GPU test's 3e-5 bound --
    and a random walk in practice"""
    rng = np.random.default_rng(11)
    a = (rng.standard_normal((m, k)) * np.exp(rng.standard_normal((m, 1)))).astype(np.float32)
    a = np.where(rng.random((m, k)) > 0.5, a * 8.0, a).astype(np.float32)
    w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    a_hi, w_hi = a.astype(np.float16), w.astype(np.float16)
    a_lo = a.astype(np.float64) - a_hi.astype(np.float64)
    w_lo16 = (w.astype(np.float64) - w_hi.astype(np.float64)).astype(np.float16)
    _, a_lo_q, _, _ = mx.pack_act(a_hi, a_lo)
    got = mx.gemm(a_hi, a_lo_q, w_hi, w_lo16)
    exact = a.astype(np.float64) @ w.astype(np.float64).T
    scale = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    rel = (np.abs(got - exact) / scale).max()
    assert rel < 3e-5, rel
    assert rel > 1e-8          # the scheme is not exact: a zero here would mean the emulation dropped a rounding
    # hi * hi alone is 2^-11 class per term (a random walk over k): the corrections buy more than a decimal digit
    rel_hh = (np.abs(a_hi.astype(np.float64) @ w_hi.astype(np.float64).T - exact) / scale).max()
    assert rel_hh > 8 * rel


def _cell_gemm_literal(a_hi16, a_lo, w_hi16, w_lo16):
    """the per-cell kernel's three products stated block by block: for every (row, 128-k step S, lane group g) the 32 values
    k = 128 S + 32 s + 8 g + j (s = 0 .. 3, j = 0 .. 7) share one scale -- no permutation, no reshape"""
    def ef_of(v16):
        return max(int(mx.f16_exp_field(np.abs(v16)).max()), 1)

    m, kk = a_hi16.shape
    n = w_hi16.shape[0]
    a_lo_q, a_hi_q = np.zeros((m, kk)), np.zeros((m, kk))
    w_hi_q, w_lo_q = np.zeros((n, kk)), np.zeros((n, kk))
    for S in range(kk // 128):
        for g in range(4):
            k = np.array([128 * S + 32 * s + 8 * g + j for s in range(4) for j in range(8)])
            for r in range(m):
                ef = ef_of(a_hi16[r, k])
                sl, sh = 2.0 ** (ef + 93 - 127), 2.0 ** (ef + 110 - 127)
                a_lo_q[r, k] = mx.e4m3_round(a_lo[r, k] / sl) * sl
                a_hi_q[r, k] = mx.e2m3_round(a_hi16[r, k].astype(np.float64) / sh) * sh
            for c in range(n):
                sh, sl = 2.0 ** (ef_of(w_hi16[c, k]) + 110 - 127), 2.0 ** (ef_of(w_lo16[c, k]) + 110 - 127)
                w_hi_q[c, k] = mx.e2m3_round(w_hi16[c, k].astype(np.float64) / sh) * sh
                w_lo_q[c, k] = mx.e2m3_round(w_lo16[c, k].astype(np.float64) / sl) * sl
    return a_hi16.astype(np.float64) @ w_hi16.astype(np.float64).T + a_lo_q @ w_hi_q.T + a_hi_q @ w_lo_q.T


def test_cell_gemm_is_the_literal_block_statement():
    """mx.cell_gemm (gemm under the column permutation hi_pos) against loops over (row, S, g) that gather k = 128 S + 32 s + 8 g + j: 7 rows
    x 48 columns of W x K = 384, rows with an outlier per 8 k, an all-zero 128-k step and fp16-subnormal hi among them.  Both sides are the
    same float64 sums of the same terms in another order: 1e-12 of sum |a w| is 10^4 roundings' worth."""
    rng = np.random.default_rng(23)
    a = (rng.standard_normal((7, 384)) * np.exp(rng.standard_normal((7, 1)))).astype(np.float32)
    a[1, 5::8] *= 4096.0
    a[2, 128:256] = 0.0
    a[3] *= 1e-6
    a[4, [5, 13, 21, 29]] *= 4096.0
    w = (rng.standard_normal((48, 384)) / np.sqrt(384) * np.exp(rng.standard_normal((1, 384)))).astype(np.float32)
    a_hi, a_lo16 = cf.split_host(a)
    w_hi, w_lo16 = cf.split_host(w)
    a_lo = a_lo16.astype(np.float64)
    got, want = mx.cell_gemm(a_hi, a_lo, w_hi, w_lo16), _cell_gemm_literal(a_hi, a_lo, w_hi, w_lo16)
    scale = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    assert np.all(np.abs(got - want) <= 1e-12 * scale), (np.abs(got - want) / scale).max()
    # the grouping matters: with 32 consecutive k per block (gemm_mx.hip) the same operands give another product
    _, lo_q, _, _ = mx.pack_act(a_hi, a_lo)
    other = mx.gemm(a_hi, lo_q, w_hi, w_lo16)
    assert (np.abs(other - want) / scale).max() > 1e-9


@pytest.mark.parametrize("family", cf.ROW_FAMILIES)
def test_cell_families_never_saturate_e4m3(family):
    """the token rows of tests/test_gpu_cell_attention_mx.py: under the scale blocks of either kernel |A lo / scale| <= 256 (the hardware
    conversion never reaches e4m3's 448), and edge_rows has what it is there for"""
    m = 3 * cf.T
    hi, lo = cf.split_host(cf.rows_f32(family, m).numpy())
    for cell_blocks in (True, False):
        q, ef = cf.lo_codes(hi, lo, cell_blocks)
        assert np.abs(q).max() <= 256.0, (family, cell_blocks, np.abs(q).max())
    if family == "edge_rows":
        q, ef = cf.lo_codes(hi, lo, True)                       # ef: [m][12], block 4 S + g
        assert np.all(ef[1::16, 4:8] == 0) and np.all(hi[1::16, 128:256] == 0)      # the clamp max(ef, 1) is taken in every block of S = 1
        sub = (np.abs(hi[2::16]) < 2.0 ** -14) & (hi[2::16] != 0)
        assert sub.all(axis=1).any() and (sub.any(axis=1) & ~sub.all(axis=1)).any()   # rows subnormal throughout, and rows that mix
        assert (np.abs(hi) == 65504).any()                      # saturated outliers: lo = 0 there
        assert np.all(lo[np.abs(hi) == 65504] == 0)
        # the 16 tokens of a wave (rows 16 w .. 16 w + 15 of a cell) do not share a scale byte: at least 4 distinct ones in every wave's block 0
        for c in range(3):
            for wv in range(6):
                assert len(set(ef[c * cf.T + 16 * wv:c * cf.T + 16 * wv + 16, 0].tolist())) >= 4, (c, wv)
        # rows 0 and T - 1 of cell 0 are the rows of `uniform`
        u_hi, u_lo = cf.split_host(cf.rows_f32("uniform", m).numpy())
        assert np.array_equal(hi[[0, cf.T - 1]], u_hi[[0, cf.T - 1]]) and np.array_equal(lo[[0, cf.T - 1]], u_lo[[0, cf.T - 1]])
