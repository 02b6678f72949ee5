"""cell_mlp.hip: proj + residual, norm2, fc1, GELU, fc2 + residual of a 144-wide block in one kernel, through its hook.

Accuracy: the reference is fp64 torch on the same packed-split-rounded inputs; the yardstick is the path the kernel replaces (residual
GEMM + finaliser, folded GELU GEMM, residual GEMM + finaliser through the existing hooks) on the same inputs.  Both are three-pass fp16
products with fp32 accumulation and differ only in summation order, so per case the new kernel's error may be at most TWICE the
replaced path's -- on z (relative to max |z| of the row), on rstd (relative) and on the mean (relative to max |z| of the row).
Every measured pair is appended to profiles/cell_mlp/gpu_tests_measured.log.

Measured on MI355X (new / replaced path; z and mean relative to the row's largest |z|, rstd relative), smallest and largest case per family
and the closest one:
    normal  M=1      z 3.0e-7 / 2.4e-7   rstd 1.5e-8 / 1.5e-8   mean 6.0e-9 / 9.1e-9
    normal  M=65541  z 8.7e-7 / 7.8e-7   rstd 1.2e-7 / 2.1e-7   mean 3.0e-8 / 3.6e-8
    heavy   M=1      z 6.4e-8 / 2.0e-7   rstd 3.1e-8 / 1.7e-7   mean 4.1e-10 / 1.7e-9
    heavy   M=65541  z 9.9e-7 / 8.2e-7   rstd 2.6e-7 / 4.2e-7   mean 2.4e-8 / 3.2e-8
    heavy   M=1717   z 7.09e-7 / 3.92e-7 (ratio 1.81, the closest of the 42 comparisons; docs/history.md has the anatomy of that element)

Contract: 0xFF guard bands around every buffer, rows >= M of z and of the statistics keep their prefill, columns 144 .. 159 of the written
rows stay zero, the attention output is not written, the bits do not depend on what the image scratch / the rows behind M held before,
two launches agree bit for bit, and rows 0 .. 100 computed alone equal the same rows inside a 1717-row call."""
import math
import os

import pytest
import torch

from multiplexed_image_annotator_amd import synth

pytestmark = pytest.mark.gpu

D, DP, H4 = 144, 160, 576
MS = [1, 63, 64, 65, 101, 1717, 65541]
M_MAX = max(MS)
TAIL = 64                 # prefilled rows behind M
GUARD = 4096              # bytes of 0xFF on either side of every buffer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "cell_mlp", "gpu_tests_measured.log")


@pytest.fixture(scope="module")
def dev():
    from multiplexed_image_annotator_amd import _lib
    return _lib.require_gpu()


def _api():
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    return check, lib(), ptr, stream_ptr


def ps_encode(x, kp, rows_pad=None):
    check, lib, ptr, stream_ptr = _api()
    r, k = x.shape
    out = torch.zeros((rows_pad or r, 2 * kp), dtype=torch.int16, device=x.device)
    check(lib.ribca_test_pack_weight(ptr(x.contiguous()), r, k, ptr(out), rows_pad or r, kp, stream_ptr()), "pack")
    return out


def ps_decode(buf, k):
    r = buf.shape[0]
    f = buf.view(torch.float16).view(r, -1, 2, 8)
    return (f[:, :, 0, :].reshape(r, -1).double() + f[:, :, 1, :].reshape(r, -1).double())[:, :k]


def _normal(tag, shape, scale=1.0):
    n = int(math.prod(shape))
    return (synth.approx_normal(synth.stream_key(41, "cell_mlp/" + tag), n).reshape(shape) * scale).to(torch.float32)


def _student_t3(tag, shape):
    n = int(math.prod(shape))
    num = synth.approx_normal(synth.stream_key(43, "cell_mlp/" + tag + "/n"), n)
    den = torch.zeros(n, dtype=torch.float64)
    for j in range(3):
        den += synth.approx_normal(synth.stream_key(43, "cell_mlp/" + tag + f"/d{j}"), n) ** 2
    return (num / torch.sqrt(den / 3.0).clamp_min(1e-3) / math.sqrt(3.0)).reshape(shape).to(torch.float32)


def _family(family, dev):
    """fp32 parameters and M_MAX input rows of one family, everything the kernels read in its packed form, and the fp64 reference of every
    row (a row's result depends on nothing but the row: the cases take slices)."""
    check, lib, ptr, stream_ptr = _api()
    if family == "normal":
        wp = _normal("wp", (D, D), 1.0 / math.sqrt(D))
        w1 = _normal("w1", (H4, D), 2.0 / math.sqrt(D))
        w2 = _normal("w2", (D, H4), 1.0 / math.sqrt(H4))
        gamma = _normal("g", (D,), 0.1) + 1.0
        z = _normal("z", (M_MAX, D), 2.0) + 0.5
    else:
        # Student-t(3) weights, LayerNorm gains 0.2 .. 5, one column per row 2^12 above the rest
        wp = _student_t3("wp", (D, D)) * (1.5 * math.sqrt(2.0 / (2 * D)))
        w1 = _student_t3("w1", (H4, D)) * (1.5 * math.sqrt(2.0 / (D + H4)))
        w2 = _student_t3("w2", (D, H4)) * (1.5 * math.sqrt(2.0 / (D + H4)))
        u = synth.uniform(synth.stream_key(47, "cell_mlp/gamma"), D)
        gamma = torch.exp((2.0 * u - 1.0) * math.log(5.0)).to(torch.float32)
        z = _normal("zh", (M_MAX, D), 1.0)
        col = (synth.hash_u24(synth.stream_key(47, "cell_mlp/col"), torch.arange(M_MAX, dtype=torch.int64)) % D).long()
        z[torch.arange(M_MAX), col] *= 4096.0
    beta = _normal(family + "/beta", (D,), 0.1)
    bp, b1, b2 = _normal(family + "/bp", (D,), 0.1), _normal(family + "/b1", (H4,), 0.1), _normal(family + "/b2", (D,), 0.1)
    xa = _normal(family + "/xa", (M_MAX, D), 1.0)
    wp, w1, w2, gamma, beta, bp, b1, b2, xa, z = (t.to(dev) for t in (wp, w1, w2, gamma, beta, bp, b1, b2, xa, z))
    f = {"bp": bp, "b2": b2}
    f["xa"] = ps_encode(xa, DP)
    f["z"] = ps_encode(z, DP)
    f["wp"] = ps_encode(wp, DP, lib.ribca_gemm_padded_n(D))
    f["w2"] = ps_encode(w2, H4, lib.ribca_gemm_padded_n(D))
    n1p = lib.ribca_gemm_padded_n(H4)
    f["w1"] = torch.zeros((n1p, 2 * DP), dtype=torch.int16, device=dev)
    f["c1"] = torch.zeros(H4, dtype=torch.float32, device=dev)
    f["b1"] = torch.zeros(H4, dtype=torch.float32, device=dev)
    check(lib.ribca_test_fold_weight(ptr(w1), H4, D, ptr(gamma), ptr(beta), ptr(b1), ptr(f["w1"]), n1p, DP, ptr(f["c1"]), ptr(f["b1"]),
                                     stream_ptr()), "fold")
    # the stored rows and their statistics as the forward has them in front of a block: re-centred once
    f["rs"] = torch.zeros((M_MAX, 2), dtype=torch.float32, device=dev)
    check(lib.ribca_test_row_stats(ptr(f["z"]), 2 * DP, M_MAX, D, ptr(f["rs"]), 1, stream_ptr()), "row_stats")
    # ---- fp64 on the rounded inputs
    xq, zq = ps_decode(f["xa"], D), ps_decode(f["z"], D)
    wpq, w1q, w2q = ps_decode(f["wp"], D)[:D], ps_decode(f["w1"], D)[:H4], ps_decode(f["w2"], H4)[:D]
    z1 = (zq - f["rs"][:, 1:2].double()) + xq @ wpq.t() + bp.double()
    mean2 = z1.mean(1, keepdim=True)
    rstd2 = 1.0 / torch.sqrt(z1.var(1, unbiased=False, keepdim=True) + 1e-6)
    # LayerNorm folded: (z1 - mean) rstd (gamma o W)^T + (b + W beta) -- the same function as norm2 + fc1, on the folded parameters the kernels hold
    x = rstd2 * (z1 @ w1q.t()) - rstd2 * mean2 * f["c1"].double() + f["b1"].double()
    h = torch.nn.functional.gelu(x)
    z2 = (z1 - mean2) + h @ w2q.t() + b2.double()
    f["ref_z"] = z2
    f["ref_mean"] = z2.mean(1)
    f["ref_rstd"] = 1.0 / torch.sqrt(z2.var(1, unbiased=False) + 1e-6)
    torch.cuda.synchronize()
    return f


@pytest.fixture(scope="module")
def families(dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _family(name, dev)
        return cache[name]
    return get


class Guarded:
    """a tensor in the middle of a buffer whose first and last GUARD bytes are 0xFF"""

    def __init__(self, t):
        nb = t.numel() * t.element_size()
        pad = (-nb) % 256
        self.whole = torch.full((GUARD + nb + pad + GUARD,), 0xFF, dtype=torch.uint8, device=t.device)
        self.t = self.whole[GUARD:GUARD + nb].view(t.dtype).view(t.shape)
        self.t.copy_(t)
        self.nb = nb

    def intact(self):
        return bool(torch.all(self.whole[:GUARD] == 0xFF)) and bool(torch.all(self.whole[GUARD + self.nb:] == 0xFF))


def _run_new(f, m, dev, fill=0x00, rows=None):
    """the hook on rows [0, m) (or the given row slice) of the family: (z buffer with TAIL prefilled rows behind, statistics likewise,
    every guarded buffer)"""
    check, lib, ptr, stream_ptr = _api()
    sl = rows or slice(0, m)
    pre16 = fill | (fill << 8)
    pre16 = pre16 - 65536 if pre16 >= 32768 else pre16      # the same two bytes as an int16
    z = torch.full((m + TAIL, 2 * DP), pre16, dtype=torch.int16, device=dev)
    z[:m] = f["z"][sl]
    rs = torch.full((m + TAIL, 2), float(fill) + 0.25, dtype=torch.float32, device=dev)
    rs[:m] = f["rs"][sl]
    img = torch.full((lib.ribca_test_cell_mlp_image_bytes(D) // 2,), pre16, dtype=torch.int16, device=dev)
    g = {"xa": Guarded(f["xa"][sl].clone()), "wp": Guarded(f["wp"]), "w1": Guarded(f["w1"]), "w2": Guarded(f["w2"]), "bp": Guarded(f["bp"]),
         "c1": Guarded(f["c1"]), "b1": Guarded(f["b1"]), "b2": Guarded(f["b2"]), "img": Guarded(img), "z": Guarded(z), "rs": Guarded(rs)}
    check(lib.ribca_test_cell_mlp(ptr(g["xa"].t), 2 * DP, ptr(g["wp"].t), ptr(g["w1"].t), ptr(g["w2"].t), ptr(g["bp"].t), ptr(g["c1"].t),
                                  ptr(g["b1"].t), ptr(g["b2"].t), ptr(g["img"].t), 1, ptr(g["z"].t), 2 * DP, ptr(g["rs"].t), m, D, stream_ptr()),
          "cell_mlp")
    torch.cuda.synchronize()
    return g, g["z"].t, g["rs"].t


def _run_parent(f, m, dev):
    """the replaced launches through the existing hooks: residual GEMM + finaliser, folded GELU GEMM, residual GEMM + finaliser"""
    check, lib, ptr, stream_ptr = _api()
    z = f["z"][:m].clone()
    xa = f["xa"][:m].clone()
    prev = f["rs"][:m].clone()
    part = torch.zeros((lib.ribca_test_resid_tiles(D), m, 2), dtype=torch.float32, device=dev)
    rs1 = torch.zeros((m, 2), dtype=torch.float32, device=dev)
    rs2 = torch.zeros((m, 2), dtype=torch.float32, device=dev)
    h = torch.zeros((m, 2 * H4), dtype=torch.int16, device=dev)
    check(lib.ribca_test_gemm_resid_ps(ptr(xa), 2 * DP, ptr(f["wp"]), 2 * DP, m, D, DP, ptr(f["bp"]), ptr(z), 2 * DP, ptr(part), ptr(rs1),
                                       ptr(prev), stream_ptr()), "proj")
    check(lib.ribca_test_gemm_fold(1, ptr(z), 2 * DP, ptr(f["w1"]), 2 * DP, m, H4, DP, ptr(f["b1"]), ptr(f["c1"]), ptr(rs1), ptr(h), 2 * H4,
                                   stream_ptr()), "fc1")
    check(lib.ribca_test_gemm_resid_ps(ptr(h), 2 * H4, ptr(f["w2"]), 2 * H4, m, D, H4, ptr(f["b2"]), ptr(z), 2 * DP, ptr(part), ptr(rs2),
                                       ptr(rs1), stream_ptr()), "fc2")
    torch.cuda.synchronize()
    return z, rs2


def _errors(f, m, z, rs):
    ref = f["ref_z"][:m]
    scale = ref.abs().max(1).values
    ez = ((ps_decode(z[:m], D) - ref).abs().max(1).values / scale).max().item()
    er = ((rs[:m, 0].double() - f["ref_rstd"][:m]).abs() / f["ref_rstd"][:m]).max().item()
    em = ((rs[:m, 1].double() - f["ref_mean"][:m]).abs() / scale).max().item()
    return ez, er, em


@pytest.mark.parametrize("family", ["normal", "heavy"])
@pytest.mark.parametrize("m", MS)
def test_cell_mlp_accuracy_and_contract(dev, families, family, m):
    f = families(family)
    g, z, rs = _run_new(f, m, dev)
    zp, rsp = _run_parent(f, m, dev)
    new, old = _errors(f, m, z, rs), _errors(f, m, zp, rsp)
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as log:
        log.write(f"{family} M={m}: z new {new[0]:.3e} parent {old[0]:.3e} | rstd new {new[1]:.3e} parent {old[1]:.3e} | "
                  f"mean new {new[2]:.3e} parent {old[2]:.3e}\n")
    print(f"[measured] cell_mlp {family} M={m}: new {new} parent {old}")
    # ---- contract
    assert all(b.intact() for b in g.values()), [k for k, b in g.items() if not b.intact()]
    pre16 = 0
    assert torch.all(z[m:] == pre16) and torch.all(rs[m:] == 0.25)           # rows behind M keep their prefill
    assert torch.all(ps_decode(z[:m], DP)[:, D:] == 0)                       # the K pad of the next product
    assert torch.equal(g["xa"].t, f["xa"][:m])                               # the attention output is read only
    assert torch.isfinite(rs[:m]).all()
    # ---- bits do not depend on what the scratch image or the rows behind M held, nor on the launch
    for fill in (0x7C, 0xFF):
        _, z_b, rs_b = _run_new(f, m, dev, fill=fill)
        assert torch.equal(z_b[:m], z[:m]) and torch.equal(rs_b[:m], rs[:m]), hex(fill)
    # ---- accuracy: at most twice the replaced path's error, per quantity
    for what, a, b in zip(("z", "rstd", "mean"), new, old):
        assert a <= 2.0 * b, (what, a, b)


@pytest.mark.parametrize("family", ["normal", "heavy"])
def test_cell_mlp_rows_do_not_depend_on_the_call(dev, families, family):
    """rows 0 .. 100 alone == the same rows inside the 1717-row call; a window that starts at another tile offset agrees as well"""
    f = families(family)
    _, z_all, rs_all = _run_new(f, 1717, dev)
    _, z_one, rs_one = _run_new(f, 101, dev)
    assert torch.equal(z_one[:101], z_all[:101]) and torch.equal(rs_one[:101], rs_all[:101])
    _, z_win, rs_win = _run_new(f, 101, dev, rows=slice(1000, 1101))
    assert torch.equal(z_win[:101], z_all[1000:1101]) and torch.equal(rs_win[:101], rs_all[1000:1101])


def test_cell_mlp_refuses_other_widths(dev):
    check, lib, ptr, stream_ptr = _api()
    assert lib.ribca_test_cell_mlp_image_bytes(288) == 0
    t = torch.zeros(16, dtype=torch.int16, device=dev)
    assert lib.ribca_test_cell_mlp(ptr(t), 2 * DP, ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), 1, ptr(t), 2 * DP, ptr(t), 1, 288,
                                   stream_ptr()) != 0
