"""What tests/test_gpu_attention_families.py and tests/test_attention_families_host.py share: the input families of the all-row attention
kernels, the conditions each family must meet on the fp64 reference, the reference itself, and the error bound derived from the operand
buffers.  Plain torch in fp64, no kernel and no device of its own: every function works on whatever device its tensors live on."""
import torch

FAMILIES = ["gaussian", "sharp", "far_negative", "far_positive", "wk0"]
SHARP_GAIN = 16.0
FAR_BIAS = 7.0
FAR_SCORE = 104.0      # exp(-104) < 2^-149: fp32 exp of a raw score beyond it is 0 (or inf) without the row maximum


def apply_family(family, w, bias, d):
    """the family's edit of the qkv weight [3 d][d] and bias [3 d] (rows 0 .. d - 1: q, d .. 2 d - 1: k), on copies"""
    w, bias = w.clone(), bias.clone()
    if family == "sharp":
        w[:d] *= SHARP_GAIN
        bias[:d] *= SHARP_GAIN
    elif family == "far_negative":
        bias[:d] = FAR_BIAS
        bias[d:2 * d] = -FAR_BIAS
    elif family == "far_positive":
        bias[:d] = FAR_BIAS
        bias[d:2 * d] = FAR_BIAS
    elif family == "wk0":
        w[d:2 * d] = 0.0
    else:
        assert family == "gaussian", family
    return w, bias


def split_heads(qkv, cells, t, heads):
    """qkv rows [cells * t][3 d] -> (q scaled by hd^-0.5, k, v), each [cells][heads][t][hd]"""
    hd = qkv.shape[1] // (3 * heads)
    x = qkv.reshape(cells, t, 3, heads, hd).permute(2, 0, 3, 1, 4)
    return x[0] * hd ** -0.5, x[1], x[2]


def attention(qs, kk, vv):
    """(scores, probabilities, output [cells][heads][t][hd]) of softmax(qs kk^T) vv"""
    s = qs @ kk.transpose(-1, -2)
    p = torch.softmax(s, dim=-1)
    return s, p, p @ vv


def merge_heads(o):
    """[cells][heads][t][hd] -> rows [cells * t][heads * hd]"""
    c, h, t, hd = o.shape
    return o.permute(0, 2, 1, 3).reshape(c * t, h * hd)


def check_family(family, s, p, o, vv):
    """the family's condition on the fp64 reference (asserted before any kernel result is looked at): a generator that drifts fails here"""
    t = s.shape[-1]
    if family == "sharp":
        top = p.max(dim=-1).values
        assert top.median().item() >= 0.9, ("sharp: median top-1 probability", top.median().item())
        hit = torch.bincount(s.argmax(dim=-1).reshape(-1), minlength=t)
        assert bool(torch.all(hit > 0)), ("sharp: keys that are no row's argmax", torch.nonzero(hit == 0).reshape(-1).tolist())
    elif family == "far_negative":
        assert s.max().item() <= -FAR_SCORE, ("far_negative: largest score", s.max().item())
    elif family == "far_positive":
        assert s.min().item() >= FAR_SCORE, ("far_positive: smallest score", s.min().item())
    elif family == "wk0":
        flat = vv.mean(dim=2, keepdim=True).expand_as(o)
        assert (o - flat).abs().max().item() <= 1e-12 * flat.abs().max().item(), "wk0: the reference is not the plain mean of v"


def error_bound(qs, kk, vv, dq, dk, dv):
    """Bound on |kernel output - fp64 output| per element [cells][heads][t][hd], and the score error E_s per query row it rests on.

    qs, kk, vv: the fp64 operands (q pre-scaled); dq, dk, dv: |operand buffer - fp64 operand|, what the attention kernel was really given.
      score      s_ij = sum_d q_id k_jd computed from the buffers: |ds_ij| <= sum_d (|dq||k| + |q||dk| + |dq||dk|), plus the kernel's own
                 arithmetic -- three fp16 passes that drop lo * lo (2^-22 of every product), a chain of fp32 MFMA accumulations, the fma in
                 front of exp2 and exp2 itself, together 2^-21 of (sum_d |q k| + the row's score spread, the range the exponent covers)
      softmax    a score error within +-E moves every probability by a factor inside exp(+-2 E), so
                 |do_id| <= 2 E max_j |v_jd - o_id|  (sum_j p_j (v_j - o) = 0 takes the common part out); E < 0.5 is asserted by the caller
      P V        v as given (max_j |dv_jd|: a convex combination of the errors), p split into fp16 hi + lo (2^-25 absolute below 2^-14) and
                 t fp32 accumulations: t 2^-24 max_j |v_jd|; the output row's own split and the dropped lo * lo: 2^-22 |o|
      store      the packed-split output has an absolute floor the relative term misses: where the lo half is an fp16 subnormal (quantum
                 2^-24) the stored value is off by up to 2^-25 whatever |o| is (test_gpu_kernels.test_pack_roundtrip states the format's
                 error as 2^-23 |x| + 2^-25).  Seen at W_k = 0, T = 2: o = 6.7e-4 between v = -3.2e-3 and 4.6e-3, the kernel exactly
                 2^-25 from the exact output of its own operands"""
    s, _, o = attention(qs, kk, vv)
    t = s.shape[-1]
    ka = kk.abs().transpose(-1, -2)
    es = (dq @ ka + qs.abs() @ dk.transpose(-1, -2) + dq @ dk.transpose(-1, -2)).max(dim=-1).values
    es = es + 2.0 ** -21 * ((qs.abs() @ ka).max(dim=-1).values + (s.max(dim=-1).values - s.min(dim=-1).values))
    vmax, vmin = vv.max(dim=2, keepdim=True).values, vv.min(dim=2, keepdim=True).values
    dev = torch.maximum(vmax - o, o - vmin)                                  # max_j |v_jd - o_id|
    bound = (2.0 * es[..., None] * dev + dv.max(dim=2, keepdim=True).values + t * 2.0 ** -24 * vv.abs().max(dim=2, keepdim=True).values
             + 2.0 ** -22 * o.abs() + 2.0 ** -25)
    return bound, es


def v_spread(vv):
    """the yardstick a bound must stay far below to mean anything: the range of v over the case"""
    return (vv.max() - vv.min()).item()


# ------------------------------------------------------------------------------------------------ defects, applied to the REFERENCE
def pad_keys(t):
    """pad keys of the kernels' last 16-key tile"""
    return (t + 15) // 16 * 16 - t


def defect_pad_in_max_and_sum(qs, kk, vv):
    """pad key rows arrive as zeros and score 0: here they are left unmasked, in the row maximum and in the sum (their v is zero)"""
    s = qs @ kk.transpose(-1, -2)
    n = pad_keys(s.shape[-1])
    s = torch.cat((s, s.new_zeros(s.shape[:-1] + (n,))), dim=-1)
    v = torch.cat((vv, vv.new_zeros(vv.shape[:2] + (n, vv.shape[-1]))), dim=2)
    return torch.softmax(s, dim=-1) @ v


def defect_maximum_before_mask(qs, kk, vv):
    """the row maximum is taken while the pad keys still score 0, then they are masked; fp32 exp as in the kernels"""
    s = qs @ kk.transpose(-1, -2)
    mx = s.max(dim=-1, keepdim=True).values
    if pad_keys(s.shape[-1]) > 0:
        mx = mx.clamp(min=0.0)
    e = torch.exp((s - mx).to(torch.float32)).double()
    return (e @ vv) / e.sum(dim=-1, keepdim=True)


def defect_normalise_over_tile(qs, kk, vv):
    """the maximum over the real keys, but the normaliser runs over all 16 NT keys of the tiles (pads score 0)"""
    s = qs @ kk.transpose(-1, -2)
    mx = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - mx)
    return (e @ vv) / (e.sum(dim=-1, keepdim=True) + pad_keys(s.shape[-1]) * torch.exp(-mx))


def defect_exp_without_maximum(qs, kk, vv):
    """fp32 exp of the raw score, no row maximum subtracted"""
    s = qs @ kk.transpose(-1, -2)
    e = torch.exp(s.to(torch.float32)).double()
    return (e @ vv) / e.sum(dim=-1, keepdim=True)


def defect_last_key_dropped(qs, kk, vv):
    """the last real key never takes part"""
    return torch.softmax(qs @ kk[:, :, :-1].transpose(-1, -2), dim=-1) @ vv[:, :, :-1]


def operand_error_model(x_abs, w_abs, bias_abs, scale=1.0):
    """|operand - fp64| of a value produced by the fp16x3 GEMM and stored packed-split, for the host tests (on the GPU the buffers are
    measured): four roundings' worth (2^-22) of sum_k |x_k w_k| + |bias| -- the three passes drop lo * lo at 2^-22 of every product, the
    fp32 accumulation and the hi + lo split of the result are below that; hardware measured 2.6e-6 (1 + |x|) at K <= 576"""
    return 2.0 ** -22 * (x_abs @ w_abs.t() + bias_abs) * scale
