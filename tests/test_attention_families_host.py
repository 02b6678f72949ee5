"""The input families of tests/test_gpu_attention_families.py catch what they are for -- shown without a GPU: each named defect is applied
to the fp64 REFERENCE (never to a kernel), and for the family aimed at it the defective output must differ from the true one by at least
ten times the bound the GPU test asserts (attention_families.error_bound, with the operand errors of the fp16x3 product modelled instead of
measured).  Token counts 2 (one real key beside the CLS), 16 (no pad key at all: the pad defects must vanish), 8 / 9 and 101."""
import math

import pytest
import torch

import attention_families as af
from multiplexed_image_annotator_amd import synth

# (D, heads, T, cells): the imputer's two geometries and the narrowest / widest classifier
SHAPES = [(768, 12, 2, 7), (768, 12, 9, 7), (768, 12, 16, 7), (512, 8, 8, 7), (512, 8, 16, 7), (144, 12, 101, 1), (576, 12, 101, 1)]
# defect -> the families that must expose it
TARGETS = {
    "pad_in_max_and_sum": (af.defect_pad_in_max_and_sum, ["far_negative", "gaussian"]),
    "maximum_before_mask": (af.defect_maximum_before_mask, ["far_negative"]),
    "normalise_over_tile": (af.defect_normalise_over_tile, ["wk0", "far_negative"]),
    "exp_without_maximum": (af.defect_exp_without_maximum, ["far_negative", "far_positive"]),
    "last_key_dropped": (af.defect_last_key_dropped, ["sharp", "wk0"]),
}
PAD_DEFECTS = ("pad_in_max_and_sum", "maximum_before_mask", "normalise_over_tile")


def _rnd(shape, seed, scale=1.0):
    n = int(torch.tensor(shape).prod())
    return (synth.approx_normal(synth.stream_key(seed, "t"), n).reshape(shape) * scale).to(torch.float32)


_CACHE = {}


def _case(d, heads, t, cells, family):
    """fp64 operands of one case, the true output, the bound of the GPU test (family condition asserted)"""
    key = (d, heads, t, cells, family)
    if key not in _CACHE:
        m = cells * t
        x = _rnd((m, d), 1100 + d).double()
        w, bias = af.apply_family(family, _rnd((3 * d, d), 1103 + d, 1.0 / math.sqrt(d)), _rnd((3 * d,), 1104 + d, 0.1), d)
        w, bias = w.double(), bias.double()
        qs, kk, vv = af.split_heads(x @ w.t() + bias, cells, t, heads)
        s, p, o = af.attention(qs, kk, vv)
        af.check_family(family, s, p, o, vv)
        dq, dk, dv = af.split_heads(af.operand_error_model(x.abs(), w.abs(), bias.abs()), cells, t, heads)
        bound, es = af.error_bound(qs, kk, vv, dq, dk, dv)
        assert es.max().item() < 0.5 and bound.max().item() < 0.05 * af.v_spread(vv)      # the bound the GPU test would assert has its power here
        _CACHE[key] = (qs, kk, vv, o, bound)
    return _CACHE[key]


def _gap(bad, o, bound):
    """largest |defective - true| / bound; a non-finite defective output is an infinite gap"""
    if not torch.isfinite(bad).all():
        return math.inf
    return ((bad - o).abs() / bound).max().item()


@pytest.mark.parametrize("d,heads,t,cells", SHAPES)
@pytest.mark.parametrize("defect", list(TARGETS))
def test_family_exposes_defect(defect, d, heads, t, cells):
    fn, families = TARGETS[defect]
    for family in families:
        qs, kk, vv, o, bound = _case(d, heads, t, cells, family)
        gap = _gap(fn(qs, kk, vv), o, bound)
        if defect in PAD_DEFECTS and af.pad_keys(t) == 0:
            assert gap <= 1e-3, (defect, family, t, gap)      # no pad key: the defect is no defect (fp64 rounding of another evaluation order)
        else:
            assert gap >= 10.0, (defect, family, t, gap)


@pytest.mark.parametrize("d,heads,t,cells", SHAPES)
def test_gaussian_family_is_blind(d, heads, t, cells):
    """why the families exist: with scores of order 1 the maximum defects are invisible -- the baseline family passes a kernel that takes the
    row maximum before masking the pads or takes none at all"""
    qs, kk, vv, o, bound = _case(d, heads, t, cells, "gaussian")
    for defect in ("maximum_before_mask", "exp_without_maximum"):
        assert _gap(TARGETS[defect][0](qs, kk, vv), o, bound) <= 1.0, defect


def test_bound_terms_scale_as_derived():
    """error_bound: no operand error leaves the kernel's own terms; doubling dq, dk doubles the operand part of E_s (to first order)"""
    qs, kk, vv, o, _ = _case(512, 8, 8, 7, "sharp")
    z = torch.zeros_like(qs)
    b0, e0 = af.error_bound(qs, kk, vv, z, z, z)
    s = qs @ kk.transpose(-1, -2)
    own = 2.0 ** -21 * ((qs.abs() @ kk.abs().transpose(-1, -2)).max(-1).values + s.max(-1).values - s.min(-1).values)
    assert torch.allclose(e0, own, rtol=1e-12, atol=0)
    dq = torch.full_like(qs, 1e-6)
    _, e1 = af.error_bound(qs, kk, vv, dq, z, z)
    _, e2 = af.error_bound(qs, kk, vv, 2 * dq, z, z)
    assert torch.allclose(e2 - e0, 2 * (e1 - e0), rtol=1e-9, atol=0)
    assert torch.all(b0 >= 8 * 2.0 ** -24 * vv.abs().max(dim=2, keepdim=True).values)
