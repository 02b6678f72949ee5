"""The identity behind csrc/cls_attention.hip, on the CPU: the attention output of token 0 needs neither K nor V of any token.

With y_j = (z_j - mean_j) rstd_j, W' = gamma o W_qkv, b' = b + W_qkv beta and S_h the rows of head h:
    q_h = W'_q[S_h] y_0 + b'_q[S_h];   g_h = scale W'_k[S_h]^T q_h;   p_hj = softmax_j(g_h . y_j);   ybar_h = sum_j p_hj y_j;
    o[S_h] = W'_v[S_h] ybar_h + b'_v[S_h]
Every term that is constant over the keys (q_h . b'_k) cancels in the softmax, and sum_j p_hj = 1 moves the v bias out of the sum.  In fp64
the restated form agrees with LayerNorm + qkv + softmax attention to rounding (asserted: 1e-12 of the largest output); in fp32 it is no
worse conditioned than the full form (printed: both errors against fp64), so a GPU bound of twice the replaced path's error
(tests/test_gpu_cls_attention.py) does not ask for the impossible."""
import math

import pytest
import torch

HEADS, TOKENS = 12, 101


def _case(d, seed):
    """101 residual rows with one token row 50 times larger than the rest, LayerNorm gains 0.2 .. 5, a k bias of +30"""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(TOKENS, d, generator=gen, dtype=torch.float64) * 2.0 + 0.5
    z[37] *= 50.0
    gamma = torch.exp((2.0 * torch.rand(d, generator=gen, dtype=torch.float64) - 1.0) * math.log(5.0))
    beta = torch.randn(d, generator=gen, dtype=torch.float64) * 0.1
    w = torch.randn(3 * d, d, generator=gen, dtype=torch.float64) / math.sqrt(d)
    b = torch.randn(3 * d, generator=gen, dtype=torch.float64) * 0.1
    b[d:2 * d] += 30.0
    return z, gamma, beta, w, b


def full_form(z, gamma, beta, w, b, dtype):
    """timm Attention on norm1(z), row 0 of the output (before proj), in `dtype`"""
    z, gamma, beta, w, b = (t.to(dtype) for t in (z, gamma, beta, w, b))
    d = z.shape[1]
    hd = d // HEADS
    x = torch.nn.functional.layer_norm(z, (d,), gamma, beta, 1e-6)
    qkv = (x @ w.t() + b).reshape(TOKENS, 3, HEADS, hd).permute(1, 2, 0, 3)
    q, k, v = qkv[0], qkv[1], qkv[2]
    att = torch.softmax((q[:, :1] * hd ** -0.5) @ k.transpose(-1, -2), dim=-1)      # [heads][1][tokens]
    return (att @ v).transpose(0, 1).reshape(d)


def restated_form(z, gamma, beta, w, b, dtype):
    """the same row from the folded parameters, without K or V"""
    d = z.shape[1]
    hd = d // HEADS
    wf = (w * gamma[None, :]).to(dtype)                  # W' = gamma o W (folded in fp64, as the packed weight is folded once at create)
    bf = (b + w @ beta).to(dtype)                        # b' = b + W beta
    z = z.to(dtype)
    mean = z.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(z.var(1, unbiased=False, keepdim=True) + 1e-6)
    y = (z - mean) * rstd
    q = (wf[:d] @ y[0] + bf[:d]).reshape(HEADS, hd)
    g = hd ** -0.5 * torch.einsum("hn,hnk->hk", q, wf[d:2 * d].reshape(HEADS, hd, d))
    p = torch.softmax(g @ y.t(), dim=-1)                 # [heads][tokens]
    ybar = p @ y                                         # [heads][d]
    o = torch.einsum("hnk,hk->hn", wf[2 * d:].reshape(HEADS, hd, d), ybar) + bf[2 * d:].reshape(HEADS, hd)
    return o.reshape(d)


@pytest.mark.parametrize("d", [144, 288, 384, 576])
def test_cls_attention_identity_fp64(d):
    case = _case(d, 1000 + d)
    ref = full_form(*case, torch.float64)
    got = restated_form(*case, torch.float64)
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"[measured] cls attention identity d={d}: fp64 difference {rel:.2e} of the largest output {ref.abs().max().item():.2f}")
    assert rel <= 1e-12, rel
    # both forms again in fp32: the restated form's rounding error beside the full form's
    e_full = ((full_form(*case, torch.float32).double() - ref).abs().max() / ref.abs().max()).item()
    e_new = ((restated_form(*case, torch.float32).double() - ref).abs().max() / ref.abs().max()).item()
    print(f"[measured] cls attention identity d={d}: fp32 error full form {e_full:.2e}, restated form {e_new:.2e} (ratio {e_new / e_full:.2f})")
    assert math.isfinite(e_new)
