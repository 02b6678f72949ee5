"""The imputer's forward at the present sets nobody had run.  ribca_mae_impute accepts any 1 <= n_present < L, so a user's panel puts the
encoder's attention at any token count 2 .. L; the forward tests run 6, 8 and 14 present markers only.  Here, for each of the three panels at
encoder depth 2 / decoder depth 1: one marker alone (first, last, middle: 2 encoder tokens), two adjacent (3), all but the first / the last
(L), every second one -- five cells in chunks of two (2 + 2 + a ragged 1) against oracle.ref_mae.impute.  Kept channels stay bit-identical;
imputed planes stay within the 5e-4 of test_gpu_kernels.test_mae_vs_oracle, for its reason: pixel values in [-1, 1] feed a classifier whose
1e-3 budget is on probabilities.

Refusals: no present marker, every marker present, a repeated and a descending list fail with the library's message (the wrapper's exception
where ops raises first), launch nothing and leave the patches and the workspace untouched."""
import ctypes

import pytest
import torch

from multiplexed_image_annotator_amd import synth

pytestmark = pytest.mark.gpu

N_CELLS, CHUNK = 5, 2
PRESENT_SETS = {
    "first alone": lambda L: [0],
    "last alone": lambda L: [L - 1],
    "middle alone": lambda L: [L // 2],
    "two adjacent": lambda L: [L // 2, L // 2 + 1],
    "all but the first": lambda L: list(range(1, L)),
    "all but the last": lambda L: list(range(L - 1)),
    "every second": lambda L: list(range(0, L, 2)),
}


@pytest.fixture(scope="module")
def dev():
    from multiplexed_image_annotator_amd import _lib
    return _lib.require_gpu()


_MODELS = {}


def _model(panel, dev):
    """(state dict, packed model, input patches) of a panel, built once"""
    if panel not in _MODELS:
        from multiplexed_image_annotator_amd import ops
        sd = synth.make_mae_state_dict(panel, 17, enc_depth=2, dec_depth=1)
        L = synth.MAE_PANELS[panel]
        u = synth.uniform(synth.stream_key(19, "present_sets/" + panel), N_CELLS * L * 1600).reshape(N_CELLS, L, 40, 40).to(torch.float32) * 2 - 1
        x = torch.where(u > 0.0, u, torch.full_like(u, -1.0))
        _MODELS[panel] = (sd, ops.MaeModel(sd, dev), x)
    return _MODELS[panel]


@pytest.mark.parametrize("which", list(PRESENT_SETS))
@pytest.mark.parametrize("panel", list(synth.MAE_PANELS))
def test_mae_present_set_vs_oracle(dev, panel, which):
    from oracle import ref_mae
    sd, model, x = _model(panel, dev)
    L = synth.MAE_PANELS[panel]
    present = PRESENT_SETS[which](L)
    assert 1 <= len(present) < L
    ref = ref_mae.impute(sd, x, present)
    got = model.impute(x.to(dev).contiguous(), present, chunk_cells=CHUNK).cpu()
    missing = [c for c in range(L) if c not in present]
    assert torch.equal(got[:, present], x[:, present]), "a kept channel was touched"
    assert torch.isfinite(got).all()
    err = (got[:, missing] - ref[:, missing]).abs().max().item()
    print(f"[measured] mae {panel} {which} ({len(present)} present, {len(present) + 1} encoder tokens): {err:.3e}")
    assert err < 5e-4, err
    assert torch.any(got[:, missing] != x[:, missing])


@pytest.mark.parametrize("panel", list(synth.MAE_PANELS))
def test_mae_refused_present_lists(dev, panel):
    from multiplexed_image_annotator_amd._lib import RibcaError, lib, ptr, stream_ptr
    _, model, x = _model(panel, dev)
    L = synth.MAE_PANELS[panel]
    xd = x.to(dev).contiguous()
    keep = xd.clone()
    # the sizes only ribca_mae_workspace_bytes can refuse: it never sees the list
    assert lib().ribca_mae_workspace_bytes(model._h, CHUNK, 0) == 0 and lib().ribca_mae_workspace_bytes(model._h, CHUNK, L) == 0
    assert lib().ribca_mae_workspace_bytes(model._h, CHUNK, L + 1) == 0 and lib().ribca_mae_workspace_bytes(model._h, CHUNK, -1) == 0
    nbytes = int(lib().ribca_mae_workspace_bytes(model._h, CHUNK, L - 1))      # the largest workspace a call of this model takes
    assert nbytes > 0
    ws = torch.full((nbytes,), 0x7C, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0

    def direct(present):
        arr = (ctypes.c_int32 * max(1, len(present)))(*present)
        st = lib().ribca_mae_impute(model._h, ptr(xd), arr, len(present), N_CELLS, ptr(ws), nbytes, CHUNK, stream_ptr())
        msg = lib().ribca_last_error()
        torch.cuda.synchronize()
        assert torch.equal(xd, keep), (present, "the patches were touched")
        assert torch.all(ws == 0x7C), (present, "something was launched: the workspace was written")
        return st, msg

    mid = L // 2
    for present, text in (([], b"need 1 <= n_present < L"), (list(range(L)), b"need 1 <= n_present < L"),
                          ([mid, mid], b"strictly increasing"), ([mid + 1, mid], b"strictly increasing")):
        st, msg = direct(present)
        assert st != 0 and msg and b"ribca_mae_impute" in msg and text in msg, (present, st, msg)
    # through the wrapper: the sizes fail in ops before the library is asked, a repeated channel fails in the library; a descending list is
    # sorted by the wrapper and is the ascending call
    for present in ([], list(range(L))):
        with pytest.raises(ValueError):
            model.impute(xd, present, chunk_cells=CHUNK)
    with pytest.raises(RibcaError, match="strictly increasing"):
        model.impute(xd, [mid, mid], chunk_cells=CHUNK)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep)
    a = model.impute(xd.clone(), [mid, mid + 1], chunk_cells=CHUNK)
    b = model.impute(xd.clone(), [mid + 1, mid], chunk_cells=CHUNK)
    assert torch.equal(a, b) and not torch.equal(a, keep)
