"""GPU tests of the pad and scratch contracts ("Pad and scratch contract"; csrc/ribca_api.hip zero_pads): every test runs the SAME code
twice or three times on the same inputs with different junk in the bytes a kernel is said not to depend on, and asks for identical bits.

* part 1 -- the pad token rows 101 .. 111 of the attention operands Q, K, V are don't-care ("never written", "never fetched"): NaN halves there
  change no output bit and are still there afterwards;
* part 2 -- a whole classifier / imputer forward does not depend on what its workspace held (0x00, 0x7C and 0xFF bytes), writes nothing beyond
  ribca_*_workspace_bytes, and its chunks are independent of each other;
* part 3 -- the same for the clustering, plot and region entry points that take a `ws`.

No tolerance, no reference, no fixture: bit equality between runs of the same code."""
import ctypes

import numpy as np
import pytest
import torch

from kernel_harness import BAND, Arena, fold_weight, ln_case, ps_decode, ps_encode, rnd, row_stats, umap_graph
from multiplexed_image_annotator_amd import synth

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0x7C, 0xFF)      # zeros / fp16 NaN halves, 5e36 as fp32, a huge e4m3 code / NaN as fp16, fp32, fp64 and -1 as every integer
NAN16 = 0x7E00                  # an fp16 NaN in every half it is written to
HEADS, NTOK, TP = 12, 101, 112


@pytest.fixture(scope="module")
def dev():
    from multiplexed_image_annotator_amd import _lib
    return _lib.require_gpu()


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().reshape(-1).view(torch.uint8)


# ------------------------------------------------------------------------------------------------ 1. pads of the attention operands
def _attn_launcher(dev, kind, d, cells):
    """launch(q, k, vt, out) of one of the three qkv + attention hooks on fixed inputs"""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    m = cells * NTOK
    dp = (d + 31) // 32 * 32
    if kind == "plain":
        y_ps = ps_encode(rnd((m, d), 12, dev), dp)
        w_ps = ps_encode(rnd((3 * d, d), 13, dev, 1.0 / np.sqrt(d)), dp, lib().ribca_gemm_padded_n(3 * d))
        bias = rnd((3 * d,), 14, dev, 0.1)

        def launch(q, k, vt, out):
            check(lib().ribca_test_qkv_attention(ptr(y_ps), 2 * dp, ptr(w_ps), 2 * dp, cells, d, dp, ptr(bias), ptr(q), ptr(k), ptr(vt), ptr(out), 2 * dp,
                                                 stream_ptr()), "qkv + attention")
        return launch
    z_ps, _, g, b, dp = ln_case(m, d, 60, dev, 0.5, 1.0)
    w = rnd((3 * d, d), 63, dev, 1.0 / np.sqrt(d))
    w_ps, csum, bias2 = fold_weight(w, g, b, rnd((3 * d,), 64, dev, 0.1), dp, dev)
    rs = row_stats(z_ps, dp, m, d, dev)
    if kind == "fold":
        def launch(q, k, vt, out):
            check(lib().ribca_test_qkv_attention_fold(ptr(z_ps), 2 * dp, ptr(w_ps), 2 * dp, cells, d, dp, ptr(bias2), ptr(csum), ptr(rs), ptr(q), ptr(k),
                                                      ptr(vt), ptr(out), 2 * dp, stream_ptr()), "qkv fold + attention")
        return launch
    assert kind == "mx"
    kz = (dp + 127) // 128 * 128

    def launch(q, k, vt, out):
        z8 = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device=dev)
        a_hi, a_l8, a_sc = z8(m, kz, dt=torch.int16), z8(m, kz), z8(m, kz // 32)
        wh, wx = z8(lib().ribca_test_mx_weight_bytes(3 * d, kz, 0)), z8(lib().ribca_test_mx_weight_bytes(3 * d, kz, 1))
        check(lib().ribca_test_qkv_attention_mx(ptr(z_ps), 2 * dp, ptr(w_ps), 2 * dp, cells, d, dp, ptr(bias2), ptr(csum), ptr(rs), ptr(a_hi), ptr(a_l8),
                                                ptr(a_sc), ptr(wh), ptr(wx), ptr(q), ptr(k), ptr(vt), ptr(out), 2 * dp, stream_ptr()), "qkv mx + attention")
        torch.cuda.synchronize()
    return launch


def _by_dim(buf, hdq):
    """[cells][heads][112][2 * hdq] packed-split rows (groups of 8 dims: 8 hi halves, 8 lo halves) -> [cells][heads][112][hi / lo][hdq]"""
    c, h, t, _ = buf.shape
    return buf.view(c, h, t, hdq // 8, 2, 8).permute(0, 1, 2, 4, 3, 5).reshape(c, h, t, 2, hdq)


ATTN_CASES = [(kind, d) for kind in ("plain", "fold") for d in (144, 288, 384, 576)] + [("mx", 384), ("mx", 576)]


@pytest.mark.parametrize("cells", [3, 1])
@pytest.mark.parametrize("kind,d", ATTN_CASES)
def test_attention_pad_token_rows_are_dont_care(dev, kind, d, cells):
    """Run Z: q, k, vt and out all zero.  Run P: token rows 101 .. 111 of q, k and vt hold 0x7E00 (an fp16 NaN) in every hi and lo half, and every
    half of the real columns of out holds it too.  The producers never write those rows, the attention kernel never fetches them from K and V
    (buffer descriptor that ends behind row 100) and a NaN in a pad row of Q stays in that query's own lanes, whose output is not stored."""
    hd = d // HEADS
    hdq = (hd + 7) // 8 * 8
    m, dp = cells * NTOK, (d + 31) // 32 * 32
    launch = _attn_launcher(dev, kind, d, cells)
    runs = {}
    for tag in "ZP":
        q, k, vt = (torch.zeros((cells, HEADS, TP, 2 * hdq), dtype=torch.int16, device=dev) for _ in range(3))
        out = torch.zeros((m, 2 * dp), dtype=torch.int16, device=dev)
        if tag == "P":
            for t in (q, k, vt):
                t[:, :, NTOK:, :] = NAN16
            out[:, :2 * d] = NAN16
        launch(q, k, vt, out)
        torch.cuda.synchronize()
        runs[tag] = (q, k, vt, out)
    out_z, out_p = runs["Z"][3], runs["P"][3]
    assert torch.any(out_z != 0)
    assert torch.equal(out_z, out_p), "an attention output depends on a pad token row of Q, K or V"
    assert torch.isfinite(ps_decode(out_p, dp)).all()
    for name, t in zip("qkv", runs["P"][:3]):
        assert torch.all(t[:, :, NTOK:, :] == NAN16), f"a producer wrote into a pad token row of {name}"
    assert not torch.any(out_p[:, :2 * d] == NAN16), "a real output half was never written"
    assert torch.all(out_p[:, 2 * d:] == 0) and torch.all(out_z[:, 2 * d:] == 0)      # the groups d .. dp (d = 144 only)
    for tag in "ZP":      # must-be-zero pads (the Q K^T product runs over them): head dims hd .. hdq of the real token rows (d = 144 only)
        for name, t in zip("qkv", runs[tag][:3]):
            assert torch.all(_by_dim(t, hdq)[:, :, :NTOK, :, hd:] == 0), f"head-dim pad of {name} is not zero (run {tag})"
            assert torch.any(_by_dim(t, hdq)[:, :, :NTOK, :, :hd] != 0)


# ------------------------------------------------------------------------------------------------ 2. the forward and its workspace
def _vit_inputs(name, n):
    c = synth.VIT_CONFIGS[name][1]
    u = synth.uniform(synth.stream_key(5, "scratch/" + name), n * c * 1600).reshape(n, c, 40, 40).to(torch.float32)
    return torch.where(u * 2 - 1 > 0.1, u * 2 - 1, torch.full_like(u, -1.0))


def _vit_call(dev, entry, model, x, chunk, fill):
    """one forward through the C entry point: operands and a workspace of exactly ribca_vit_workspace_bytes inside an arena whose every other
    byte holds `fill` too; probs prefilled with 0xFF"""
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    n, c_img = x.shape[0], x.shape[1]
    nbytes = int(lib().ribca_vit_workspace_bytes(model._h, chunk))
    assert nbytes > 0
    ar = Arena(dev, fill, capacity=nbytes + x.numel() * 4 + 64 * BAND)
    xp = ar.put(x)
    src = ar.put(torch.arange(c_img, dtype=torch.int32, device=dev))
    probs = ar.empty((n, model.K), torch.float32)
    _bytes(probs).fill_(0xFF)
    ws = ar.empty((nbytes,), torch.uint8)
    ws.fill_(fill)
    assert ws.data_ptr() % 256 == 0
    check(getattr(lib(), entry)(model._h, ptr(xp), c_img, ptr(src), n, ptr(probs), ptr(ws), nbytes, chunk, stream_ptr()), entry)
    torch.cuda.synchronize()
    assert ar.bands_intact(), f"{entry} wrote outside its operands / beyond workspace_bytes (fill {fill:#x})"
    assert torch.equal(xp, x)
    return probs.clone()


@pytest.mark.parametrize("depth", [2, 1])
@pytest.mark.parametrize("name", list(synth.VIT_CONFIGS))
def test_vit_forward_ignores_workspace_content(dev, monkeypatch, name, depth):
    """19 cells in chunks of 8 (8 + 8 + a ragged 3: stale rows of chunk 2 lie behind chunk 3) and 1 cell in a workspace for 8 (everything beyond
    the first 101 rows is junk), fast and precise entry point, depth 2 and depth 1 (the last-block-CLS path alone: no earlier block leaves finite
    values behind).  The fast entry point is called whatever a load-time probe would say about the weights: the MX kernels' scratch is the point."""
    from multiplexed_image_annotator_amd import ops
    monkeypatch.setenv("RIBCA_MARGIN_PROBE", "0")      # handles only: no probe forwards at load
    model = ops.VitModel(synth.make_vit_state_dict(name, synth.SEED_BASE + 7, depth=depth), dev)
    x = _vit_inputs(name, 19).to(dev)
    for entry in ("ribca_vit_forward", "ribca_vit_forward_precise"):
        for n in (19, 1):
            outs = [_vit_call(dev, entry, model, x[:n].contiguous(), 8, fill) for fill in FILLS]
            for fill, o in zip(FILLS, outs):
                assert torch.isfinite(o).all(), f"{entry}, {n} cells: non-finite or unwritten probabilities (fill {fill:#x})"
                assert torch.equal(o, outs[0]), f"{entry}, {n} cells: the result depends on the workspace content (fill {fill:#x} against 0x00)"
            assert torch.allclose(outs[0].sum(1), torch.ones(n, device=dev), atol=1e-5)
            if n == 19:
                whole = outs[0]
        parts = [_vit_call(dev, entry, model, x[a:b].contiguous(), 8, 0xFF) for a, b in ((0, 8), (8, 16), (16, 19))]
        assert torch.equal(torch.cat(parts), whole), f"{entry}: a chunk depends on the chunk before it"


MAE_CASES = [("immune_base", [1, 2, 3, 4, 5, 6]), ("immune_extended", [0, 1, 2, 3, 5, 6, 7, 9]), ("immune_full", [c for c in range(15) if c != 6])]


def _mae_call(dev, model, x, present, chunk, fill):
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    n, L = x.shape[0], x.shape[1]
    missing = [c for c in range(L) if c not in present]
    nbytes = int(lib().ribca_mae_workspace_bytes(model._h, chunk, len(present)))
    assert nbytes > 0
    ar = Arena(dev, fill, capacity=nbytes + x.numel() * 4 + 64 * BAND)
    xp = ar.put(x)
    xp.view(torch.int32)[:, missing] = -1      # 0xFF bytes in every plane to impute
    ws = ar.empty((nbytes,), torch.uint8)
    ws.fill_(fill)
    arr = (ctypes.c_int32 * len(present))(*present)
    check(lib().ribca_mae_impute(model._h, ptr(xp), arr, len(present), n, ptr(ws), nbytes, chunk, stream_ptr()), "ribca_mae_impute")
    torch.cuda.synchronize()
    assert ar.bands_intact(), f"ribca_mae_impute wrote outside its operands / beyond workspace_bytes (fill {fill:#x})"
    return xp.clone()


@pytest.mark.parametrize("panel,present", MAE_CASES)
def test_mae_impute_ignores_workspace_content(dev, monkeypatch, panel, present):
    """11 cells in chunks of 4 (4 + 4 + a ragged 3).  The encoder / decoder attention has ONE 16-token tile (NT = 1): its V^T pad keys are read
    under P = 0 and must be zero, every other pad and every scratch buffer is junk."""
    from multiplexed_image_annotator_amd import ops
    monkeypatch.setenv("RIBCA_MARGIN_PROBE", "0")      # the folded (fast) handle itself, no second handle for a probe
    model = ops.MaeModel(synth.make_mae_state_dict(panel, 17, enc_depth=2, dec_depth=2), dev)
    L = synth.MAE_PANELS[panel]
    u = synth.uniform(synth.stream_key(18, "scratch/mae/" + panel), 11 * L * 1600).reshape(11, L, 40, 40).to(torch.float32) * 2 - 1
    x = torch.where(u > 0.0, u, torch.full_like(u, -1.0)).to(dev)
    missing = [c for c in range(L) if c not in present]
    outs = [_mae_call(dev, model, x, present, 4, fill) for fill in FILLS]
    for fill, o in zip(FILLS, outs):
        assert torch.isfinite(o).all(), f"non-finite or unwritten imputed planes (fill {fill:#x})"
        assert torch.equal(o[:, present], x[:, present]), "a present channel was touched"
        assert torch.equal(o, outs[0]), f"the imputed planes depend on the workspace content (fill {fill:#x} against 0x00)"
    assert torch.any(outs[0][:, missing] != -1.0)
    parts = [_mae_call(dev, model, x[a:b].contiguous(), present, 4, 0xFF) for a, b in ((0, 4), (4, 8), (8, 11))]
    assert torch.equal(torch.cat(parts), outs[0]), "a chunk depends on the chunk before it"


def test_shared_workspace_slot_content_does_not_matter(dev):
    """ops.workspace() slot 0 as the product uses it: one grow-only torch.empty buffer under all classifiers and the imputer.  The widest
    classifier sizes it, then `nerve`, the imputer and `nerve` again each find 0x7C bytes in all of it."""
    from multiplexed_image_annotator_amd import ops
    full = ops.VitModel(synth.make_vit_state_dict("immune_full", synth.SEED_BASE + 7, depth=2), dev)
    nerve = ops.VitModel(synth.make_vit_state_dict("nerve", synth.SEED_BASE + 7, depth=2), dev)
    mae = ops.MaeModel(synth.make_mae_state_dict("immune_base", 17, enc_depth=2, dec_depth=2), dev)
    xf, xn = _vit_inputs("immune_full", 19).to(dev), _vit_inputs("nerve", 19).to(dev)
    u = synth.uniform(synth.stream_key(18, "scratch/mae/shared"), 11 * 7 * 1600).reshape(11, 7, 40, 40).to(torch.float32) * 2 - 1
    xm = torch.where(u > 0.0, u, torch.full_like(u, -1.0)).to(dev).contiguous()

    def poison():
        torch.cuda.synchronize()
        held = [t for t in ops._WS.values() if t is not None]
        assert held
        for t in held:
            t.fill_(0x7C)

    assert torch.isfinite(full.predict_proba(xf, list(range(15)), chunk_cells=8)).all()
    poison()
    first = nerve.predict_proba(xn, [0, 1, 2], chunk_cells=8).clone()
    poison()
    imputed = mae.impute(xm.clone(), [1, 2, 3, 4, 5, 6], chunk_cells=4)
    poison()
    second = nerve.predict_proba(xn, [0, 1, 2], chunk_cells=8)
    torch.cuda.synchronize()
    assert torch.isfinite(first).all() and torch.isfinite(imputed).all()
    assert torch.equal(first, second), "a classifier result depends on what the shared workspace slot held"


# ------------------------------------------------------------------------------------------------ 3. the other entry points that take scratch
def _f64(rng, *shape):
    return torch.from_numpy(rng.randn(*shape))


def _case_region_gram(dev, n, f):
    from multiplexed_image_annotator_amd import ops
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    c = torch.from_numpy(np.random.RandomState(n + f).randint(0, 201, size=(n, f)).astype(np.int16)).to(dev)

    def direct(ar, ws):
        cd, colsum, gram = ar.put(c), ar.empty((f,), torch.int64), ar.empty((f, f), torch.int64)
        check(lib().ribca_region_gram(ptr(cd), n, f, ptr(colsum), ptr(gram), ptr(ws), ws.numel(), stream_ptr()), "ribca_region_gram")
        return {"colsum": colsum, "gram": gram}

    return ops.region_gram_ws_bytes(n, f), direct, lambda ws: dict(zip(("colsum", "gram"), ops.region_gram(c, ws=ws)))


def _case_kmeans_trials(dev, n, d, n_cand, with_closest):
    from multiplexed_image_annotator_amd import ops
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    rng = np.random.RandomState(n + d)
    y = _f64(rng, n, d).to(dev)
    cand = torch.from_numpy(rng.choice(n, n_cand, replace=False).astype(np.int32)).to(dev)
    closest = (_f64(rng, n) ** 2).to(dev) if with_closest else None

    def direct(ar, ws):
        yd, cd, cl = ar.put(y), ar.put(cand), (ar.put(closest) if with_closest else None)
        d2, pot = ar.empty((n_cand, n), torch.float64), ar.empty((n_cand,), torch.float64)
        check(lib().ribca_kmeans_trials(ptr(yd), n, d, ptr(cd), n_cand, ptr(cl), ptr(d2), ptr(pot), ptr(ws), ws.numel(), stream_ptr()), "ribca_kmeans_trials")
        return {"cand_d2": d2, "pot": pot}

    return ops.kmeans_trials_ws_bytes(n, n_cand), direct, lambda ws: dict(zip(("cand_d2", "pot"), ops.kmeans_trials(y, cand, closest, ws=ws)))


def _case_kmeans_update(dev, n, d, k):
    from multiplexed_image_annotator_amd import ops
    rng = np.random.RandomState(n + d + k)
    y, old = _f64(rng, n, d).to(dev), _f64(rng, k, d).to(dev)
    labels = rng.randint(0, k, n).astype(np.int32)
    labels[labels == k - 1] = 0      # an empty cluster: its centre stays the old one
    labels = torch.from_numpy(labels).to(dev)
    changed = torch.tensor([3], dtype=torch.int32, device=dev)

    def run(ws, alloc, put):
        new, sums, counts, stat = alloc((k, d), torch.float64), alloc((k, d), torch.float64), alloc((k,), torch.int32), alloc((1 + 2 * k,), torch.float64)
        ops.kmeans_update(put(y), put(labels), put(old), new, sums, counts, put(changed), stat, ws)
        return {"centres_new": new, "sums": sums, "counts": counts, "stat": stat}

    plain = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    return ops.kmeans_update_ws_bytes(n, d, k), (lambda ar, ws: run(ws, ar.empty, ar.put)), (lambda ws: run(ws, plain, lambda t: t))


def _points(seed, n, dim):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, dim).astype(np.float32) * 3
    x[n - 37:] = x[rng.randint(n - 37, size=37)]      # duplicated rows: ties
    return x


def _case_core_distance(dev, n, dim, ms):
    from multiplexed_image_annotator_amd import ops
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    x = torch.from_numpy(_points(n + dim, n, dim)).to(dev)

    def direct(ar, ws):
        xd, core2 = ar.put(x), ar.empty((n,), torch.float32)
        check(lib().ribca_core_distance(ptr(xd), n, dim, ms, ptr(core2), ptr(ws), ws.numel(), stream_ptr()), "ribca_core_distance")
        return {"core2": core2}

    return ops.core_distance_ws_bytes(n, dim, ms), direct, lambda ws: {"core2": ops.core_distance(x, ms, ws=ws)}


def _case_mreach_mst(dev, n, dim, ms):
    from multiplexed_image_annotator_amd import ops
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    x = torch.from_numpy(_points(n + dim, n, dim)).to(dev)
    core2 = ops.core_distance(x, ms)

    def direct(ar, ws):
        xd, cd = ar.put(x), ar.put(core2)
        u, v, w = ar.empty((n - 1,), torch.int32), ar.empty((n - 1,), torch.int32), ar.empty((n - 1,), torch.float32)
        check(lib().ribca_mreach_mst(ptr(xd), n, dim, ptr(cd), ptr(u), ptr(v), ptr(w), ptr(ws), ws.numel(), stream_ptr()), "ribca_mreach_mst")
        return {"u": u, "v": v, "w": w}

    return ops.mreach_mst_ws_bytes(n), direct, lambda ws: dict(zip("uvw", ops.mreach_mst(x, core2, ws=ws)))


def _case_spectral_gram(dev, n, p, q):
    from multiplexed_image_annotator_amd import ops
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    rng = np.random.RandomState(n + p)
    u, v = _f64(rng, n, p).to(dev), _f64(rng, n, q).to(dev)

    def direct(ar, ws):
        ud, vd, g = ar.put(u), ar.put(v), ar.empty((p, q), torch.float64)
        check(lib().ribca_spectral_gram(ptr(ud), ptr(vd), n, p, q, ptr(g), ptr(ws), ws.numel(), stream_ptr()), "ribca_spectral_gram")
        return {"g": g}

    return ops.spectral_gram_ws_bytes(n, p, q), direct, lambda ws: {"g": ops.spectral_gram(u, v, ws=ws)}


def _case_scatter_raster(dev, h, w, n):
    from multiplexed_image_annotator_amd import ops
    from multiplexed_image_annotator_amd._lib import check, lib, ptr, stream_ptr
    rng = np.random.RandomState(h)
    pts = (rng.randn(n, 2) * [3.0, 0.7] + [10.0, -4.0]).astype(np.float32)
    pts[17] = np.nan
    aff = ops.scatter_affine(pts, h, w)
    pd, rgb = torch.from_numpy(pts).to(dev), torch.from_numpy(rng.randint(0, 256, (n, 3)).astype(np.uint8)).to(dev)

    def direct(ar, ws):
        p, c, out = ar.put(pd), ar.put(rgb), ar.empty((h, w, 3), torch.uint8)
        skipped = ctypes.c_int64(-1)
        check(lib().ribca_scatter_raster(ptr(p), ptr(c), n, aff[0], aff[1], aff[2], aff[3], h, w, 2, ptr(out), ctypes.byref(skipped), ptr(ws), ws.numel(),
                                         stream_ptr()), "ribca_scatter_raster")
        return {"out": out, "skipped": torch.tensor([skipped.value], device=dev)}

    def wrapped(ws):
        out, skipped = ops.scatter_raster(pd, rgb, h, w, aff, 2, ws=ws)
        return {"out": out, "skipped": torch.tensor([skipped], device=dev)}

    return int(lib().ribca_scatter_raster_ws_bytes(h, w)), direct, wrapped


def _case_umap_optimize(dev, n, dim, epochs):
    from multiplexed_image_annotator_amd import manifold, ops
    g, eps, rev = umap_graph(n, dim)
    a, b = manifold.find_ab_params()
    emb0 = torch.from_numpy(np.ascontiguousarray(manifold.initial_embedding(g, dim, 0), dtype=np.float32)).to(dev)
    indptr, indices = torch.from_numpy(g.indptr.astype(np.int64)).to(dev), torch.from_numpy(g.indices.astype(np.int32)).to(dev)
    revd, epsd = torch.from_numpy(rev).to(dev), torch.from_numpy(eps).to(dev)

    def direct(ar, ws):
        e = ar.put(emb0)
        return {"emb": ops.umap_optimize(e, ar.put(indptr), ar.put(indices), ar.put(revd), ar.put(epsd), a, b, epochs, 7, ws=ws)}

    return ops.umap_optimize_ws_bytes(n, dim, int(indices.numel())), direct, lambda ws: direct(_Plain(), ws)


class _Plain:
    """the `put` of an Arena without an arena: an ordinary copy"""

    @staticmethod
    def put(t):
        return t.clone()


SCRATCH_CASES = {
    "region_gram-1237x16": (_case_region_gram, (1237, 16)),
    "region_gram-2049x264": (_case_region_gram, (2049, 264)),
    "kmeans_trials-1025x5": (_case_kmeans_trials, (1025, 5, 3, False)),
    "kmeans_trials-5003x43": (_case_kmeans_trials, (5003, 43, 5, True)),
    "kmeans_update-1025x5-k7": (_case_kmeans_update, (1025, 5, 7)),
    "kmeans_update-2311x43-k64": (_case_kmeans_update, (2311, 43, 64)),
    "core_distance-1237x5-ms5": (_case_core_distance, (1237, 5, 5)),
    "core_distance-1025x15-ms65": (_case_core_distance, (1025, 15, 65)),      # above 64: the bisection path
    "mreach_mst-515x64": (_case_mreach_mst, (515, 64, 6)),
    "mreach_mst-1025x3": (_case_mreach_mst, (1025, 3, 10)),
    "spectral_gram-1025x9x24": (_case_spectral_gram, (1025, 9, 24)),
    "spectral_gram-3089x48x48": (_case_spectral_gram, (3 * 1024 + 17, 48, 48)),
    "scatter_raster-64x96": (_case_scatter_raster, (64, 96, 5000)),
    "umap_optimize-400x2": (_case_umap_optimize, (400, 2, 10)),
    "umap_optimize-1025x5": (_case_umap_optimize, (1025, 5, 10)),
}


@pytest.mark.parametrize("case", sorted(SCRATCH_CASES))
def test_entry_point_ignores_scratch_and_output_content(dev, case):
    """ws (exactly the size the library asks for) and every output prefilled with 0x00, then with 0xFF, inside an arena of the same bytes: the
    outputs are byte-identical, nothing outside them is written, and the `ws=` keyword of the ops wrapper gives the same bytes again."""
    make, args = SCRATCH_CASES[case]
    nws, direct, wrapped = make(dev, *args)
    nws = int(nws)
    assert nws > 0
    got = []
    for fill in (0x00, 0xFF):
        ar = Arena(dev, fill, capacity=32 << 20)
        ws = ar.empty((nws,), torch.uint8)
        ws.fill_(fill)
        outs = direct(ar, ws)
        torch.cuda.synchronize()
        assert ar.bands_intact(), f"{case}: a write outside the outputs and the {nws} bytes of ws (fill {fill:#x})"
        got.append({k: _bytes(v).clone() for k, v in outs.items()})
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), f"{case}: {k} depends on what ws or the outputs held"
    again = wrapped(torch.full((nws,), 0xFF, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    for k in got[0]:
        assert torch.equal(_bytes(again[k]), got[0][k]), f"{case}: {k} through the ops wrapper's ws= differs"
