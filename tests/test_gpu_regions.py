"""GPU tissue regions (csrc/regions.hip, multiplexed_image_annotator_amd/regions.py, Annotator.tissue_region_analysis): the integer PCA
statistics equal to numpy's, the projection, the k-means++ picks, every Lloyd iteration and the final labels bit for bit against the numpy
oracle (tests/regions_numpy.py), statuses for requests out of range, and the Annotator: reproducible files, the seed, the backend switch,
two ranks, and parity with scikit-learn from the same initial centres on planted bands."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import regions_numpy as R
from batch_harness import two_ranks
from multiplexed_image_annotator_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    from multiplexed_image_annotator_amd import _lib
    return _lib.require_gpu()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _random_counts(seed, n, t):
    """(n, 8, t) int16 in 0 .. 200 with both ends present in every column block"""
    rng = np.random.RandomState(seed)
    c = rng.randint(0, 201, size=(n, 8, t)).astype(np.int16)
    c[rng.randint(n, size=n // 7)] = 0
    c[0] = 200
    c[n - 1] = 200
    c[1] = 0
    return c


@pytest.mark.parametrize("t", [2, 13, 33, 254])
@pytest.mark.parametrize("n", [1237, 5003])
def test_gram_and_column_sums_equal_numpy_integers(n, t):
    from multiplexed_image_annotator_amd import ops
    c = _random_counts(n + t, n, t).reshape(n, 8 * t)
    colsum, gram = ops.region_gram(torch.from_numpy(c).to(_dev()))
    if 8 * t <= 300:
        ref_sum, ref = R.gram(c)
    else:      # every entry is below 5003 * 200^2 < 2^53: the fp64 product is the exact integer product, through BLAS
        cf = c.astype(np.float64)
        ref_sum, ref = c.astype(np.int64).sum(axis=0), (cf.T @ cf).astype(np.int64)
    assert colsum.dtype == torch.int64 and gram.dtype == torch.int64
    assert np.array_equal(colsum.cpu().numpy(), ref_sum)
    assert np.array_equal(gram.cpu().numpy(), ref)
    again = ops.region_gram(torch.from_numpy(c).to(_dev()))[1]
    assert torch.equal(again, gram)


def test_gram_refuses_counts_out_of_range():
    from multiplexed_image_annotator_amd import _lib, ops
    c = _random_counts(1, 300, 3).reshape(300, 24)
    c[17, 5] = 256
    with pytest.raises(_lib.RibcaError, match="outside 0 .. 255"):
        ops.region_gram(torch.from_numpy(c).to(_dev()))
    c[17, 5] = -1
    with pytest.raises(_lib.RibcaError, match="outside 0 .. 255"):
        ops.region_gram(torch.from_numpy(c).to(_dev()))


@pytest.mark.parametrize("d", [1, 5, 43, 150])
def test_projection_bit_equal_to_numpy_loop(d):
    from multiplexed_image_annotator_amd import ops
    n, t = 1237, 19
    rng = np.random.RandomState(d)
    c = _random_counts(d, n, t).reshape(n, 8 * t)
    size_col = R.size_columns(R.SIZES, t)
    mean = rng.uniform(0.0, 1.0, 8 * t)
    comps = np.linalg.qr(rng.randn(8 * t, 8 * t))[0][:d].copy()
    dev = _dev()
    y = ops.region_project(torch.from_numpy(c).to(dev), torch.from_numpy(size_col).to(dev), torch.from_numpy(mean).to(dev),
                           torch.from_numpy(comps).to(dev)).cpu().numpy()
    ref = R.project(c, size_col, mean, comps)
    assert y.shape == (n, d) and np.array_equal(_bits(y), _bits(ref)), np.abs(y - ref).max()


@pytest.mark.parametrize("n,t,bands", [(3000, 6, 3), (5003, 13, 5)])
def test_pca_project_on_planted_counts(n, t, bands):
    """GPU counts = the k-d tree's, Gram exact, and -- fed the same eigenvectors -- the projection equal to the oracle's bit for bit"""
    from multiplexed_image_annotator_amd import ops, regions
    x, y, types, _ = synth.planted_bands(n, t, bands, 77 + n)
    counts = ops.knn_composition_counts(x, y, types, t)
    ref_counts, _ = R.planted_counts(n, t, bands, 77 + n)
    assert np.array_equal(counts.cpu().numpy(), ref_counts)
    info = {}
    emb = regions.pca_project(counts, R.SIZES, info=info).cpu().numpy()
    c2 = ref_counts.reshape(n, -1)
    colsum, g = R.gram(c2)
    mean, comps, lam, d = R.pca_from_gram(g, colsum, n, R.size_columns(R.SIZES, t))
    assert d == info["d"] == emb.shape[1] and np.array_equal(mean, info["mean"]) and np.array_equal(comps, info["components"])
    assert np.array_equal(_bits(emb), _bits(R.project(c2, R.size_columns(R.SIZES, t), mean, comps)))


def _rows(seed, n, d):
    """n rows (no multiple of any tile or chunk), the last 41 of them copies of earlier rows, in a few loose groups"""
    rng = np.random.RandomState(seed)
    y = rng.randn(n, d) + 3.0 * rng.randn(5, d)[rng.randint(5, size=n)]
    y[n - 41:] = y[rng.randint(n - 41, size=41)]
    return y


@pytest.mark.parametrize("d,k", [(1, 1), (1, 7), (5, 2), (5, 64), (43, 7), (43, 1), (150, 64), (150, 2)])
def test_kmeans_bit_equal_to_numpy_oracle(d, k):
    from multiplexed_image_annotator_amd import regions
    n = 2311
    y = _rows(100 * d + k, n, d)
    ref_trace = []
    ref_labels, ref_centres, ref_iters, ref_inertia, ref_picks = R.kmeans(y, k, seed=5, trace=ref_trace)
    trace, info = [], {}
    labels = regions.kmeans(y, k, seed=5, timings=info, trace=trace)
    assert info["picks"] == ref_picks
    assert info["iterations"] == ref_iters == len(trace) == len(ref_trace)
    for it, ((gl, gc), (rl, rc)) in enumerate(zip(trace, ref_trace)):
        assert np.array_equal(gl, rl), f"labels of iteration {it}"
        assert np.array_equal(_bits(gc), _bits(rc)), f"centres of iteration {it}"
    assert labels.dtype == np.int64 and np.array_equal(labels, ref_labels)
    assert np.array_equal(_bits(info["centres"]), _bits(ref_centres))
    assert np.array_equal(_bits(np.float64(info["inertia"])), _bits(np.float64(ref_inertia)))
    info2 = {}
    assert np.array_equal(regions.kmeans(y, k, seed=5, timings=info2), labels) and np.array_equal(_bits(info2["centres"]), _bits(info["centres"]))
    if k > 1:
        other = {}
        regions.kmeans(y, k, seed=6, timings=other)
        assert other["picks"] != info["picks"]


def test_kmeans_plusplus_device_steps_bit_equal():
    """the distance work of one k-means++ step: min with the running minimum and the fixed-order potentials"""
    from multiplexed_image_annotator_amd import ops
    n, d = 5003, 43
    y = _rows(9, n, d)
    yd = torch.from_numpy(y).to(_dev())
    closest = R.dist2(y, y[[17]])[:, 0]
    cand = [3, 4100, 17, 5002, 2999]
    d2, pot = ops.kmeans_trials(yd, torch.tensor(cand, dtype=torch.int32, device=yd.device), torch.from_numpy(closest).to(yd.device))
    ref = np.minimum(closest[:, None], R.dist2(y, y[cand]))
    assert np.array_equal(_bits(d2.cpu().numpy().T), _bits(ref))
    assert np.array_equal(_bits(pot.cpu().numpy()), _bits(np.array([R.chunked_sum(ref[:, t]) for t in range(len(cand))])))
    first, _ = ops.kmeans_trials(yd, torch.tensor([17], dtype=torch.int32, device=yd.device), None)
    assert np.array_equal(_bits(first.cpu().numpy()[0]), _bits(closest))


def test_kmeans_empty_cluster_case_bit_equal():
    from multiplexed_image_annotator_amd import regions
    base = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 9.0]])
    y = np.repeat(base, 40, axis=0)[np.random.RandomState(0).permutation(120)]
    ref_trace, trace, info = [], [], {}
    ref_labels, ref_centres, ref_iters, _, ref_picks = R.kmeans(y, 5, seed=0, trace=ref_trace)
    labels = regions.kmeans(y, 5, seed=0, timings=info, trace=trace)
    assert info["picks"] == ref_picks and info["iterations"] == ref_iters
    for (gl, gc), (rl, rc) in zip(trace, ref_trace):
        assert np.array_equal(gl, rl) and np.array_equal(_bits(gc), _bits(rc))
    assert np.array_equal(labels, ref_labels)


def test_requests_out_of_range_are_statuses_or_value_errors():
    from multiplexed_image_annotator_amd import _lib, ops, regions
    dev = _dev()
    y = torch.from_numpy(_rows(1, 300, 4)).to(dev)
    labels = torch.full((300,), -1, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.RibcaError, match="k <= 256"):
        ops.kmeans_assign(y, torch.zeros((257, 4), dtype=torch.float64, device=dev), labels, None, changed)
    with pytest.raises(_lib.RibcaError, match="k <= n"):
        ops.kmeans_assign(y[:3].contiguous(), torch.zeros((5, 4), dtype=torch.float64, device=dev), labels, None, changed)
    wide = torch.zeros((4, 2033), dtype=torch.float64, device=dev)
    with pytest.raises(_lib.RibcaError, match="d <= 2032"):
        ops.kmeans_assign(wide, wide[:2].contiguous(), labels, None, changed)
    with pytest.raises(ValueError, match="n_samples=300 should be >= n_clusters=301"):
        regions.kmeans(y, 301)
    with pytest.raises(ValueError, match="n_clusters"):
        regions.kmeans(y, 0)
    assert (labels == -1).all()      # nothing ran


def test_planted_bands_match_sklearn_from_the_same_centres():
    """>= 3000 cells in planted bands, from the centroids on: GPU counts -> PCA -> k-means.  From the same initial centres scikit-learn's Lloyd
    gives the same labels, and the planted bands are recovered no worse than by scikit-learn's own PCA + KMeans (adjusted Rand index)."""
    from sklearn.cluster import KMeans
    from sklearn.decomposition import PCA
    from sklearn.metrics import adjusted_rand_score
    from multiplexed_image_annotator_amd import ops, regions
    n, t, bands = 4000, 9, 4
    x, y, types, band = synth.planted_bands(n, t, bands, 4242)
    counts = ops.knn_composition_counts(x, y, types, t)
    emb = regions.pca_project(counts, ops.TISSUE_NEIGHBOURHOODS)
    info = {}
    labels = regions.kmeans(emb, bands, seed=0, timings=info)
    yh = emb.cpu().numpy()
    km = KMeans(n_clusters=bands, init=yh[info["picks"]], n_init=1).fit(yh)
    assert np.array_equal(km.labels_, labels) and km.n_iter_ == info["iterations"]
    table = ops.knn_compositions(x, y, types, t)
    sk = KMeans(n_clusters=bands, random_state=0).fit_predict(PCA(n_components=0.99).fit_transform(table))
    ari_gpu, ari_sk = adjusted_rand_score(band, labels), adjusted_rand_score(band, sk)
    print(f"[regions] planted bands: ARI gpu {ari_gpu:.4f}, scikit-learn {ari_sk:.4f}", file=sys.__stdout__, flush=True)
    assert ari_gpu >= ari_sk - 0.01


# ------------------------------------------------------------------------------------------------------------------------ Annotator
def _write_case(root, seed):
    mask, img = synth.make_mask_and_image(320, 352, 330, 7, seed)
    os.makedirs(root, exist_ok=True)
    np.save(os.path.join(root, "img.npy"), img.numpy().astype(np.uint16))
    np.save(os.path.join(root, "mask.npy"), mask.numpy().astype(np.int32))
    with open(os.path.join(root, "markers.txt"), "w") as f:
        f.write("\n".join(synth.BASIC_PANEL_MARKERS) + "\n")
    with open(os.path.join(root, "images.csv"), "w") as f:
        f.write(f"image_path,mask_path\n{os.path.join(root, 'img.npy')},{os.path.join(root, 'mask.npy')}\n")


def _run(root, out, seed, write=True):
    """the image of test_tissue_regions_end_to_end through predict -> tissue_region_analysis(3) -> export -> colorize"""
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", os.path.join(root, out), "t", True, False, -1, True,
                  0.3, 99.8, 0.3, 30, None)
    a.set_weights({"immune_base": synth.make_vit_state_dict("immune_base", seed, depth=2)})
    a.preprocess()
    a.predict(32)
    a.tissue_region_analysis(3)
    if write:
        a.export_annotations()
        a.colorize(from_script=True)
    return a


def _files(root, out):
    res = os.path.join(root, out, "results")
    return open(os.path.join(res, "t_annotation_0.csv"), "rb").read(), open(os.path.join(res, "t_tissue_region_0.png"), "rb").read()


def test_annotator_regions_are_reproducible_and_seeded(tmp_path, monkeypatch):
    monkeypatch.delenv("RIBCA_REGIONS", raising=False)
    monkeypatch.delenv("RIBCA_REGION_SEED", raising=False)
    seed = synth.SEED_BASE + 81
    root = str(tmp_path)
    _write_case(root, seed)
    a, b = _run(root, "a", seed), _run(root, "b", seed)
    assert a.tissue_regions == b.tissue_regions and set(a.tissue_regions[0].values()) <= {0, 1, 2}
    assert all(type(v) is int for v in a.tissue_regions[0].values())
    assert _files(root, "a") == _files(root, "b")
    st = a.region_stats[0]
    assert st["backend"] == "gpu" and st["seed"] == 0 and st["k"] == 3 and st["n"] == len(a.preprocessor.cell_ids[0])
    assert st["F"] == 8 * len(a.cell_types) and 1 <= st["d"] <= st["F"] and 1 <= st["iterations"] <= 300
    assert st["pca_ms"] > 0 and st["kmeans_ms"] > 0
    monkeypatch.setenv("RIBCA_REGION_SEED", "1")
    c = _run(root, "c", seed, write=False)
    assert c.region_stats[0]["seed"] == 1 and sorted(c.tissue_regions[0]) == sorted(a.tissue_regions[0])
    with pytest.raises(ValueError, match="n_clusters"):
        c.tissue_region_analysis(0)
    monkeypatch.setenv("RIBCA_REGIONS", "host")
    with pytest.raises(ValueError, match="RIBCA_REGIONS"):
        c.tissue_region_analysis(3)


_CHILD = """
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import test_gpu_regions as T
from multiplexed_image_annotator_amd import synth
a = T._run({case!r}, "child_" + os.environ["RIBCA_REGIONS"], synth.SEED_BASE + 81, write=False)
assert len(a.tissue_regions[0]) == len(a.preprocessor.cell_ids[0]) and set(a.tissue_regions[0].values()) <= {{0, 1, 2}}
print("SKLEARN_IMPORTED", int(any(m == "sklearn" or m.startswith("sklearn.") for m in sys.modules)))
"""


@pytest.mark.parametrize("backend", ["gpu", "sklearn"])
def test_backend_switch_decides_whether_scikit_learn_is_imported(tmp_path, backend):
    root = str(tmp_path)
    _write_case(root, synth.SEED_BASE + 81)
    env = dict(os.environ, RIBCA_REGIONS=backend)
    env.pop("RIBCA_REGION_SEED", None)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, case=root)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"SKLEARN_IMPORTED {1 if backend == 'sklearn' else 0}" in r.stdout, r.stdout


def _rank_body(rank, root, seed):
    """One rank of the cell-sharded Annotator (both ranks share the device; gloo carries the all-gather): every rank computes the regions on
    its own, no collective, and returns them."""
    a = _run(root, "sharded", seed, write=False)
    return sorted(a.tissue_regions[0].items())


def test_two_ranks_agree_with_each_other_and_with_one_rank(tmp_path, monkeypatch):
    monkeypatch.delenv("RIBCA_REGIONS", raising=False)
    monkeypatch.delenv("RIBCA_REGION_SEED", raising=False)
    seed = synth.SEED_BASE + 81
    root = str(tmp_path)
    _write_case(root, seed)
    r0, r1 = two_ranks(_rank_body, root, seed, tile=None)
    one = _run(root, "single", seed, write=False)
    assert r0 == r1 == [[k, v] for k, v in sorted(one.tissue_regions[0].items())]
