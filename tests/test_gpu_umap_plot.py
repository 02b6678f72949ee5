"""The whole-batch UMAP plot: csrc/scatter.hip against tests/scatter_numpy.py byte for byte, the 2-D embedding from the GPU spectral start on planted
blobs, and Annotator.umap_visualization() end to end (reference model.py:746-765)."""
import os

import numpy as np
import pytest
import torch

import scatter_numpy as SC
import umap_restatement as R
from batch_harness import planted_case, run_annotator, two_ranks
from multiplexed_image_annotator_amd import _lib, manifold, ops

pytestmark = pytest.mark.gpu


def _gpu_raster(pts, rgb, h, w, aff, radius):
    dev = _lib.require_gpu()
    img, skipped = ops.scatter_raster(torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(dev), torch.from_numpy(rgb).to(dev), h, w, aff, radius)
    return img.cpu().numpy(), skipped


def test_raster_small_cases():
    h, w = 9, 12
    ident = (1.0, 0.0, 1.0, 0.0)
    red, green, blue = [200, 10, 10], [10, 200, 10], [10, 10, 200]
    # one point
    img, skipped = _gpu_raster([[5.0, 4.0]], np.array([red], dtype=np.uint8), h, w, ident, 2)
    want, _, index = SC.raster([[5.0, 4.0]], [red], h, w, ident, 2)
    assert skipped == 0 and np.array_equal(img, want) and (index > 0).sum() == 21 and (img[4, 5] == red).all() and (img[0, 0] == 255).all()
    # two coincident points: the later colour wins everywhere
    img, _ = _gpu_raster([[5.0, 4.0], [5.0, 4.0]], np.array([red, green], dtype=np.uint8), h, w, ident, 2)
    assert np.array_equal(img, SC.raster([[5.0, 4.0]], [green], h, w, ident, 2)[0])
    # points on the canvas edge and corners (discs clipped), just off it (skipped), a half-way centre (rint: half to even) and bad rows
    pts = np.array([[0.0, 0.0], [11.0, 8.0], [11.4, 8.4], [11.5, 8.0], [-0.5, 0.0], [-0.6, 3.0], [2.5, 3.5], [np.nan, 1.0], [1.0, np.inf],
                    [-np.inf, np.nan], [3e38, 3e38]], dtype=np.float32)
    rgb = np.random.RandomState(0).randint(0, 255, (len(pts), 3)).astype(np.uint8)
    for radius in (0, 2):
        img, skipped = _gpu_raster(pts, rgb, h, w, ident, radius)
        want, wskip, index = SC.raster(pts, rgb, h, w, ident, radius)
        assert skipped == wskip == 6 and np.array_equal(img, want)      # 11.5 -> 12 and -0.6 -> -1 are off; -0.5 -> -0 is on
        assert index[4, 2] == 7 or radius == 2      # (2.5, 3.5) -> column 2, row 4
    # no point at all: a white canvas
    img, skipped = _gpu_raster(np.zeros((0, 2), dtype=np.float32), np.zeros((0, 3), dtype=np.uint8), h, w, ident, 2)
    assert skipped == 0 and (img == 255).all()
    dev = _lib.require_gpu()
    with pytest.raises(ValueError):
        ops.scatter_raster(torch.zeros((3, 2), dtype=torch.float64, device=dev), torch.zeros((3, 3), dtype=torch.uint8, device=dev), h, w, ident)
    with pytest.raises(_lib.RibcaError, match="ribca_scatter_raster"):
        ops.scatter_raster(torch.zeros((3, 2), device=dev), torch.zeros((3, 3), dtype=torch.uint8, device=dev), h, w, ident, radius=17)


@pytest.mark.parametrize("h,w", [(64, 96), (1200, 1600)])
def test_raster_random_points_match_numpy(h, w):
    rng = np.random.RandomState(h)
    pts = (rng.randn(5000, 2) * [3.0, 0.7] + [10.0, -4.0]).astype(np.float32)
    pts[17] = np.nan
    rgb = rng.randint(0, 256, (5000, 3)).astype(np.uint8)
    aff = ops.scatter_affine(pts, h, w)
    assert np.allclose(aff, SC.affine(pts, h, w), rtol=1e-15, atol=0)
    for radius in (0, 2):
        img, skipped = _gpu_raster(pts, rgb, h, w, aff, radius)
        want, wskip, index = SC.raster(pts, rgb, h, w, aff, radius)
        assert skipped == wskip == 1
        assert np.array_equal(img, want)
        assert (index > 0).sum() > (2000 if h > 100 else 500)      # the oracle drew something: overlaps exist, later points on top


BLOB_SIZES = (45, 90, 135, 180, 225, 300, 375, 450)      # umap_restatement.planted_blobs scaled to 1 800 blob points + 90 noise points


def test_two_component_embedding_from_the_gpu_start():
    """ARI >= 0.95 and trustworthiness >= 0.9, the thresholds of tests/test_gpu_umap.py for 5 components: confirmed for 2 components on the
    numpy restatement (tests/umap_restatement.py with the start of either backend, seeds 0..2; the values are in DESIGN.md section 12)."""
    from sklearn.cluster import HDBSCAN
    from sklearn.manifold import trustworthiness
    from sklearn.metrics import adjusted_rand_score
    x, y = R.planted_blobs(0, sizes=BLOB_SIZES)
    assert len(x) == 1890
    t = {}
    emb = manifold.umap_embed(x, n_components=2, seed=0, spectral="gpu", timings=t)
    assert emb.shape == (1890, 2) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert t["spectral_backend"] == "gpu" and t["spectral_iterations"] >= 1 and t["spectral_spmm"] > 0 and t["init"] > 0
    assert np.array_equal(emb, manifold.umap_embed(x, n_components=2, seed=0, spectral="gpu"))
    t2 = {}
    other = manifold.umap_embed(x, n_components=2, seed=0, timings=t2)      # the default stays on eigsh
    assert t2["spectral_backend"] == "scipy" and "spectral_iterations" not in t2 and other.shape == emb.shape
    lab = HDBSCAN(min_cluster_size=20).fit(emb).labels_
    blob = y >= 0
    ari = adjusted_rand_score(y[blob], lab[blob])
    tw = trustworthiness(x, emb, n_neighbors=5)
    print(f"[umap 2-D, gpu start] n = {len(x)}: ARI {ari:.4f} on the blob points, trustworthiness {tw:.4f}; {t}")
    assert ari >= 0.95 and tw >= 0.9


def _files(out, batch):
    res = os.path.join(out, "results")
    return open(os.path.join(res, f"{batch}_umap.png"), "rb").read(), open(os.path.join(res, f"{batch}_umap.csv")).read()


def _check_plot(a, emb, out, batch):
    from PIL import Image
    n = sum(len(x) for x in a.annotations)
    assert emb.shape == (n, 2) and emb.dtype == np.float32
    png, csv = _files(out, batch)
    img = np.array(Image.open(os.path.join(out, "results", f"{batch}_umap.png")))
    h, w = a.UMAP_CANVAS
    assert img.shape == (h, w, 3) and (h, w) == (1200, 1600)
    names = [name for per in a.annotations for name in per]
    types = {str(c): k for k, c in enumerate(a.cell_types)}
    rgb = np.array(a.colors, dtype=np.uint8)[[types[n_] for n_ in names]]
    want, skipped, index = SC.raster(emb, rgb, h, w, SC.affine(emb, h, w), 2)
    assert skipped == 0 and np.array_equal(img, want)
    assert np.array_equal((img != 255).any(axis=2), ((want != 255).any(axis=2)))
    lines = csv.strip().split("\n")
    assert lines[0] == "Image,Cell Index,Cell Type,UMAP 1,UMAP 2" and len(lines) == n + 1
    ids = [int(c) for i in range(len(a.annotations)) for c in a.preprocessor.cell_ids[i]]
    for k in range(0, n, 13):
        img_no, cell, name, u, v = lines[1 + k].split(",")
        assert int(img_no) == 0 and int(cell) == ids[k] and name == names[k]
        assert np.float32(u) == emb[k, 0] and np.float32(v) == emb[k, 1]
    return png, csv


def test_umap_visualization_end_to_end(tmp_path, monkeypatch):
    monkeypatch.delenv("RIBCA_SPECTRAL", raising=False)
    # the planted profiles may fall apart into components of about a hundred cells, which the rule would leave on eigsh: lower the
    # threshold so that the GPU solver lays out every component of this small batch
    monkeypatch.setattr(manifold, "SPECTRAL_GPU_MIN_ROWS", 16)
    root = str(tmp_path / "case")
    planted_case(root)
    out1, out2, out3 = (str(tmp_path / d) for d in ("one", "two", "three"))
    a = run_annotator(root, out1, -1, 0.0)
    emb = a.umap_visualization()
    assert emb is not None      # the parent commit logs "skipped", returns None and writes nothing
    png, csv = _check_plot(a, emb, out1, "x")
    s = a.umap_stats
    assert s["n"] == len(emb) and s["spectral_backend"] == "gpu" and s["spectral_gpu_components"] >= 1 and s["spectral_iterations"] >= 0 and s["seed"] == 0 and s["skipped_points"] == 0
    assert len(set(a.annotations[0])) >= 2      # more than one colour on the canvas
    b = run_annotator(root, out2, -1, 0.0)
    assert np.array_equal(b.umap_visualization(), emb)
    assert _files(out2, "x") == (png, csv)
    monkeypatch.setenv("RIBCA_SPECTRAL", "scipy")
    c = run_annotator(root, out3, -1, 0.0)
    emb_c = c.umap_visualization()
    _check_plot(c, emb_c, out3, "x")
    assert c.umap_stats["spectral_backend"] == "scipy" and c.umap_stats["spectral_iterations"] is None
    monkeypatch.setenv("RIBCA_SPECTRAL", "bogus")
    with pytest.raises(ValueError, match="RIBCA_SPECTRAL"):
        c.umap_visualization()


def test_umap_visualization_before_predict_and_on_tiny_batches(tmp_path):
    from multiplexed_image_annotator_amd.annotator import Annotator
    root = str(tmp_path / "case")
    planted_case(root, n_cells=150, h=256, w=300)
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", str(tmp_path / "o"), "t", False, False, -1, True, 0.3,
                  99.8, 0.0, 30, None)
    with pytest.raises(ValueError, match="No annotations to visualize"):
        a.umap_visualization()
    a.annotations = [["Others", "Others", "B cell"]]      # fewer than 4 cells: logged and skipped, as before
    assert a.umap_visualization() is None
    assert not os.path.exists(os.path.join(str(tmp_path / "o"), "results", "t_umap.png"))


def _rank_body(rank, root):
    a = run_annotator(root, os.path.join(root, "sharded"), -1, 0.0, batch="r")
    assert not a.tile_mode
    emb = a.umap_visualization()
    assert emb is not None and emb.shape == (sum(len(x) for x in a.annotations), 2)
    np.save(os.path.join(root, f"emb_rank{rank}.npy"), emb)


def test_two_ranks_only_rank0_writes(tmp_path):
    root = str(tmp_path / "case")
    planted_case(root, n_cells=200, h=300, w=340)
    two_ranks(_rank_body, root, tile=None)
    e0, e1 = np.load(os.path.join(root, "emb_rank0.npy")), np.load(os.path.join(root, "emb_rank1.npy"))
    assert np.array_equal(e0, e1)
    one = run_annotator(root, os.path.join(root, "single"), -1, 0.0, batch="r")
    assert np.array_equal(one.umap_visualization(), e0)
    assert _files(os.path.join(root, "sharded"), "r") == _files(os.path.join(root, "single"), "r")
    found = [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(root, "sharded")) for f in fs if "umap" in f]
    assert sorted(os.path.basename(f) for f in found) == ["r_umap.csv", "r_umap.png"], found
