"""The spatial autocorrelation on the GPU: ribca_autocorr_observed and ribca_autocorr_perm (csrc/autocorr.hip) against tests/autocorr_numpy.py bit
for bit (workspace and outputs pre-filled with junk), batch edges, split invariance, skipped neighbours, and
Annotator.spatial_autocorrelation() end to end: files, the CSV against the oracle computed from the same tables, the PNG rectangle against the
rasteriser, reruns, seeds, per-image files, two ranks."""
import io
import os

import numpy as np
import pytest
import torch

import autocorr_numpy as AN
import enrichment_numpy as EN
from batch_harness import cli_runs, preprocessed, result_files, run_annotator, two_image_case, two_ranks
from kernel_harness import junk
from multiplexed_image_annotator_amd import _lib, autocorr, colors, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _gpu_observed(z, idx):
    dev = _lib.require_gpu()
    n, c = z.shape
    zd = torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
    need = ops.autocorr_observed_ws_bytes(n, c)
    ws = junk(need, dev)
    out = junk(2 * c * 8, dev).view(torch.float64).reshape(2, c)
    status = lib().ribca_autocorr_observed(ptr(zd), ptr(idx_d), n, c, idx.shape[1], ptr(out), ptr(ws), need, stream_ptr())
    torch.cuda.synchronize()
    return status, out.cpu().numpy()


def _gpu_perm(z, idx, seed, image, p0, p):
    dev = _lib.require_gpu()
    n, c = z.shape
    zd = torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
    need = ops.autocorr_perm_ws_bytes(n, c, p)
    ws = junk(need, dev)
    out = junk(p * 2 * c * 8, dev).view(torch.float64).reshape(p, 2, c)
    status = lib().ribca_autocorr_perm(ptr(zd), ptr(idx_d), n, c, idx.shape[1], seed, image, p0, p, ptr(out), ptr(ws), need, stream_ptr())
    torch.cuda.synchronize()
    return status, out.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n,c,m", AN.SHAPES)
def test_bit_equal_to_numpy(n, c, m):
    z, idx = AN.random_table(n, c, m)
    status, got = _gpu_observed(z, idx)
    assert status == 0, lib().ribca_last_error()
    assert _same_bits(got, AN.observed(z, idx)), (n, c, m)
    for p, seed, image, p0 in ((3, 0, 0, 0), (3, 12345678901234567890, 3, 40)):
        status, got = _gpu_perm(z, idx, seed, image, p0, p)
        assert status == 0, lib().ribca_last_error()
        assert _same_bits(got, AN.perm(z, idx, seed, image, p0, p)), (n, c, m, seed)
        assert np.isfinite(got).all()      # no junk of the workspace or the output survives


def test_batch_edges():
    # more permutations than one batch of rows holds (32)
    z, idx = AN.random_table(300, 5, 6)
    status, got = _gpu_perm(z, idx, 2, 1, 0, 33)
    assert status == 0 and _same_bits(got, AN.perm(z, idx, 2, 1, 0, 33))
    # the byte rule: 64 MiB of rows hold 14 permutations of 9000 cells x 64 channels, P = 15 takes a batch of 14 and one of 1
    n, c, m, p = 9000, 64, 3, 15
    rows = ops.autocorr_perm_ws_bytes(n, c, p) - (36 * 14 * 2 * c * 8 + 255) // 256 * 256
    assert rows == 14 * n * c * 8 and rows <= 64 << 20 < 15 * n * c * 8
    z, idx = AN.random_table(n, c, m)
    status, got = _gpu_perm(z, idx, 0, 0, 0, p)
    assert status == 0 and _same_bits(got, AN.perm(z, idx, 0, 0, 0, p))


def test_split_invariance_and_repeatability():
    z, idx = AN.random_table(700, 15, 24)
    status, all7 = _gpu_perm(z, idx, 4, 2, 0, 7)
    assert status == 0
    status, last2 = _gpu_perm(z, idx, 4, 2, 5, 2)
    assert status == 0 and _same_bits(all7[5:], last2)
    status, again = _gpu_perm(z, idx, 4, 2, 0, 7)
    assert status == 0 and _same_bits(again, all7)
    status, o1 = _gpu_observed(z, idx)
    status2, o2 = _gpu_observed(z, idx)
    assert status == 0 and status2 == 0 and _same_bits(o1, o2)
    # the wrappers: the same numbers; another image number or seed, other permutations
    dev = _lib.require_gpu()
    zd, idx_d = torch.from_numpy(z).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev)
    assert _same_bits(ops.autocorr_observed(zd, idx_d).cpu().numpy(), o1)
    assert _same_bits(ops.autocorr_perm(zd, idx_d, 4, 2, 0, 7).cpu().numpy(), all7)
    ws = junk(ops.autocorr_perm_ws_bytes(700, 15, 7), dev)
    assert _same_bits(ops.autocorr_perm(zd, idx_d, 4, 2, 0, 7, ws=ws).cpu().numpy(), all7)
    assert not _same_bits(ops.autocorr_perm(zd, idx_d, 4, 3, 0, 7).cpu().numpy(), all7)
    assert not _same_bits(ops.autocorr_perm(zd, idx_d, 5, 2, 0, 7).cpu().numpy(), all7)
    with pytest.raises(ValueError, match="not finite"):
        ops.autocorr_observed(torch.full_like(zd, float("nan")), idx_d)
    with pytest.raises(_lib.RibcaError, match="ribca_autocorr_perm"):
        ops.autocorr_perm(zd, idx_d, 0, 0, 0, 0)


def test_neighbours_out_of_range_are_skipped():
    n, c, m = 300, 3, 6
    z, idx = AN.random_table(n, c, m)
    idx[7, 2], idx[9, 0], idx[11, 5], idx[299, 3] = n, -1, 2 ** 31 - 1, -(2 ** 31)
    idx[20] = -1      # a cell without a neighbour: s = g = +0.0
    s, g = np.zeros((n, c)), np.zeros((n, c))
    for i in range(n):
        for q in range(m):
            if 0 <= idx[i, q] < n:
                s[i] = s[i] + z[idx[i, q]]
                g[i] = g[i] + (z[i] - z[idx[i, q]]) * (z[i] - z[idx[i, q]])
    want = np.stack([AN.tree(z * s), AN.tree(g)])
    status, got = _gpu_observed(z, idx)
    assert status == 0 and _same_bits(got, want) and _same_bits(got, AN.observed(z, idx))
    status, got = _gpu_perm(z, idx, 1, 0, 0, 3)
    assert status == 0 and _same_bits(got, AN.perm(z, idx, 1, 0, 0, 3))


def test_refusals_are_a_status_and_nothing_runs():
    dev = _lib.require_gpu()
    z, idx = AN.random_table(100, 3, 24)
    zd, idx_d = torch.from_numpy(z).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev)
    out = torch.full((2, 2, 3), -1.0, dtype=torch.float64, device=dev)
    need = ops.autocorr_perm_ws_bytes(100, 3, 2)
    ws = junk(need, dev)
    assert lib().ribca_autocorr_perm(ptr(zd), ptr(idx_d), 100, 3, 24, 0, 0, 0, 2, ptr(out), ptr(ws), need - 1, stream_ptr()) == 1
    assert lib().ribca_last_error() == b"ribca_autocorr_perm: workspace too small"
    assert lib().ribca_autocorr_perm(ptr(zd), ptr(idx_d), 100, 3, 32, 0, 0, 0, 2, ptr(out), ptr(ws), need, stream_ptr()) == 1
    assert lib().ribca_last_error() == b"ribca_autocorr_perm: needs 1 <= m <= 31"
    assert lib().ribca_autocorr_observed(ptr(zd), ptr(idx_d), 100, 65, 24, ptr(out), ptr(ws), need, stream_ptr()) == 1
    assert lib().ribca_last_error() == b"ribca_autocorr_observed: needs 1 <= C <= 64"
    assert lib().ribca_autocorr_observed(ptr(zd), None, 100, 3, 24, ptr(out), ptr(ws), need, stream_ptr()) == 1
    assert lib().ribca_last_error() == b"ribca_autocorr_observed: NULL buffer"
    torch.cuda.synchronize()
    assert (out == -1.0).all() and (ws == 255).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
P_TEST = 12


def _analyse(a):
    assert a.spatial_autocorrelation(n_perms=P_TEST, integrate=True) is None
    integrated = list(a.autocorr_stats)
    assert a.spatial_autocorrelation(n_perms=P_TEST, integrate=False) is None
    return integrated


EXPECTED = sorted(f"x_{s}.{e}" for s in ("integrated_spatial_autocorr", "spatial_autocorr_0", "spatial_autocorr_1") for e in ("csv", "png"))


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    os.environ.pop("RIBCA_AUTOCORR_SEED", None)
    tmp = tmp_path_factory.mktemp("autocorr")
    root = str(tmp / "case")
    os.makedirs(root)
    two_image_case(root)
    out = str(tmp / "one")
    a = run_annotator(root, out, -1, 0.0)
    integrated = _analyse(a)
    return {"root": root, "tmp": str(tmp), "a": a, "out": out, "integrated": integrated, "files": result_files(out, "spatial_autocorr")}


def _oracle(a, images, seed, p, k=25):
    """from the same tables: per image the centring and the sums of squares in the order of ribca_group_sums, the brute-force list, the numpy
    numerators keyed with the batch-wide image number; the images added from +0.0 in ascending order"""
    width = a.preprocessor.intensity_full[images[0]].shape[1]
    obs, null, m2, cells = np.zeros((2, width)), np.zeros((p, 2, width)), np.zeros(width), 0
    for i in images:
        tab = a.preprocessor.cell_tables[i]
        x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
        y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
        z, d = AN.centred(a.preprocessor.intensity_full[i])
        idx = EN.knn_list(x, y, k)
        obs = obs + AN.observed(z, idx)
        null = null + AN.perm(z, idx, seed, a._image_number(i), 0, p)
        m2 = m2 + d
        cells += len(z)
    return autocorr.statistics(obs, null, m2, cells, k - 1), cells


def _check(a, files, stem, images, stats, seed=0):
    from PIL import Image
    want, cells = _oracle(a, images, seed, P_TEST)
    markers = [str(m) for m in a.channel_parser.markers]
    assert files[stem + ".csv"].decode() == autocorr.table_csv(markers, cells, want)
    lines = files[stem + ".csv"].decode().strip().split("\n")
    assert lines[0] == autocorr.COLUMNS and [l.split(",")[0] for l in lines[1:]] == markers and len(markers) >= 3
    first = lines[1].split(",")
    assert np.array([float(first[2])]).tobytes() == np.array([want["i"][0]]).tobytes() and int(first[1]) == cells
    assert stats["file"] == stem + ".png" and stats["n"] == cells and stats["C"] == len(markers) and stats["P"] == P_TEST and stats["seed"] == seed
    assert stats["neighbors"] == 25 and all(stats[k] >= 0.0 for k in ("knn_ms", "perm_ms", "draw_ms"))
    img = np.array(Image.open(io.BytesIO(files[stem + ".png"])))
    top, left = stats["rect"]
    values = autocorr.figure_values(want)
    rect = img[top:top + len(markers) * a.HEATMAP_CELL, left:left + 2 * a.HEATMAP_CELL]
    dev = _lib.require_gpu()
    lut = colors.diverging_table()
    raster = ops.table_raster(torch.from_numpy(values).to(dev), torch.from_numpy(lut).to(dev), a.HEATMAP_CELL, a.HEATMAP_GAP, -1.0, 1.0).cpu().numpy()
    assert np.array_equal(rect, raster) and np.array_equal(rect, EN.table_raster(values, lut, a.HEATMAP_CELL, a.HEATMAP_GAP, -1.0, 1.0))
    return want


def test_files_and_table_are_the_oracle_s(batch):
    a, files = batch["a"], batch["files"]
    assert sorted(files) == EXPECTED
    assert len(batch["integrated"]) == 1 and len(a.autocorr_stats) == 2
    want = _check(a, files, "x_integrated_spatial_autocorr", [0, 1], batch["integrated"][0])
    assert np.isfinite(want["i"]).any() and (want["i_null_std"] > 0).any() and np.isfinite(want["c_z"]).any()
    for i in (0, 1):
        _check(a, files, f"x_spatial_autocorr_{i}", [i], a.autocorr_stats[i])
    log = open(a.logger.log_file_path).read()
    assert log.count("Spatial autocorrelation x_integrated_spatial_autocorr.png: ") == 1


def test_a_second_run_writes_the_same_bytes_and_a_seed_changes_the_null(batch, monkeypatch):
    out = os.path.join(batch["tmp"], "two")
    b = preprocessed(batch["root"], out)
    _analyse(b)
    assert len(b.annotations) == 0 and result_files(out, "spatial_autocorr") == batch["files"]      # no predict(): the step needs none, and writes the same bytes without
    monkeypatch.setenv("RIBCA_AUTOCORR_SEED", "5")
    b.spatial_autocorrelation(n_perms=P_TEST, integrate=True)
    seeded = result_files(out, "spatial_autocorr")
    name = "x_integrated_spatial_autocorr.csv"
    assert seeded[name] != batch["files"][name] and b.autocorr_stats[0]["seed"] == 5
    cut = lambda text: [l.split(",")[:3] + l.split(",")[8:9] for l in text.decode().strip().split("\n")]      # marker, cells, I and C stay
    assert cut(seeded[name]) == cut(batch["files"][name])
    _check(b, seeded, "x_integrated_spatial_autocorr", [0, 1], b.autocorr_stats[0], seed=5)
    assert {k: v for k, v in seeded.items() if "integrated" not in k} == {k: v for k, v in batch["files"].items() if "integrated" not in k}
    assert seeded["x_integrated_spatial_autocorr.png"] == batch["files"]["x_integrated_spatial_autocorr.png"]      # the figure shows I and C alone


def test_errors_leave_the_files_alone(batch):
    a = batch["a"]
    with pytest.raises(ValueError, match="n_perms"):
        a.spatial_autocorrelation(n_perms=0)
    with pytest.raises(ValueError, match="fewer than n_neighbors"):
        a.spatial_autocorrelation(n_neighbors=100000, n_perms=2)
    with pytest.raises(_lib.RibcaError, match="k must be in"):
        a.spatial_autocorrelation(n_neighbors=33, n_perms=2, integrate=False)
    assert result_files(batch["out"], "spatial_autocorr") == batch["files"]
    from multiplexed_image_annotator_amd.annotator import Annotator
    fresh = Annotator(os.path.join(batch["root"], "markers.txt"), os.path.join(batch["root"], "images.csv"), "cuda", os.path.join(batch["tmp"], "fresh"), "x",
                      False, False, -1, True, 0.3, 99.8, 0.0, 30, None)
    with pytest.raises(ValueError, match="preprocess"):
        fresh.spatial_autocorrelation(n_perms=2)


def test_pipeline_switch(tmp_path):
    """--autocorr-perms 0 (the default) writes no such file; N > 0 writes the integrated pair beside the neighbourhood matrix"""
    import main as cli
    listing, common = cli_runs(tmp_path, {"off": [], "on": ["--autocorr-perms", "8"]}, "autocorr")
    on = listing["on"]
    assert [f for f in on if "autocorr" in f] == ["c_integrated_spatial_autocorr.csv", "c_integrated_spatial_autocorr.png"]
    assert cli.parse_args(common + ["--main-dir", "x"]).autocorr_perms == 0


def _rank_body(rank, root):
    os.environ["RIBCA_SHARE_GPU"] = "1"
    a = run_annotator(root, os.path.join(root, "tiles"), -1, 0.0)
    assert a.tile_mode
    _analyse(a)
    return [s["file"] for s in a.autocorr_stats]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], unset=("RIBCA_AUTOCORR_SEED",))
    assert result_files(os.path.join(batch["root"], "tiles"), "spatial_autocorr") == batch["files"]
    assert wrote == [["x_spatial_autocorr_0.png"], ["x_spatial_autocorr_1.png"]]      # the per-image call came last
