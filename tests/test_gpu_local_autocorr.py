"""The local indicators of spatial association on the GPU: ribca_local_lag and ribca_local_perm_counts (csrc/local_autocorr.hip) against
tests/local_autocorr_numpy.py byte for byte (workspace and outputs pre-filled with junk), skipped neighbours, batch edges, split additivity,
repeatability, seeds, and Annotator.local_autocorrelation() end to end: files, the CSVs against the oracle computed from the same tables, every
painted pixel, reruns, seeds, a marker selection, errors, two ranks."""
import io
import os

import numpy as np
import pytest
import torch

import autocorr_numpy as AN
import enrichment_numpy as EN
import local_autocorr_numpy as LN
from batch_harness import planted_case, preprocessed, result_files, two_image_case, two_ranks, weights
from kernel_harness import junk
from multiplexed_image_annotator_amd import _lib, colors, local_autocorr, ops
from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _gpu_lag(z, idx):
    dev = _lib.require_gpu()
    n, c = z.shape
    zd = torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
    out = junk(n * c * 8, dev).view(torch.float64).reshape(n, c)
    status = lib().ribca_local_lag(ptr(zd), ptr(idx_d), n, c, idx.shape[1], ptr(out), stream_ptr())
    torch.cuda.synchronize()
    return status, out.cpu().numpy()


def _gpu_counts(z, idx, lag, seed, image, p0, p):
    dev = _lib.require_gpu()
    n, c = z.shape
    zd = torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
    lag_d = torch.from_numpy(np.ascontiguousarray(lag)).to(dev)
    need = ops.local_perm_counts_ws_bytes(n, c, p)
    ws = junk(need, dev)
    ge = junk(n * c * 4, dev).view(torch.int32).reshape(n, c)
    le = junk(n * c * 4, dev).view(torch.int32).reshape(n, c)
    status = lib().ribca_local_perm_counts(ptr(zd), ptr(idx_d), ptr(lag_d), n, c, idx.shape[1], seed, image, p0, p, ptr(ge), ptr(le), ptr(ws), need,
                                           stream_ptr())
    torch.cuda.synchronize()
    return status, ge.cpu().numpy().astype(np.int64), le.cpu().numpy().astype(np.int64)


def _check_counts(z, idx, seed, image, p0, p):
    lag = LN.lag(z, idx)
    status, ge, le = _gpu_counts(z, idx, lag, seed, image, p0, p)
    assert status == 0, lib().ribca_last_error()
    want_ge, want_le = LN.perm_counts(z, idx, lag, seed, image, p0, p)
    assert np.array_equal(ge, want_ge) and np.array_equal(le, want_le), (z.shape, idx.shape[1], seed, image, p0, p)
    return ge, le


@pytest.mark.parametrize("n,c,m", AN.SHAPES)
def test_byte_equal_to_numpy(n, c, m):
    """the lists are random over [0, n): self entries, duplicates and sigma(j) == i all occur (at n = 2 and 5 in most permutations)"""
    z, idx = AN.random_table(n, c, m)
    status, got = _gpu_lag(z, idx)
    assert status == 0, lib().ribca_last_error()
    assert got.tobytes() == LN.lag(z, idx).tobytes(), (n, c, m)
    for p, seed, image, p0 in ((3, 0, 0, 0), (3, 12345678901234567890, 3, 40)):
        ge, le = _check_counts(z, idx, seed, image, p0, p)
        assert ge.max() <= p and le.max() <= p and (ge + le >= p).all()      # no junk of the workspace or the outputs survives


def test_neighbours_out_of_range_are_skipped():
    n, c, m = 300, 3, 6
    z, idx = AN.random_table(n, c, m)
    idx[7, 2], idx[9, 0], idx[11, 5], idx[299, 3] = n, -1, 2 ** 31 - 1, -(2 ** 31)
    idx[20] = -1      # a cell without a neighbour: lag = +0.0, every permuted sum ties with it
    idx[30, 1] = 30
    status, got = _gpu_lag(z, idx)
    assert status == 0 and got.tobytes() == LN.lag(z, idx).tobytes()
    assert (got[20] == 0.0).all() and not np.signbit(got[20]).any()
    ge, le = _check_counts(z, idx, 1, 0, 0, 3)
    assert (ge[20] == 3).all() and (le[20] == 3).all()


def test_batch_edges():
    # more permutations than one batch of rows holds (32)
    z, idx = AN.random_table(300, 5, 6)
    _check_counts(z, idx, 2, 1, 0, 33)
    # the byte rule: 64 MiB of rows hold 14 permutations of 9000 cells x 64 channels, P = 15 takes a batch of 14 and one of 1
    n, c, m, p = 9000, 64, 3, 15
    need = ops.local_perm_counts_ws_bytes(n, c, p)
    assert need == 14 * n * c * 8 + (14 * n * 4 + 255) // 256 * 256 and 14 * n * c * 8 <= 64 << 20 < 15 * n * c * 8
    z, idx = AN.random_table(n, c, m)
    _check_counts(z, idx, 0, 0, 0, p)


def test_split_additivity_repeatability_seeds_and_the_wrappers():
    z, idx = AN.random_table(700, 15, 24)
    lag = LN.lag(z, idx)
    status, ge7, le7 = _gpu_counts(z, idx, lag, 4, 2, 0, 7)
    assert status == 0
    status, ge5, le5 = _gpu_counts(z, idx, lag, 4, 2, 0, 5)
    assert status == 0
    status, ge2, le2 = _gpu_counts(z, idx, lag, 4, 2, 5, 2)
    assert status == 0 and np.array_equal(ge7, ge5 + ge2) and np.array_equal(le7, le5 + le2)
    status, ge, le = _gpu_counts(z, idx, lag, 4, 2, 0, 7)
    assert status == 0 and np.array_equal(ge, ge7) and np.array_equal(le, le7)
    # the wrappers: the same numbers; another image number or seed, other counts
    dev = _lib.require_gpu()
    zd, idx_d = torch.from_numpy(z).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev)
    lag_d = ops.local_lag(zd, idx_d)
    assert lag_d.cpu().numpy().tobytes() == lag.tobytes()
    counts = lambda *key, **kw: [t.cpu().numpy() for t in ops.local_perm_counts(zd, idx_d, lag_d, *key, **kw)]
    got = counts(4, 2, 0, 7)
    assert got[0].dtype == np.int64 and np.array_equal(got[0], ge7) and np.array_equal(got[1], le7)
    got = counts(4, 2, 0, 7, ws=junk(ops.local_perm_counts_ws_bytes(700, 15, 7), dev))
    assert np.array_equal(got[0], ge7) and np.array_equal(got[1], le7)
    assert not np.array_equal(counts(4, 3, 0, 7)[0], ge7)
    assert not np.array_equal(counts(5, 2, 0, 7)[0], ge7)
    with pytest.raises(ValueError, match="not finite"):
        ops.local_lag(torch.full_like(zd, float("nan")), idx_d)
    with pytest.raises(ValueError, match="not finite"):
        ops.local_perm_counts(torch.full_like(zd, float("inf")), idx_d, lag_d, 0, 0, 0, 1)
    with pytest.raises(ValueError, match="local_perm_counts"):
        ops.local_perm_counts(zd, idx_d, lag_d[:5], 0, 0, 0, 1)
    with pytest.raises(_lib.RibcaError, match="ribca_local_perm_counts"):
        ops.local_perm_counts(zd, idx_d, lag_d, 0, 0, 0, 0)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
P_TEST = 39      # with alpha = 1/20: significant iff no permutation reaches the observed lag on one side


def _slugs(a):
    return [''.join(ch if ch.isascii() and ch.isalnum() else '_' for ch in str(m)) for m in a.channel_parser.markers]


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    os.environ.pop("RIBCA_LOCAL_SEED", None)
    tmp = tmp_path_factory.mktemp("local_autocorr")
    root = str(tmp / "case")
    os.makedirs(root)
    two_image_case(root)
    out = str(tmp / "one")
    a = preprocessed(root, out)
    assert a.local_autocorrelation(n_perms=P_TEST) is None
    return {"root": root, "tmp": str(tmp), "a": a, "out": out, "files": result_files(out, "local_autocorr"), "stats": list(a.local_autocorr_stats)}


def _oracle(a, i, seed, p, k=25, alpha=0.05):
    """from the same tables: the centring and the sums of squares in the order of ribca_group_sums, the brute-force list, the numpy counts
    keyed with the batch-wide image number"""
    tab = a.preprocessor.cell_tables[i]
    x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
    y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
    z, d = AN.centred(a.preprocessor.intensity_full[i])
    idx = EN.knn_list(x, y, k)
    lag = LN.lag(z, idx)
    ge, le = LN.perm_counts(z, idx, lag, seed, a._image_number(i), 0, p)
    return local_autocorr.statistics(z, lag, ge, le, d, k - 1, p, alpha)


def test_files_tables_and_maps_are_the_oracle_s(batch):
    from PIL import Image
    a, files = batch["a"], batch["files"]
    markers = [str(m) for m in a.channel_parser.markers]
    slugs = _slugs(a)
    assert len(markers) >= 3
    assert sorted(files) == sorted(f"x_local_autocorr_{i}{tail}" for i in (0, 1) for tail in [".csv", "_summary.csv"] + [f"_{s}.png" for s in slugs])
    assert len(batch["stats"]) == 2
    for i in (0, 1):
        want = _oracle(a, i, 0, P_TEST)
        ids = a.preprocessor.cell_ids[i]
        text = files[f"x_local_autocorr_{i}.csv"].decode()
        assert text == local_autocorr.table_csv(ids, markers, want)
        rows = [l.split(",") for l in text.strip().split("\n")]
        assert [int(r[0]) for r in rows[1:]] == [int(v) for v in ids] and len(rows[0]) == 1 + 8 * len(markers)
        cls = np.array([[int(r[8 + 8 * k]) for k in range(len(markers))] for r in rows[1:]])
        assert np.array_equal(cls, want["class"])
        summary = files[f"x_local_autocorr_{i}_summary.csv"].decode().strip().split("\n")
        assert summary[0] == "marker,cells,not_significant,HH,LH,LL,HL"
        for k, line in enumerate(summary[1:]):
            assert line.split(",") == [markers[k], str(len(ids))] + [str(int((cls[:, k] == v).sum())) for v in range(5)]
        mask = a.preprocessor.masks[i]
        for k, s in enumerate(slugs):
            img = np.array(Image.open(io.BytesIO(files[f"x_local_autocorr_{i}_{s}.png"])))
            expect = np.zeros(mask.shape + (3,), dtype=np.uint8)      # the background stays 0
            lut = np.zeros((int(mask.max()) + 1, 3), dtype=np.uint8)
            lut[np.asarray(ids, dtype=np.int64)] = colors.LISA_COLORS[cls[:, k]]
            expect[mask > 0] = lut[mask[mask > 0]]
            assert np.array_equal(img, expect), (i, s)
        rec = batch["stats"][i]
        assert rec["file"] == f"x_local_autocorr_{i}.csv" and rec["n"] == len(ids) and rec["C"] == len(markers) and rec["P"] == P_TEST
        assert rec["seed"] == 0 and rec["neighbors"] == 25 and rec["alpha"] == (1, 20) and rec["significant"] == int((cls > 0).sum())
        assert all(rec[t] >= 0.0 for t in ("knn_ms", "perm_ms", "draw_ms")) and len(rec["files"]) == 2 + len(markers)
    log = open(a.logger.log_file_path).read()
    assert log.count("Local autocorrelation x_local_autocorr_0.csv: ") == 1


def test_rerun_seed_and_marker_selection(batch, monkeypatch):
    out = os.path.join(batch["tmp"], "two")
    b = preprocessed(batch["root"], out)
    b.local_autocorrelation(n_perms=P_TEST)
    assert result_files(out, "local_autocorr") == batch["files"]
    monkeypatch.setenv("RIBCA_LOCAL_SEED", "5")
    b.local_autocorrelation(n_perms=P_TEST)
    seeded = result_files(out, "local_autocorr")
    name = "x_local_autocorr_1.csv"
    assert seeded[name] != batch["files"][name] and b.local_autocorr_stats[1]["seed"] == 5
    markers = [str(m) for m in b.channel_parser.markers]
    assert seeded[name].decode() == local_autocorr.table_csv(b.preprocessor.cell_ids[1], markers, _oracle(b, 1, 5, P_TEST))
    keep = [0] + [1 + 8 * k + f for k in range(len(markers)) for f in range(4)]      # cell_id, z, lag, local_i, gi_star: no permutation in them
    cut = lambda text: [[l.split(",")[j] for j in keep] for l in text.decode().strip().split("\n")]
    assert cut(seeded[name]) == cut(batch["files"][name])
    monkeypatch.delenv("RIBCA_LOCAL_SEED")
    # one marker: its columns and its PNG alone, the same numbers
    one = os.path.join(batch["tmp"], "three")
    c = preprocessed(batch["root"], one)
    c.local_autocorrelation(n_perms=P_TEST, markers=[markers[1]])
    got = result_files(one, "local_autocorr")
    assert sorted(got) == sorted(f"x_local_autocorr_{i}{tail}" for i in (0, 1) for tail in (".csv", "_summary.csv", f"_{_slugs(c)[1]}.png"))
    for i in (0, 1):
        full = [l.split(",") for l in batch["files"][f"x_local_autocorr_{i}.csv"].decode().strip().split("\n")]
        assert [l.split(",") for l in got[f"x_local_autocorr_{i}.csv"].decode().strip().split("\n")] == [r[:1] + r[9:17] for r in full]
        png = f"x_local_autocorr_{i}_{_slugs(c)[1]}.png"
        assert got[png] == batch["files"][png]
    assert c.local_autocorr_stats[0]["C"] == 1 and c.local_autocorr_stats[0]["markers"] == [markers[1]]


def test_errors_leave_the_files_alone(batch):
    a = batch["a"]
    with pytest.raises(ValueError, match="n_perms"):
        a.local_autocorrelation(n_perms=0)
    with pytest.raises(ValueError, match="fewer than n_neighbors"):
        a.local_autocorrelation(n_neighbors=100000, n_perms=2)
    with pytest.raises(ValueError, match="is not one of the markers"):
        a.local_autocorrelation(n_perms=2, markers=["no such marker"])
    with pytest.raises(ValueError, match="alpha"):
        a.local_autocorrelation(n_perms=2, alpha=0)
    wide = a.preprocessor.intensity_full
    a.preprocessor.intensity_full = [np.zeros((len(t), 65)) for t in wide]
    try:
        with pytest.raises(ValueError, match="at most 64 channels"):
            a.local_autocorrelation(n_perms=2)
    finally:
        a.preprocessor.intensity_full = wide
    assert result_files(batch["out"], "local_autocorr") == batch["files"]
    from multiplexed_image_annotator_amd.annotator import Annotator
    fresh = Annotator(os.path.join(batch["root"], "markers.txt"), os.path.join(batch["root"], "images.csv"), "cuda", os.path.join(batch["tmp"], "fresh"), "x",
                      False, False, -1, True, 0.3, 99.8, 0.0, 30, None)
    with pytest.raises(ValueError, match="preprocess"):
        fresh.local_autocorrelation(n_perms=2)


def test_pipeline_switch(tmp_path):
    """--local-autocorr-perms 0 (the default) is off; N > 0 writes the per-image files beside the neighbourhood matrix"""
    import main as cli
    root = str(tmp_path / "case")
    planted_case(root, n_cells=150, h=256, w=300)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        mdir = "src/multiplexed_image_annotator/cell_type_annotation/models"
        os.makedirs(mdir)
        for m, sd in weights().items():
            torch.save({"model": sd}, os.path.join(mdir, m + ".pth"))
        common = ["--marker-list-path", os.path.join(root, "markers.txt"), "--image-path", os.path.join(root, "img.npy"), "--mask-path",
                  os.path.join(root, "mask.npy"), "--batch-id", "c", "--no-infer", "--bs", "16", "--confidence", "0.0", "--n-regions", "0"]
        assert cli.parse_args(common + ["--main-dir", "x"]).local_autocorr_perms == 0
        cli.main(common + ["--main-dir", str(tmp_path / "on"), "--local-autocorr-perms", "8"])
    finally:
        os.chdir(cwd)
    on = sorted(f for f in os.listdir(tmp_path / "on" / "results") if "local_autocorr" in f)
    markers = [l.strip() for l in open(os.path.join(root, "markers.txt")) if l.strip()]
    assert "c_local_autocorr_0.csv" in on and "c_local_autocorr_0_summary.csv" in on and len(on) == 2 + len(markers)


def _rank_body(rank, root):
    os.environ["RIBCA_SHARE_GPU"] = "1"
    a = preprocessed(root, os.path.join(root, "tiles"))
    assert a.tile_mode
    a.local_autocorrelation(n_perms=P_TEST)
    return [s["file"] for s in a.local_autocorr_stats]


def test_two_ranks_tile_per_rank_write_the_single_rank_bytes(batch):
    wrote = two_ranks(_rank_body, batch["root"], unset=("RIBCA_LOCAL_SEED",))
    assert result_files(os.path.join(batch["root"], "tiles"), "local_autocorr") == batch["files"]
    assert wrote == [["x_local_autocorr_0.csv"], ["x_local_autocorr_1.csv"]]
