"""Annotator(min_cells > 0) end to end (reference model.py:642-675): the "Others" cells of a planted image are re-clustered into
"Additional type c" labels that reach the CSV, the colourised index image and the neighbourhood analysis."""
import os

import numpy as np
import pytest
import torch

from batch_harness import planted_case, run_annotator, threshold, two_ranks, weights

pytestmark = pytest.mark.gpu


def test_extra_cell_types_end_to_end(tmp_path):
    from sklearn.metrics import adjusted_rand_score
    from multiplexed_image_annotator_amd import ops
    root = str(tmp_path / "case")
    planted = planted_case(root)
    thr = threshold(root, str(tmp_path))
    base = run_annotator(root, str(tmp_path / "base"), -1, thr)
    a = run_annotator(root, str(tmp_path / "extra"), 20, thr)
    ids = a.preprocessor.cell_ids[0].tolist()
    others = [j for j, n in enumerate(base.annotations[0]) if n == "Others"]
    assert 0.5 * len(ids) < len(others) < len(ids)
    # non-"Others" cells are untouched
    for j, n in enumerate(base.annotations[0]):
        if n != "Others":
            assert a.annotations[0][j] == n and a.confidence[0][j] == base.confidence[0][j]
    # every pooled cell: confidence -1, a new name or "Others"
    got = [a.annotations[0][j] for j in others]
    assert all(a.confidence[0][j] == -1 for j in others)
    assert all(n == "Others" or n.startswith("Additional type ") for n in got)
    lab = np.array([int(n.split()[-1]) if n != "Others" else -1 for n in got])
    truth = np.array([planted[ids[j]] for j in others])
    clustered = lab >= 0
    assert clustered.mean() > 0.9, clustered.mean()
    ari = adjusted_rand_score(truth[clustered], lab[clustered])
    print(f"[extra cell types] {len(others)} pooled, {lab.max() + 1} clusters, {int((~clustered).sum())} noise, ARI {ari:.3f}; {a.extra_stats}")
    assert ari >= 0.9
    # CSV carries the new names, and two runs write the same bytes
    csv = open(tmp_path / "extra" / "results" / "x_annotation_0.csv").read()
    assert "Additional type 0" in csv
    b = run_annotator(root, str(tmp_path / "extra2"), 20, thr)
    assert open(tmp_path / "extra2" / "results" / "x_annotation_0.csv").read() == csv
    # cell types: np.sort of the names, "Others" last; colorize / neighbourhood use the same indices
    assert list(a.cell_types[:-1]) == sorted(a.cell_types[:-1]) and a.cell_types[-1] == "Others"
    _, _, tidx = (t.cpu().numpy() for t in a.paint(0))
    mk = a.preprocessor.masks[0] if isinstance(a.preprocessor.masks[0], np.ndarray) else np.load(os.path.join(root, "mask.npy"))
    names = list(a.cell_types)
    for j in range(0, len(ids), 7):
        px = tidx[mk == ids[j]]
        assert (px == names.index(a.annotations[0][j]) + 1).all()
    ints = a._cell_type_ints(0)
    assert [names[t] for t in ints] == a.annotations[0]
    a.neighborhood_analysis(integrate=True, normalize=False)
    m = a.neighborhood_matrix([0], 25)
    assert m.shape == (len(names), len(names)) and m.sum() == 24 * len(ids)
    from oracle import ref_spatial
    tab = a.preprocessor.cell_tables[0]
    x = tab[:, 5].astype(np.float64) / tab[:, 6]
    y = tab[:, 4].astype(np.float64) / tab[:, 6]
    assert np.array_equal(m, ref_spatial.cooccurrence(x, y, ints, len(names), 25))


def test_cli_min_cells_runs_to_the_end(tmp_path):
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
        cli.main(["--marker-list-path", os.path.join(root, "markers.txt"), "--image-path", os.path.join(root, "img.npy"), "--mask-path",
                  os.path.join(root, "mask.npy"), "--batch-id", "c", "--main-dir", str(tmp_path / "out"), "--no-infer", "--bs", "16",
                  "--min-cells", "10", "--confidence", "0.9"])
    finally:
        os.chdir(cwd)
    res = tmp_path / "out" / "results"
    assert (res / "c_annotation_0.csv").exists() and (res / "c_colorized_annotation_0.png").exists()
    assert (res / "c_integrated_neighborhood.csv").exists()


def _rank_body(rank, root, thr):
    a = run_annotator(root, os.path.join(root, "sharded"), 20, thr, batch="r")
    assert not a.tile_mode


def test_two_ranks_match_single_rank_with_extra_types(tmp_path):
    root = str(tmp_path / "case")
    planted_case(root, n_cells=200, h=300, w=340)
    thr = threshold(root, str(tmp_path))
    two_ranks(_rank_body, root, thr, tile=None)
    one = run_annotator(root, os.path.join(root, "single"), 20, thr, batch="r")
    assert any(n.startswith("Additional type") for n in one.annotations[0])
    a = open(os.path.join(root, "sharded", "results", "r_annotation_0.csv")).read()
    b = open(os.path.join(root, "single", "results", "r_annotation_0.csv")).read()
    assert a == b
