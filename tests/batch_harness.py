"""What the end-to-end tests of the Annotator share: the planted cases and their synthetic weights, one annotated two-image batch per analysis,
the command line run with and without an analysis' switch, and two gloo ranks on one device.  A plain module: the tests import what they use
by name, and nothing here needs a GPU before it is called."""
import hashlib
import json
import os
import socket
import tempfile

import numpy as np
import torch

from multiplexed_image_annotator_amd import synth

# the immune_base panel and five markers no panel uses: one classifier, whose vote sends a cell below the confidence threshold to "Others"
MARKERS = ['CD45', 'CD20', 'CD4', 'CD8', 'DAPI', 'CD11c', 'CD3', 'Ki67', 'HLA-DR', 'CD14', 'CD57', 'Bcl2']
SEED = synth.SEED_BASE + 83


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
def planted_case(root, n_cells=400, h=416, w=480):
    """the synth mask; every cell gets one of 4 marker profiles (a few bright channels each) with 5 % multiplicative pixel noise"""
    mask, _ = synth.make_mask_and_image(h, w, n_cells, len(MARKERS), SEED, want_image=False)
    mk = mask.numpy().astype(np.int32)
    rng = np.random.RandomState(SEED % (1 << 32))
    prof = np.full((4, len(MARKERS)), 150.0)
    for p in range(4):
        prof[p, rng.choice(len(MARKERS), 3, replace=False)] = rng.uniform(3000, 8000, 3)
    ids = np.unique(mk[mk > 0])
    planted = {int(c): int(rng.randint(4)) for c in ids}
    lut = np.zeros((mk.max() + 1, len(MARKERS)))
    for c, p in planted.items():
        lut[c] = prof[p]
    img = lut[mk].transpose(2, 0, 1) * (1 + 0.05 * rng.randn(len(MARKERS), h, w))
    raw = np.clip(img, 0, 65535).astype(np.uint16)
    os.makedirs(root, exist_ok=True)
    np.save(os.path.join(root, "img.npy"), raw)
    np.save(os.path.join(root, "mask.npy"), mk)
    with open(os.path.join(root, "markers.txt"), "w") as f:
        f.write("\n".join(MARKERS) + "\n")
    with open(os.path.join(root, "images.csv"), "w") as f:
        f.write(f"image_path,mask_path\n{os.path.join(root, 'img.npy')},{os.path.join(root, 'mask.npy')}\n")
    return planted


def two_image_case(root):
    """two planted images of different sizes in one batch CSV"""
    planted_case(os.path.join(root, "a"))
    planted_case(os.path.join(root, "b"), n_cells=250, h=320, w=360)
    with open(os.path.join(root, "markers.txt"), "w") as f:
        f.write(open(os.path.join(root, "a", "markers.txt")).read())
    with open(os.path.join(root, "images.csv"), "w") as f:
        f.write("image_path,mask_path\n")
        for d in ("a", "b"):
            f.write(f"{os.path.join(root, d, 'img.npy')},{os.path.join(root, d, 'mask.npy')}\n")


def write_case(tmp_path, raw, mask, markers):
    np.save(tmp_path / "img.npy", raw)
    np.save(tmp_path / "mask.npy", mask)
    (tmp_path / "markers.txt").write_text("\n".join(markers) + "\n")
    (tmp_path / "images.csv").write_text(f"image_path,mask_path\n{tmp_path / 'img.npy'},{tmp_path / 'mask.npy'}\n")
    return str(tmp_path / "markers.txt"), str(tmp_path / "images.csv")


def paint_faults(mask):
    """the four faults, placed by what the mask holds; returns the label of the cell whose hole keeps a foreign speck"""
    from scipy import ndimage
    mask = mask.copy()
    h, w = mask.shape
    solid = (ndimage.minimum_filter(mask, size=9) == ndimage.maximum_filter(mask, size=9)) & (mask > 0)      # 9 x 9 of one label around
    rr, cc = np.nonzero(solid)
    centres = {}
    for r, c in zip(rr.tolist(), cc.tolist()):
        centres.setdefault(int(mask[r, c]), (r, c))
    ids = sorted(centres)
    assert len(ids) >= 6
    a, b, holed, outer, foreign = ids[0], ids[-1], ids[1], ids[2], ids[3]
    mask[mask == b] = a                                   # a label torn in two: cell b becomes a second piece of a
    r, c = centres[holed]
    mask[r, c] = 0                                        # a hole of one pixel
    r, c = centres[outer]
    mask[r - 2:r + 3, c - 2:c + 3] = 0                    # a hole of 5 x 5 ...
    mask[r:r + 2, c:c + 2] = foreign                      # ... with four pixels of another cell's label inside
    empty = ndimage.maximum_filter(mask, size=7) == 0
    r, c = np.argwhere(empty)[0]
    mask[r, c:c + 2] = ids[4]                             # a speck of two pixels in open background
    return mask, outer


def load_config1(golden_dir, tmp_path):
    """BASELINE.json configs[0] stand-in: the reference's example_1 mask (1850 cells, from cellpos.npz) + the seeded 7-channel image."""
    meta = json.load(open(os.path.join(golden_dir, "config1.json")))
    arrs = np.load(os.path.join(golden_dir, "config1.npz"))
    mask = np.load(os.path.join(golden_dir, "cellpos.npz"))["example1_mask"].astype(np.int32)
    raw = synth.make_image_for_mask(torch.from_numpy(mask), len(meta["markers"]), meta["seed"]).numpy().astype(np.uint16)
    assert hashlib.sha256(raw.tobytes()).hexdigest() == meta["img_sha"]
    assert hashlib.sha256(mask.tobytes()).hexdigest() == meta["mask_sha"]
    sd = synth.make_vit_state_dict("immune_base", meta["seed"])
    sd["head.bias"] = torch.from_numpy(arrs["head_bias"])
    mf = tmp_path / "markers.txt"
    mf.write_text("\n".join(meta["markers"]) + "\n")
    return meta, arrs, raw, mask, {"immune_base": sd}, str(mf)


def neighborhood_inputs(golden_dir, cname):
    """the centroids, cell types and type names behind the golden neighbourhood CSVs of ``cname``, and those goldens"""
    from oracle import ref_preprocess, ref_spatial
    g = json.load(open(os.path.join(golden_dir, "neighborhood.json")))
    if cname == "big":
        mask, _ = synth.make_mask_and_image(640, 700, 1500, 1, synth.SEED_BASE + 151, want_image=False)
        types, names = np.array(g["big_types"]), ["A", "B", "C", "D", "E", "Others"]
    else:
        m = json.load(open(os.path.join(golden_dir, "e2e.json")))[cname]
        mask, _ = synth.make_mask_and_image(m["h"], m["w"], m["cells"], len(m["markers"]), m["seed"], want_image=False)
        types, names = np.array(m["type_ints"]), m["cell_types"]
    ids, table = ref_preprocess.cell_table(mask.numpy().astype(np.int32))
    x, y = ref_spatial.centroids(table)
    return g, x, y, types, names


# ---- one annotated run ---------------------------------------------------------------------------------------------------------------------------
def weights():
    sd = synth.make_vit_state_dict("immune_base", SEED, depth=2)
    sd["head.bias"] = sd["head.bias"].clone()
    sd["head.bias"][3] -= 10.0      # class 3 of immune_base is "Others": the random model then votes a cell type, and the threshold decides
    return {"immune_base": sd}


def run_annotator(root, out, min_cells, confidence, batch="x"):
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", out, batch, False, False, min_cells, True, 0.3,
                  99.8, confidence, 30, None)
    a.set_weights(weights())
    a.preprocess()
    a.predict(16)
    a.export_annotations()
    return a


def preprocessed(root, out, batch="x"):
    """preprocess() only, for the steps that need no classifier"""
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = Annotator(os.path.join(root, "markers.txt"), os.path.join(root, "images.csv"), "cuda", out, batch, False, False, -1, True, 0.3, 99.8, 0.0, 30,
                  None)
    a.preprocess()
    return a


def threshold(root, tmp):
    """a confidence threshold that sends most, not all, cells to "Others": the 85th percentile of the unthresholded confidences"""
    a = run_annotator(root, os.path.join(tmp, "probe"), -1, 0.0)
    return float(np.quantile(a._conf_arrays[0], 0.85))


def result_files(out, needle):
    """{name: bytes} of out/results, sorted, for the names that contain ``needle`` (a tuple: any of them)"""
    needles = (needle,) if isinstance(needle, str) else needle
    res = os.path.join(out, "results")
    return {f: open(os.path.join(res, f), "rb").read() for f in sorted(os.listdir(res)) if any(k in f for k in needles)}


def annotated_batch(tmp_path_factory, name, analyse, needle):
    """the two-image batch annotated once, with a confidence threshold at the median so that "Others" is one of the cell types, and analysed:
    ``analyse(a)`` returns what the fixture keeps as "integrated" """
    tmp = tmp_path_factory.mktemp(name)
    root = str(tmp / "case")
    os.makedirs(root)
    two_image_case(root)
    probe = run_annotator(root, str(tmp / "probe"), -1, 0.0)
    thr = float(np.median(np.concatenate(probe._conf_arrays)))
    out = str(tmp / "one")
    a = run_annotator(root, out, -1, thr)
    integrated = analyse(a)
    return {"root": root, "tmp": str(tmp), "thr": thr, "a": a, "out": out, "integrated": integrated, "files": result_files(out, needle)}


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------
def cli_runs(tmp_path, runs, needle, case=None):
    """main.main on one planted image once per entry of ``runs`` ({directory under tmp_path: extra arguments}; "off": [] is one of them).
    Without the switch no file of the analysis is written, and a run with it leaves every other file name as it was.  Returns the sorted
    listing of every run's results and the arguments all of them share."""
    import main as cli
    assert runs["off"] == []
    root = str(tmp_path / "case")
    planted_case(root, **(case or {"n_cells": 150, "h": 256, "w": 300}))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        mdir = "src/multiplexed_image_annotator/cell_type_annotation/models"
        os.makedirs(mdir)
        for m, sd in weights().items():
            torch.save({"model": sd}, os.path.join(mdir, m + ".pth"))
        common = ["--marker-list-path", os.path.join(root, "markers.txt"), "--image-path", os.path.join(root, "img.npy"), "--mask-path",
                  os.path.join(root, "mask.npy"), "--batch-id", "c", "--no-infer", "--bs", "16", "--confidence", "0.0", "--n-regions", "0"]
        for name, extra in runs.items():
            cli.main(common + ["--main-dir", str(tmp_path / name)] + extra)
    finally:
        os.chdir(cwd)
    listing = {name: sorted(os.listdir(tmp_path / name / "results")) for name in runs}
    off = listing["off"]
    assert not [f for f in off if needle in f]
    for name in runs:
        if name != "off":
            assert [f for f in listing[name] if needle not in f] == off, name
    return listing, common


# ---- two ranks -----------------------------------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank(rank, port, tile, unset, results, body, args):
    import torch.distributed as tdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if tile is not None:
        os.environ["RIBCA_TILE_MODE"] = "1" if tile else "0"
    for name in unset:
        os.environ.pop(name, None)
    tdist.init_process_group("gloo", rank=rank, world_size=2)
    with open(os.path.join(results, f"rank{rank}.json"), "w") as f:
        json.dump(body(rank, *args), f)
    tdist.barrier()
    tdist.destroy_process_group()


def two_ranks(body, *args, tile=True, unset=()):
    """``body(rank, *args)``, a module-level function of the calling test file, on two gloo ranks that share the device; returns what the two
    calls returned (through JSON).  ``tile``: RIBCA_TILE_MODE=1 / 0 in the children, None: the batch decides; ``unset``: variables they drop."""
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as results:
        mp.spawn(_rank, args=(free_port(), tile, tuple(unset), results, body, args), nprocs=2, join=True)
        return [json.load(open(os.path.join(results, f"rank{r}.json"))) for r in (0, 1)]
