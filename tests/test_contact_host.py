"""The cell contact graph without a GPU: the two forms of the restatement against each other (tests/contact_numpy.py), the version, every refusal
of the two entry points and their workspace queries (a status whose text names the entry point, before any HIP call), the host module on a
hand-made graph of five cells whose every number is written out here, the command-line switches, the refusals of Annotator.contact_analysis that
need no device, and the statistic on a planted contact, restatement only."""
import ctypes
import types

import numpy as np
import pytest

import contact_numpy as CN
from multiplexed_image_annotator_amd import _lib, contact, enrichment

CAP = 1 << 21


def test_version():
    assert _lib.lib().ribca_version() >= 106


def test_the_offsets_of_the_disk():
    assert [len(CN.offsets(d)) for d in range(1, 9)] == [4, 12, 28, 48, 80, 112, 148, 196] == list(contact.DISK_OFFSETS)
    assert sorted(CN.offsets(1)) == [(-1, 0), (0, -1), (0, 1), (1, 0)]


def test_the_two_forms_of_the_restatement_agree():
    mask = CN.random_mask(60, 70, 40, 11)
    mask[mask == 7] = 90          # a label past the table
    mask[0:2, 0:3] = -4           # negative labels
    mask[58:60, 60:70] = 3        # the label 3 in a second blob
    table, n = CN.identity_table(np.where(mask < 60, mask, 0))
    table[5] = -1                 # an unmapped label
    table[9] = n + 3              # mapped past the cells
    for d in (1, 2, 3):
        loop = CN.pair_weights_loop(mask, table, n, d)
        fast = CN.pair_weights(mask, table, n, d)
        assert loop == fast and len(loop) > 20
        assert all(loop[(j, i)] == w for (i, j), w in loop.items())      # w is symmetric
        assert all(i != j and 0 <= i < n and 0 <= j < n for i, j in loop)
        assert not [k for k in loop if 4 in k or 8 in k or 6 in k]          # the cells of the labels 5, 9 and 7 own no pixel
    # at d = 1 the weight is the shared border in pixel edges: two 3 x 4 blocks side by side share 3
    two = np.zeros((5, 10), dtype=np.int32)
    two[1:4, 1:5], two[1:4, 5:9] = 1, 2
    assert CN.pair_weights(two, np.array([-1, 0, 1], dtype=np.int32), 2, 1) == {(0, 1): 3, (1, 0): 3}
    nbr, pairs, degree = CN.table(CN.pair_weights(two, np.array([-1, 0, 1], dtype=np.int32), 2, 2), 2, 8)
    assert nbr.tolist() == [[1] + [-1] * 7, [0] + [-1] * 7] and pairs[:, 0].tolist() == [3 + 2 * 2 + 2 * 3, 13] and degree.tolist() == [1, 1]


def test_refusals_are_a_status_naming_the_entry_point():
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)      # never dereferenced: every case below is refused by its sizes, before any HIP call
    big = 1 << 40

    def refused(status, text):
        assert status == 1
        msg = lib.ribca_last_error()
        assert msg and msg.startswith(text.encode()), (text, msg)

    name = "ribca_contact_table"

    def table(mask=p, H=64, W=64, l2c=p, L=10, n=9, d=1, S=32, nbr=p, pairs=p, degree=p, over=p, ws=p, ws_bytes=big):
        return lib.ribca_contact_table(mask, H, W, l2c, L, n, d, S, nbr, pairs, degree, over, ws, ws_bytes, None)

    for hole in ("mask", "l2c", "nbr", "pairs", "degree", "over", "ws"):
        refused(table(**{hole: None}), f"{name}: NULL buffer")
    sizes = f"{name}: needs 1 <= H, W and H W < 2^31"
    refused(table(H=0), sizes)
    refused(table(W=0), sizes)
    refused(table(H=1 << 16, W=1 << 15), sizes)
    refused(table(L=0), f"{name}: needs 1 <= L")
    refused(table(n=0), f"{name}: needs 1 <= n <= 2^21")
    refused(table(n=CAP + 1), f"{name}: needs 1 <= n <= 2^21")
    refused(table(d=0), f"{name}: needs 1 <= d <= 8")
    refused(table(d=9), f"{name}: needs 1 <= d <= 8")
    for s in (0, 4, 24, 2048, -32):
        refused(table(S=s), f"{name}: S must be a power of two in 8 .. 1024")
    need = lib.ribca_contact_table_ws_bytes(64, 64, 9, 32)
    assert need > 0 and need % 256 == 0 and need >= 12 * 9 * 32 + 4 * 9
    refused(table(ws_bytes=need - 1), f"{name}: workspace too small")
    for h, w, n, s in ((0, 64, 9, 32), (64, 0, 9, 32), (1 << 16, 1 << 15, 9, 32), (64, 64, 0, 32), (64, 64, CAP + 1, 32), (64, 64, 9, 0), (64, 64, 9, 24),
                       (64, 64, 9, 2048)):
        assert lib.ribca_contact_table_ws_bytes(h, w, n, s) == 0
    assert lib.ribca_contact_table_ws_bytes((1 << 16) - 1, 1 << 15, 9, 32) == need      # the mask is read in place: no piece depends on H, W
    assert lib.ribca_contact_table_ws_bytes(64, 64, 1024, 64) - lib.ribca_contact_table_ws_bytes(64, 64, 1024, 32) == 12 * 1024 * 32

    name = "ribca_edge_perm_counts"

    def null(src=p, dst=p, E=5, t=p, n=8, T=3, image=0, p0=0, P=4, counts=p, ws=p, ws_bytes=big):
        return lib.ribca_edge_perm_counts(src, dst, E, t, n, T, 0, image, p0, P, counts, ws, ws_bytes, None)

    for hole in ("src", "dst", "t", "counts", "ws"):
        refused(null(**{hole: None}), f"{name}: NULL buffer")
    refused(null(E=0), f"{name}: needs 1 <= E < 2^31")
    refused(null(E=1 << 31), f"{name}: needs 1 <= E < 2^31")
    refused(null(n=0), f"{name}: needs 1 <= n <= 2^30")
    refused(null(n=(1 << 30) + 1), f"{name}: needs 1 <= n <= 2^30")
    refused(null(T=0), f"{name}: needs 1 <= T <= 64")
    refused(null(T=65), f"{name}: needs 1 <= T <= 64")
    window = f"{name}: needs image >= 0, p0 >= 0, 1 <= P, p0 + P <= 2^31"
    refused(null(P=0), window)
    refused(null(p0=(1 << 31) - 3, P=4), window)
    refused(null(p0=-1), window)
    refused(null(image=-1), window)
    need = lib.ribca_edge_perm_counts_ws_bytes(8, 4)
    assert need > 0 and need % 256 == 0
    refused(null(ws_bytes=need - 1), f"{name}: workspace too small")
    for n, pp in ((0, 4), ((1 << 30) + 1, 4), (8, 0), (-1, 4)):
        assert lib.ribca_edge_perm_counts_ws_bytes(n, pp) == 0
    # the label rows of a batch: min(P, 128, max(1, 64 MiB / n)) of them, n bytes each
    assert lib.ribca_edge_perm_counts_ws_bytes(1024, 129) == lib.ribca_edge_perm_counts_ws_bytes(1024, 128)
    assert lib.ribca_edge_perm_counts_ws_bytes(1024, 128) - lib.ribca_edge_perm_counts_ws_bytes(1024, 127) == 1024
    assert lib.ribca_edge_perm_counts_ws_bytes(1 << 30, 9) == 1 << 30


# ---- five cells: 2 - 3, 2 - 5, 3 - 5, 5 - 8 touch, 9 touches nobody; types A B A B A, the type C has no cell ----------------------------------------
IDS = np.array([2, 3, 5, 8, 9])
LABELS = np.array([0, 1, 0, 1, 0])
NAMES = ["A", "B c", "C"]
SRC = np.array([0, 0, 1, 1, 2, 2, 2, 3], dtype=np.int32)
DST = np.array([1, 2, 0, 2, 0, 1, 3, 2], dtype=np.int32)
PAIRS = np.array([3, 2, 3, 5, 2, 5, 1, 1], dtype=np.int64)
DEGREE = np.array([2, 2, 3, 1, 0], dtype=np.int32)
EDGES = np.array([[2, 3, 0], [3, 0, 0], [0, 0, 0]])
WEIGHT = np.array([[4, 9, 0], [9, 0, 0], [0, 0, 0]])


def test_observed_on_the_hand_made_graph():
    edges, weight = contact.observed(SRC, DST, PAIRS, LABELS, 3)
    assert edges.dtype == np.int64 and weight.dtype == np.int64
    assert np.array_equal(edges, EDGES) and np.array_equal(weight, WEIGHT)
    assert np.array_equal(edges, CN.edge_pair_counts(SRC, DST, LABELS, 3))
    odd = LABELS.copy()
    odd[3] = 7      # a label outside [0, T) drops both directions of 5 - 8
    edges, weight = contact.observed(SRC, DST, PAIRS, odd, 3)
    assert edges.tolist() == [[2, 2, 0], [2, 0, 0], [0, 0, 0]] and weight.tolist() == [[4, 8, 0], [8, 0, 0], [0, 0, 0]]
    assert np.array_equal(edges, CN.edge_pair_counts(SRC, DST, odd, 3))
    none = contact.observed(SRC[:0], DST[:0], PAIRS[:0], LABELS, 3)
    assert not none[0].any() and not none[1].any() and none[0].shape == (3, 3)
    with pytest.raises(ValueError):
        contact.observed(SRC, DST[:3], PAIRS, LABELS, 3)
    # sums past 2^53 stay exact
    big = contact.observed([0, 0], [1, 1], [(1 << 60) + 1, 2], [0, 1], 2)[1]
    assert int(big[0, 1]) == (1 << 60) + 3


def test_the_csv_writers_on_the_hand_made_graph():
    assert contact.edges_csv(IDS, LABELS, NAMES, SRC, DST, PAIRS) == ("cell_id_a,cell_id_b,cell_type_a,cell_type_b,pixel_pairs\n"
                                                                      "2,3,A,B c,3\n"
                                                                      "2,5,A,A,2\n"
                                                                      "3,5,B c,A,5\n"
                                                                      "5,8,A,B c,1\n")
    assert contact.cells_csv(IDS, LABELS, NAMES, SRC, DST, PAIRS, DEGREE) == ("cell_id,cell_type,degree,pixel_pairs,n_A,n_B_c,n_C\n"
                                                                              "2,A,2,5,1,1,0\n"
                                                                              "3,B c,2,8,2,0,0\n"
                                                                              "5,A,3,8,1,2,0\n"
                                                                              "8,B c,1,1,1,0,0\n"
                                                                              "9,A,0,0,0,0,0\n")
    rows = contact.table_csv(NAMES, EDGES, WEIGHT).split("\n")
    assert rows == ["cell_type,neighbour,edges,pixel_pairs", "A,A,2,4", "A,B c,3,9", "A,C,0,0", "B c,A,3,9", "B c,B c,0,0", "B c,C,0,0", "C,A,0,0",
                    "C,B c,0,0", "C,C,0,0", ""]
    null = np.array([[[2, 3, 0], [3, 0, 0], [0, 0, 0]], [[4, 1, 0], [1, 2, 0], [0, 0, 0]]], dtype=np.int64)
    stats = enrichment.z_scores(EDGES, null)
    rows = contact.table_csv(NAMES, EDGES, WEIGHT, stats).split("\n")
    assert rows[0] == "cell_type,neighbour,edges,pixel_pairs,null_mean,null_std,z,n_ge,n_le"
    assert rows[1] == "A,A,2,4,3,1,-1,2,1" and rows[2] == "A,B c,3,9,2,1,1,1,2" and rows[5] == "B c,B c,0,0,1,1,-1,2,1" and rows[9] == "C,C,0,0,0,0,nan,2,2"
    third = np.array([[[1, 0, 0], [0, 0, 0], [0, 0, 0]]] * 3, dtype=np.int64)
    third[1, 0, 0] = 2      # mean 4 / 3, std sqrt(2) / 3: every float parses back to the double it was written from
    stats = enrichment.z_scores(EDGES, third)
    cols = contact.table_csv(NAMES, EDGES, WEIGHT, stats).split("\n")[1].split(",")
    assert [float(cols[4]), float(cols[5]), float(cols[6])] == [stats["mean"][0, 0], stats["std"][0, 0], stats["z"][0, 0]] and len(cols[4]) >= 18
    # a group without an edge: NaN statistics, the counts 0
    empty = contact.nan_stats(3)
    rows = contact.table_csv(NAMES, np.zeros((3, 3), dtype=np.int64), np.zeros((3, 3), dtype=np.int64), empty).split("\n")
    assert rows[1] == "A,A,0,0,nan,nan,nan,0,0" and len(rows) == 11
    assert enrichment.matrix_csv(NAMES, empty["z"]).split("\n")[1] == "A,nan,nan,nan,"
    with pytest.raises(ValueError):
        contact.table_csv(NAMES[:2], EDGES, WEIGHT)
    with pytest.raises(ValueError):
        contact.cells_csv(IDS, LABELS, NAMES, SRC, DST, PAIRS, DEGREE[:4])
    # no cell at all
    assert contact.edges_csv(IDS[:0], LABELS[:0], NAMES, SRC[:0], DST[:0], PAIRS[:0]) == "cell_id_a,cell_id_b,cell_type_a,cell_type_b,pixel_pairs\n"
    assert contact.cells_csv(IDS[:0], LABELS[:0], NAMES, SRC[:0], DST[:0], PAIRS[:0], DEGREE[:0]) == "cell_id,cell_type,degree,pixel_pairs,n_A,n_B_c,n_C\n"


def test_the_seed_the_shares_and_the_colour_index(monkeypatch):
    monkeypatch.delenv("RIBCA_CONTACT_SEED", raising=False)
    assert contact.default_seed() == 0
    monkeypatch.setenv("RIBCA_CONTACT_SEED", "41")
    assert contact.default_seed() == 41
    monkeypatch.setenv("RIBCA_CONTACT_SEED", "")
    assert contact.default_seed() == 0
    assert contact.row_normalised(WEIGHT).tolist() == [[4 / 13, 9 / 13, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    # int(min(degree / 12, 1) * 255): 0 for no contact, 127 at six neighbours, 255 from twelve on
    assert contact.DEGREE_SCALE == 12
    assert contact.degree_colour_index(np.array([0, 1, 6, 11, 12, 13, 48])).tolist() == [0, 21, 127, 233, 255, 255, 255]
    assert contact.degree_colour_index(np.zeros(0, dtype=np.int32)).shape == (0,)


def test_the_command_line_switches():
    """both flags default to 0; the pipeline calls the method only with --contact-distance > 0, beside the other steps and without a cell-count guard"""
    import main as cli
    common = ["--marker-list-path", "m.txt", "--image-path", "i.npy", "--mask-path", "k.npy", "--batch-id", "c"]
    args = cli.parse_args(common)
    assert args.contact_distance == 0 and args.contact_perms == 0
    args = cli.parse_args(common + ["--contact-distance", "4", "--contact-perms", "9"])
    assert args.contact_distance == 4 and args.contact_perms == 9
    for bad in ("9", "-1"):
        with pytest.raises(SystemExit):
            cli.parse_args(common + ["--contact-distance", bad])

    class Recorder:
        cell_size = 30
        channel_parser = types.SimpleNamespace(immune_base=True, immune_extended=False, immune_full=False, struct=False, nerve=False)

        def __init__(self):
            self.calls = []

        def min_cells_per_image(self):
            return 0

        def __getattr__(self, name):
            return lambda *a, **kw: self.calls.append((name, a, kw))

    off = Recorder()
    cli._pipeline(off, 16, 0)
    cli._pipeline(off, 16, 0, contact_perms=9)      # read only with --contact-distance > 0
    assert "contact_analysis" not in [c[0] for c in off.calls]
    on = Recorder()
    cli._pipeline(on, 16, 0, contact_distance=3, contact_perms=9)
    got = [c for c in on.calls if c[0] == "contact_analysis"]
    assert len(got) == 1 and got[0][2] == {"distance": 3, "n_perms": 9, "integrate": True}
    assert [c[0] for c in on.calls if c[0] != "contact_analysis"] == [c[0] for c in off.calls][:len(off.calls) // 2]
    both = Recorder()
    cli._pipeline(both, 16, 0, cooccurrence_bands=2, contact_distance=1)
    order = [c[0] for c in both.calls]
    assert order.index("cooccurrence_by_distance") < order.index("contact_analysis") < order.index("colorize")
    import inspect
    for fn in (cli._pipeline, cli.run, cli.batch_run):
        assert list(inspect.signature(fn).parameters)[-2:] == ["contact_distance", "contact_perms"]


def test_the_refusals_of_contact_analysis_come_before_any_launch():
    """on an Annotator that owns nothing but labels: every refusal below is raised before the method looks at a mask, the device or a file"""
    from multiplexed_image_annotator_amd.annotator import Annotator
    a = object.__new__(Annotator)
    a.tile_mode = False
    a.preprocessor = types.SimpleNamespace(_n_images=0)
    a.annotations = []
    a.cell_types = ["A", "B"]
    with pytest.raises(ValueError, match="No annotations"):
        a.contact_analysis()
    a.annotations = [["A", "B"]]
    for bad in (0, 9, -1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="distance must be an integer from 1 to 8"):
            a.contact_analysis(distance=bad)
    with pytest.raises(ValueError, match="must not be negative"):
        a.contact_analysis(distance=2, n_perms=-1)
    a.cell_types = [f"type {k}" for k in range(65)]
    with pytest.raises(ValueError, match="at most 64 cell types"):
        a.contact_analysis(n_perms=1)
    a.cell_types = [f"type {k}" for k in range(255)]
    with pytest.raises(ValueError, match="at most 254 cell types"):
        a.contact_analysis()
    assert not hasattr(a, "contact_stats")


def test_planted_contact_restatement_only():
    """RandomState(500) on 240 x 240, a 20 x 20 grid of 12-px sites (contact_numpy.planted_mask): 120 random sites hold an A | B domino of two
    touching 5 x 5 squares, every other site one jittered 5 x 5 square of type C or D: 520 cells, 200 permutations of the keyed bijection, seed 0,
    image 0.  A prototype of this layout with another draw order gave z[A][B] = 31.5 over 240 directed edges at d = 1 and 22.7 over 610 at d = 4,
    and 1.9 for the largest |z| of the labelling of permutation 200 against the same null.  The generator committed here (printed below, DESIGN.md
    section 19): 31.13 over 248 edges at d = 1, 26.09 over 558 at d = 4, and 0.93 / 0.83 for permutation 200.  The bounds are two thirds of these
    values, which is above the two thirds of the prototype's."""
    mask, labels = CN.planted_mask()
    assert mask.shape == (240, 240) and len(labels) == 520 and np.bincount(labels)[:2].tolist() == [120, 120]
    table, n = CN.identity_table(mask)
    for d, bound in ((1, 20.7), (4, 17.3)):
        src, dst, pairs = CN.edge_list(CN.pair_weights(mask, table, n, d))
        edges, weight = contact.observed(src, dst, pairs, labels, 4)
        assert edges[0, 1] == edges[1, 0] >= 120 and np.array_equal(weight, weight.T)
        null = CN.edge_perm_counts(src, dst, labels, 4, 0, 0, 0, 200)
        assert (null.sum(axis=(1, 2)) == len(src)).all()
        z = enrichment.z_scores(edges, null)["z"]
        other = CN.edge_perm_counts(src, dst, labels, 4, 0, 0, 200, 1)[0]
        zo = enrichment.z_scores(other, null)["z"]
        print("d", d, "edges", len(src), "z[A][B]", z[0, 1], "z[B][A]", z[1, 0], "permutation 200: largest |z|", np.abs(zo[np.isfinite(zo)]).max())
        assert z[0, 1] > bound and z[1, 0] > bound
        assert np.isfinite(zo).any() and (np.abs(zo[np.isfinite(zo)]) < 4.5).all()
