#!/usr/bin/env python3
"""Times the post-predict consumers on the GPU at the BASELINE config-3 size (4096 x 4096 mask, ~100 k cells): label painting
(ribca_colorize), the 25-nearest-neighbour co-occurrence (ribca_knn_cooccurrence), the neighbourhood compositions and the tissue regions
(PCA + k-means of csrc/regions.hip on the composition counts, 5 regions), the per-cell-type table of the heat map (ribca_group_sums over a 15-column
fp64 intensity table, 12 cell types) with the two rasterisers, and, for the same table, the reference's own Python loop (model.py:708-715) restated
on the host; and the neighbourhood enrichment (csrc/enrichment.hip): the 25-nearest-neighbour list, 1000 label permutations over it at 12 cell types,
and, for scale, the numpy restatement of tests/enrichment_numpy.py on 10 of the same permutations; and the co-occurrence by distance
(csrc/cooccurrence.hip): the cell-type pair counts in 16 and 32 bands of one cell size (30 px) at 12 cell types, one band reaching over the whole
image (every pair in range: the weight of the LDS atomics), and as the host yardstick scipy's cKDTree.count_neighbors over the same radii and type
pairs and the numpy oracle of tests/cooccurrence_numpy.py on the first 10 000 cells, scaled by n^2; and the spatial autocorrelation
(csrc/autocorr.hip): the observed numerators of Moran's I and Geary's C of the 15-column table over the 25-nearest-neighbour list, 1000 row
permutations, and the numpy restatement of tests/autocorr_numpy.py on 10 of the same permutations; and the local indicators
(csrc/local_autocorr.hip): the per-cell neighbour sums and the counts of 999 conditional permutations of the same table, and the numpy restatement
of tests/local_autocorr_numpy.py on one of them; and the nearest cell of every type (csrc/nearest.hip): the (n, 12) distance table and 100 label
permutations of the nearest-distance band counts in 16 bands of 30 px, inputs on the device, for a uniform label mix and for one with half the cells
of one type, and the numpy restatement of tests/nearest_numpy.py on the first 10 000 cells, scaled by n^2 (``--nearest``: this section alone); and
the contact graph of the mask (csrc/contact.hip): the (n, 32) contact table at the reaches 1, 4 and 8 px, mask and label table on the device, then
1000 label permutations over the directed edges of each at 12 cell types, and the numpy restatement of tests/contact_numpy.py on the top-left
1024 x 1024 crop of the same mask, scaled by the area (``--contact``: this section alone); and the morphology sums of the mask
(csrc/morphology.hip): the (n, 16) table and the boxes with the crop windows as rectangles, mask, label table and outputs on the device, and the
numpy restatement of tests/morphology_numpy.py on the same crop, scaled by the area (``--morphology``: this section alone); and the per-cell
marker intensities (csrc/intensities.hip): the kernel alone on a 15-channel fp32 image of the same tile, device events, for the five quartile
ranks and for the median alone, the host features, and the numpy restatement of tests/intensities_numpy.py on the same crop, scaled by the area
(``--intensities``: this section alone); and the expansion of the mask's labels (csrc/expand.hip): the kernel alone at D = 2, 8 and 32, device
events, mask, outputs and workspace on the device, and as the host yardstick scipy's distance_transform_edt(return_indices=True) on the same mask,
whose composition at D = 8 is compared with the kernel's output (``--expand``: this section alone); and the repair of the mask
(csrc/components.hip): the connected components of the same mask with 4000 injected faults, device events, the whole ops.repair_labels on the
host clock, and scipy.ndimage.label of the same mask on the host (``--repair``: this section alone); and the cell outlines
(csrc/outlines.hip): ribca_mask_rings and ribca_mask_ring_vertices on the same mask, device events, the whole ops.mask_rings and the GeoJSON text
on the host clock, and the restatement of tests/outlines_numpy.py on a crop, scaled by boundary edges (``--outlines``: this section alone); and the
matching of a second mask (csrc/overlap.hip): ribca_mask_overlap and ribca_mask_compartments against a shifted copy of the same mask with labels
dropped and merged, device events, beside ribca_contact_table at d = 1 in the same process, the whole ops.overlap_pairs and the rules of
matching.py on the host clock, and np.unique over the 64-bit pair keys of the same two masks on the host (``--matching``: this section alone); and the
marker localisation (csrc/localization.hip): ribca_mask_depth at D = 8 and 32 and ribca_cell_shell_sums on the 15-channel image of the same tile,
device events, the whole ops calls and the host features on the host clock, scipy's distance_transform_edt of the foreground on the host, and the
restatement of tests/localization_numpy.py on a crop, scaled by the area (``--localization``: this section alone); and the marker colocalisation
(csrc/colocalization.hip): ribca_cell_coloc on the 15-channel image of the same tile at K = 15 and K = 4, device events, beside
ribca_cell_intensities in the same process, the whole ops.cell_coloc and the host features on the host clock, and the restatement of
tests/coloc_numpy.py on a crop, scaled by the area (``--colocalization``: this section alone)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from multiplexed_image_annotator_amd import _lib, colors, ops, regions, synth

dev = _lib.require_gpu()
mask, _ = synth.make_mask_and_image(4096, 4096, 100000, 1, synth.SEED_BASE + 3, device=dev, want_image=False)
mask = mask.to(torch.int32)
ids, tab = ops.label_table(mask)
n = len(ids)
rng = np.random.default_rng(0)
tidx = rng.integers(0, 12, n)
conf = rng.random(n).astype(np.float32)
pal = np.array(colors.get_colors(12), np.uint8)
x = tab[:, 5] / tab[:, 6]
y = tab[:, 4] / tab[:, 6]


# ---- the nearest cell of every type (csrc/nearest.hip): n cells, T = 12; the distance table, and P = 100 label permutations of the band counts ----
def time_nearest():
    """inputs, outputs and workspaces on the device before the clock starts: the entry points themselves, median of five calls after a warm-up"""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nearest_numpy as NN
    from multiplexed_image_annotator_amd import cooccurrence
    from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr
    perms, t = 100, 12
    radii = cooccurrence.default_radii(30, 16)
    r2 = np.ascontiguousarray(radii * radii)
    edges = r2.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    xd, yd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(dev)
    skew = np.random.default_rng(1).choice(t, n, p=[0.5, 0.2, 0.1] + [0.2 / 9] * 9)
    near2 = torch.empty((n, t), dtype=torch.float64, device=dev)
    arg = torch.empty((n, t), dtype=torch.int32, device=dev)
    counts = torch.zeros((perms, 16, t, t), dtype=torch.int64, device=dev)
    ws1 = torch.empty(ops.nearest_by_type_ws_bytes(n, t), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(ops.nearest_perm_counts_ws_bytes(n, t, perms), dtype=torch.uint8, device=dev)
    for mix, labels in (("12 types, uniform", tidx), ("12 types, half the cells of one type", skew)):
        td = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(dev)

        def table():
            _lib.check(lib().ribca_nearest_by_type(ptr(xd), ptr(yd), ptr(td), n, t, ptr(near2), ptr(arg), ptr(ws1), ws1.numel(), stream_ptr()), "nearest")

        def null():
            counts.zero_()
            _lib.check(lib().ribca_nearest_perm_counts(ptr(xd), ptr(yd), ptr(td), n, t, edges, 16, 0, 0, 0, perms, ptr(counts), ptr(ws2), ws2.numel(),
                                                       stream_ptr()), "nearest")

        for name, fn in ((f"nearest cell of every type, distance table ({mix})", table),
                         (f"nearest-distance band counts, {perms} label permutations, 16 bands up to 480 px ({mix}, {ws2.numel() / 2 ** 20:.1f} MiB workspace)", null)):
            fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(5):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0))
            print(f"{name}: median {sorted(times)[2]:.1f} ms, min {min(times):.1f}, max {max(times):.1f} of 5 for {n} cells, "
                  f"{n * (n - 1) * (perms if fn is null else 1):.3g} distance evaluations")
    m, few = 10000, 2
    t0 = time.perf_counter()
    want2, want_arg = NN.nearest_by_type(x[:m], y[:m], tidx[:m], t)
    table_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = NN.perm_counts(x[:m], y[:m], tidx[:m], t, r2, 0, 0, 0, few)
    oracle_ms = 1e3 * (time.perf_counter() - t0)
    got2, got_arg = ops.nearest_by_type(x[:m], y[:m], tidx[:m], t)
    same = (got2.cpu().numpy().tobytes() == want2.tobytes() and np.array_equal(got_arg.cpu().numpy(), want_arg)
            and np.array_equal(ops.nearest_perm_counts(x[:m], y[:m], tidx[:m], t, radii, 0, 0, 0, few).cpu().numpy(), want))
    scale = (n / m) ** 2
    print(f"numpy restatement, first {m} cells (host): table {table_ms:.0f} ms -> {table_ms * scale / 1e3:.1f} s at {n} cells; {few} permutations "
          f"{oracle_ms:.0f} ms -> {oracle_ms * scale * perms / few / 1e3:.0f} s for {perms} at {n} cells; equal to the GPU table and counts of the same "
          f"cells: {same}")


# ---- the contact graph of the mask (csrc/contact.hip): the table at d = 1, 4, 8 and P = 1000 label permutations over its edges, T = 12 ----------------
def time_contact():
    """mask, label table, outputs and workspaces on the device before the clock starts: the entry points themselves, median of five calls after a
    warm-up; then the restatement on a crop, checked against the GPU on the same crop"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import contact_numpy as CN
    from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr
    perms, t, slots = 1000, 12, 32
    h, w = mask.shape
    table = np.full(int(ids.max()) + 1, -1, dtype=np.int32)
    table[ids] = np.arange(n, dtype=np.int32)
    tab_d = torch.from_numpy(table).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(tidx, dtype=np.int32)).to(dev)
    nbr = torch.empty((n, slots), dtype=torch.int32, device=dev)
    pairs = torch.empty((n, slots), dtype=torch.int64, device=dev)
    degree = torch.empty((n,), dtype=torch.int32, device=dev)
    over = torch.empty((2,), dtype=torch.int32, device=dev)
    ws1 = torch.empty(ops.contact_table_ws_bytes(h, w, n, slots), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(ops.edge_perm_counts_ws_bytes(n, perms), dtype=torch.uint8, device=dev)
    counts = torch.zeros((perms, t, t), dtype=torch.int64, device=dev)

    def median_of_five(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return f"median {sorted(times)[2]:.2f} ms, min {min(times):.2f}, max {max(times):.2f} of 5"

    for d in (1, 4, 8):
        def graph():
            _lib.check(lib().ribca_contact_table(ptr(mask), h, w, ptr(tab_d), tab_d.numel(), n, d, slots, ptr(nbr), ptr(pairs), ptr(degree), ptr(over),
                                                 ptr(ws1), ws1.numel(), stream_ptr()), "contact")

        line = median_of_five(graph)
        g = ops.contact_graph(mask, ids, d)
        print(f"contact table, d = {d}, {slots} slots ({ws1.numel() / 2 ** 20:.1f} MiB workspace): {line} for {n} cells, {h}x{w}; {len(g['src'])} directed "
              f"edges, largest degree {int(g['degree'].max())}, overflow {over.tolist()}")
        if len(g["src"]) == 0:
            continue
        sd, dd = torch.from_numpy(g["src"]).to(dev), torch.from_numpy(g["dst"]).to(dev)

        def null():
            counts.zero_()
            _lib.check(lib().ribca_edge_perm_counts(ptr(sd), ptr(dd), sd.numel(), ptr(td), n, t, 0, 0, 0, perms, ptr(counts), ptr(ws2), ws2.numel(),
                                                    stream_ptr()), "contact")

        print(f"edge type pairs, {perms} label permutations, d = {d} ({ws2.numel() / 2 ** 20:.1f} MiB workspace): {median_of_five(null)} for {len(g['src'])} "
              f"directed edges")
    side = 1024
    crop = np.ascontiguousarray(mask[:side, :side].cpu().numpy())
    crop_d = torch.from_numpy(crop).to(dev)
    for d in (1, 4, 8):
        t0 = time.perf_counter()
        want = CN.edge_list(CN.pair_weights(crop, table, n, d))
        host_ms = 1e3 * (time.perf_counter() - t0)
        g = ops.contact_graph(crop_d, ids, d)
        same = all(np.array_equal(a, b) for a, b in zip(want, (g["src"], g["dst"], g["pairs"])))
        print(f"numpy restatement, d = {d}, top-left {side}x{side} crop (host): {host_ms:.0f} ms -> {host_ms * (h * w) / (side * side) / 1e3:.1f} s scaled by "
              f"area to {h}x{w}; equal to the GPU edge list of the same crop: {same}")
    few = 10
    g = ops.contact_graph(mask, ids, 4)
    t0 = time.perf_counter()
    want = CN.edge_perm_counts(g["src"], g["dst"], tidx, t, 0, 0, 0, few)
    host_ms = 1e3 * (time.perf_counter() - t0)
    same = np.array_equal(ops.edge_perm_counts(g["src"], g["dst"], tidx, t, 0, 0, 0, few).cpu().numpy(), want)
    print(f"numpy restatement of the null, d = 4, {few} permutations over {len(g['src'])} edges (host): {host_ms:.0f} ms -> "
          f"{host_ms * perms / few / 1e3:.1f} s for {perms}; equal to the GPU counts: {same}")


# ---- the morphology sums of the mask (csrc/morphology.hip): the (n, 16) table and the boxes, the crop windows of a 40-px patch as rectangles ----------
def time_morphology():
    """mask, label table, rectangles, outputs and workspace on the device before the clock starts: the entry point itself, median of five calls
    after a warm-up; then the restatement on a crop, checked against the GPU on the same crop"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import morphology_numpy as MN
    from multiplexed_image_annotator_amd import morphology
    from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr
    h, w = mask.shape
    table = np.full(int(ids.max()) + 1, -1, dtype=np.int32)
    table[ids] = np.arange(n, dtype=np.int32)
    tab_d = torch.from_numpy(table).to(dev)
    rect = morphology.patch_rect(tab[:, :4], h, w, 40)
    rect_d = torch.from_numpy(rect).to(dev)
    sums = torch.empty((n, 16), dtype=torch.int64, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    ws = torch.empty(max(ops.mask_morphology_ws_bytes(h, w, n), 1), dtype=torch.uint8, device=dev)

    def call():
        _lib.check(lib().ribca_mask_morphology(ptr(mask), h, w, ptr(tab_d), tab_d.numel(), n, ptr(rect_d), ptr(sums), ptr(bbox), ptr(ws), ws.numel(),
                                               stream_ptr()), "morphology")

    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    got = sums.cpu().numpy()
    feat = morphology.features(got, bbox.cpu().numpy())
    same_boxes = np.array_equal(bbox.cpu().numpy(), tab[:, :4]) and np.array_equal(got[:, 0], tab[:, 6])
    print(f"morphology sums (init + tiles): median {sorted(times)[2]:.2f} ms, min {min(times):.2f}, max {max(times):.2f} of 5 for {n} cells, {h}x{w}; "
          f"boxes and areas equal to the label table: {same_boxes}; Euler number other than 1: {int((feat['euler'] != 1).sum())} cells, larger than the "
          f"40-px window: {int((feat['patch_coverage'] < 1.0).sum())}, on the image border: {int(feat['on_image_edge'].sum())}, mean contact fraction "
          f"{float(np.nanmean(feat['contact_fraction'])):.4f}")
    t0 = time.perf_counter()
    morphology.features(got, bbox.cpu().numpy())
    print(f"morphology.features on the host, {n} cells: {1e3 * (time.perf_counter() - t0):.0f} ms")
    side = 1024
    crop = np.ascontiguousarray(mask[:side, :side].cpu().numpy())
    crop_rect = morphology.patch_rect(MN.sums_arrays(crop, table, n)[1], side, side, 40)
    t0 = time.perf_counter()
    want = MN.sums_arrays(crop, table, n, crop_rect)
    host_ms = 1e3 * (time.perf_counter() - t0)
    g = ops.mask_morphology(torch.from_numpy(crop).to(dev), ids, crop_rect)
    same = np.array_equal(g["sums"], want[0]) and np.array_equal(g["bbox"], want[1])
    print(f"numpy restatement, top-left {side}x{side} crop (host): {host_ms:.0f} ms -> {host_ms * (h * w) / (side * side) / 1e3:.1f} s scaled by area to "
          f"{h}x{w}; equal to the GPU table of the same crop: {same}")


# ---- the per-cell marker intensities (csrc/intensities.hip): sums and order statistics of 15 channels over every cell's own pixels ------------------
HBM_BYTES_PER_S = 6.29e12      # the measured copy rate of the MI355X: the time to read the image once at it is the floor of this step


def time_intensities():
    """image, mask, ids, boxes and outputs on the device before the clock starts: the entry point itself between two device events, median of
    five calls after a warm-up, for Q = 5 (min, quartiles, max) and Q = 1 (the median); then the host features and the restatement on a crop,
    checked against the GPU on the same crop"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import intensities_numpy as IN
    from multiplexed_image_annotator_amd import intensities
    h, w = mask.shape
    c = 15
    _, raw = synth.make_mask_and_image(h, w, 100000, c, synth.SEED_BASE + 3, device=dev)
    image = (raw.to(torch.float32) / 32767.5 - 1.0).contiguous()      # the normalised range, with the background's ties
    del raw
    ids_d = torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(dev)
    bbox_d = torch.from_numpy(np.ascontiguousarray(tab[:, :4], dtype=np.int32)).to(dev)
    floor_ms = 1e3 * image.numel() * 4 / HBM_BYTES_PER_S
    got = None
    for q_num, q_den, what in ((intensities.Q_NUM, intensities.Q_DEN, "Q = 5 (min, quartiles, max)"), ((1,), 2, "Q = 1 (median)")):
        out = (torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n, c, 2), dtype=torch.float64, device=dev),
               torch.empty((n, c, len(q_num), 2), dtype=torch.float32, device=dev))
        ops.cell_intensities(image, mask, ids_d, bbox_d, q_num, q_den, out=out)
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            ops.cell_intensities(image, mask, ids_d, bbox_d, q_num, q_den, out=out)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        area = out[0].cpu().numpy()
        print(f"cell intensities, {what}: median {sorted(times)[2]:.2f} ms, min {min(times):.2f}, max {max(times):.2f} of 5 (device events) for {n} cells, "
              f"{c} channels, {h}x{w}; one read of the {image.numel() * 4 / 1e9:.2f} GB image at {HBM_BYTES_PER_S / 1e12:.2f} TB/s: {floor_ms:.2f} ms; areas equal "
              f"to the label table: {np.array_equal(area, tab[:, 6])}; mean area {area.mean():.0f}, max {area.max()}, above {ops.INTENSITY_RESIDENT} pixels: "
              f"{int((area > ops.INTENSITY_RESIDENT).sum())}")
        if got is None:
            got = tuple(t.cpu().numpy() for t in out)
    t0 = time.perf_counter()
    intensities.features(*got)
    print(f"intensities.features on the host, {n} cells x {c} channels: {1e3 * (time.perf_counter() - t0):.0f} ms")
    side = 1024
    crop_mask = np.ascontiguousarray(mask[:side, :side].cpu().numpy())
    crop_image = np.ascontiguousarray(image[:, :side, :side].cpu().numpy())
    crop_ids = np.unique(crop_mask[crop_mask > 0]).astype(np.int32)
    crop_box = IN.boxes_of_all(crop_mask, crop_ids)
    t0 = time.perf_counter()
    want = IN.arrays(crop_image, crop_mask, crop_ids, crop_box)
    host_ms = 1e3 * (time.perf_counter() - t0)
    g = ops.cell_intensities(torch.from_numpy(crop_image).to(dev), torch.from_numpy(crop_mask).to(dev), crop_ids, crop_box)
    same = np.array_equal(g[0], want[0]) and np.array_equal(g[1].view(np.int64), want[1].view(np.int64)) and np.array_equal(g[2].view(np.int32),
                                                                                                                   want[2].view(np.int32))
    print(f"numpy restatement, top-left {side}x{side} crop, {len(crop_ids)} cells (host): {host_ms:.0f} ms -> {host_ms * (h * w) / (side * side) / 1e3:.1f} s scaled by "
          f"area to {h}x{w}; equal to the GPU outputs of the same crop, byte for byte: {same}")


# ---- growing the labels of the mask (csrc/expand.hip): every background pixel within D pixels of a cell takes the nearest cell's label --------------
def time_expand():
    """mask, outputs and workspace on the device before the clock starts: the entry point itself between two device events, median of five calls
    after a warm-up, with and without the squared distances; then scipy's exact Euclidean distance transform of the same mask on the host, which
    gives every distance at once, and the comparison of its composition with the kernel at D = 8 (labels may differ on tie pixels only)"""
    from scipy import ndimage
    from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr
    h, w = mask.shape
    background = int((mask <= 0).sum())
    out = torch.empty_like(mask)
    dist2 = torch.empty_like(mask)
    kept = {}
    for d in (2, 8, 32):
        ws = torch.empty(max(ops.expand_labels_ws_bytes(h, w, d), 1), dtype=torch.uint8, device=dev)
        for what, d2 in (("labels and squared distances", dist2), ("labels alone", None)):
            def call():
                _lib.check(lib().ribca_expand_labels(ptr(mask), h, w, d, ptr(out), ptr(d2), ptr(ws), ws.numel(), stream_ptr()), "expand")

            call()
            torch.cuda.synchronize()
            times = []
            for _ in range(5):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                call()
                stop.record()
                torch.cuda.synchronize()
                times.append(start.elapsed_time(stop))
            grown = int(((out > 0) & (mask <= 0)).sum())
            print(f"expand labels, D = {d}, {what}: median {sorted(times)[2]:.3f} ms, min {min(times):.3f}, max {max(times):.3f} of 5 (device events) for {n} "
                  f"cells, {h}x{w}; {grown} of {background} background pixels grown; read + write of {(2 if d2 is None else 3) * h * w * 4 / 1e9:.2f} GB at "
                  f"{HBM_BYTES_PER_S / 1e12:.2f} TB/s: {1e3 * (2 if d2 is None else 3) * h * w * 4 / HBM_BYTES_PER_S:.3f} ms")
        if d == 8:
            _lib.check(lib().ribca_expand_labels(ptr(mask), h, w, d, ptr(out), ptr(dist2), ptr(ws), ws.numel(), stream_ptr()), "expand")
            kept = {"out": out.cpu().numpy(), "dist2": dist2.cpu().numpy()}
    host = mask.cpu().numpy()
    t0 = time.perf_counter()
    dist, idx = ndimage.distance_transform_edt(host <= 0, return_indices=True)
    host_ms = 1e3 * (time.perf_counter() - t0)
    grown = (host <= 0) & (dist <= 8)
    ref = host.copy()
    ref[grown] = host[idx[0][grown], idx[1][grown]]
    same_support = np.array_equal((kept["out"] > 0) & (host <= 0), grown)
    same_dist = np.array_equal(kept["dist2"][grown], np.rint(dist[grown] ** 2).astype(np.int64))
    differ = int((kept["out"] != ref).sum())
    print(f"scipy distance_transform_edt(return_indices=True), {h}x{w} (host): {host_ms:.0f} ms; at D = 8 the grown pixels are the kernel's: {same_support}, "
          f"the squared distances equal: {same_dist}, labels that differ (tie pixels, scan order against smallest label): {differ} of {int(grown.sum())}")


# ---- repairing the mask (csrc/components.hip, repair.py): connected components, torn labels split, specks dropped, holes filled -----------------------
def time_repair():
    """the mask with a few thousand injected faults -- 1000 cells given another cell's label, a one-pixel hole at the centroid of 2000 cells, 1000
    specks of one pixel -- on the device before the clock starts: ribca_mask_components alone between two device events, median of five calls
    after a warm-up; the whole ops.repair_labels (two component runs, two relabels, the compaction, the copies of the rows and the host's
    decisions) on the host clock, synchronised; then scipy.ndimage.label on the host, once for the foreground at 8-connectivity and once for
    the background at 4-connectivity -- one call each, where a per-label repair would call it per label -- and its component count beside the
    kernel's"""
    from scipy import ndimage
    from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr
    h, w = mask.shape
    fault_rng = np.random.default_rng(7)
    picks = fault_rng.permutation(n)[:4000]
    lut = np.arange(int(ids.max()) + 1, dtype=np.int32)
    lut[ids[picks[:1000]]] = ids[picks[1000:2000]]      # 1000 labels now name two cells each
    damaged = torch.from_numpy(lut).to(dev)[mask.long()].contiguous()
    cr, cc = (tab[:, 4] // tab[:, 6]), (tab[:, 5] // tab[:, 6])
    holes = picks[2000:4000]
    damaged[torch.from_numpy(cr[holes]).to(dev), torch.from_numpy(cc[holes]).to(dev)] = 0
    sr, sc = fault_rng.integers(0, h, 1000), fault_rng.integers(0, w, 1000)
    damaged[torch.from_numpy(sr).to(dev), torch.from_numpy(sc).to(dev)] = torch.from_numpy(ids[fault_rng.integers(0, n, 1000)].astype(np.int32)).to(dev)
    root = torch.empty_like(damaged)
    stats = torch.empty((h * w, 4), dtype=torch.int32, device=dev)
    ws = torch.empty(max(ops.mask_components_ws_bytes(h, w), 1), dtype=torch.uint8, device=dev)

    def call():
        _lib.check(lib().ribca_mask_components(ptr(damaged), h, w, ptr(root), ptr(stats), ptr(ws), ws.numel(), stream_ptr()), "components")

    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    rows = stats[:, 0] > 0
    comps = int(rows.sum())
    background = int((rows & (damaged.reshape(-1) <= 0)).sum())
    floor = 2 * h * w * 4
    print(f"mask components: median {sorted(times)[2]:.3f} ms, min {min(times):.3f}, max {max(times):.3f} of 5 (device events) for {h}x{w}, {n} cells with "
          f"4000 injected faults; {comps - background} foreground and {background} background components; one read of the mask and one write of "
          f"root, {floor / 1e9:.2f} GB at {HBM_BYTES_PER_S / 1e12:.2f} TB/s: {1e3 * floor / HBM_BYTES_PER_S:.3f} ms; the stats rows are {4 * h * w * 4 / 1e9:.2f} GB more")
    ops.repair_labels(damaged, 3)
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, comp_rows, record = ops.repair_labels(damaged, 3)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    print(f"ops.repair_labels(min_area=3), whole: median {sorted(times)[2]:.2f} ms, min {min(times):.2f}, max {max(times):.2f} of 5 (host clock, synchronised); "
          f"{record}")
    host = damaged.cpu().numpy()
    t0 = time.perf_counter()
    _, n_fg = ndimage.label(host > 0, structure=np.ones((3, 3), dtype=int))
    fg_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    _, n_bg = ndimage.label(host <= 0)
    bg_ms = 1e3 * (time.perf_counter() - t0)
    print(f"scipy.ndimage.label, {h}x{w} (host): {fg_ms:.0f} ms for the foreground as one class at 8-connectivity ({n_fg} blobs; the kernel separates "
          f"labels), {bg_ms:.0f} ms for the background at 4-connectivity; its {n_bg} background components are the kernel's: {n_bg == background}")


# ---- the cell outlines (csrc/outlines.hip, outlines.py): rings of the mask, their vertices, polygons and GeoJSON ------------------------------------
def time_outlines():
    """mask, label table, outputs and workspace on the device before the clock starts: ribca_mask_rings and ribca_mask_ring_vertices each between
    two device events, median of five calls after a warm-up (the vertices over the sorted rows of the rings call); the whole ops.mask_rings -- the
    label table, both kernels, the sort, the prefix sum and the copies back -- and outlines.geojson / cells_csv on the host clock; then the
    restatement of tests/outlines_numpy.py on a crop, checked against the GPU on the same crop and scaled by boundary edges.  scikit-image and
    OpenCV, whose contour tracers a host pipeline would use, are not installed here: the restatement is the only host yardstick."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import outlines_numpy as ON
    from multiplexed_image_annotator_amd import outlines
    from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr
    h, w = mask.shape
    table = np.full(int(ids.max()) + 1, -1, dtype=np.int32)
    table[ids] = np.arange(n, dtype=np.int32)
    tab_d = torch.from_numpy(table).to(dev)
    cap = 2 * n + ops.OUTLINES_SPARE_ROWS
    rings = torch.empty((cap, 6), dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(ops.mask_rings_ws_bytes(h, w, n), 1), dtype=torch.uint8, device=dev)

    def rings_call():
        _lib.check(lib().ribca_mask_rings(ptr(mask), h, w, ptr(tab_d), tab_d.numel(), n, cap, ptr(rings), ptr(total), ptr(ws), ws.numel(), stream_ptr()),
                   "rings")

    def events(call):
        call()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        return f"median {sorted(times)[2]:.3f} ms, min {min(times):.3f}, max {max(times):.3f} of 5 (device events)"

    text = events(rings_call)
    found = int(total.item())
    rows = rings[:found]
    rows = rows.index_select(0, torch.argsort(rows[:, 0] * ((h + 1) * (w + 1)) + rows[:, 1])).contiguous()
    first = torch.zeros(found + 1, dtype=torch.int64, device=dev)
    first[1:] = torch.cumsum(rows[:, 2], 0)
    vertices = torch.empty((int(first[-1].item()), 2), dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    edges = int(rows[:, 3].sum().item())
    floor = h * w * 4
    print(f"mask rings (init + tiles + walkers): {text} for {h}x{w}, {n} cells; {found} rings, {int((rows[:, 4] < 0).sum())} of them holes, {edges} boundary "
          f"edges, longest ring {int(rows[:, 3].max())} edges, {int(rows[:, 5].sum())} saddle passes; workspace {ws.numel() / 1e6:.0f} MB; one read of the "
          f"mask, {floor / 1e9:.3f} GB at {HBM_BYTES_PER_S / 1e12:.2f} TB/s: {1e3 * floor / HBM_BYTES_PER_S:.3f} ms")

    def vertices_call():
        _lib.check(lib().ribca_mask_ring_vertices(ptr(mask), h, w, ptr(tab_d), tab_d.numel(), n, ptr(rows), found, ptr(first), ptr(vertices), ptr(bad),
                                                  stream_ptr()), "ring vertices")

    text = events(vertices_call)
    print(f"mask ring vertices (one thread per ring): {text}; {vertices.shape[0]} vertices, bad = {int(bad.item())}")
    ops.mask_rings(mask, ids)
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = ops.mask_rings(mask, ids)
        times.append(1e3 * (time.perf_counter() - t0))
    print(f"ops.mask_rings, whole: median {sorted(times)[2]:.2f} ms, min {min(times):.2f}, max {max(times):.2f} of 5 (host clock; it ends synchronised), "
          f"{got['calls']} call(s) of the rings kernel")
    t0 = time.perf_counter()
    doc = outlines.geojson(got["rings"], got["first"], got["vertices"], ids)
    t1 = time.perf_counter()
    csv = outlines.cells_csv(got["rings"], ids)
    print(f"outlines.geojson on the host, {n} cells: {1e3 * (t1 - t0):.0f} ms for {len(doc) / 1e6:.1f} MB of text; outlines.cells_csv: "
          f"{1e3 * (time.perf_counter() - t1):.0f} ms for {len(csv) / 1e6:.1f} MB")
    side = 512
    crop = np.ascontiguousarray(mask[:side, :side].cpu().numpy())
    t0 = time.perf_counter()
    want = ON.trace(crop, table, n)
    host_ms = 1e3 * (time.perf_counter() - t0)
    g = ops.mask_rings(torch.from_numpy(crop).to(dev), ids)
    same = all(np.array_equal(g[k], v) for k, v in zip(("rings", "first", "vertices"), want))
    crop_edges = int(want[0][:, 3].sum())
    print(f"numpy restatement, top-left {side}x{side} crop (host): {host_ms:.0f} ms for {crop_edges} boundary edges -> "
          f"{host_ms * edges / max(crop_edges, 1) / 1e3:.1f} s scaled by boundary edges to {h}x{w}; equal to the GPU rings and vertices of the same crop: {same}")


# ---- matching a second mask (csrc/overlap.hip, matching.py): the pair table of two masks, the compartments, the host rules --------------------------
def time_matching():
    """Mask B is the mask moved three columns to the right with one label in 50 dropped and one in 50 merged into the label before it.  Both masks,
    both tables, outputs and workspace on the device before the clock starts; device events around 20 calls, the median of five such windows
    after a warm-up, for ribca_mask_overlap, ribca_mask_compartments and, the yardstick, ribca_contact_table at d = 1 on the same mask.  Then the
    whole ops.overlap_pairs -- label tables to the device, the kernels, the copies back -- and the rules of matching.py on the host clock, and the
    numpy restatement, np.unique over the 64-bit pair keys of the same 16.7 M pixels, checked against the GPU's pairs."""
    from multiplexed_image_annotator_amd import matching
    from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr
    h, w = mask.shape
    host_a = mask.cpu().numpy()
    host_b = np.zeros_like(host_a)
    host_b[:, 3:] = host_a[:, :-3]
    relabel = np.arange(int(host_a.max()) + 1, dtype=np.int32)
    relabel[ids[49::50]] = 0                          # dropped
    keep, gone = ids[24::50], ids[25::50]
    relabel[gone] = keep[:len(gone)]                  # merged into the label before it in the id list
    host_b = relabel[host_b]
    mask_b = torch.from_numpy(host_b).to(dev)
    ids_b = ops.label_table(mask_b)[0]
    m, slots = len(ids_b), ops.OVERLAP_FIRST_SLOTS
    tab_a, tab_b = ops._cell_table(ids, dev), ops._cell_table(ids_b, dev)
    partner = torch.empty((n, slots), dtype=torch.int32, device=dev)
    inter = torch.empty((n, slots), dtype=torch.int64, device=dev)
    degree, area_a = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
    area_b = torch.empty((m,), dtype=torch.int32, device=dev)
    over = torch.empty((2,), dtype=torch.int32, device=dev)
    ws = torch.empty(ops.mask_overlap_ws_bytes(h, w, n, slots), dtype=torch.uint8, device=dev)
    c_slots = 32
    nbr, c_pairs = torch.empty((n, c_slots), dtype=torch.int32, device=dev), torch.empty((n, c_slots), dtype=torch.int64, device=dev)
    c_ws = torch.empty(ops.contact_table_ws_bytes(h, w, n, c_slots), dtype=torch.uint8, device=dev)
    inner, outer = torch.empty_like(mask), torch.empty_like(mask)
    g = ops.overlap_pairs(mask, ids, mask_b, ids_b)
    owner, inside = matching.owners(g["cell"], g["obj"], g["inter"], g["area_b"])
    owner_d = torch.from_numpy(owner).to(dev)

    def overlap():
        _lib.check(lib().ribca_mask_overlap(ptr(mask), ptr(mask_b), h, w, ptr(tab_a), tab_a.numel(), n, ptr(tab_b), tab_b.numel(), m, slots, ptr(partner),
                                            ptr(inter), ptr(degree), ptr(area_a), ptr(area_b), ptr(over), ptr(ws), ws.numel(), stream_ptr()), "overlap")

    def compartments():
        _lib.check(lib().ribca_mask_compartments(ptr(mask), ptr(mask_b), h, w, ptr(tab_a), tab_a.numel(), n, ptr(tab_b), tab_b.numel(), m, ptr(owner_d),
                                                 ptr(inner), ptr(outer), stream_ptr()), "compartments")

    def contact():
        _lib.check(lib().ribca_contact_table(ptr(mask), h, w, ptr(tab_a), tab_a.numel(), n, 1, c_slots, ptr(nbr), ptr(c_pairs), ptr(degree), ptr(over),
                                             ptr(c_ws), c_ws.numel(), stream_ptr()), "contact")

    def events(fn, calls=20, windows=5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(windows):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop) / calls)
        return f"median {sorted(times)[windows // 2]:.3f} ms per call, min {min(times):.3f}, max {max(times):.3f} of {windows} windows of {calls} calls"

    hbm_ms = 2 * h * w * 4 / 6.29e12 * 1e3      # one read of both masks at the measured HBM copy rate DESIGN.md quotes
    for kind in ("first", "second"):              # the three alternate, twice: the spread between the rounds is the noise
        print(f"{kind} round: ribca_mask_overlap, {slots} slots ({ws.numel() / 2 ** 20:.1f} MiB workspace): {events(overlap)}")
        print(f"{kind} round: ribca_contact_table, d = 1, {c_slots} slots ({c_ws.numel() / 2 ** 20:.1f} MiB workspace): {events(contact)}")
        print(f"{kind} round: ribca_mask_compartments: {events(compartments)}")
    overlap()
    torch.cuda.synchronize()
    print(f"{n} cells, {m} objects, {len(g['cell'])} pairs, largest degree {int(g['degree'].max())}, overflow {over.tolist()}, {h}x{w}; one read of both "
          f"masks at 6.29 TB/s: {hbm_ms:.4f} ms; the compartments read two masks and write two: {2 * hbm_ms:.4f} ms")
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = ops.overlap_pairs(mask, ids, mask_b, ids_b)
        times.append(1e3 * (time.perf_counter() - t0))
    print(f"whole ops.overlap_pairs (tables up, kernels, copies back, the pair list): median {sorted(times)[2]:.1f} ms, min {min(times):.1f}, max {max(times):.1f} of 5")
    t0 = time.perf_counter()
    owner, inside = matching.owners(g["cell"], g["obj"], g["inter"], g["area_b"])
    cells = matching.cell_rows(g["cell"], g["obj"], g["inter"], g["area_a"], ids_b, owner)
    objects = matching.object_rows(g["cell"], g["obj"], g["inter"], g["area_b"], ids, owner, inside)
    union, iou = matching.pair_rows(g["cell"], g["obj"], g["inter"], g["area_a"], g["area_b"])
    counts, sums = matching.agreement_counts(g["cell"], g["obj"], g["inter"], g["area_a"], g["area_b"])
    rules_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    texts = (matching.cells_csv(ids, cells), matching.objects_csv(ids_b, objects), matching.pairs_csv(ids, ids_b, g["cell"], g["obj"], g["inter"], union, iou))
    text_ms = 1e3 * (time.perf_counter() - t0)
    table = matching.agreement_table(counts, sums)
    print(f"matching.py on the host: owners, cell, object and pair rows, agreement {rules_ms:.0f} ms; the three CSV texts ({sum(len(t) for t in texts) / 1e6:.1f} MB) "
          f"{text_ms:.0f} ms; cells none / single / multi {np.bincount(cells['status'], minlength=3).tolist()}, orphans {int((owner < 0).sum())}, "
          f"tp at IoU 0.5 / 0.75 / 0.95: {int(table[0, 2])} / {int(table[5, 2])} / {int(table[9, 2])}, PQ at 0.5 {table[0, 9]:.4f}")
    t0 = time.perf_counter()
    ta, tb = ops._cell_table(ids), ops._cell_table(ids_b)
    ca, cb = ta[host_a].astype(np.int64), tb[host_b].astype(np.int64)
    both = (ca >= 0) & (cb >= 0)
    keys, count = np.unique((ca[both] << 32) | cb[both], return_counts=True)
    host_ms = 1e3 * (time.perf_counter() - t0)
    same = (np.array_equal(keys >> 32, g["cell"]) and np.array_equal(keys & 0xFFFFFFFF, g["obj"]) and np.array_equal(count, g["inter"])
            and np.array_equal(np.bincount(ca[ca >= 0], minlength=n), g["area_a"]) and np.array_equal(np.bincount(cb[cb >= 0], minlength=m), g["area_b"]))
    print(f"numpy restatement (host): both tables applied and np.unique over {int(both.sum())} 64-bit pair keys {host_ms:.0f} ms; equal to the GPU pairs and areas: {same}")


# ---- marker localisation (csrc/localization.hip): the depth of every labelled pixel below its cell's edge, then the marker sums per depth shell -------
def time_localization():
    """mask, image, ids, boxes, outputs and workspace on the device before the clock starts: each entry point between two device events, median of
    five calls after a warm-up -- ribca_mask_depth at D = 8 and D = 32, ribca_cell_shell_sums on the 15-channel image at the product's seven
    shells; then the whole ops calls with their copies and the host features on the host clock, scipy's exact distance transform of the
    foreground of the same mask (the yardstick of the expansion: it measures to the background only, not to the neighbour), and the numpy
    restatement on a crop, checked against the GPU on the same crop"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import intensities_numpy as IN
    import localization_numpy as LN
    from multiplexed_image_annotator_amd import localization
    from multiplexed_image_annotator_amd._lib import lib, ptr, stream_ptr
    h, w = mask.shape
    c = 15

    def events(call):
        call()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        return f"median {sorted(times)[2]:.3f} ms, min {min(times):.3f}, max {max(times):.3f} of 5 (device events)"

    depth2 = torch.empty_like(mask)
    labelled = int((mask > 0).sum())
    for d in (8, 32):
        ws = torch.empty(max(ops.mask_depth_ws_bytes(h, w, d), 1), dtype=torch.uint8, device=dev)
        took = events(lambda: _lib.check(lib().ribca_mask_depth(ptr(mask), h, w, d, ptr(depth2), ptr(ws), ws.numel(), stream_ptr()), "depth"))
        print(f"mask depth, D = {d}: {took} for {n} cells, {h}x{w}; {int((depth2 == -1).sum())} of {labelled} labelled pixels deeper than D; read + write of "
              f"{2 * h * w * 4 / 1e9:.2f} GB at {HBM_BYTES_PER_S / 1e12:.2f} TB/s: {1e3 * 2 * h * w * 4 / HBM_BYTES_PER_S:.3f} ms")
    depth2 = ops.mask_depth(mask, localization.DEPTH)
    _, raw = synth.make_mask_and_image(h, w, 100000, c, synth.SEED_BASE + 3, device=dev)
    image = (raw.to(torch.float32) / 32767.5 - 1.0).contiguous()      # the normalised range, with the background's ties
    del raw
    ids_d = torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(dev)
    bbox_d = torch.from_numpy(np.ascontiguousarray(tab[:, :4], dtype=np.int32)).to(dev)
    e2 = localization.edges2()
    shells = len(e2) + 1
    out = (torch.empty((n, shells), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev),
           torch.empty((n, c, shells), dtype=torch.float64, device=dev))
    took = events(lambda: ops.cell_shell_sums(image, mask, depth2, ids_d, bbox_d, e2, out=out))
    count = out[0].cpu().numpy()
    print(f"cell shell sums, S = {shells}: {took} for {n} cells, {c} channels, {h}x{w}; one read of the {image.numel() * 4 / 1e9:.2f} GB image at "
          f"{HBM_BYTES_PER_S / 1e12:.2f} TB/s: {1e3 * image.numel() * 4 / HBM_BYTES_PER_S:.2f} ms; counts add up to the label table's areas: "
          f"{np.array_equal(count.sum(axis=1), tab[:, 6])}; pixels per shell {count.sum(axis=0).tolist()}; cells deeper than {localization.DEPTH} px: "
          f"{int((out[1] == -1).sum())}")
    for name, fn in ((f"ops.mask_depth, D = {localization.DEPTH} (scratch allocated, depth2 left on the device)", lambda: ops.mask_depth(mask, localization.DEPTH)),
                     ("ops.cell_shell_sums with the copy of its outputs to the host", lambda: ops.cell_shell_sums(image, mask, depth2, ids_d, bbox_d, e2))):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        print(f"{name}: median {sorted(times)[2]:.2f} ms, min {min(times):.2f}, max {max(times):.2f} of 5 (host clock)")
    t0 = time.perf_counter()
    feat = localization.features(*got, 2)
    print(f"localization.features on the host, band 2, {n} cells x {c} channels: {1e3 * (time.perf_counter() - t0):.0f} ms; cells without a contrast: "
          f"{int(np.isnan(feat['contrast']).all(axis=1).sum())}")
    host = mask.cpu().numpy()
    try:
        from scipy import ndimage
        t0 = time.perf_counter()
        dist = ndimage.distance_transform_edt(host > 0)
        host_ms = 1e3 * (time.perf_counter() - t0)
        near = (host > 0) & (dist <= localization.DEPTH)
        got2 = depth2.cpu().numpy()
        # scipy measures to the background alone: where cells touch, the kernel's depth is the smaller
        print(f"scipy distance_transform_edt of the foreground, {h}x{w} (host): {host_ms:.0f} ms; within {localization.DEPTH} px of the background the "
              f"kernel's depth is never larger: {bool((got2[near] <= np.rint(dist[near] ** 2)).all())}, and smaller, next to another cell, on "
              f"{int((got2[near] < np.rint(dist[near] ** 2)).sum())} of {int(near.sum())} pixels")
    except ImportError:
        print("scipy is not installed: no distance_transform_edt yardstick")
    side = 1024
    crop_mask = np.ascontiguousarray(host[:side, :side])
    crop_image = np.ascontiguousarray(image[:, :side, :side].cpu().numpy())
    crop_ids = np.unique(crop_mask[crop_mask > 0]).astype(np.int32)
    crop_box = IN.boxes_of_all(crop_mask, crop_ids)
    t0 = time.perf_counter()
    want_depth = LN.depth(crop_mask, localization.DEPTH)
    depth_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = LN.shell_sums(crop_image, crop_mask, want_depth, crop_ids, crop_box, e2)
    sums_ms = 1e3 * (time.perf_counter() - t0)
    crop_dev = torch.from_numpy(crop_mask).to(dev)
    g_depth = ops.mask_depth(crop_dev, localization.DEPTH)
    g = ops.cell_shell_sums(torch.from_numpy(crop_image).to(dev), crop_dev, g_depth, crop_ids, crop_box, e2)
    same = (np.array_equal(g_depth.cpu().numpy(), want_depth) and np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1])
            and np.array_equal(g[2].view(np.int64), want[2].view(np.int64)))
    scale = (h * w) / (side * side)
    print(f"numpy restatement, top-left {side}x{side} crop, {len(crop_ids)} cells (host): depth {depth_ms:.0f} ms, shell sums {sums_ms:.0f} ms -> "
          f"{depth_ms * scale / 1e3:.1f} s and {sums_ms * scale / 1e3:.1f} s scaled by area to {h}x{w}; equal to the GPU outputs of the same crop, byte for byte: {same}")


def time_colocalization():
    """mask, image, ids, boxes and outputs on the device before the clock starts: ribca_cell_coloc between two device events, median of five
    calls after a warm-up, at K = 15 (every channel) and at K = 4, and ribca_cell_intensities (median alone) in the same process as the
    yardstick -- 30 trees per cell against the 15 + 120 + 225 of K = 15; then the whole ops.cell_coloc with its copies and the host features on
    the host clock, and the numpy restatement on a crop, checked against the GPU on the same crop"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import coloc_numpy as CN
    import intensities_numpy as IN
    from multiplexed_image_annotator_amd import colocalization
    h, w = mask.shape
    c = 15

    def events(call):
        call()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        return f"median {sorted(times)[2]:.3f} ms, min {min(times):.3f}, max {max(times):.3f} of 5 (device events)"

    _, raw = synth.make_mask_and_image(h, w, 100000, c, synth.SEED_BASE + 3, device=dev)
    image = (raw.to(torch.float32) / 32767.5 - 1.0).contiguous()      # the normalised range, with the background's ties
    del raw
    ids_d = torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(dev)
    bbox_d = torch.from_numpy(np.ascontiguousarray(tab[:, :4], dtype=np.int32)).to(dev)
    hbm = f"one read of the {image.numel() * 4 / 1e9:.2f} GB image at {HBM_BYTES_PER_S / 1e12:.2f} TB/s: {1e3 * image.numel() * 4 / HBM_BYTES_PER_S:.2f} ms"
    for k in (c, 4):
        chan, thr = list(range(k)), colocalization.gates(colocalization.THRESHOLD, k)
        p = k * (k + 1) // 2
        out = (torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n, p), dtype=torch.int32, device=dev),
               torch.empty((n, k), dtype=torch.float64, device=dev), torch.empty((n, p), dtype=torch.float64, device=dev),
               torch.empty((n, k, k), dtype=torch.float64, device=dev))
        took = events(lambda: ops.cell_coloc(image, mask, ids_d, bbox_d, chan, thr, out=out))
        area = out[0].cpu().numpy()
        print(f"cell coloc, K = {k}: {took} for {n} cells, {k + p + k * k} trees per cell, {h}x{w}; {hbm}; areas are the label table's: "
              f"{np.array_equal(area, tab[:, 6])}; cells above {ops.COLOC_RESIDENT} px (streamed): {int((area > ops.COLOC_RESIDENT).sum())}")
    q_num = np.array([1], dtype=np.int32)
    out_i = (torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n, c, 2), dtype=torch.float64, device=dev),
             torch.empty((n, c, 1, 2), dtype=torch.float32, device=dev))
    took = events(lambda: ops.cell_intensities(image, mask, ids_d, bbox_d, q_num, 2, out=out_i))
    print(f"cell intensities, the median alone, same process (the yardstick: {2 * c} trees per cell): {took}")
    chan, thr = list(range(c)), colocalization.gates(colocalization.THRESHOLD, c)
    fn = lambda: ops.cell_coloc(image, mask, ids_d, bbox_d, chan, thr)      # noqa: E731
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    print(f"ops.cell_coloc, K = {c}, with the copy of its outputs to the host: median {sorted(times)[2]:.2f} ms, min {min(times):.2f}, max {max(times):.2f} "
          f"of 5 (host clock)")
    t0 = time.perf_counter()
    feat = colocalization.features(*got)
    print(f"colocalization.features on the host, {n} cells x {c * (c - 1) // 2} pairs: {1e3 * (time.perf_counter() - t0):.0f} ms; cells without any r: "
          f"{int(np.isnan(feat['r']).all(axis=1).sum())}")
    side = 1024
    host = mask.cpu().numpy()
    crop_mask = np.ascontiguousarray(host[:side, :side])
    crop_image = np.ascontiguousarray(image[:, :side, :side].cpu().numpy())
    crop_ids = np.unique(crop_mask[crop_mask > 0]).astype(np.int32)
    crop_box = IN.boxes_of_all(crop_mask, crop_ids)
    t0 = time.perf_counter()
    want = CN.coloc(crop_image, crop_mask, crop_ids, crop_box, chan, thr)
    host_ms = 1e3 * (time.perf_counter() - t0)
    g = ops.cell_coloc(torch.from_numpy(crop_image).to(dev), torch.from_numpy(crop_mask).to(dev), crop_ids, crop_box, chan, thr)
    same = all(a.tobytes() == b.tobytes() for a, b in zip(g, want))
    scale = (h * w) / (side * side)
    print(f"numpy restatement, K = {c}, top-left {side}x{side} crop, {len(crop_ids)} cells (host): {host_ms:.0f} ms -> {host_ms * scale / 1e3:.1f} s scaled "
          f"by area to {h}x{w}; equal to the GPU outputs of the same crop, byte for byte: {same}")


if "--colocalization" in sys.argv:      # this section alone
    time_colocalization()
    sys.exit(0)
if "--localization" in sys.argv:      # this section alone
    time_localization()
    sys.exit(0)
if "--matching" in sys.argv:      # this section alone
    time_matching()
    sys.exit(0)
if "--outlines" in sys.argv:      # this section alone
    time_outlines()
    sys.exit(0)
if "--repair" in sys.argv:      # this section alone
    time_repair()
    sys.exit(0)
if "--expand" in sys.argv:      # this section alone
    time_expand()
    sys.exit(0)
if "--intensities" in sys.argv:      # this section alone
    time_intensities()
    sys.exit(0)
if "--morphology" in sys.argv:      # this section alone
    time_morphology()
    sys.exit(0)
if "--nearest" in sys.argv:      # this section alone
    time_nearest()
    sys.exit(0)
if "--contact" in sys.argv:      # this section alone
    time_contact()
    sys.exit(0)

for name, fn in (("colorize", lambda: ops.colorize(mask, ids, pal[tidx], colors.confidence_colors(conf), (tidx + 1).astype(np.uint8))),
                 ("knn25", lambda: ops.knn_cooccurrence(x, y, tidx, 12, 25)),
                 ("compositions (201-NN, 8 sizes)", lambda: ops.knn_compositions(x, y, tidx, 12)),
                 ("tissue regions (PCA 0.99 + k-means 5 on the counts)",
                  lambda: regions.kmeans(regions.pca_project(ops.knn_composition_counts(x, y, tidx, 12), ops.TISSUE_NEIGHBOURHOODS), 5, 0))):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    print(f"{name}: {1e3 * (time.perf_counter() - t0):.1f} ms for {n} cells, 4096x4096 (host table upload included)")


# ---- the cell-type heat map and composition pie (csrc/celltype_stats.hip) --------------------------------------------------------------
from multiplexed_image_annotator_amd import plots  # noqa: E402

names = np.array([f"type {k:02d}" for k in range(12)])
intensity = rng.random((n, 15))
x_dev, g_dev = torch.from_numpy(intensity).to(dev), torch.from_numpy(tidx.astype(np.int32)).to(dev)
lut = torch.from_numpy(colors.diverging_table()).to(dev)


def heatmap_table(upload):
    xd, gd = (torch.from_numpy(intensity).to(dev), torch.from_numpy(tidx.astype(np.int32)).to(dev)) if upload else (x_dev, g_dev)
    return ops.group_sums(xd, gd, 12)


def pie():
    kept, rays = plots.pie_wedges(np.bincount(tidx, minlength=12))
    return ops.pie_raster(torch.from_numpy(rays).to(dev), torch.from_numpy(pal[kept]).to(dev), 480, 200)


sums, counts, _ = heatmap_table(False)
for name, fn in (("heat-map table (group_sums, 12 types x 15 channels), table on the device", lambda: heatmap_table(False)),
                 ("heat-map table (group_sums), 12 MB host table uploaded", lambda: heatmap_table(True)),
                 ("heat-map raster (12 x 15 cells of 24 px)", lambda: ops.heatmap_raster(sums, counts, lut, 24, 1)),
                 ("pie raster (480 px, 12 wedges)", pie)):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    print(f"{name}: {1e3 * (time.perf_counter() - t0):.2f} ms for {n} cells")

# the reference's loop for the same table: one list comprehension over all cells per cell type, np.mean of a list of rows
annotations = names[tidx].tolist()
rows = list(intensity)
t0 = time.perf_counter()
celltypes = np.unique(annotations)
table = np.zeros((len(celltypes), 15))
for j in range(len(celltypes)):
    indices = [k for k in range(len(annotations)) if annotations[k] == celltypes[j]]
    table[j] = np.mean([rows[k] for k in indices], axis=0)
host_ms = 1e3 * (time.perf_counter() - t0)
err = np.abs(table - (sums / counts[:, None]).cpu().numpy()).max()
print(f"reference's Python loop for the same table (host, model.py:708-715): {host_ms:.1f} ms for {n} cells; max |difference| to the GPU table {err:.2e}")


# ---- the neighbourhood enrichment (csrc/knn.hip, csrc/enrichment.hip): n cells, k = 25, T = 12, P = 1000 ---------------------------------------
sys.path.insert(0, os.path.join(ROOT, "tests"))
import enrichment_numpy as EN  # noqa: E402

PERMS = 1000
idx = ops.knn_neighbours(x, y, 25)
ws = torch.empty(ops.nhood_perm_counts_ws_bytes(n, PERMS), dtype=torch.uint8, device=dev)
for name, fn in (("kNN list (k = 25, host table upload included)", lambda: ops.knn_neighbours(x, y, 25)),
                 (f"{PERMS} label permutations counted (T = 12, m = 24, labels uploaded once per call)", lambda: ops.nhood_perm_counts(idx, tidx, 12, 0, 0, 0, PERMS, ws=ws))):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    print(f"{name}: median {sorted(times)[2]:.1f} ms, min {min(times):.1f}, max {max(times):.1f} of 5 for {n} cells")
idx_host = idx.cpu().numpy()
t0 = time.perf_counter()
want = EN.perm_counts(idx_host, tidx, 12, 0, 0, 0, 10)
oracle_ms = 1e3 * (time.perf_counter() - t0)
same = np.array_equal(out[:10].cpu().numpy(), want)
print(f"numpy restatement, 10 permutations (host): {oracle_ms:.0f} ms -> {oracle_ms * PERMS / 10 / 1e3:.1f} s for {PERMS}; equal to the GPU counts: {same}")


# ---- the co-occurrence by distance (csrc/cooccurrence.hip): n cells, T = 12, bands of 30 px ---------------------------------------------------
import cooccurrence_numpy as CO  # noqa: E402
from multiplexed_image_annotator_amd import cooccurrence  # noqa: E402

xd, yd = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
radial = {}
for name, radii in (("16 bands up to 480 px", cooccurrence.default_radii(30, 16)), ("32 bands up to 960 px", cooccurrence.default_radii(30, 32)),
                    ("1 band up to 480 px", [480.0]), ("1 band over the whole image (every pair counted)", [8192.0]),
                    ("32 bands up to 8192 px (every pair counted)", np.linspace(256.0, 8192.0, 32))):
    fn = lambda: ops.radial_pair_counts(xd, yd, tidx, 12, radii)  # noqa: E731
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    radial[name] = out.cpu().numpy()
    print(f"radial pair counts, {name}: median {sorted(times)[2]:.1f} ms, min {min(times):.1f}, max {max(times):.1f} of 5 for {n} cells, "
          f"{int(out.sum())} of {n * (n - 1)} pairs in range (host table upload included)")
for bands in (16, 32):
    radii = cooccurrence.default_radii(30, bands)
    got = radial[f"{bands} bands up to {30 * bands} px"]
    try:
        from scipy.spatial import cKDTree
        pts = np.stack([xd, yd], axis=1)
        t0 = time.perf_counter()
        trees = [cKDTree(pts[tidx == k]) for k in range(12)]
        cum = np.zeros((bands, 12, 12), dtype=np.int64)
        for a in range(12):
            for c in range(a, 12):
                cum[:, a, c] = cum[:, c, a] = trees[a].count_neighbors(trees[c], radii)
            cum[:, a, a] -= int((tidx == a).sum())      # the tree counts every cell with itself
        tree_ms = 1e3 * (time.perf_counter() - t0)
        ring = np.diff(cum, axis=0, prepend=0)
        print(f"scipy cKDTree.count_neighbors, {bands} radii x 78 type pairs (host, one thread): {tree_ms:.0f} ms; bands differ from the GPU counts in "
              f"{int((ring != got).sum())} of {ring.size} entries (the tree compares distances its own way: a pair on a band edge may move)")
    except ImportError:
        print("scipy is not installed: no cKDTree yardstick")
    m = 10000
    t0 = time.perf_counter()
    want = CO.pair_counts(xd[:m], yd[:m], tidx[:m], 12, radii * radii)
    oracle_ms = 1e3 * (time.perf_counter() - t0)
    same = np.array_equal(ops.radial_pair_counts(xd[:m], yd[:m], tidx[:m], 12, radii).cpu().numpy(), want)
    print(f"numpy oracle, {bands} bands, first {m} cells (host): {oracle_ms:.0f} ms -> {oracle_ms * (n / m) ** 2 / 1e3:.1f} s at {n} cells; equal to the GPU "
          f"counts of the same cells: {same}")


# ---- the spatial autocorrelation (csrc/autocorr.hip): n cells, C = 15, k = 25, P = 1000 -----------------------------------------------------------
import autocorr_numpy as AN  # noqa: E402

z_host = intensity - intensity.mean(axis=0)
z_dev = torch.from_numpy(z_host).to(dev)
ws = torch.empty(ops.autocorr_perm_ws_bytes(n, 15, PERMS), dtype=torch.uint8, device=dev)
for name, fn in (("autocorrelation numerators, observed (C = 15, m = 24, table on the device)", lambda: ops.autocorr_observed(z_dev, idx)),
                 (f"autocorrelation numerators, {PERMS} row permutations (C = 15, m = 24, table on the device, {ws.numel() / 2 ** 20:.1f} MiB workspace)",
                  lambda: ops.autocorr_perm(z_dev, idx, 0, 0, 0, PERMS, ws=ws))):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    print(f"{name}: median {sorted(times)[2]:.1f} ms, min {min(times):.1f}, max {max(times):.1f} of 5 for {n} cells")
t0 = time.perf_counter()
want = AN.perm(z_host, idx_host, 0, 0, 0, 10)
oracle_ms = 1e3 * (time.perf_counter() - t0)
same = out[:10].cpu().numpy().tobytes() == want.tobytes()
print(f"numpy restatement, 10 row permutations (host): {oracle_ms:.0f} ms -> {oracle_ms * PERMS / 10 / 1e3:.1f} s for {PERMS}; bit-equal to the GPU numerators: {same}")


# ---- the local indicators (csrc/local_autocorr.hip): the same table and list, 999 conditional permutations ----------------------------------------
import local_autocorr_numpy as LN  # noqa: E402

LOCAL_PERMS = 999
ws = torch.empty(ops.local_perm_counts_ws_bytes(n, 15, LOCAL_PERMS), dtype=torch.uint8, device=dev)
lag = ops.local_lag(z_dev, idx)
for name, fn in (("local lags (C = 15, m = 24, table on the device)", lambda: ops.local_lag(z_dev, idx)),
                 (f"local counts, {LOCAL_PERMS} conditional permutations (C = 15, m = 24, table on the device, {ws.numel() / 2 ** 20:.1f} MiB workspace)",
                  lambda: ops.local_perm_counts(z_dev, idx, lag, 0, 0, 0, LOCAL_PERMS, ws=ws))):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    print(f"{name}: median {sorted(times)[2]:.1f} ms, min {min(times):.1f}, max {max(times):.1f} of 5 for {n} cells")
lag_host = lag.cpu().numpy()
t0 = time.perf_counter()
want = LN.perm_counts(z_host, idx_host, lag_host, 0, 0, 0, 1)
oracle_ms = 1e3 * (time.perf_counter() - t0)
got = [t.cpu().numpy() for t in ops.local_perm_counts(z_dev, idx, lag, 0, 0, 0, 1)]
same = lag_host.tobytes() == LN.lag(z_host, idx_host).tobytes() and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
print(f"numpy restatement, 1 conditional permutation (host): {oracle_ms:.0f} ms -> {oracle_ms * LOCAL_PERMS / 1e3:.1f} s for {LOCAL_PERMS}; equal to the GPU "
      f"lags and counts: {same}")


# ---- the nearest cell of every type: defined above, beside the switch that runs it alone ------------------------------------------------------------
time_nearest()

# ---- the contact graph of the mask: defined above as well -----------------------------------------------------------------------------------------
time_contact()

# ---- the morphology sums of the mask: defined above as well ----------------------------------------------------------------------------------------
time_morphology()

# ---- the per-cell marker intensities: defined above as well ----------------------------------------------------------------------------------------
time_intensities()

# ---- growing the labels of the mask: defined above as well ------------------------------------------------------------------------------------------
time_expand()
time_repair()
time_outlines()

# ---- matching a second mask: defined above as well ----------------------------------------------------------------------------------------------
time_matching()
