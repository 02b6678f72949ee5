"""``Analyses``: the spatial analyses of an annotated batch, as a mixin of ``Annotator`` (annotator.py), and the idioms they share: the
centroids of an image, the rank gate and the group list, the file names of a group, text files and painted maps, the two exchanges of a
tile-per-rank run, the ranges of a permutation null, the selection of cell types and the marker names.  The methods read the state that
``Annotator`` holds (``preprocessor``, ``annotations``, ``cell_types``, ``label_ids``, rank and mode) and its small accessors.  The host side
of each analysis -- statistics and CSV text -- lives in the module of its name, imported where it is used.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib, colors, dist, ops


def _groups(integrate, n_local: int):
    """the images that share a set of files: the batch with ``integrate``, else every image on its own"""
    return [list(range(n_local))] if integrate else [[i] for i in range(n_local)]


def _all_reduce_counts(arrays, scalars):
    """The tile-per-rank sum of a group's counts: int64 arrays of any shape and integer scalars in ONE fp64 all-reduce (exact below 2^53, which
    the callers check before any collective).  Returns the arrays, shapes and dtype restored, and the scalars as ints."""
    flat = [torch.from_numpy(a.reshape(-1).astype(np.float64)) for a in arrays] + [torch.tensor([float(s) for s in scalars], dtype=torch.float64)]
    buf = dist.all_reduce_sum(torch.cat(flat)).numpy()
    out, at = [], 0
    for a in arrays:
        out.append(buf[at:at + a.size].astype(np.int64).reshape(a.shape))
        at += a.size
    return out, [int(v) for v in buf[at:]]


class Analyses(object):
    """Every analysis works per group (``_groups``) and names its files with ``_group_stem``.  MULTI-RANK RUNS, unless a method says otherwise:
    cell-sharded, rank 0 computes and writes (``_computes_here``: every rank holds the same tables); tile-per-rank, every rank does its own
    images and writes their files, and the integrated group takes one collective every rank enters, after which rank 0 writes the bytes of a
    single-rank run.  Every method raises its ValueErrors first, resets its ``*_stats``, and only then applies the rank gate."""

    NULL_BYTES = 64 << 20      # the permutation counts of one call stay under this on the device; longer nulls go in ranges of permutations

    # ---- the shared idioms ---------------------------------------------------------------------------------------------------------
    def _centroids(self, i: int):
        """(x, y) fp64 of every cell of local image i: np.mean(Column), np.mean(Row) of the reference, from the label table's sums"""
        tab = self.preprocessor.cell_tables[i]
        area = tab[:, 6].astype(np.float64)
        return tab[:, 5].astype(np.float64) / area, tab[:, 4].astype(np.float64) / area

    def _computes_here(self) -> bool:
        """False on the ranks other than 0 of a cell-sharded run, which hold rank 0's tables and leave the analysis to it"""
        return not (self.world_size > 1 and not self.tile_mode and self.rank != 0)

    def _group_stem(self, kind: str, integrate, members):
        """(stem, tail) of a group's file names: ``{batch_id}_integrated_{kind}`` and nothing, or ``{batch_id}_{kind}`` and the image number,
        which goes at the end of each name as neighborhood_analysis places it"""
        if integrate:
            return f"{self.batch_id}_integrated_{kind}", ""
        return f"{self.batch_id}_{kind}", f"_{self._image_number(members[0])}"

    def _write_text(self, name: str, text: str) -> None:
        with open(os.path.join(self.result_dir, name), "w") as f:
            f.write(text)

    def _paint_map(self, i: int, rgb: np.ndarray, idx: np.ndarray, name: str) -> None:
        """``name``: the mask of local image i with every cell in its row of ``rgb`` (n, 3), background 0 -- one ops.colorize call"""
        from PIL import Image
        pre = self.preprocessor
        painted = ops.colorize(pre.masks_dev[i], pre.cell_ids[i], rgb, rgb, idx)[0].cpu().numpy()
        Image.fromarray(painted).save(os.path.join(self.result_dir, name))

    def _gather_rows(self, table: np.ndarray, extra=()):
        """The tile-per-rank exchange of per-cell rows (image number, cell id, ...): one all-reduce of the rows per rank, which also sums the
        integers ``extra``, and one all-gather of equal padded shards.  Returns the rows of every rank by (image number, cell id), the order of
        a single-rank run, and the summed extras."""
        ws = self.world_size
        counts = np.zeros(ws + len(extra), dtype=np.float64)
        counts[self.rank], counts[ws:] = len(table), extra
        counts = dist.all_reduce_sum(torch.from_numpy(counts)).numpy().astype(np.int64)
        cap = int(counts[:ws].max())
        send = np.zeros((cap, table.shape[1]), dtype=np.float64)
        send[:len(table)] = table
        full = dist.all_gather_rows(torch.from_numpy(send), cap * ws).numpy() if cap else send      # equal shards of cap rows
        table = np.concatenate([full[r * cap:r * cap + int(counts[r])] for r in range(ws)], axis=0)
        return table[np.lexsort((table[:, 1], table[:, 0]))], [int(v) for v in counts[ws:]]

    def _null_in_ranges(self, p: int, bytes_per_perm: int):
        """(first permutation, how many) of each call of a null of p permutations: the entry points are pure in the permutation index, so the
        ranges are invisible in the result"""
        per_call = max(1, self.NULL_BYTES // bytes_per_perm)
        for q0 in range(0, p, per_call):
            yield q0, min(per_call, p - q0)

    def _select_types(self, selection, what: str):
        """``anchors`` / ``targets``: cell-type names or indices into ``cell_types`` as a list of indices; None stays None"""
        if selection is None:
            return None
        names = [str(c) for c in self.cell_types]
        wanted = []
        for a in selection:
            k = names.index(a) if isinstance(a, str) and a in names else a
            if isinstance(k, (str, bool)) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < len(names):
                raise ValueError(f"{what} {a!r} is not one of the cell types {names}")
            wanted.append(int(k))
        return wanted

    def _marker_names(self, width: int):
        """the marker list cut or padded (``channel j``) to the channels of the images"""
        markers = [str(m) for m in self.channel_parser.markers]
        return (markers + [f"channel {j}" for j in range(len(markers), width)])[:width]

    def _check_exact(self, who: str, unit: str, per_image, bound: int, integrate) -> None:
        """Refuses a group whose counts could pass 2^53, before any collective.  ``per_image``: what no count of a local image passes;
        ``bound``: the same for any image -- every rank of a tile-per-rank run knows the number of images of the batch, not their sizes, and
        has to reach the same verdict."""
        if integrate and self.tile_mode:
            worst = self.preprocessor._n_images * bound
        else:
            worst = sum(per_image) if integrate else max(list(per_image) + [0])
        if worst >= 2 ** 53:
            raise ValueError(f"{who}: a group of up to {worst} {unit} does not count exactly in fp64 (2^53)")

    def _check_intensities(self, n_perms, n_neighbors):
        """the first checks of the two autocorrelation methods; returns (permutations, k)"""
        if (len(self.preprocessor.intensity_full) == 0 or self._n_images == 0) and not (self.tile_mode and self.preprocessor._n_images > 0):
            raise ValueError("No intensities: call preprocess() first")
        p = int(n_perms)
        if p < 1:
            raise ValueError(f"n_perms must be at least 1, got {n_perms}")
        return p, int(n_neighbors)

    def _intensity_tables(self, k: int, who: str, markers=None):
        """``preprocessor.intensity_full`` as fp64 tables, checked for ``who``: the channel limit, then the selection ``markers`` (names out
        of the marker list; None = all), then that every image has k cells and a table of its shape.  Returns (tables, channels, marker names,
        selected channels)."""
        full = self.preprocessor.intensity_full
        tables = [None if full[i] is None else np.ascontiguousarray(full[i], dtype=np.float64) for i in range(self._n_images)]      # None: an image without cells
        width = next((t.shape[1] for t in tables if t is not None), len(self.channel_parser.markers))
        if width > ops.AUTOCORR_MAX_CHANNELS:
            raise ValueError(f"{who} handles at most {ops.AUTOCORR_MAX_CHANNELS} channels, got {width}")
        names = self._marker_names(width)
        chosen = list(range(width))
        if markers is not None:
            chosen = []
            for name in markers:
                if str(name) not in names:
                    raise ValueError(f"marker {name!r} is not one of the markers {names}")
                chosen.append(names.index(str(name)))
            if not chosen:
                raise ValueError("markers selects no channel")
        for i, t in enumerate(tables):
            if t is None or len(t) < k:
                raise ValueError(f"image {self._image_number(i)} has {0 if t is None else len(t)} cells, fewer than n_neighbors = {k}")
            if t.ndim != 2 or t.shape[1] != width or len(t) != len(self.preprocessor.cell_tables[i]):
                raise ValueError(f"image {self._image_number(i)}: an intensity table of shape {t.shape} for {len(self.preprocessor.cell_tables[i])} "
                                 f"cells of {width} channels")
        return tables, width, names, chosen

    @staticmethod
    def _centred(table: np.ndarray, group: torch.Tensor):
        """One image's table minus its channel means, and the sums of squares of the result per channel: both ordered fp64 sums on the device
        (two ops.group_sums calls over the single group ``group``)"""
        dev = group.device
        mean = ops.group_sums(torch.from_numpy(table).to(dev), group, 1)[0].cpu().numpy()[0] / float(len(table))
        z = table - mean
        return z, ops.group_sums(torch.from_numpy(z * z).to(dev), group, 1)[0].cpu().numpy()[0]

    @staticmethod
    def _add_in_order(tables: np.ndarray) -> np.ndarray:
        """the (T, C) tables of the images added from +0.0 in ascending image order"""
        total = np.zeros(tables.shape[1:], dtype=tables.dtype)
        for t in tables:
            total = total + t
        return total

    # ---- neighbourhood analysis (model.py:798-800 -> spatial_methods.py:13-130) -----------------------------------------
    def neighborhood_matrix(self, image_indices, n_neighbors=25) -> np.ndarray:
        """Counts of (cell type, neighbour cell type) over every cell's n_neighbors - 1 nearest other cells, summed over the images."""
        t = len(self.cell_types)
        acc = None
        for i in image_indices:
            x, y = self._centroids(i)
            acc = ops.knn_cooccurrence(x, y, self._cell_type_ints(i), t, n_neighbors, out=acc)
        if acc is None:      # a rank that owns no image of the batch (tile-per-rank mode forced on a batch smaller than the world)
            return np.zeros((t, t), dtype=np.float64)
        return acc.cpu().numpy().astype(np.float64)

    def neighborhood_analysis(self, n_neighbors=25, integrate=True, normalize=True):
        """Writes the same CSVs as the reference (``{batch_id}_integrated_neighborhood.csv`` or one ``{batch_id}_neighborhood_{i}.csv``
        per image) and, beside each, the reference's heat map of the matrix as ``.png`` (spatial_methods.py:51-55, 110-114: seaborn's default scaling,
        the matrix min .. max; ops.table_raster, colors.diverging_table, plots.heatmap_figure).  Records ``neighborhood_stats``, one record
        per figure written by this rank.  Multi-rank runs: every rank computes; rank 0 writes, and in tile-per-rank mode every rank writes the
        per-image files of its own images."""
        if len(self.annotations) == 0:
            raise ValueError("No annotations")
        self.neighborhood_stats = []
        for g, idx in enumerate(_groups(integrate, self._n_images)):
            m = self.neighborhood_matrix(idx, n_neighbors)
            if integrate and self.tile_mode:
                # the integrated matrix sums over ALL images of the batch: T x T counts from every rank (cell_types is the batch-wide union on
                # every rank, _get_unique_cell_types, so the type axes agree)
                m = dist.all_reduce_sum(torch.from_numpy(m)).numpy()
            if normalize:
                sums = m.sum(axis=1, keepdims=True)
                m = np.divide(m, sums, out=m.copy(), where=sums > 0)
            name = f"{self.batch_id}_integrated_neighborhood.csv" if integrate else f"{self.batch_id}_neighborhood_{self._image_number(g)}.csv"
            if self.rank == 0 or (self.tile_mode and not integrate):
                with open(os.path.join(self.result_dir, name), "w") as f:
                    f.write("cell_type," + "".join(f"{c}," for c in self.cell_types) + "\n")
                    for r, c in enumerate(self.cell_types):
                        f.write(f"{c}," + "".join(f"{m[r][j]:.3f}," for j in range(len(self.cell_types))) + "\n")
                self.neighborhood_stats.append(self._write_table_figure(name[:-4], m, float(m.min()), float(m.max())))

    def _write_table_figure(self, stem: str, table: np.ndarray, vmin: float, vmax: float, row_names=None, col_names=None) -> dict:
        """``{stem}.png``: the (T, T) table over ``self.cell_types`` -- or the (rows, columns) table over ``row_names`` and ``col_names`` -- on the
        colour scale vmin .. vmax: the rectangle from ops.table_raster, the labels and the colour bar from plots.heatmap_figure.  Returns the
        record of the figure."""
        import time
        from . import plots
        names = [str(c) for c in self.cell_types] if row_names is None else [str(c) for c in row_names]
        columns = names if col_names is None else [str(c) for c in col_names]
        dev = _lib.require_gpu()
        lut = colors.diverging_table()
        t0 = time.perf_counter()
        rect = ops.table_raster(torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).to(dev), torch.from_numpy(lut).to(dev), self.HEATMAP_CELL,
                                self.HEATMAP_GAP, vmin, vmax).cpu().numpy()
        raster_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        fig, lay = plots.heatmap_figure(rect, lut, vmin, vmax, names, columns, self.HEATMAP_CELL)
        fig.save(os.path.join(self.result_dir, stem + ".png"))
        return {"file": stem + ".png", "rows": len(names), "columns": len(columns), "vmin": vmin, "vmax": vmax, "rect": (lay["top"], lay["left"]),
                "raster_ms": raster_ms, "draw_ms": (time.perf_counter() - t0) * 1e3}

    # ---- neighbourhood enrichment: the permutation z-score beside the co-occurrence matrix (histoCAT, squidpy's nhood_enrichment) -----------------
    def neighborhood_enrichment(self, n_neighbors=25, n_perms=1000, integrate=True):
        """z = (observed - mean) / std of every (cell type, neighbour type) count of ``neighborhood_matrix`` against its permutation null: the
        k-NN graph stays, the cell-type labels are shuffled within each image n_perms times (a keyed bijection per (seed, image number,
        permutation); seed = RIBCA_ENRICH_SEED, default 0) and recounted on the GPU (ops.knn_neighbours, ops.nhood_perm_counts), the images of a
        group accumulated into one (n_perms, T, T) tensor.  Per group (the batch with ``integrate``, else every image) it writes
        ``{stem}_neighborhood_enrichment.csv`` (the layout of the neighbourhood CSV, z with three decimals), ``..._enrichment_table.csv`` (long
        form: observed, null mean and std, z, and the permutations at or above / at or below the observed count) and ``..._enrichment.png`` (z on
        the symmetric scale +- max |z|), with stem = ``{batch_id}_integrated`` or ``{batch_id}`` and the image number at the end as
        neighborhood_analysis names its files.  Records ``enrichment_stats``, one record per group written by this rank (``knn_ms``: the observed
        counts and the list; ``perm_ms``: the permutations; ``draw_ms``: everything after them on the host -- z-scores, both CSVs, raster and PNG).
        Multi-rank runs as the class states; the integrated tensor takes the all-reduce (counts are exact in fp64)."""
        import time
        from . import enrichment
        self._check_annotated("No annotations")
        t = len(self.cell_types)
        p = int(n_perms)
        if p < 1:
            raise ValueError(f"n_perms must be at least 1, got {n_perms}")
        if t > ops.NHOOD_MAX_TYPES:
            raise ValueError(f"neighborhood_enrichment handles at most {ops.NHOOD_MAX_TYPES} cell types, got {t}")
        self.enrichment_stats = []
        if not self._computes_here():
            return None
        seed = enrichment.default_seed()
        dev = _lib.require_gpu()
        for members in _groups(integrate, len(self.annotations)):
            obs = torch.zeros((t, t), dtype=torch.int64, device=dev)
            perm = torch.zeros((p, t, t), dtype=torch.int64, device=dev)
            cells, knn_ms, perm_ms = 0, 0.0, 0.0
            for i in members:
                x, y = self._centroids(i)
                types = self._cell_type_ints(i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                obs = ops.knn_cooccurrence(x, y, types, t, n_neighbors, out=obs)
                idx = ops.knn_neighbours(x, y, n_neighbors)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                perm = ops.nhood_perm_counts(idx, types, t, seed, self._image_number(i), 0, p, out=perm)
                torch.cuda.synchronize()
                knn_ms += (t1 - t0) * 1e3
                perm_ms += (time.perf_counter() - t1) * 1e3
                cells += len(x)
            both = torch.cat([obs.reshape(-1), perm.reshape(-1)]).cpu().numpy()      # one copy to the host, before the collective
            if integrate and self.tile_mode:
                (both,), (cells,) = _all_reduce_counts([both], [cells])
            if integrate and self.rank != 0:
                continue
            observed, null = both[:t * t].reshape(t, t), both[t * t:].reshape(p, t, t)
            t0 = time.perf_counter()
            stats = enrichment.z_scores(observed, null)
            names = [str(c) for c in self.cell_types]
            stem, tail = self._group_stem("neighborhood_enrichment", integrate, members)
            self._write_text(stem + tail + ".csv", enrichment.matrix_csv(names, stats["z"]))
            self._write_text(stem + "_table" + tail + ".csv", enrichment.table_csv(names, observed, stats))
            lim = enrichment.colour_limit(stats["z"])
            fig = self._write_table_figure(stem + tail, stats["z"], -lim, lim)
            draw_ms = (time.perf_counter() - t0) * 1e3
            rec = {"file": fig["file"], "n": cells, "T": t, "P": p, "seed": seed, "neighbors": int(n_neighbors), "limit": lim, "rect": fig["rect"],
                   "knn_ms": knn_ms, "perm_ms": perm_ms, "draw_ms": draw_ms}
            self.enrichment_stats.append(rec)
            self.logger.log("Neighbourhood enrichment {}: {} cells, {} cell types, {} permutations (seed {}), |z| up to {:.4g}; kNN {:.1f}, "
                            "permutations {:.1f}, z-scores and drawing {:.1f} ms.".format(rec["file"], cells, t, p, seed, lim, knn_ms, perm_ms, draw_ms))

    # ---- co-occurrence by distance: which cell types attract or avoid each other at which physical distance ------------------------------------
    def cooccurrence_by_distance(self, radii=None, integrate=True, anchors=None):
        """Counts the ordered pairs of cells of one image by (radius band, cell type, neighbour type) on the GPU (ops.radial_pair_counts: band b
        holds radii[b - 1] < distance <= radii[b], in pixels; ``radii`` None = cooccurrence.default_radii(cell_size)) and writes, per group (the
        batch with ``integrate``, the images accumulated into one tensor, else every image), the long table ``{stem}.csv`` -- count, lift and
        their cumulative forms, cooccurrence.table_csv -- and one ``{stem}_{slug}.png`` per anchor cell type: rows = the neighbour types,
        columns = the bands labelled with their outer radius, log2 of the lift on the symmetric scale +- its largest finite magnitude, NaN (no
        pair, or no such cell) silver.  stem = ``{batch_id}_integrated_cooccurrence`` or ``{batch_id}_cooccurrence`` with the image number at the
        end of each name, as neighborhood_analysis places it; slug = cooccurrence.slug(cell type).  ``anchors``: cell-type names (or indices
        into ``cell_types``); None = every cell type with at least one cell in the group.  Records ``cooccurrence_stats``, one record per group
        written by this rank.  Multi-rank runs as the class states; the integrated tensor takes the all-reduce (counts are exact in fp64 below
        2^53; a group that could pass that is refused before any collective)."""
        import time
        from . import cooccurrence, enrichment
        self._check_annotated("No annotations")
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        r = cooccurrence.check_radii(cooccurrence.default_radii(self.cell_size) if radii is None else radii, ops.RADIAL_MAX_BANDS)
        nb = len(r)
        if t > 254:
            raise ValueError(f"cooccurrence_by_distance handles at most 254 cell types, got {t}")
        wanted = self._select_types(anchors, "anchor")
        self.cooccurrence_stats = []
        if not self._computes_here():
            return None
        cap = ops.RADIAL_MAX_CELLS
        sizes = [len(self.preprocessor.cell_ids[i]) for i in range(len(self.annotations))]
        if any(n > cap for n in sizes):
            raise ValueError(f"cooccurrence_by_distance takes at most {cap} cells per image, got {max(sizes)}")
        self._check_exact("cooccurrence_by_distance", "pairs", [n * (n - 1) for n in sizes], cap * (cap - 1), integrate)
        dev = _lib.require_gpu()
        for members in _groups(integrate, len(sizes)):
            acc = torch.zeros((nb, t, t), dtype=torch.int64, device=dev)
            present = np.zeros(t, dtype=np.int64)
            cells, count_ms = 0, 0.0
            for i in members:
                if len(self.preprocessor.cell_tables[i]) == 0:      # an image without cells has no pair
                    continue
                x, y = self._centroids(i)
                types = self._cell_type_ints(i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                acc = ops.radial_pair_counts(x, y, types, t, r, out=acc)      # pairs are only ever formed within one image
                torch.cuda.synchronize()
                count_ms += (time.perf_counter() - t0) * 1e3
                present += np.bincount(types, minlength=t)[:t]
                cells += len(x)
            counts = acc.cpu().numpy()
            if integrate and self.tile_mode:
                (counts, present), (cells,) = _all_reduce_counts([counts, present], [cells])
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            stem, tail = self._group_stem("cooccurrence", integrate, members)
            files = [stem + tail + ".csv"]
            self._write_text(files[0], cooccurrence.table_csv(names, r, counts))
            values = cooccurrence.figure_values(counts, cooccurrence.lift(counts))
            labels = [f"{v:g}" for v in r]
            figures = []
            for a in (wanted if wanted is not None else [k for k in range(t) if present[k] > 0]):
                table = np.ascontiguousarray(values[:, a, :].T)      # rows: neighbour types, columns: bands
                lim = enrichment.colour_limit(table)
                fig = self._write_table_figure(f"{stem}_{cooccurrence.slug(names[a])}{tail}", table, -lim, lim, row_names=names, col_names=labels)
                figures.append({"file": fig["file"], "anchor": names[a], "limit": lim, "rect": fig["rect"]})
                files.append(fig["file"])
            draw_ms = (time.perf_counter() - t0) * 1e3
            rec = {"file": files[0], "files": files, "figures": figures, "n": cells, "T": t, "B": nb, "radii": [float(v) for v in r],
                   "pairs": int(counts.sum()), "count_ms": count_ms, "draw_ms": draw_ms}
            self.cooccurrence_stats.append(rec)
            self.logger.log("Co-occurrence by distance {}: {} cells, {} cell types, {} bands up to {:g} px, {} pairs in range, {} figures; counting {:.1f}, "
                            "table and drawing {:.1f} ms.".format(files[0], cells, t, nb, float(r[-1]), rec["pairs"], len(figures), count_ms, draw_ms))

    # ---- nearest cell of every type: how far is each cell from the nearest cell of type b (scimap's spatial_distance, spatstat's Gcross) ---------
    def nearest_type_distances(self, radii=None, n_perms=0, integrate=True, targets=None):
        """Per cell and cell type the distance to the nearest OTHER cell of that type, searched on the GPU in fp64 (ops.nearest_by_type,
        csrc/nearest.hip; reproducible bits), and from it the cross-type nearest-neighbour distribution G_ab(r): the fraction of a-cells whose
        nearest b-cell lies within r, for r = each of ``radii`` (pixels; None = cooccurrence.default_radii(cell_size)).  No edge correction.
        ``n_perms`` > 0 adds a label-permutation null -- the positions stay, the cell-type labels are shuffled within each image (the keyed
        bijection of neighborhood_enrichment per (seed, image number, permutation); seed = RIBCA_NEAREST_SEED, default 0) and the nearest
        distances are searched again (ops.nearest_perm_counts) -- and z = (observed - mean) / std of every cumulative count; no p-value and no
        multiple-testing correction.  Per image it writes ``{batch_id}_nearest_{image number}.csv`` (nearest.cells_csv: one line per cell in
        ``cell_ids`` order, distance and id of the nearest cell of every type) and one map ``{batch_id}_nearest_{slug}_{image number}.png`` per
        target type: the mask painted through ops.colorize with viridis at int(min(d / r_max, 1) * 255), r_max the last radius, background 0;
        an image without a cell of that type is silver.  ``targets``: cell-type names (or indices into ``cell_types``); None = every type with
        a cell in the image.  Per group (the batch with ``integrate``, the images added up, else every image) ``{stem}.csv`` (nearest.table_csv)
        and one ``{stem}_{slug}.png`` per anchor type present -- rows = the target types, columns = the radii, G on the fixed scale 0 .. 1 --
        and with a null ``{stem}_{slug}_z.png`` on the scale +- its largest finite |z|; stem = ``{batch_id}_integrated_nearest_table`` or
        ``{batch_id}_nearest_table`` with the image number at the end of each name.  Records ``nearest_stats``, one record per group written by
        this rank.  Multi-rank runs as the class states; the integrated counts take the all-reduce (exact in fp64 below 2^53; a group that
        could pass that is refused before any collective)."""
        import time
        from . import cooccurrence, enrichment, nearest
        self._check_annotated("No annotations")
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        r = cooccurrence.check_radii(cooccurrence.default_radii(self.cell_size) if radii is None else radii, ops.RADIAL_MAX_BANDS)
        nb = len(r)
        p = int(n_perms)
        if p < 0:
            raise ValueError(f"n_perms must not be negative, got {n_perms}")
        if t > ops.NEAREST_MAX_TYPES:
            raise ValueError(f"nearest_type_distances handles at most {ops.NEAREST_MAX_TYPES} cell types, got {t}")
        if p > 0 and t > ops.NEAREST_PERM_MAX_TYPES:
            raise ValueError(f"nearest_type_distances with a permutation null handles at most {ops.NEAREST_PERM_MAX_TYPES} cell types, got {t}")
        wanted = self._select_types(targets, "target")
        cap = ops.NEAREST_MAX_CELLS
        sizes = [len(self.preprocessor.cell_ids[i]) for i in range(len(self.annotations))]
        if any(n > cap for n in sizes):
            raise ValueError(f"nearest_type_distances takes at most {cap} cells per image, got {max(sizes)}")
        self._check_exact("nearest_type_distances", "cells", sizes, cap, integrate)      # no count passes the cells of its group
        self.nearest_stats = []
        if not self._computes_here():
            return None
        seed = nearest.default_seed()
        r2 = r * r
        r_max = float(r[-1])
        lut = colors.viridis_table()
        for members in _groups(integrate, len(sizes)):
            observed = np.zeros((nb, t, t), dtype=np.int64)
            null = np.zeros((p, nb, t, t), dtype=np.int64)
            present = np.zeros(t, dtype=np.int64)
            cells, distance_ms, perm_ms, draw_ms = 0, 0.0, 0.0, 0.0
            image_files = []
            for i in members:
                ids = self.preprocessor.cell_ids[i]
                n = len(self.preprocessor.cell_tables[i])
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                near2, arg = np.full((0, t), np.inf), np.full((0, t), -1, dtype=np.int32)
                if n:
                    x, y = self._centroids(i)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    near2_d, arg_d = ops.nearest_by_type(x, y, types, t)
                    near2, arg = near2_d.cpu().numpy(), arg_d.cpu().numpy()
                    t1 = time.perf_counter()
                    for q0, q in self._null_in_ranges(p, 8 * nb * t * t):
                        null[q0:q0 + q] += ops.nearest_perm_counts(x, y, types, t, r, seed, self._image_number(i), q0, q).cpu().numpy()
                    distance_ms += (t1 - t0) * 1e3
                    perm_ms += (time.perf_counter() - t1) * 1e3
                    observed += nearest.observed_counts(near2, types, t, r2)
                here = np.bincount(types, minlength=t)[:t]
                present += here
                cells += n
                t0 = time.perf_counter()
                number = self._image_number(i)
                image_files.append(f"{self.batch_id}_nearest_{number}.csv")
                self._write_text(image_files[-1], nearest.cells_csv(ids, types, names, near2, arg))
                for b in (wanted if wanted is not None else [k for k in range(t) if here[k] > 0]):
                    idx = nearest.distance_colour_index(near2[:, b], r_max)
                    rgb = lut[idx] if here[b] > 0 else np.tile(np.array(colors.SILVER, dtype=np.uint8), (n, 1))
                    image_files.append(f"{self.batch_id}_nearest_{cooccurrence.slug(names[b])}_{number}.png")
                    self._paint_map(i, rgb, idx, image_files[-1])
                draw_ms += (time.perf_counter() - t0) * 1e3
            if integrate and self.tile_mode:
                (observed, null, present), (cells,) = _all_reduce_counts([observed, null, present], [cells])
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            stats = nearest.statistics(observed, null if p > 0 else None, present)
            stem, tail = self._group_stem("nearest_table", integrate, members)
            files = [stem + tail + ".csv"]
            self._write_text(files[0], nearest.table_csv(names, r, observed, present, stats))
            labels = [f"{v:g}" for v in r]
            figures = []
            for a in [k for k in range(t) if present[k] > 0]:
                table = np.ascontiguousarray(stats["G"][:, a, :].T)      # rows: target types, columns: radii
                fig = self._write_table_figure(f"{stem}_{cooccurrence.slug(names[a])}{tail}", table, 0.0, 1.0, row_names=names, col_names=labels)
                figures.append({"file": fig["file"], "anchor": names[a], "what": "G", "limit": 1.0, "rect": fig["rect"]})
                files.append(fig["file"])
                if p > 0:
                    table = np.ascontiguousarray(stats["z"][:, a, :].T)
                    lim = enrichment.colour_limit(table)
                    fig = self._write_table_figure(f"{stem}_{cooccurrence.slug(names[a])}_z{tail}", table, -lim, lim, row_names=names, col_names=labels)
                    figures.append({"file": fig["file"], "anchor": names[a], "what": "z", "limit": lim, "rect": fig["rect"]})
                    files.append(fig["file"])
            draw_ms += (time.perf_counter() - t0) * 1e3
            rec = {"file": files[0], "files": files, "image_files": image_files, "figures": figures, "n": cells, "T": t, "B": nb, "P": p, "seed": seed,
                   "radii": [float(v) for v in r], "distance_ms": distance_ms, "perm_ms": perm_ms, "draw_ms": draw_ms}
            self.nearest_stats.append(rec)
            self.logger.log("Nearest cell of every type {}: {} cells, {} cell types, {} radii up to {:g} px, {} permutations (seed {}), {} figures; "
                            "distances {:.1f}, permutations {:.1f}, tables and drawing {:.1f} ms.".format(
                                files[0], cells, t, nb, r_max, p, seed, len(figures), distance_ms, perm_ms, draw_ms))

    # ---- contact graph: which cells actually touch, read off the segmentation mask (histoCAT's neighbourhood analysis, steinbock's expansion graph) --
    def contact_analysis(self, distance=1, n_perms=0, integrate=True):
        """The contact graph of every image, built on the GPU from the segmentation mask (ops.contact_graph, csrc/contact.hip): two cells are
        neighbours when pixels of theirs lie within ``distance`` pixels of each other (an integer 1 .. 8, Euclidean; 1 = they share a border), and
        every contact carries its number of ordered pixel pairs within that reach (at distance 1 the length of the shared border).  No edge
        correction and no physical units.  ``n_perms`` > 0 adds the label-permutation null of neighborhood_enrichment on THIS graph -- the graph
        stays, the cell-type labels are shuffled within each image (the same keyed bijection per (seed, image number, permutation); seed =
        RIBCA_CONTACT_SEED, default 0; ops.edge_perm_counts) -- and z = (observed - mean) / std of every (cell type, neighbour type) count of
        directed edges (enrichment.z_scores); no p-value and no multiple-testing correction.  Per image it writes
        ``{batch_id}_contact_edges_{image number}.csv`` (every contact once, contact.edges_csv), ``{batch_id}_contact_cells_{image number}.csv``
        (degree, pixel pairs and the neighbours of every type per cell, contact.cells_csv) and ``{batch_id}_contact_degree_{image number}.png``:
        the mask painted through ops.colorize with viridis at int(min(degree / 12, 1) * 255), background 0 -- twelve is a FIXED scale, so that the
        maps of different images compare.  Per group (the batch with ``integrate``, the images added up, else every image), with stem =
        ``{batch_id}_integrated_contact`` or ``{batch_id}_contact`` and the image number at the end of each name: ``{stem}_table.csv``
        (contact.table_csv), ``{stem}_pairs.png`` (the pixel-pair matrix, every row over its sum, on the scale 0 .. its maximum) and with a null
        ``{stem}.csv`` (the z matrix, enrichment.matrix_csv) and ``{stem}.png`` (z on the symmetric scale +- its largest finite magnitude).  A
        group without any edge writes its tables with NaN statistics and launches no null.  Records ``contact_stats``, one record per group
        written by this rank (``max_degree`` and ``slots`` over this rank's images).  Multi-rank runs as the class states; the integrated counts
        take the all-reduce (exact in fp64 below 2^53; a group that could pass that is refused before any collective)."""
        import time
        from . import contact, enrichment
        self._check_annotated("No annotations")
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        if isinstance(distance, bool) or not isinstance(distance, (int, np.integer)) or not 1 <= int(distance) <= ops.CONTACT_MAX_REACH:
            raise ValueError(f"distance must be an integer from 1 to {ops.CONTACT_MAX_REACH} pixels, got {distance!r}")
        d = int(distance)
        p = int(n_perms)
        if p < 0:
            raise ValueError(f"n_perms must not be negative, got {n_perms}")
        if t > ops.CONTACT_MAX_TYPES:
            raise ValueError(f"contact_analysis handles at most {ops.CONTACT_MAX_TYPES} cell types, got {t}")
        if p > 0 and t > ops.CONTACT_PERM_MAX_TYPES:
            raise ValueError(f"contact_analysis with a permutation null handles at most {ops.CONTACT_PERM_MAX_TYPES} cell types, got {t}")
        n_local = len(self.annotations)
        # no sum of pixel pairs passes pixels x offsets of its group (a mask holds fewer than 2^31 pixels)
        reach = contact.DISK_OFFSETS[d - 1]
        self._check_exact("contact_analysis", "pixel pairs", [int(self.preprocessor.masks_dev[i].numel()) * reach for i in range(n_local)],
                          (2 ** 31) * reach, integrate)
        self.contact_stats = []
        if not self._computes_here():
            return None
        seed = contact.default_seed()
        lut = colors.viridis_table()
        dev = _lib.require_gpu()
        for members in _groups(integrate, n_local):
            edges = np.zeros((t, t), dtype=np.int64)
            weight = np.zeros((t, t), dtype=np.int64)
            null = np.zeros((p, t, t), dtype=np.int64)
            cells, n_edges, max_degree, slots, graph_ms, perm_ms, draw_ms = 0, 0, 0, 0, 0.0, 0.0, 0.0
            image_files = []
            for i in members:
                ids = self.preprocessor.cell_ids[i]
                n = len(ids)
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                graph = ops.contact_graph(self.preprocessor.masks_dev[i], ids, d)
                t1 = time.perf_counter()
                src, dst, pairs, degree = graph["src"], graph["dst"], graph["pairs"], graph["degree"]
                if p > 0 and len(src) > 0:
                    src_d, dst_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
                    for q0, q in self._null_in_ranges(p, 8 * t * t):
                        null[q0:q0 + q] += ops.edge_perm_counts(src_d, dst_d, types, t, seed, self._image_number(i), q0, q).cpu().numpy()
                graph_ms += (t1 - t0) * 1e3
                perm_ms += (time.perf_counter() - t1) * 1e3
                here_edges, here_weight = contact.observed(src, dst, pairs, types, t)
                edges += here_edges
                weight += here_weight
                cells += n
                n_edges += len(src)
                max_degree = max(max_degree, int(degree.max()) if n else 0)
                slots = max(slots, int(graph["slots"]))
                t0 = time.perf_counter()
                number = self._image_number(i)
                image_files += [f"{self.batch_id}_contact_edges_{number}.csv", f"{self.batch_id}_contact_cells_{number}.csv",
                                f"{self.batch_id}_contact_degree_{number}.png"]
                self._write_text(image_files[-3], contact.edges_csv(ids, types, names, src, dst, pairs))
                self._write_text(image_files[-2], contact.cells_csv(ids, types, names, src, dst, pairs, degree))
                idx = contact.degree_colour_index(degree)
                self._paint_map(i, lut[idx], idx, image_files[-1])
                draw_ms += (time.perf_counter() - t0) * 1e3
            if integrate and self.tile_mode:
                (edges, weight, null), (cells, n_edges) = _all_reduce_counts([edges, weight, null], [cells, n_edges])
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            stats = None
            if p > 0:
                stats = enrichment.z_scores(edges, null) if n_edges > 0 else contact.nan_stats(t)
            stem, tail = self._group_stem("contact", integrate, members)
            files = [stem + "_table" + tail + ".csv"]
            self._write_text(files[0], contact.table_csv(names, edges, weight, stats))
            share = contact.row_normalised(weight)
            top = float(share.max()) if share.size else 0.0
            fig = self._write_table_figure(stem + "_pairs" + tail, share, 0.0, top if top > 0.0 else 1.0)
            figures = [{"file": fig["file"], "what": "pairs", "limit": top, "rect": fig["rect"]}]
            files.append(fig["file"])
            if p > 0:
                files.append(stem + tail + ".csv")
                self._write_text(files[-1], enrichment.matrix_csv(names, stats["z"]))
                lim = enrichment.colour_limit(stats["z"])
                fig = self._write_table_figure(stem + tail, stats["z"], -lim, lim)
                figures.append({"file": fig["file"], "what": "z", "limit": lim, "rect": fig["rect"]})
                files.append(fig["file"])
            draw_ms += (time.perf_counter() - t0) * 1e3
            rec = {"file": files[0], "files": files, "image_files": image_files, "figures": figures, "n": cells, "E": n_edges, "T": t, "P": p, "d": d,
                   "seed": seed, "max_degree": max_degree, "slots": slots, "graph_ms": graph_ms, "perm_ms": perm_ms, "draw_ms": draw_ms}
            self.contact_stats.append(rec)
            self.logger.log("Contact graph {}: {} cells, {} directed edges within {} px, {} cell types, largest degree {} ({} slots), {} permutations "
                            "(seed {}); graph {:.1f}, permutations {:.1f}, tables and drawing {:.1f} ms.".format(
                                files[0], cells, n_edges, d, t, max_degree, slots, p, seed, graph_ms, perm_ms, draw_ms))

    # ---- cell morphology: what the cells themselves look like, read off the segmentation mask (steinbock's regionprops, MCMICRO's quantification) --
    def cell_morphology(self, integrate=True):
        """The morphology table of every image, built on the GPU from the segmentation mask (ops.mask_morphology, csrc/morphology.hip: integer
        sums per cell) and finished on the host in fp64 (morphology.features, which states every formula): area, centroid, bounding box, extent,
        equivalent diameter, major and minor axis, eccentricity, orientation, the 4-neighbourhood perimeter and circularity, the Euler number of
        the label (1 for one solid blob: a fragmented label or one with holes shows here), the share of the outline that faces other cells,
        whether the cell touches the image border, and ``patch_coverage``, the share of the cell inside the window its classifiers saw
        (morphology.patch_rect at the run's patch size).  Pixel units.  Per image it writes ``{batch_id}_morphology_{image number}.csv``
        (morphology.cells_csv, one line per cell in id order) and two maps painted through ops.colorize with viridis on FIXED scales, background
        0: ``{batch_id}_morphology_diameter_{image number}.png`` at int(min(equivalent_diameter / (2 cell_size), 1) * 255) and
        ``{batch_id}_morphology_coverage_{image number}.png`` at int(patch_coverage * 255).  Per group (the batch with ``integrate``, else every
        image), with stem = ``{batch_id}_integrated_morphology`` or ``{batch_id}_morphology`` and the image number at the end of each name:
        ``{stem}_summary.csv`` (morphology.summary_csv: n, mean, std, min, quartiles, max per cell type and feature), ``{stem}.csv``
        (morphology.standardised_means: (mean of the type - mean of all) / std of all) and ``{stem}.png``, that matrix on +- 3; for a single image
        these two are ``{batch_id}_morphology_means_{image number}.csv`` / ``.png``, since ``{batch_id}_morphology_{image number}.csv`` is its cell
        table.  Records ``morphology_stats``, one record per group written by this rank; its ``kernel_ms`` is the host's clock around
        ops.mask_morphology -- the label table, the copies to the device, both kernels and the copy of the sums back -- not the time of the
        kernels alone (tools/time_consumers.py --morphology times those).  Multi-rank runs as the class states; the integrated group takes one
        all-reduce of the cell counts and one all-gather of the feature rows, which rank 0 orders by (image number, cell id) (``_gather_rows``)."""
        import time
        from . import morphology
        self._check_annotated("No annotations")
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        self.morphology_stats = []
        if not self._computes_here():
            return None
        lut = colors.viridis_table()
        width = 3 + len(morphology.FEATURES)      # image number, cell id, cell type, the features: a row of the tile-per-rank exchange
        for members in _groups(integrate, len(self.annotations)):
            rows, image_files, kernel_ms, draw_ms = [np.zeros((0, width))], [], 0.0, 0.0
            for i in members:
                ids = np.asarray(self.preprocessor.cell_ids[i], dtype=np.int64)
                mask = self.preprocessor.masks_dev[i]
                n = len(ids)
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                h, w = (int(v) for v in mask.shape)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                boxes = np.asarray(self.preprocessor.cell_tables[i])[:, :4].reshape(n, 4)      # of the label table: what the crop was centred on
                got = ops.mask_morphology(mask, ids, morphology.patch_rect(boxes, h, w, self.preprocessor.patch_size))
                kernel_ms += (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                feat = morphology.features(got["sums"], got["bbox"])
                number = self._image_number(i)
                image_files += [f"{self.batch_id}_morphology_{number}.csv", f"{self.batch_id}_morphology_diameter_{number}.png",
                                f"{self.batch_id}_morphology_coverage_{number}.png"]
                self._write_text(image_files[-3], morphology.cells_csv(ids, types, names, feat))
                for name, idx in ((image_files[-2], morphology.diameter_colour_index(feat["equivalent_diameter"], self.cell_size)),
                                  (image_files[-1], morphology.coverage_colour_index(feat["patch_coverage"]))):
                    self._paint_map(i, lut[idx], idx, name)
                rows.append(np.concatenate([np.full((n, 1), float(number)), ids.reshape(n, 1).astype(np.float64), types.reshape(n, 1).astype(np.float64),
                                            morphology.feature_matrix(feat)], axis=1))
                draw_ms += (time.perf_counter() - t0) * 1e3
            table = np.concatenate(rows, axis=0)
            if integrate and self.tile_mode:
                table, _ = self._gather_rows(table)
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            types = table[:, 2].astype(np.int64)
            feat = morphology.from_matrix(table[:, 3:])
            stem, tail = self._group_stem("morphology", integrate, members)
            mid = "" if integrate else "_means"      # {batch_id}_morphology_{image number}.csv is the image's cell table
            files = [stem + "_summary" + tail + ".csv", stem + mid + tail + ".csv"]
            self._write_text(files[0], morphology.summary_csv(names, morphology.summary(types, t, feat)))
            z = morphology.standardised_means(types, t, feat)
            self._write_text(files[1], morphology.matrix_csv(names, z))
            fig = self._write_table_figure(stem + mid + tail, z, -morphology.Z_LIMIT, morphology.Z_LIMIT, row_names=names, col_names=morphology.FEATURES)
            files.append(fig["file"])
            draw_ms += (time.perf_counter() - t0) * 1e3
            cells = len(table)
            odd = int((feat["euler"] != 1).sum())
            cut = int((feat["patch_coverage"] < 1.0).sum())
            on_edge = int((feat["on_image_edge"] > 0).sum())
            rec = {"file": files[0], "files": files, "image_files": image_files, "figure": {"file": fig["file"], "limit": morphology.Z_LIMIT, "rect": fig["rect"]},
                   "n": cells, "T": t, "euler_not_one": odd, "patch_truncated": cut, "on_image_edge": on_edge, "kernel_ms": kernel_ms, "draw_ms": draw_ms}
            self.morphology_stats.append(rec)
            self.logger.log("Cell morphology {}: {} cells, {} cell types; {} labels with an Euler number other than 1, {} cells larger than their "
                            "classifier window, {} on the image border; ops.mask_morphology with its copies {:.1f}, tables and drawing {:.1f} ms.".format(
                                files[0], cells, t, odd, cut, on_edge, kernel_ms, draw_ms))

    # ---- cell outlines: every cell as a polygon with properties, for QuPath, napari and anything that reads GeoJSON ---------------------------------
    def cell_outlines(self):
        """The outline of every cell of every image as polygons, traced on the GPU from the segmentation mask the run works on -- after
        ``repair_mask`` and ``expand_mask`` -- (ops.mask_rings, csrc/outlines.hip: exact closed rings of lattice vertices, exterior rings and
        holes, pixels that touch only at a corner joined as the Euler number of cell_morphology joins them) and written per image as
        ``{batch_id}_outlines_{image number}.geojson`` (outlines.geojson: one FeatureCollection in the layout of QuPath's own export, one
        detection per cell with its id, area and -- after predict() -- cell type, the colour ``colorize`` paints that type and the confidence
        ``export_annotations`` prints; coordinates are [column, row] lattice vertices in pixel units, vertex (r, c) the top-left corner of
        pixel (r, c)) and ``{batch_id}_outlines_{image number}.csv`` (outlines.cells_csv: per cell the area, the exterior and hole rings, the
        vertices, the boundary edges and the saddle passes).  Needs preprocess() only; before predict() the classification and the confidence
        are absent.  Per image only, no collective: cell-sharded runs write on rank 0, tile-per-rank runs on the rank that owns the image.
        Records ``outline_stats``, one record per image written by this rank; its ``kernel_ms`` is the host's clock around ops.mask_rings --
        the label table, both kernels, the sort and the copies back -- (tools/time_consumers.py --outlines times the kernels alone) and
        ``write_ms`` the polygons, both texts and the files."""
        import time
        from . import outlines
        pre = self.preprocessor
        if len(pre.masks_dev) == 0 and not (self.tile_mode and pre._n_images > 0):
            raise ValueError("No masks: call preprocess() first")
        self.outline_stats = []
        if not self._computes_here():
            return None
        annotated = len(self.annotations) == len(pre.masks_dev) and len(self.annotations) > 0
        names = [str(c) for c in self.cell_types]
        for i in range(len(pre.masks_dev)):
            ids = np.asarray(pre.cell_ids[i], dtype=np.int64)
            n = len(ids)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ops.mask_rings(pre.masks_dev[i], ids)
            kernel_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            types = colours = conf = None
            if annotated:
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                colours = np.array(self.colors, dtype=np.uint8).reshape(-1, 3)
                conf = self._confidence_text(i)
            number = self._image_number(i)
            files = [f"{self.batch_id}_outlines_{number}.geojson", f"{self.batch_id}_outlines_{number}.csv"]
            self._write_text(files[0], outlines.geojson(got["rings"], got["first"], got["vertices"], ids, types, names, colours, conf))
            self._write_text(files[1], outlines.cells_csv(got["rings"], ids, types, names))
            write_ms = (time.perf_counter() - t0) * 1e3
            rec = {"file": files[0], "files": files, "annotated": annotated, "calls": int(got["calls"]), "kernel_ms": kernel_ms, "write_ms": write_ms}
            rec.update(outlines.image_stats(got["rings"], n))
            self.outline_stats.append(rec)
            self.logger.log("Cell outlines {}: {} cells, {} rings ({} holes, {} cells in several parts), {} vertices, {} saddle passes, longest ring {} "
                            "edges; ops.mask_rings with its copies {:.1f} ({} call(s)), polygons and files {:.1f} ms.".format(
                                files[0], n, rec["rings"], rec["holes"], rec["multi_part"], rec["vertices"], rec["saddles"], rec["longest_ring"],
                                kernel_ms, rec["calls"], write_ms))

    # ---- mask matching: a second mask of the same images -- nuclei, another tool's cells -- against the cells -----------------------------------------
    def _second_masks(self, second_masks):
        """The second mask of every LOCAL image as (H, W) int32 host arrays, read and checked before ``mask_matching`` changes anything:
        ``second_masks`` (one entry per row of the batch CSV: a path for preprocess.read_image or an (H, W) integer array) or, for None, the
        column ``second_mask_path`` of the batch CSV.  ValueError without either, for an entry that is missing or no integer image, and for a
        shape other than that of the image's mask."""
        from .preprocess import read_image
        pre = self.preprocessor
        source = second_masks if second_masks is not None else getattr(pre, "second_mask_paths", None)
        if source is None:
            raise ValueError("mask_matching needs a second mask per image: pass second_masks or add the column second_mask_path to the batch CSV")
        source = list(source)
        if len(source) != pre._n_images:
            raise ValueError(f"mask_matching takes one second mask per row of the batch CSV, got {len(source)} for {pre._n_images} images")
        out = []
        for i in range(len(pre.masks_dev)):
            number = self._image_number(i)
            entry = source[number]
            if entry is None or (isinstance(entry, float) and entry != entry):
                raise ValueError(f"mask_matching: image {number} has no second mask")
            mask = read_image(entry) if isinstance(entry, (str, os.PathLike)) else np.asarray(entry)
            if mask.ndim == 3 and isinstance(entry, (str, os.PathLike)):
                mask = mask[:, :, 0]                      # as the first mask is read: the first channel holds the labels
            want = tuple(int(v) for v in pre.masks_dev[i].shape)
            if mask.ndim != 2 or not (np.issubdtype(mask.dtype, np.integer) or isinstance(entry, (str, os.PathLike))) or tuple(mask.shape) != want:
                raise ValueError(f"mask_matching: the second mask of image {number} must be an integer image of shape {want}, got {mask.dtype} {tuple(mask.shape)}")
            out.append(np.ascontiguousarray(mask.astype(np.int32)))
        return out

    def mask_matching(self, second_masks=None, min_overlap=50, intensities=False, save_masks=False, integrate=True):
        """Matches a SECOND mask of every image to the cells.  Mask A is the mask the run works on (``preprocessor.masks_dev``, after
        ``repair_mask`` and ``expand_mask``), its cells the run's cells; mask B is ``second_masks[row of the batch CSV]`` -- a path or an (H, W)
        integer array -- or, for None, the file in the column ``second_mask_path`` of the batch CSV, used as read (neither repaired nor
        expanded), its OBJECTS the labels of ops.label_table(B): nuclei beside whole cells, or another tool's segmentation of the same image.
        The pixels every (cell, object) pair shares are counted on the GPU (ops.overlap_pairs, csrc/overlap.hip: exact integers), the rules
        are matching.py's, in int64 and fp64: an object is OWNED by the cell that holds most of it when that is at least ``min_overlap``
        percent (1 .. 100) of the object, else it is an orphan.  Needs preprocess() only; after predict() the tables carry the cell types.
        Per image it writes ``{batch_id}_matching_cells_{k}.csv`` (matching.cells_csv: area, owned objects, nuclear fraction, status none /
        single / multi), ``{batch_id}_matching_objects_{k}.csv`` (matching.objects_csv: owner, share inside it, status matched / split /
        orphan), ``{batch_id}_matching_pairs_{k}.csv`` (every overlapping pair with its intersection, union and IoU) and
        ``{batch_id}_matching_fraction_{k}.png``, the cells painted through ops.colorize with viridis at int(clip(inner_fraction, 0, 1) * 255);
        with ``save_masks`` the two compartments of ops.mask_compartments as ``{batch_id}_matching_inner_{k}.npy`` / ``_outer_{k}.npy`` (int32:
        the cell's label on its pixels inside an owned object / on its other pixels); with ``intensities`` ``{batch_id}_intensities_inner_{k}.csv``
        / ``_outer_{k}.csv``, ops.cell_intensities over those two masks with the cells' own ids and boxes through intensities.features and
        intensities.cells_csv (no maps, no ``_vs_window``), the per-cell means kept as ``self.intensity_inner`` / ``self.intensity_outer``.
        Per group (the batch with ``integrate``, else every image), stem from ``_group_stem("matching", ...)``: ``{stem}_agreement.csv``
        (matching.agreement_table: true positives, precision, recall, F1, mean matched IoU and panoptic quality at IoU 0.5 .. 0.95, the counts and
        IoU sums of the images added in image order) and ``{stem}_summary.csv`` (matching.type_summary per cell type and over all cells).
        Every ValueError -- no masks, a bad ``min_overlap``, no second mask, a second mask of another shape -- is raised BEFORE anything is
        written or any state changes.  Records ``matching_stats``, one record per group written by this rank; its ``kernel_ms`` is the host's
        clock around the ops calls (tools/time_consumers.py --matching times the kernels alone).  Multi-rank runs as cell_morphology: the
        integrated group of a tile-per-rank run takes two ``_gather_rows`` exchanges, the per-cell rows and one row per image."""
        import time
        from . import intensities as cell_stats
        from . import matching
        pre = self.preprocessor
        if len(pre.masks_dev) == 0 and not (self.tile_mode and pre._n_images > 0):
            raise ValueError("No masks: call preprocess() first")
        percent = matching.check_min_overlap(min_overlap)
        seconds = self._second_masks(second_masks)
        self.matching_stats = []
        kept = {"inner": [], "outer": []}
        if intensities:
            self.intensity_inner, self.intensity_outer = kept["inner"], kept["outer"]
        if not self._computes_here():
            return None
        n_local = len(pre.masks_dev)
        annotated = len(self.annotations) == n_local and n_local > 0
        names = [str(c) for c in self.cell_types] if annotated or n_local == 0 else []
        t = len(names)
        lut = colors.viridis_table()
        stats = cell_stats.statistic_names()
        k_thr = len(matching.THRESHOLDS)
        cell_width, image_width = 5, 6 + 4 * k_thr      # image number, cell id, type, status, inner fraction / image number, 0, m, pairs, orphans, slots, counts, IoU sums
        for members in _groups(integrate, n_local):
            cell_rows, image_rows, image_files, kernel_ms, draw_ms = [np.zeros((0, cell_width))], [np.zeros((0, image_width))], [], 0.0, 0.0
            for i in members:
                ids = np.asarray(pre.cell_ids[i], dtype=np.int64)
                n = len(ids)
                mask_a = pre.masks_dev[i]
                types = self._cell_type_ints(i) if annotated and n else np.full(n, -1, dtype=np.int64)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mask_b = torch.from_numpy(seconds[i]).to(mask_a.device)
                ids_b = ops.label_table(mask_b)[0]
                got = ops.overlap_pairs(mask_a, ids, mask_b, ids_b)
                kernel_ms += (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                cell, obj, inter = got["cell"], got["obj"], got["inter"]
                owner, inside = matching.owners(cell, obj, inter, got["area_b"], percent)
                cells = matching.cell_rows(cell, obj, inter, got["area_a"], ids_b, owner)
                objects = matching.object_rows(cell, obj, inter, got["area_b"], ids, owner, inside)
                union, iou = matching.pair_rows(cell, obj, inter, got["area_a"], got["area_b"])
                counts, sums = matching.agreement_counts(cell, obj, inter, got["area_a"], got["area_b"])
                number = self._image_number(i)
                files = [f"{self.batch_id}_matching_{what}_{number}.csv" for what in ("cells", "objects", "pairs")]
                self._write_text(files[0], matching.cells_csv(ids, cells, types, names))
                self._write_text(files[1], matching.objects_csv(ids_b, objects))
                self._write_text(files[2], matching.pairs_csv(ids, ids_b, cell, obj, inter, union, iou))
                files.append(f"{self.batch_id}_matching_fraction_{number}.png")
                idx = matching.fraction_colour_index(cells["inner_fraction"])
                self._paint_map(i, lut[idx], idx, files[-1])
                draw_ms += (time.perf_counter() - t0) * 1e3
                if save_masks or intensities:
                    t0 = time.perf_counter()
                    parts = dict(zip(("inner", "outer"), ops.mask_compartments(mask_a, ids, mask_b, ids_b, owner)))
                    torch.cuda.synchronize()
                    kernel_ms += (time.perf_counter() - t0) * 1e3
                    for part in ("inner", "outer") if save_masks else ():
                        files.append(f"{self.batch_id}_matching_{part}_{number}.npy")
                        np.save(os.path.join(self.result_dir, files[-1]), parts[part].cpu().numpy().astype(np.int32))
                    for part in ("inner", "outer") if intensities else ():
                        image = pre.images_dev[i]
                        t0 = time.perf_counter()
                        area, sums_c, order = ops.cell_intensities(image, parts[part], pre.cell_ids_dev[i], pre.cell_bbox_dev[i], cell_stats.Q_NUM, cell_stats.Q_DEN)
                        kernel_ms += (time.perf_counter() - t0) * 1e3
                        t0 = time.perf_counter()
                        feat = cell_stats.features(area, sums_c, order, cell_stats.Q_NUM, cell_stats.Q_DEN)
                        kept[part].append(feat[:, :, 0].copy())
                        files.append(f"{self.batch_id}_intensities_{part}_{number}.csv")
                        self._write_text(files[-1], cell_stats.cells_csv(ids, types, names, area, self._marker_names(int(image.shape[0])), stats, feat))
                        draw_ms += (time.perf_counter() - t0) * 1e3
                image_files += files
                cell_rows.append(np.stack([np.full(n, float(number)), ids.astype(np.float64), types.astype(np.float64), cells["status"].astype(np.float64),
                                           cells["inner_fraction"]], axis=1).reshape(n, cell_width))
                image_rows.append(np.concatenate([[float(number), 0.0, float(len(ids_b)), float(len(cell)), float((owner < 0).sum()), float(got["slots"])],
                                                  counts.reshape(-1).astype(np.float64), sums]).reshape(1, image_width))
            table, per_image = np.concatenate(cell_rows, axis=0), np.concatenate(image_rows, axis=0)
            if integrate and self.tile_mode:
                table, _ = self._gather_rows(table)
                per_image, _ = self._gather_rows(per_image)
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            counts, sums = matching.add_agreement([(row[6:6 + 3 * k_thr].astype(np.int64).reshape(k_thr, 3), row[6 + 3 * k_thr:]) for row in per_image])
            stem, tail = self._group_stem("matching", integrate, members)
            files = [stem + "_agreement" + tail + ".csv", stem + "_summary" + tail + ".csv"]
            self._write_text(files[0], matching.agreement_csv(matching.agreement_table(counts, sums)))
            status = table[:, 3].astype(np.int64)
            self._write_text(files[1], matching.summary_csv(names, matching.type_summary(table[:, 2].astype(np.int64), t, status, table[:, 4])))
            draw_ms += (time.perf_counter() - t0) * 1e3
            rec = {"file": files[0], "files": files, "image_files": image_files, "n": len(table), "m": int(per_image[:, 2].sum()),
                   "pairs": int(per_image[:, 3].sum()), "none": int((status == 0).sum()), "multi": int((status == 2).sum()),
                   "orphans": int(per_image[:, 4].sum()), "slots": int(per_image[:, 5].max()) if len(per_image) else 0, "min_overlap": percent,
                   "annotated": annotated, "kernel_ms": kernel_ms, "draw_ms": draw_ms}
            self.matching_stats.append(rec)
            self.logger.log("Mask matching {}: {} cells, {} objects of the second mask, {} overlapping pairs; {} cells without an object, {} with "
                            "several, {} orphan objects (an owner needs {} % of its object); ops.overlap_pairs and the compartments with their copies "
                            "{:.1f}, tables and drawing {:.1f} ms.".format(files[0], rec["n"], rec["m"], rec["pairs"], rec["none"], rec["multi"],
                                                                           rec["orphans"], percent, kernel_ms, draw_ms))

    # ---- cell intensities: the marker columns of the single-cell table, over each cell's own pixels (steinbock's measure intensities) ------------
    def cell_intensities(self, integrate=True, maps=True, compartment="cell"):
        """The marker intensity table of every image: per cell and image channel the mean, population std, min, quartiles and max over the cell's
        OWN pixels -- the pixels of its box whose mask value is its id -- from ops.cell_intensities (csrc/intensities.hip: fp64 sums in a fixed
        order, exact order statistics) finished on the host in fp64 (intensities.features, which states every formula), on the scale of
        ``preprocessor.intensity_full``.  That table stays what it is, the reference's soft-mask-weighted mean over every labelled pixel of the
        crop window; this one is the table to export.  Per image it writes ``{batch_id}_intensities_{image number}.csv`` (intensities.cells_csv, one
        line per cell in id order) and, with ``maps``, one ``{batch_id}_intensity_{marker}_{image number}.png`` per marker painted through
        ops.colorize with viridis at int(clip(mean, 0, 1) * 255), background 0 (characters of the marker name outside [A-Za-z0-9] become ``_``).
        Per group (the batch with ``integrate``, else every image), with stem = ``{batch_id}_integrated_intensities`` or ``{batch_id}_intensities``
        and the image number at the end of each name: ``{stem}_summary.csv`` (intensities.summary_csv: n, mean and median of the per-cell means,
        median of the per-cell medians per cell type and marker), ``{stem}.csv`` / ``.png`` (intensities.standardised_medians on +- 3; for a single
        image ``{batch_id}_intensities_medians_{image number}``, since ``{batch_id}_intensities_{image number}.csv`` is its cell table) and, when
        ``intensity_full`` exists for every member, ``{stem}_vs_window.csv`` (intensities.vs_window: how far the window table is from the exact
        mask mean).  Keeps the per-cell means as ``self.intensity_mask``, one (n, C) array per local image, and records ``intensity_stats``, one
        record per group written by this rank; its ``kernel_ms`` is the host's clock around ops.cell_intensities -- the kernel and the copy of
        its outputs back -- (tools/time_consumers.py --intensities times the kernel alone).  Multi-rank runs as cell_morphology.
        ``compartment``: ``"cell"`` is all of the above.  In a run with ``expand_mask`` > 0, where the mask was grown from nuclei, ``"core"``
        measures over the mask as read (``preprocessor.masks_core_dev`` with the boxes of its own label table) and ``"ring"`` over the grown
        mask with the core's pixels set to 0 and the grown boxes -- what the expansion added: cytoplasm and membrane; a cell whose ring is
        empty is an empty cell of the table (area 0).  Both put ``_core`` / ``_ring`` after ``intensities`` / ``intensity`` in every file
        name, write no ``_vs_window.csv``, leave ``intensity_mask`` alone and keep their means as ``self.intensity_core`` /
        ``self.intensity_ring``; without an expansion they raise ValueError.  Every record of ``intensity_stats`` names its ``compartment``."""
        import time
        from . import intensities
        self._check_annotated("No annotations")
        if compartment not in ("cell", "core", "ring"):
            raise ValueError(f"compartment must be 'cell', 'core' or 'ring', got {compartment!r}")
        if compartment != "cell" and not getattr(self.preprocessor, "expand_mask", 0) > 0:
            raise ValueError(f"compartment {compartment!r} needs a run with expand_mask > 0: without an expansion the mask has one compartment")
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        self.intensity_stats = []
        sfx = "" if compartment == "cell" else "_" + compartment
        kept = []      # the per-cell means of this compartment, one (n, C) array per local image
        setattr(self, "intensity_mask" if compartment == "cell" else "intensity_" + compartment, kept)
        if not self._computes_here():
            return None
        n_local = len(self.annotations)
        lut = colors.viridis_table()
        stats = intensities.statistic_names()
        median = stats.index("median")
        full = self.preprocessor.intensity_full
        c_img = int(self.preprocessor.images_dev[0].shape[0]) if n_local else len(self.channel_parser.markers)
        markers = self._marker_names(c_img)
        width = 4 + 3 * c_img      # image number, cell id, cell type, area, then the means, the medians and the window table: a row of the exchange
        for members in _groups(integrate, n_local):
            rows, image_files, kernel_ms, draw_ms, missing = [np.zeros((0, width))], [], 0.0, 0.0, 0
            for i in members:
                ids = np.asarray(self.preprocessor.cell_ids[i], dtype=np.int64)
                mask, boxes = self.preprocessor.masks_dev[i], self.preprocessor.cell_bbox_dev[i]
                if compartment == "core":
                    mask, boxes = self.preprocessor.masks_core_dev[i], self.preprocessor.core_bbox_dev[i]
                elif compartment == "ring":
                    core = self.preprocessor.masks_core_dev[i]
                    mask = torch.where(core > 0, torch.zeros_like(mask), mask)
                image = self.preprocessor.images_dev[i]
                n = len(ids)
                if int(image.shape[0]) != c_img:
                    raise ValueError(f"image {self._image_number(i)} has {int(image.shape[0])} channels, the batch {c_img}")
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                area, sums, order = ops.cell_intensities(image, mask, self.preprocessor.cell_ids_dev[i], boxes, intensities.Q_NUM, intensities.Q_DEN)
                kernel_ms += (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                feat = intensities.features(area, sums, order, intensities.Q_NUM, intensities.Q_DEN)
                kept.append(feat[:, :, 0].copy())
                number = self._image_number(i)
                image_files.append(f"{self.batch_id}_intensities{sfx}_{number}.csv")
                self._write_text(image_files[-1], intensities.cells_csv(ids, types, names, area, markers, stats, feat))
                if maps:
                    for c, marker in enumerate(markers):
                        image_files.append(f"{self.batch_id}_intensity{sfx}_{intensities.file_slug(marker)}_{number}.png")
                        idx = intensities.colour_index(feat[:, c, 0])
                        self._paint_map(i, lut[idx], idx, image_files[-1])
                window = full[i] if i < len(full) else None
                if n == 0:
                    window = np.zeros((0, c_img))
                elif window is None or np.asarray(window).shape != (n, c_img):
                    window, missing = np.full((n, c_img), np.nan), missing + 1
                rows.append(np.concatenate([np.full((n, 1), float(number)), ids.reshape(n, 1).astype(np.float64), types.reshape(n, 1).astype(np.float64),
                                            area.reshape(n, 1).astype(np.float64), feat[:, :, 0], feat[:, :, median],
                                            np.asarray(window, dtype=np.float64)], axis=1))
                draw_ms += (time.perf_counter() - t0) * 1e3
            table = np.concatenate(rows, axis=0)
            if integrate and self.tile_mode:
                table, (missing,) = self._gather_rows(table, extra=(missing,))      # with the images without a window table, over the ranks
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            types = table[:, 2].astype(np.int64)
            means, medians, window = table[:, 4:4 + c_img], table[:, 4 + c_img:4 + 2 * c_img], table[:, 4 + 2 * c_img:]
            empty, streamed = int((table[:, 3] == 0).sum()), int((table[:, 3] > ops.INTENSITY_RESIDENT).sum())
            stem, tail = self._group_stem("intensities" + sfx, integrate, members)
            mid = "" if integrate else "_medians"      # {batch_id}_intensities_{image number}.csv is the image's cell table
            files = [stem + "_summary" + tail + ".csv", stem + mid + tail + ".csv"]
            self._write_text(files[0], intensities.summary_csv(names, markers, intensities.type_summary(types, t, means, medians)))
            z = intensities.standardised_medians(types, t, means)
            self._write_text(files[1], intensities.matrix_csv(names, markers, z))
            fig = self._write_table_figure(stem + mid + tail, z, -intensities.Z_LIMIT, intensities.Z_LIMIT, row_names=names, col_names=markers)
            files.append(fig["file"])
            if not missing and compartment == "cell":
                files.append(stem + "_vs_window" + tail + ".csv")
                self._write_text(files[-1], intensities.vs_window_csv(markers, intensities.vs_window(means, window)))
            draw_ms += (time.perf_counter() - t0) * 1e3
            cells = len(table)
            rec = {"file": files[0], "files": files, "image_files": image_files, "figure": {"file": fig["file"], "limit": intensities.Z_LIMIT, "rect": fig["rect"]},
                   "n": cells, "C": c_img, "T": t, "compartment": compartment, "area_zero": empty, "streamed": streamed, "kernel_ms": kernel_ms, "draw_ms": draw_ms}
            self.intensity_stats.append(rec)
            self.logger.log("Cell intensities {}: {} cells, {} markers, {} cell types; {} cells without a pixel, {} above {} pixels (streaming form); "
                            "ops.cell_intensities with its copies {:.1f}, tables and drawing {:.1f} ms.".format(
                                files[0], cells, c_img, t, empty, streamed, ops.INTENSITY_RESIDENT, kernel_ms, draw_ms))

    # ---- marker localisation: rim or blob, this cell's rim or the neighbour's spill (CellProfiler's MeasureObjectIntensityDistribution) ----------
    def marker_localization(self, band=2, integrate=True, maps=True):
        """Where every marker sits in every cell, from the segmentation mask the run works on -- after ``repair_mask`` and ``expand_mask``.
        ops.mask_depth (csrc/localization.hip) gives every labelled pixel its depth below the edge of its own cell, the distance to the nearest
        pixel of the background OR of another cell, up to localization.DEPTH pixels; ops.cell_shell_sums adds every marker over the cell's
        pixels per depth shell (localization.EDGES: seven shells) in a fixed fp64 order; localization.features, which states every formula,
        finishes on the host: the mean over the EDGE compartment (depth <= ``band`` pixels, ``band`` one of localization.EDGES) and over the
        INNER compartment (the rest), ``contrast = (edge - inner) / (edge + inner)`` -- near +1 for a membrane marker, near -1 for a nuclear
        one, NaN for a cell too small to have both compartments -- and ``inradius``, the radius of the largest disc inside the cell.  A cell cut
        by the image border is measured from its visible edge only.  Per image it writes ``{batch_id}_localization_{image number}.csv``
        (localization.cells_csv, one line per cell in id order) and, with ``maps``, one ``{batch_id}_localization_{marker}_{image number}.png``
        per marker (intensities.file_slug), the contrast painted through ops.colorize with the diverging table on +- 1
        (localization.colour_index; NaN cells at index 0, background 0).  Per group (the batch with ``integrate``, else every image), with stem
        = ``{batch_id}_integrated_localization`` or ``{batch_id}_localization`` and the image number at the end of each name:
        ``{stem}_profile.csv`` (localization.profile_csv: pixels and pooled mean per cell type, marker and shell), ``{stem}_summary.csv``
        (localization.summary_csv: n, cells with a NaN contrast, mean and median contrast per cell type and marker) and ``{stem}.csv`` /
        ``.png``, the median contrast per type and marker on +- 1 (for a single image ``{batch_id}_localization_medians_{image number}``, since
        ``{batch_id}_localization_{image number}.csv`` is its cell table).  Keeps the per-cell contrasts as ``self.localization_contrast``, one
        (n, C) array per local image, and records ``localization_stats``, one record per group written by this rank; its ``kernel_ms`` is the
        host's clock around ops.mask_depth and ops.cell_shell_sums with the copy of the outputs back (tools/time_consumers.py --localization
        times the kernels alone).  Multi-rank runs as cell_intensities.  A wrong ``band`` raises ValueError before anything is written or
        set."""
        import time
        from . import intensities, localization
        self._check_annotated("No annotations")
        band = localization.check_band(band)
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        self.localization_stats = []
        kept = self.localization_contrast = []
        if not self._computes_here():
            return None
        n_local = len(self.annotations)
        lut = colors.diverging_table()
        e2 = localization.edges2()
        shells = len(e2) + 1
        c_img = int(self.preprocessor.images_dev[0].shape[0]) if n_local else len(self.channel_parser.markers)
        markers = self._marker_names(c_img)
        width = 4 + shells + c_img * shells      # image number, cell id, cell type, deepest, then the counts and the sums: a row of the exchange
        for members in _groups(integrate, n_local):
            rows, image_files, kernel_ms, draw_ms = [np.zeros((0, width))], [], 0.0, 0.0
            for i in members:
                ids = np.asarray(self.preprocessor.cell_ids[i], dtype=np.int64)
                mask, image = self.preprocessor.masks_dev[i], self.preprocessor.images_dev[i]
                n = len(ids)
                if int(image.shape[0]) != c_img:
                    raise ValueError(f"image {self._image_number(i)} has {int(image.shape[0])} channels, the batch {c_img}")
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                depth2 = ops.mask_depth(mask, localization.DEPTH)
                count, deepest, sums = ops.cell_shell_sums(image, mask, depth2, self.preprocessor.cell_ids_dev[i], self.preprocessor.cell_bbox_dev[i], e2)
                kernel_ms += (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                feat = localization.features(count, deepest, sums, band)
                kept.append(feat["contrast"].copy())
                number = self._image_number(i)
                image_files.append(f"{self.batch_id}_localization_{number}.csv")
                self._write_text(image_files[-1], localization.cells_csv(ids, types, names, markers, feat))
                if maps:
                    for c, marker in enumerate(markers):
                        image_files.append(f"{self.batch_id}_localization_{intensities.file_slug(marker)}_{number}.png")
                        idx = localization.colour_index(feat["contrast"][:, c])
                        self._paint_map(i, lut[idx], idx, image_files[-1])
                rows.append(np.concatenate([np.full((n, 1), float(number)), ids.reshape(n, 1).astype(np.float64), types.reshape(n, 1).astype(np.float64),
                                            deepest.reshape(n, 1).astype(np.float64), count.reshape(n, shells).astype(np.float64),
                                            sums.reshape(n, c_img * shells)], axis=1))
                draw_ms += (time.perf_counter() - t0) * 1e3
            table = np.concatenate(rows, axis=0)
            if integrate and self.tile_mode:
                table, _ = self._gather_rows(table)
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            cells = len(table)
            types = table[:, 2].astype(np.int64)
            deepest, count = table[:, 3].astype(np.int64), table[:, 4:4 + shells].astype(np.int64)
            sums = table[:, 4 + shells:].reshape(cells, c_img, shells)
            feat = localization.features(count, deepest, sums, band)
            stem, tail = self._group_stem("localization", integrate, members)
            mid = "" if integrate else "_medians"      # {batch_id}_localization_{image number}.csv is the image's cell table
            files = [stem + "_profile" + tail + ".csv", stem + "_summary" + tail + ".csv", stem + mid + tail + ".csv"]
            self._write_text(files[0], localization.profile_csv(names, markers, *localization.profile(types, t, count, sums)))
            summary = localization.summary(types, t, feat["contrast"])
            self._write_text(files[1], localization.summary_csv(names, markers, summary))
            self._write_text(files[2], localization.matrix_csv(names, markers, summary[:, :, 3]))
            fig = self._write_table_figure(stem + mid + tail, summary[:, :, 3], -localization.LIMIT, localization.LIMIT, row_names=names, col_names=markers)
            files.append(fig["file"])
            draw_ms += (time.perf_counter() - t0) * 1e3
            deeper = int((deepest == -1).sum())
            undefined = int(np.isnan(feat["contrast"]).all(axis=1).sum()) if c_img else 0
            rec = {"file": files[0], "files": files, "image_files": image_files, "figure": {"file": fig["file"], "limit": localization.LIMIT, "rect": fig["rect"]},
                   "n": cells, "C": c_img, "T": t, "band": band, "deeper": deeper, "undefined": undefined, "kernel_ms": kernel_ms, "draw_ms": draw_ms}
            self.localization_stats.append(rec)
            self.logger.log("Marker localization {}: {} cells, {} markers, {} cell types, edge band {} px; {} cells deeper than {} px, {} without a "
                            "contrast; ops.mask_depth and ops.cell_shell_sums with their copies {:.1f}, tables and drawing {:.1f} ms.".format(
                                files[0], cells, c_img, t, band, deeper, localization.DEPTH, undefined, kernel_ms, draw_ms))

    # ---- marker colocalisation: do two markers sit on the same pixels of a cell (CellProfiler's MeasureColocalization) ----------------------------
    def marker_colocalization(self, markers=None, pairs=None, threshold=0.15, integrate=True, maps=True):
        """Whether two markers sit on the same pixels of a cell, from the segmentation mask the run works on -- after ``repair_mask`` and
        ``expand_mask``: a real double positive (the two rise and fall together over the cell's pixels), a segmentation doublet (separate
        lobes) or a neighbour's spill (one fills the cell, the other hugs the rim) read differently.  ops.cell_coloc
        (csrc/colocalization.hip) adds, per cell and in a fixed fp64 order, the selected markers, their centred cross products and each marker
        over the pixels where another is above its gate, and counts the pixels above both gates; colocalization.features, which states every
        formula, finishes on the host: Pearson's ``r``, the Manders ``overlap`` coefficient, the Manders fractions ``m1`` and ``m2``,
        ``both_fraction`` and ``jaccard`` per cell and marker pair.  ``markers``: the names of the channels to correlate, 2 to 32 of them, each
        once (None: every image channel; more than 32 channels need a selection).  ``pairs``: names ``"A:B"`` of selected markers for which the
        full statistics and the maps are written.  ``threshold``: the gate T, 0 <= T < 1, on the normalised scale of ``intensity_full`` -- 0.15
        is CellProfiler's default of 15 %, a default for a setting, not a measured value; the kernel compares the image with
        ``np.float32(2 T - 1)``, strictly.  Per image it writes ``{batch_id}_colocalization_{image number}.csv`` (colocalization.cells_csv,
        one line per cell in id order: ``id``, ``cell type``, ``area``, then ``{A}~{B}_r`` per pair), with ``pairs``
        ``{batch_id}_colocalization_pairs_{image number}.csv`` (colocalization.pairs_csv) and, with ``maps`` too, one
        ``{batch_id}_colocalization_{A}_{B}_{image number}.png`` per named pair (intensities.file_slug), r painted through ops.colorize with
        the diverging table on +- 1 (colocalization.colour_index; NaN cells at index 0, background 0).  Per group (the batch with
        ``integrate``, else every image), with stem = ``{batch_id}_integrated_colocalization`` or ``{batch_id}_colocalization`` and the image
        number at the end of each name: ``{stem}_summary.csv`` (colocalization.summary_csv, per cell type and pair), ``{stem}.csv`` / ``.png``,
        the K x K matrix of the median r over all cells, and ``{stem}_{cell type}.csv`` / ``.png``, the same per cell type present (for a
        single image ``{batch_id}_colocalization_medians...``, since ``{batch_id}_colocalization_{image number}.csv`` is its cell table).
        Keeps the per-cell r as ``self.colocalization_r``, one (n, K (K - 1) / 2) array per local image, and records
        ``colocalization_stats``, one record per group written by this rank; its ``kernel_ms`` is the host's clock around ops.cell_coloc with
        the copy of the outputs back (tools/time_consumers.py --colocalization times the kernel alone).  Multi-rank runs as cell_intensities.
        A wrong argument raises ValueError before anything is written or set."""
        import time
        from . import colocalization, intensities
        self._check_annotated("No annotations")
        n_local = len(self.annotations) if self._computes_here() else 0
        c_img = int(self.preprocessor.images_dev[0].shape[0]) if n_local else len(self.channel_parser.markers)
        all_markers = self._marker_names(c_img)
        if markers is None:
            if c_img > colocalization.MAX_MARKERS:
                raise ValueError(f"marker_colocalization correlates at most {colocalization.MAX_MARKERS} markers and the images have {c_img} "
                                 f"channels: select some with markers=[...]")
            chan = list(range(c_img))
        else:
            chosen = [str(m) for m in markers]
            for m in chosen:
                if all_markers.count(m) != 1 or chosen.count(m) != 1:
                    raise ValueError(f"marker_colocalization: {m!r} is not one marker of {all_markers}, named once")
            chan = [all_markers.index(m) for m in chosen]
        if not 2 <= len(chan) <= colocalization.MAX_MARKERS:
            raise ValueError(f"marker_colocalization correlates 2 to {colocalization.MAX_MARKERS} markers, got {len(chan)}: select some with markers=[...]")
        sel = [all_markers[c] for c in chan]
        k = len(chan)
        p, off = k * (k + 1) // 2, colocalization.off_pairs(k)
        columns = colocalization.parse_pairs(pairs, sel)
        thr = colocalization.gates(threshold, k)
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        self.colocalization_stats = []
        kept = self.colocalization_r = []
        if not self._computes_here():
            return None
        lut = colors.diverging_table()
        width = 4 + p + k + p + k * k      # image number, cell id, cell type, area, then both, sums, cross, gated: a row of the exchange
        for members in _groups(integrate, n_local):
            rows, image_files, kernel_ms, draw_ms = [np.zeros((0, width))], [], 0.0, 0.0
            for i in members:
                ids = np.asarray(self.preprocessor.cell_ids[i], dtype=np.int64)
                mask, image = self.preprocessor.masks_dev[i], self.preprocessor.images_dev[i]
                n = len(ids)
                if int(image.shape[0]) != c_img:
                    raise ValueError(f"image {self._image_number(i)} has {int(image.shape[0])} channels, the batch {c_img}")
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                area, both, sums, cross, gated = ops.cell_coloc(image, mask, self.preprocessor.cell_ids_dev[i], self.preprocessor.cell_bbox_dev[i], chan, thr)
                kernel_ms += (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                feat = colocalization.features(area, both, sums, cross, gated)
                kept.append(feat["r"].copy())
                number = self._image_number(i)
                image_files.append(f"{self.batch_id}_colocalization_{number}.csv")
                self._write_text(image_files[-1], colocalization.cells_csv(ids, types, names, sel, area, feat["r"]))
                if columns:
                    image_files.append(f"{self.batch_id}_colocalization_pairs_{number}.csv")
                    self._write_text(image_files[-1], colocalization.pairs_csv(ids, types, names, sel, columns, area, feat))
                    for col in columns if maps else ():
                        a, b = off[col]
                        image_files.append(f"{self.batch_id}_colocalization_{intensities.file_slug(sel[a])}_{intensities.file_slug(sel[b])}_{number}.png")
                        idx = colocalization.colour_index(feat["r"][:, col])
                        self._paint_map(i, lut[idx], idx, image_files[-1])
                rows.append(np.concatenate([np.full((n, 1), float(number)), ids.reshape(n, 1).astype(np.float64), types.reshape(n, 1).astype(np.float64),
                                            area.reshape(n, 1).astype(np.float64), both.reshape(n, p).astype(np.float64), sums.reshape(n, k),
                                            cross.reshape(n, p), gated.reshape(n, k * k)], axis=1))
                draw_ms += (time.perf_counter() - t0) * 1e3
            table = np.concatenate(rows, axis=0)
            if integrate and self.tile_mode:
                table, _ = self._gather_rows(table)
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            cells = len(table)
            types = table[:, 2].astype(np.int64)
            area, both = table[:, 3].astype(np.int64), table[:, 4:4 + p].astype(np.int64)
            sums, cross = table[:, 4 + p:4 + p + k], table[:, 4 + p + k:4 + 2 * p + k]
            gated = table[:, 4 + 2 * p + k:].reshape(cells, k, k)
            feat = colocalization.features(area, both, sums, cross, gated)
            stem, tail = self._group_stem("colocalization", integrate, members)
            mid = "" if integrate else "_medians"      # {batch_id}_colocalization_{image number}.csv is the image's cell table
            files = [stem + "_summary" + tail + ".csv"]
            self._write_text(files[0], colocalization.summary_csv(names, sel, colocalization.summary(types, t, feat)))
            figures = []
            groups = [("", None)] + [("_" + intensities.file_slug(names[a]), types == a) for a in range(t) if (types == a).any()]
            for suffix, of_type in groups:
                matrix = colocalization.median_matrix(feat["r"], k, of_type)
                files.append(stem + mid + suffix + tail + ".csv")
                self._write_text(files[-1], colocalization.matrix_csv(sel, matrix))
                fig = self._write_table_figure(stem + mid + suffix + tail, matrix, -colocalization.LIMIT, colocalization.LIMIT, row_names=sel, col_names=sel)
                files.append(fig["file"])
                figures.append({"file": fig["file"], "limit": colocalization.LIMIT, "rect": fig["rect"]})
            draw_ms += (time.perf_counter() - t0) * 1e3
            valid = int((~np.isnan(feat["r"])).any(axis=1).sum()) if cells else 0
            rec = {"file": files[0], "files": files, "image_files": image_files, "figure": figures[0], "figures": figures, "n": cells, "K": k, "T": t,
                   "markers": sel, "pairs": [colocalization.pair_names(sel)[c] for c in columns], "threshold": float(threshold), "valid": valid,
                   "kernel_ms": kernel_ms, "draw_ms": draw_ms}
            self.colocalization_stats.append(rec)
            self.logger.log("Marker colocalization {}: {} cells, {} markers, {} cell types, gate {:g}; {} cells with a valid r; ops.cell_coloc with "
                            "its copies {:.1f}, tables and drawing {:.1f} ms.".format(files[0], cells, k, t, float(threshold), valid, kernel_ms, draw_ms))

    # ---- spatial autocorrelation: which markers are spatially structured, before any label is trusted (squidpy's spatial_autocorr) ----------------
    def spatial_autocorrelation(self, n_neighbors=25, n_perms=1000, integrate=True):
        """Moran's I and Geary's C of every image channel over the k-NN graph of the cell centroids (``n_neighbors`` counts the cell itself, as
        in neighborhood_analysis: n_neighbors - 1 neighbours per cell, unit weights), with a permutation null: the graph stays and whole rows of
        ``preprocessor.intensity_full`` move within each image n_perms times (the keyed bijection of neighborhood_enrichment per (seed, image
        number, permutation); seed = RIBCA_AUTOCORR_SEED, default 0).  Needs ``preprocess()`` only -- no classifier, no label.  Per image the
        channel means are ordered fp64 sums (ops.group_sums) divided by the cells, the table is centred on the host, and the numerators come
        from ops.autocorr_observed / ops.autocorr_perm (csrc/autocorr.hip; reproducible bits).  CENTRING IS PER IMAGE: with ``integrate`` the
        statistic is the pooled within-image one -- the numerators and the sums of squares of the images are added from +0.0 in ascending
        image number and n is the total number of cells -- so a slide-to-slide staining difference does not register as autocorrelation.
        Per group (the batch, or every image) it writes ``{batch_id}_integrated_spatial_autocorr.csv`` or
        ``{batch_id}_spatial_autocorr_{image number}.csv`` (autocorr.table_csv: one line per marker with I, C, the mean and population std of
        their nulls, z and the permutations at or above / at or below the observed value; no p-value is formed) and ``.png`` beside it: rows =
        the markers, columns = Moran I and 1 - Geary C on the fixed scale -1 .. 1, NaN (a constant channel) silver.  Records
        ``autocorr_stats``, one record per group written by this rank (``knn_ms``: centring and the list; ``perm_ms``: the observed numerators
        and the permutations; ``draw_ms``: statistics, CSV, raster and PNG).  Multi-rank runs as the class states; the integrated table takes
        one all-reduce every rank enters, each image's numbers in that image's row and +0.0 elsewhere, so they arrive as computed."""
        import time
        from . import autocorr
        p, k = self._check_intensities(n_perms, n_neighbors)
        tables, width, markers, _ = self._intensity_tables(k, "spatial_autocorrelation")
        self.autocorr_stats = []
        if not self._computes_here():
            return None
        seed = autocorr.default_seed()
        dev = _lib.require_gpu()
        one = (p + 1) * 2 * width      # per image: the observed and the permuted numerators, then the sums of squares, then the cells
        for members in _groups(integrate, self._n_images):
            rows = np.zeros((len(members), one + width + 1), dtype=np.float64)
            knn_ms, perm_ms = 0.0, 0.0
            for r, i in enumerate(members):
                x, y = self._centroids(i)
                n = len(tables[i])
                group = torch.zeros(n, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                z, rows[r, one:one + width] = self._centred(tables[i], group)
                zd = torch.from_numpy(z).to(dev)
                idx = ops.knn_neighbours(x, y, k)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                obs = ops.autocorr_observed(zd, idx)
                null = ops.autocorr_perm(zd, idx, seed, self._image_number(i), 0, p)
                rows[r, :one] = torch.cat([obs.reshape(-1), null.reshape(-1)]).cpu().numpy()
                knn_ms += (t1 - t0) * 1e3
                perm_ms += (time.perf_counter() - t1) * 1e3
                rows[r, -1] = float(n)
            if integrate and self.tile_mode:
                buf = np.zeros((self.preprocessor._n_images, rows.shape[1]), dtype=np.float64)
                for r, i in enumerate(members):
                    buf[self._image_number(i)] = rows[r]
                rows = dist.all_reduce_sum(torch.from_numpy(buf)).numpy()
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            total = self._add_in_order(rows)
            cells = int(total[-1])
            stats = autocorr.statistics(total[:2 * width].reshape(2, width), total[2 * width:one].reshape(p, 2, width), total[one:one + width], cells, k - 1)
            stem = "".join(self._group_stem("spatial_autocorr", integrate, members))
            self._write_text(stem + ".csv", autocorr.table_csv(markers, cells, stats))
            fig = self._write_table_figure(stem, autocorr.figure_values(stats), -1.0, 1.0, row_names=markers, col_names=["Moran I", "1 - Geary C"])
            draw_ms = (time.perf_counter() - t0) * 1e3
            rec = {"file": fig["file"], "n": cells, "C": width, "P": p, "seed": seed, "neighbors": k, "rect": fig["rect"], "knn_ms": knn_ms,
                   "perm_ms": perm_ms, "draw_ms": draw_ms}
            self.autocorr_stats.append(rec)
            finite = stats["i"][np.isfinite(stats["i"])]
            self.logger.log("Spatial autocorrelation {}: {} cells, {} markers, {} permutations (seed {}), Moran's I {:.4g} .. {:.4g}; centring and kNN "
                            "{:.1f}, permutations {:.1f}, statistics and drawing {:.1f} ms.".format(
                                rec["file"], cells, width, p, seed, float(finite.min()) if finite.size else float("nan"),
                                float(finite.max()) if finite.size else float("nan"), knn_ms, perm_ms, draw_ms))

    # ---- local indicators of spatial association: WHERE a marker is structured (PySAL's esda.Moran_Local / G_Local) ------------------------------
    def local_autocorrelation(self, n_neighbors=25, n_perms=999, alpha=0.05, markers=None):
        """Local Moran's I and Getis-Ord Gi* of every cell for every selected image channel over the k-NN graph of spatial_autocorrelation
        (``n_neighbors`` counts the cell itself), with a conditional-permutation pseudo-p-value per cell: the cell keeps its row, the other rows
        of ``preprocessor.intensity_full`` move around it n_perms times (the keyed bijection of neighborhood_enrichment per (seed, image number,
        permutation); seed = RIBCA_LOCAL_SEED, default 0), and the neighbour sums are recounted on the GPU (ops.local_lag,
        ops.local_perm_counts, csrc/local_autocorr.hip; reproducible bits).  Needs ``preprocess()`` only.  Centring and the list are per image
        and exactly those of spatial_autocorrelation, so the mean of ``local_i`` over an image is that image's Moran's I.  p =
        min(1, 2 (min(n_ge, n_le) + 1) / (n_perms + 1)), two-sided; a cell with p <= alpha (decided in integers, local_autocorr.statistics) is
        classed HH / LH / LL / HL by the signs of its centred value and its neighbour sum.  NO MULTIPLE-TESTING CORRECTION IS APPLIED: about
        alpha of the cells of an unstructured channel are flagged.  ``markers``: names out of the marker list; None = all.  Per image it writes
        ``{batch_id}_local_autocorr_{image number}.csv`` (local_autocorr.table_csv: one line per cell in ``cell_ids`` order),
        ``..._{image number}_summary.csv`` (the cells per class and marker) and one ``..._{image number}_{marker}.png`` per selected marker:
        the mask painted by class through ops.colorize with colors.LISA_COLORS, background 0.  There is no integrated form and no collective:
        cell-sharded multi-rank runs, rank 0 computes and writes; tile-per-rank, every rank writes its own images' files.  Records
        ``local_autocorr_stats``, one record per image written by this rank (``knn_ms``: centring, the list and the observed sums;
        ``perm_ms``: the permutations; ``draw_ms``: statistics, CSVs, painting and PNGs)."""
        import time
        from . import cooccurrence, local_autocorr
        p, k = self._check_intensities(n_perms, n_neighbors)
        num_den = local_autocorr.alpha_fraction(alpha)
        tables, _, names, chosen = self._intensity_tables(k, "local_autocorrelation", markers)
        self.local_autocorr_stats = []
        if not self._computes_here():
            return None
        seed = local_autocorr.default_seed()
        selected = [names[c] for c in chosen]
        dev = _lib.require_gpu()
        for i in range(self._n_images):
            x, y = self._centroids(i)
            n = len(tables[i])
            group = torch.zeros(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            z, m2 = self._centred(tables[i], group)
            m2 = m2[chosen]
            z = np.ascontiguousarray(z[:, chosen])      # every channel is computed on its own: only the selected ones go to the device
            zd = torch.from_numpy(z).to(dev)
            idx = ops.knn_neighbours(x, y, k)
            lag = ops.local_lag(zd, idx)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ge, le = ops.local_perm_counts(zd, idx, lag, seed, self._image_number(i), 0, p)
            ge, le = ge.cpu().numpy(), le.cpu().numpy()
            t2 = time.perf_counter()
            stats = local_autocorr.statistics(z, lag.cpu().numpy(), ge, le, m2, k - 1, p, alpha)
            stem = f"{self.batch_id}_local_autocorr_{self._image_number(i)}"
            files = [stem + ".csv", stem + "_summary.csv"]
            self._write_text(files[0], local_autocorr.table_csv(self.preprocessor.cell_ids[i], selected, stats))
            self._write_text(files[1], local_autocorr.summary_csv(selected, stats["class"]))
            for c, name in enumerate(selected):
                cls = np.ascontiguousarray(stats["class"][:, c])
                files.append(f"{stem}_{cooccurrence.slug(name)}.png")
                self._paint_map(i, colors.LISA_COLORS[cls], cls, files[-1])
            counts = local_autocorr.class_counts(stats["class"])
            rec = {"file": files[0], "files": files, "n": n, "C": len(chosen), "P": p, "seed": seed, "neighbors": k, "alpha": num_den,
                   "markers": selected, "significant": int(counts[:, 1:].sum()), "knn_ms": (t1 - t0) * 1e3, "perm_ms": (t2 - t1) * 1e3,
                   "draw_ms": (time.perf_counter() - t2) * 1e3}
            self.local_autocorr_stats.append(rec)
            self.logger.log("Local autocorrelation {}: {} cells, {} markers, {} permutations (seed {}), {} significant (cell, marker) pairs at alpha "
                            "{}/{}; centring, kNN and lags {:.1f}, permutations {:.1f}, statistics and drawing {:.1f} ms.".format(
                                files[0], n, len(chosen), p, seed, rec["significant"], num_den[0], num_den[1], rec["knn_ms"], rec["perm_ms"],
                                rec["draw_ms"]))

    # ---- tissue regions (model.py:802-804 -> spatial_methods.py:133-198) -------------------------------------------------
    def tissue_region_analysis(self, n, method="kmeans"):
        """Per-cell region labels from the cell-type make-up of each cell's 10 ... 200 nearest neighbours.  The 201-NN search and the
        counting run on the GPU; for method="kmeans" so do PCA(0.99) and k-means (regions.pca_project / regions.kmeans: scikit-learn's
        defaults restated and seeded with RIBCA_REGION_SEED, so the labels are a pure function of the tables every rank holds), or, with
        RIBCA_REGIONS=sklearn, the reference's two unseeded host calls.  The other methods are the reference's scikit-learn calls."""
        if method == "kmeans":
            from . import regions
            backend = regions.region_backend()
            if backend == "gpu":
                return self._tissue_regions_gpu(n)
        from sklearn.cluster import HDBSCAN, KMeans, SpectralClustering
        from sklearn.decomposition import PCA
        self.n_regions = n
        self.tissue_regions = []
        for i in range(self._n_images):
            x, y = self._centroids(i)
            types = self._cell_type_ints(i)
            comp = ops.knn_compositions(x, y, types, int(types.max()) + 1)
            comp = PCA(n_components=0.99).fit_transform(comp)
            if method == "kmeans":
                clusterer = KMeans(n_clusters=n)
            elif method == "hdbscan":
                clusterer = HDBSCAN(n_clusters=n)        # as written in the reference (raises there too: HDBSCAN has no n_clusters)
            elif method == "spectral":
                clusterer = SpectralClustering(n_clusters=n, n_jobs=self.n_jobs if self.n_jobs and self.n_jobs > 0 else None)
            else:
                raise UnboundLocalError("local variable 'clusterer' referenced before assignment")
            labels = clusterer.fit_predict(comp)
            self.tissue_regions.append({int(k): labels[j] for j, k in enumerate(self.preprocessor.cell_ids[i].tolist())})

    def _tissue_regions_gpu(self, n):
        """method="kmeans" on the GPU, no scikit-learn import.  ``region_stats`` holds one record per image."""
        import time
        from . import regions
        seed = regions.default_seed()
        # what KMeans.fit would raise, before any launch
        regions.validate_n_clusters(n, min((len(ids) for ids in self.preprocessor.cell_ids[:self._n_images]), default=None))
        self.n_regions = n
        self.tissue_regions = []
        self.region_stats = []
        for i in range(self._n_images):
            x, y = self._centroids(i)
            types = self._cell_type_ints(i)
            counts = ops.knn_composition_counts(x, y, types, int(types.max()) + 1)
            t0 = time.perf_counter()
            emb = regions.pca_project(counts, ops.TISSUE_NEIGHBOURHOODS)
            torch.cuda.synchronize()
            pca_ms = (time.perf_counter() - t0) * 1e3
            info = {}
            t0 = time.perf_counter()
            labels = regions.kmeans(emb, n, seed, timings=info)
            kmeans_ms = (time.perf_counter() - t0) * 1e3
            self.tissue_regions.append({int(k): int(labels[j]) for j, k in enumerate(self.preprocessor.cell_ids[i].tolist())})
            stats = {"n": int(counts.shape[0]), "F": int(counts.shape[1] * counts.shape[2]), "d": int(emb.shape[1]), "k": int(n),
                     "iterations": int(info["iterations"]), "pca_ms": pca_ms, "kmeans_ms": kmeans_ms, "backend": "gpu", "seed": seed}
            self.region_stats.append(stats)
            self.logger.log("Tissue regions, image {}: {} cells, {} columns -> {} components, k = {}, {} Lloyd iterations; PCA {:.1f} ms, "
                            "k-means {:.1f} ms (gpu, seed {}).".format(i, stats["n"], stats["F"], stats["d"], n, stats["iterations"], pca_ms,
                                                                       kmeans_ms, seed))
