"""``Annotator``: drop-in for the reference orchestrator on its hot path (cell_type_annotation/model.py:90-919):
same constructor, ``preprocess()``, ``predict(batch_size)``, ``export_annotations()``, ``clear_tmp()``,
``get_cell_type_names()`` and the attributes downstream code reads (``annotations``, ``confidence``, ``annotations_all``,
``cell_types``, ``channel_parser``, ``preprocessor``, ``*_pred``).  Compute runs in the HIP library, the plots included:
``generate_heatmap()`` and ``cell_type_composition()`` reduce and rasterise on the GPU and write a CSV beside every PNG, and
``umap_visualization()`` embeds and draws there, so the reference's own call sequence (main.py:19-28) runs in full against this class.
This file holds the pipeline and those plots; the spatial analyses are the ``Analyses`` mixin (analyses.py).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, colors, dist, ops
from .analyses import Analyses
from .logger import Logger
from .marker_parse import MarkerParser
from .preprocess import ImageProcessor

#: per-model class order (model.py:247-252, 266-270, 284-287, 309-312, 334)
CLASS_NAMES: Dict[str, List[str]] = {
    "immune_full": ["CD4 T cell", "CD8 T cell", "Dendritic cell", "B cell", "M1 macrophage cell", "M2 macrophage cell",
                    "Regulatory T cell", "Granulocyte cell", "Plasma cell", "Natural killer cell", "Mast cell", "Others"],
    "immune_extended": ["CD4 T cell", "CD8 T cell", "Dendritic cell", "B cell", "M1 macrophage cell", "M2 macrophage cell",
                        "Natural killer cell", "Others"],
    "immune_base": ["B cell", "CD4 T cell", "CD8 T cell", "Others", "Dendritic cell"],
    "struct": ["Stroma cell", "Smooth muscle", "Endothelial cell", "Epithelial cell", "Proliferating/tumor cell", "Others"],
    "nerve": ["Nerve cell", "Others"],
}
#: model name -> (parser panel name, checkpoint file under MODEL_DIR)
MODEL_PANEL = {"immune_base": "immune_base", "immune_extended": "immune_extended", "immune_full": "immune_full",
               "struct": "structure", "nerve": "nerve_cell"}
MODEL_DIR = "src/multiplexed_image_annotator/cell_type_annotation/models"   # CWD-relative, as in model.py:189-231
_GID = {name: i for i, name in enumerate(ops.GLOBAL_NAMES)}


def tile_mode_env(min_cells) -> Optional[str]:
    """RIBCA_TILE_MODE as the sharding rule (dist.tile_mode) sees it.  The extra-cell-types step (min_cells > 0) pools the "Others" cells of
    every image of the batch, which tile-per-rank mode keeps on different ranks: there the rule picks cell sharding, and an explicit
    RIBCA_TILE_MODE=1 is refused (on every rank alike, before anything else runs)."""
    env = os.environ.get("RIBCA_TILE_MODE")
    if min_cells is not None and min_cells > 0:
        if env == "1":
            raise ValueError("RIBCA_TILE_MODE=1 cannot be combined with min_cells > 0: the extra cell types are clustered over the 'Others' "
                             "cells of all images together, which tile-per-rank mode keeps on different ranks")
        return "0"
    return env


class _LazyPredictions:
    """list of {cell type: probability} dicts (model.py:412-414) built on first access from the (n, K) table."""

    def __init__(self, model: str, probs: np.ndarray):
        self.model, self.probs, self._dicts = model, probs, None

    def _get(self):
        if self._dicts is None:
            names = CLASS_NAMES[self.model]
            self._dicts = [{names[i]: row[i] for i in range(len(row))} for row in self.probs]
        return self._dicts

    def __len__(self):
        return len(self.probs)

    def __getitem__(self, i):
        return self._get()[i]

    def __iter__(self):
        return iter(self._get())



def _load_state_dict(path: str) -> Dict[str, torch.Tensor]:
    """``{"model": state_dict}`` checkpoint as the reference stores it (model.py:189-231, markerImputer.py:260-271).

    The reference unpickles with ``weights_only=False``; a state dict is plain tensors, so the drop-in uses the loader that executes
    nothing from the file.  MAE-style training scripts (the lineage of the reference's checkpoints) save an ``args`` Namespace, an epoch
    number and optimizer / scaler state beside ``"model"``: ``argparse.Namespace`` is allow-listed for this one load -- rebuilding it
    runs no code from the file (its state is a dict the restricted unpickler has already vetted) -- so such a checkpoint loads as it does
    in the reference.  Anything else the restricted loader refuses is reported with the file name and the remedy; I/O errors (missing
    file, permissions, truncated archive) propagate as what they are.
    """
    import argparse
    import pickle
    try:
        with torch.serialization.safe_globals([argparse.Namespace]):
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except OSError:
        raise
    except (pickle.UnpicklingError, RuntimeError) as e:      # a global outside the allow-list: pickle.UnpicklingError (torch >= 2.4) / RuntimeError
        if isinstance(e, RuntimeError) and "weights_only" not in str(e).lower() and "unpickl" not in str(e).lower() and "global" not in str(e).lower():
            raise      # a truncated or corrupt archive, not a refused global: torch's own message says what is wrong
        raise RuntimeError(
            "{}: not a plain tensor checkpoint (torch.load(weights_only=True) refused it: {}). Re-save it as "
            "torch.save({{'model': model.state_dict()}}, path).".format(path, e)) from e
    if not isinstance(ckpt, dict) or "model" not in ckpt:
        raise RuntimeError("{}: expected a dict with a 'model' state dict".format(path))
    return ckpt["model"]


class Annotator(Analyses):
    def __init__(self, marker_list_path, image_path, device, main_dir='./', batch_id='', strict=True, infer=True, min_cells=-1,
                 normalize=True, blur=False, amax=1, confidence=0.25, cell_size=30, cell_type_confidence=None, n_jobs=0, expand_mask=0, repair_mask=0):
        tile_env = tile_mode_env(min_cells)      # refuses RIBCA_TILE_MODE=1 with min_cells > 0 before any file is read
        self.device = device
        self.cell_types = ["B cell", "CD4 T cell", "CD8 T cell", "Dendritic cell", "Regulatory T cell", "Granulocyte cell", "Mast cell",
                           "M1 macrophage cell", "M2 macrophage cell", "Natural killer cell", "Plasma cell", "Endothelial cell",
                           "Epithelial cell", "Stroma cell", "Smooth muscle", "Proliferating/tumor cell", "Nerve cell", "Others"]
        self.batch_id = batch_id
        self.rank, self.world_size = dist.world()
        log_dir = main_dir if self.rank == 0 else os.path.join(main_dir, f".rank{self.rank}")
        os.makedirs(log_dir, exist_ok=True)
        self.logger = Logger(log_dir)
        self.logger.log_all_hyperparameters({
            "Batch name": batch_id, "Strictly match panel(s)": strict, "Normalize image(s)": normalize,
            "Image blurring kernel size": blur, "Percentile of intensity to upper clip": amax, "Confidence threshold": confidence,
            "Estimated cell size (in pixels)": cell_size})
        self.logger.log("")
        self.logger.log("Start parsing the marker list.")
        self.channel_parser = MarkerParser(strict=strict, logger=self.logger)
        self.channel_parser.parse(marker_list_path)
        self.preprocessor = ImageProcessor(image_path, self.channel_parser, log_dir, device, batch_id, infer, normalize, blur, amax,
                                           cell_size, self.logger, n_jobs=n_jobs, expand_mask=expand_mask, repair_mask=repair_mask)
        self.expand_mask = self.preprocessor.expand_mask      # validated there: 0, or the pixels every label of the mask is grown by
        self.expansion_stats: List[Dict[str, float]] = []     # per local image of an expanded run: n, D, pixels_grown, cells_unchanged, expand_ms
        self.repair_mask = self.preprocessor.repair_mask      # validated there: 0, or the pixels below which a piece of a label is dropped
        self.repair_stats: List[Dict[str, float]] = []        # per local image of a repairing run: the counts of repair.stats and repair_ms
        # multi-rank runs: whole images per rank when the batch CSV has at least one per rank (reference main.py:39-52 batch_run; BASELINE
        # config 5: replicas only, nothing exchanged, every rank writes the CSVs of its own images under their batch-wide numbers), cells of
        # every image otherwise (contiguous shards, one all-gather per image, rank 0 writes)
        self.tile_mode = dist.tile_mode(self.preprocessor._n_images, self.world_size, tile_env)
        self._loaded = False
        self.n_jobs = n_jobs
        self.cell_size = cell_size
        self._n_images = 0
        self.min_cells = min_cells
        self.infer = infer
        self.annotations: List[List[str]] = []
        self.confidence: List[list] = []
        self.immune_annotations, self.struct_annotations, self.nerve_annotations = [], [], []
        self.immune_base_pred, self.immune_extended_pred, self.immune_full_pred = [], [], []
        self.struct_pred, self.nerve_pred = [], []
        self.confidence_thresh = confidence
        self.extra_cell_types = self.min_cells > 0
        self.extra_names: List[str] = []      # "Additional type c" of this run: label id len(ops.GLOBAL_NAMES) + position
        self.extra_stats: Dict[str, float] = {}
        self.n_regions = 0
        self.temp_dir = os.path.join(log_dir, "tmp")
        self.result_dir = os.path.join(main_dir, "results")
        os.makedirs(self.result_dir, exist_ok=True)
        if cell_type_confidence is None:
            self.cell_type_confidence = {name: -1 for name in self.cell_types}
        else:
            self.cell_type_confidence = cell_type_confidence
        self.models: Dict[str, ops.VitModel] = {}
        self.imputers: Dict[str, ops.MaeModel] = {}
        self._weights: Dict[str, Dict[str, torch.Tensor]] = {}
        self.probs: List[Dict[str, np.ndarray]] = []       # per image: model -> (n, K) fp32 host table
        self._conf_arrays: List[np.ndarray] = []           # per image: the float32 confidences behind self.confidence (-1.0 = thresholded)
        self.recheck_stats: List[Dict[str, int]] = []      # per image: cells, re-evaluated near a decision boundary, still within the noise floor
        self.label_ids: List[np.ndarray] = []
        self.chunk_cells = int(os.environ.get("RIBCA_CHUNK_CELLS", "1024"))
        self.streams = int(os.environ.get("RIBCA_STREAMS", "3"))      # cell segments in flight per classifier (ops.VitModel.predict_proba)

    # ---- weights ---------------------------------------------------------------------------------------------------
    def set_weights(self, weights: Dict[str, Dict[str, torch.Tensor]]) -> None:
        """Provide state dicts directly (timm key names) instead of the CWD-relative ``.pth`` files."""
        self._weights.update(weights)

    def load_models(self):
        """model.py:188-239: every checkpoint that exists is loaded; a missing one is reported and skipped."""
        dev = _lib.require_gpu()
        for name in ("immune_base", "immune_extended", "immune_full", "struct", "nerve"):
            sd = self._weights.get(name)
            path = os.path.join(MODEL_DIR, name + ".pth")
            if sd is None and os.path.exists(path):
                sd = _load_state_dict(path)
            if sd is None:
                msg = {"immune_base": "Immune base", "immune_extended": "Immune extended", "immune_full": "Immune full",
                       "struct": "Tissue structure", "nerve": "Nerve cell"}[name] + " model not found"
                print(msg)
                self.logger.log(msg)
                continue
            self.models[name] = ops.VitModel(sd, dev)
        self._loaded = True

    def _imputer(self, panel: str) -> "ops.MaeModel":
        """markerImputer.py:258-287: ``<panel>_impute.pth`` next to the classifier checkpoints, else ValueError("Panel not found")."""
        if panel not in self.imputers:
            sd = self._weights.get(panel + "_impute")
            path = os.path.join(MODEL_DIR, panel + "_impute.pth")
            if sd is None and panel in ("immune_full", "immune_extended", "immune_base") and os.path.exists(path):
                sd = _load_state_dict(path)
            if sd is None:
                raise ValueError("Panel not found")
            self.imputers[panel] = ops.MaeModel(sd, _lib.require_gpu())
            index = self.channel_parser.indices[panel]
            n_present = sum(1 for c in index if c != -1)
            # preprocess.py:272-279, including its loop bound (only the first len(present) entries are inspected)
            msg = "Imputer for {} is created. Marker(s) ".format(panel)
            for ii in range(n_present):
                if index[ii] == -1:
                    msg += "{} ".format(self.channel_parser.panels[panel][ii])
            msg += "are imputed."
            print("Imputer for {} is created".format(panel))
            self.logger.log(msg)
        return self.imputers[panel]

    def _panels_to_impute(self) -> List[str]:
        """preprocess.py:268: panels whose index list holds a -1, unless infer is off (never 'structure'; the reference's
        "nerve" test never matches the real panel name 'nerve_cell', whose panel tolerates no missing marker anyway)."""
        out = []
        for panel in self.channel_parser.panels:
            index = self.channel_parser.indices.get(panel)
            if index is not None and self.infer and -1 in index and panel not in ("structure", "nerve"):
                out.append(panel)
        return out

    # ---- pipeline --------------------------------------------------------------------------------------------------
    def preprocess(self):
        rank, ws = self.rank, self.world_size
        # The reference builds each MarkerImputer inside transform() (preprocess.py:272): a missing ``<panel>_impute.pth`` raises
        # ValueError("Panel not found") there, not in predict().  Here they are built up front, so that every rank fails before
        # any collective is entered (a rank raising later would leave the others waiting in the all-gather).
        for panel in self._panels_to_impute():
            self._imputer(panel)
        if self.tile_mode:
            self.preprocessor.transform(image_filter=lambda i: dist.owns_image(i, rank, ws))
            self._n_images = len(self.preprocessor.image_ids)      # every per-image list below is indexed by LOCAL position
            self.logger.log("rank {} of {}: tile-per-rank mode, images {} of {}".format(rank, ws, self.preprocessor.image_ids,
                                                                                        self.preprocessor._n_images))
            self._record_repair()
            self._record_expansion()
            return
        if ws > 1 and os.environ.get("RIBCA_NORM_SHARD") == "1":
            self.preprocessor.norm_shard = (rank, ws)
        self.preprocessor.transform(shard_fn=(lambda n: dist.shard_bounds(n, rank, ws)) if ws > 1 else None,
                                    gather_fn=(lambda t, n: dist.all_gather_rows(t, n)) if ws > 1 else None)
        self._n_images = self.preprocessor._n_images
        self._record_repair()
        self._record_expansion()

    def _record_repair(self):
        """With repair_mask = A > 0 the mask every stage reads is the mask of the batch CSV repaired by the rules of repair.py
        (ImageProcessor._mask_to_device, ops.repair_labels, csrc/components.hip), before any expansion.  Per local image this writes
        ``{batch_id}_repaired_mask_{image number}.npy`` (int32, the repaired mask before the expansion) and ``{batch_id}_repair_{image
        number}.csv`` (repair.cells_csv: one line per foreground component of the mask as read) and records ``repair_stats``; its ``repair_ms``
        is the host's clock around ops.repair_labels, synchronised (tools/time_consumers.py --repair times the kernel alone).  Multi-rank runs
        as _record_expansion: cell-sharded ranks each repair the whole mask -- integers, the same on every rank -- and rank 0 writes."""
        from . import repair
        self.repair_stats = []
        pre = self.preprocessor
        if self.repair_mask == 0:
            return
        for i in range(len(pre.masks)):
            rec = dict(pre.repair_records[i])
            number = self._image_number(i)
            rec["files"] = [f"{self.batch_id}_repaired_mask_{number}.npy", f"{self.batch_id}_repair_{number}.csv"]
            self.repair_stats.append(rec)
            if self._writes_files():
                np.save(os.path.join(self.result_dir, rec["files"][0]), pre.masks_core_dev[i].cpu().numpy().astype(np.int32))
                with open(os.path.join(self.result_dir, rec["files"][1]), "w") as f:
                    f.write(repair.cells_csv(pre.repair_rows[i]))
            self.logger.log("Mask repair {}: {} labels in, {} out; {} components split off, {} dropped ({} pixels, {} labels removed entirely); "
                            "{} holes filled ({} pixels), {} enclosed by several labels left; ops.repair_labels {:.1f} ms.".format(
                                rec["files"][1], rec["labels_in"], rec["labels_out"], rec["components_split"], rec["components_dropped"],
                                rec["dropped_pixels"], rec["labels_removed"], rec["holes_filled"], rec["hole_pixels"], rec["holes_left"],
                                rec["repair_ms"]))

    def _record_expansion(self):
        """With expand_mask = D > 0 the mask every stage reads is the mask of the batch CSV with each label grown by D pixels
        (ImageProcessor._mask_to_device, ops.expand_labels, csrc/expand.hip; the mask as read stays in ``preprocessor.masks_core_dev``).  Per
        local image this writes ``{batch_id}_expanded_mask_{image number}.npy`` (int32) and ``{batch_id}_expansion_{image number}.csv``
        (expand.cells_csv: id, area_core, area_cell, grown and the box of the grown cell, one line per cell in id order, the areas from the two
        label tables) and records ``expansion_stats``; its ``expand_ms`` is the host's clock around ops.expand_labels, synchronised
        (tools/time_consumers.py --expand times the kernel alone).  Multi-rank runs: tile-per-rank ranks expand and write their own images;
        cell-sharded ranks each expand the whole mask -- integers, the same on every rank, no collective -- and rank 0 writes."""
        from . import expand
        self.expansion_stats = []
        pre = self.preprocessor
        if self.expand_mask == 0:
            return
        for i in range(len(pre.masks)):
            table = expand.rows(pre.cell_ids[i], pre.core_tables[i], pre.cell_tables[i])
            rec = expand.stats(table, self.expand_mask, pre.expand_ms[i])
            number = self._image_number(i)
            rec["files"] = [f"{self.batch_id}_expanded_mask_{number}.npy", f"{self.batch_id}_expansion_{number}.csv"]
            self.expansion_stats.append(rec)
            if self._writes_files():
                np.save(os.path.join(self.result_dir, rec["files"][0]), np.ascontiguousarray(pre.masks[i], dtype=np.int32))
                with open(os.path.join(self.result_dir, rec["files"][1]), "w") as f:
                    f.write(expand.cells_csv(table))
            self.logger.log("Mask expansion {}: {} cells grown by up to {} pixels, {} pixels added, {} cells unchanged; ops.expand_labels {:.1f} ms.".format(
                rec["files"][1], rec["n"], rec["D"], rec["pixels_grown"], rec["cells_unchanged"], rec["expand_ms"]))

    def clear(self):
        self.immune_base_pred, self.immune_extended_pred, self.immune_full_pred = [], [], []
        self.struct_pred, self.nerve_pred = [], []
        self.annotations = []
        self._conf_arrays = []
        self.recheck_stats: List[Dict[str, int]] = []      # per image: cells, re-evaluated near a boundary, still within the noise floor

    def _active_models(self) -> Dict[str, Optional[str]]:
        """model.py:241-349: one immune model (full > extended > base) plus struct / nerve when their panels apply."""
        p = self.channel_parser
        immune = "immune_full" if p.immune_full else ("immune_extended" if p.immune_extended else ("immune_base" if p.immune_base else None))
        return {"immune": immune, "struct": "struct" if p.struct else None, "nerve": "nerve" if p.nerve else None}

    def _predict_cell_types(self, image_idx, model_name, batch_size=None, rows: Optional[torch.Tensor] = None, precise: bool = False) -> torch.Tensor:
        """softmax(model(x), dim=1) for THIS RANK's cells of one image: (n_local, K) device table (predict() gathers).  ``rows``: only
        these local cells (device index tensor); ``precise``: three fp16 passes per product whatever the width (the re-evaluation of
        cells near a decision boundary, see predict())."""
        pre = self.preprocessor
        model = self.models[model_name]
        index = self.channel_parser.indices[MODEL_PANEL[model_name]]
        c_img = pre.images_dev[image_idx].shape[0]
        src = ops.resolve_channels(index, c_img)
        patches = pre.panel_patches(image_idx)
        if rows is not None:
            patches = patches.index_select(0, rows)
        # preprocess.py:268-281: missing markers of an immune panel are imputed unless infer is off (never for structure / nerve)
        if self.infer and -1 in index and MODEL_PANEL[model_name] not in ("structure", "nerve"):
            imputer = self._imputer(MODEL_PANEL[model_name])
            sel = torch.tensor([max(c, 0) for c in src], dtype=torch.long, device=patches.device)
            panel = patches.index_select(1, sel).contiguous()           # channel gather (layout only); blanks are overwritten below
            present = [i for i, c in enumerate(index) if c != -1]
            imputer.impute(panel, present, chunk_cells=ops.MaeModel.CHUNK_FACTOR * self.chunk_cells)
            patches, src = panel, list(range(len(index)))
        if precise:
            return model._forward(patches, src, chunk_cells=self.chunk_cells, streams=1, precise=True)
        return model.predict_proba(patches, src, chunk_cells=self.chunk_cells, streams=self.streams)

    # cells whose vote lies this close to a decision boundary are re-evaluated with three fp16 passes per product (ops.VitModel.RECHECK_MARGIN);
    # those still within NOISE_FLOOR afterwards are counted and logged: two correct fp32 evaluations need not agree on their label
    NOISE_FLOOR = 2.0e-4

    def _recheck_near_boundaries(self, image_idx, tables, pair, tc) -> Dict[str, int]:
        """The MX arithmetic (csrc/gemm_mx.hip) moves softmax outputs by a few 1e-5: a cell whose vote sits within 1e-3 of a boundary
        (top-2 margin, "Others", confidence thresholds -- ops.decision_distance) is recomputed at the full 22-bit operand precision, for
        every model of the voting pair, and its table rows are replaced.  Returns the counts that predict() logs."""
        others = {k: (CLASS_NAMES[k].index("Others") if "Others" in CLASS_NAMES[k] else None) for k in pair if k}
        thresholds = [self.confidence_thresh] + [t for t in tc if t is not None and t >= 0]
        def distance():
            pb = tables[pair[1]] if pair[1] else None
            return ops.decision_distance(tables[pair[0]], others[pair[0]], pb, others.get(pair[1]) if pair[1] else None, thresholds)
        stats = {"cells": int(tables[pair[0]].shape[0]), "re_evaluated": 0, "within_noise_floor": 0}
        if stats["cells"] == 0:
            return stats
        d = distance()
        uses_mx = [k for k in pair if k and self.models[k].uses_mx]
        if uses_mx:
            margin = max(self.models[k].recheck_margin for k in uses_mx)
            stats["margin"] = margin
            rows = torch.nonzero(d < margin).flatten()
            if rows.numel():
                moved = 0.0
                for k in uses_mx:
                    again = self._predict_cell_types(image_idx, k, rows=rows, precise=True)
                    # how far the full-precision result lies from the fast one on these cells: the quantity RECHECK_MARGIN has to dominate
                    moved = max(moved, float((again - tables[k].index_select(0, rows)).abs().max().item()))
                    tables[k].index_copy_(0, rows, again)
                stats["re_evaluated"] = int(rows.numel())
                stats["max_fast_minus_full_precision"] = moved
                d = distance()
        stats["within_noise_floor"] = int((d < self.NOISE_FLOOR).sum().item())
        return stats

    def predict(self, batch_size=32):
        self.logger.log("\nStart predicting cell types and tissue structures.")
        if not self._loaded:
            self.load_models()
        active = self._active_models()
        for role, name in active.items():
            if name is not None and name not in self.models:
                raise AttributeError(f"'Annotator' object has no attribute '{name}_model'")   # what the reference ends up raising
        dev = _lib.require_gpu()
        tc = [self.cell_type_confidence[n] for n in ops.GLOBAL_NAMES]
        for image_idx in range(self._n_images):
            tables: Dict[str, torch.Tensor] = {}
            for role in ("immune", "struct", "nerve"):
                name = active[role]
                if name is None:
                    msg = {"immune": "No immune cell model to predict", "struct": "No structure model to predict",
                           "nerve": "No nerve cell model to predict"}[role]
                    print(msg)
                    self.logger.log(msg)
                    continue
                tables[name] = self._predict_cell_types(image_idx, name, batch_size)
            if not tables:
                raise ValueError("No predictions to merge")
            imm, st, nv = active["immune"], active["struct"], active["nerve"]
            if not (imm == "immune_full" and st and nv):      # (that combination raises below, as the reference does)
                pair0 = (imm, st) if imm and st else (st, nv) if st and nv else (imm, nv) if imm and nv else (imm or st or nv, None)
                rs = self._recheck_near_boundaries(image_idx, tables, pair0, tc)
                self.recheck_stats.append(rs)      # (this rank's shard: the counts are logged per rank, no collective for a log line)
                msg = ("{} of {} cells lay within {:g} of a decision boundary and were re-evaluated at full operand precision; {} remain within "
                       "{:g} (inside the arithmetic's noise floor: another correct fp32 evaluation may label them differently)."
                       ).format(rs["re_evaluated"], rs["cells"], rs.get("margin", ops.VitModel.RECHECK_MARGIN), rs["within_noise_floor"], self.NOISE_FLOOR)
                if "max_fast_minus_full_precision" in rs:
                    msg += " Largest move of a confidence under the re-evaluation: {:.1e} (margin {:g}).".format(rs["max_fast_minus_full_precision"],
                                                                                                                 rs.get("margin", ops.VitModel.RECHECK_MARGIN))
                self.logger.log(msg if self.world_size == 1 else "rank {}: {}".format(self.rank, msg))
            if self.world_size > 1 and not self.tile_mode:
                # ONE all-gather per image: the models' probability columns side by side (<= 33 floats per cell), SURVEY 8(e)
                names = list(tables)
                widths = [tables[k].shape[1] for k in names]
                full = dist.all_gather_rows(torch.cat([tables[k] for k in names], dim=1), len(self.preprocessor.cell_ids[image_idx]))
                tables = {k: t.contiguous() for k, t in zip(names, torch.split(full, widths, dim=1))}
            if imm == "immune_full" and st and nv:
                raise KeyError("Others")       # reference branch 1 (model.py:483-510) fails exactly like this
            if imm and st:
                pair = (imm, st)
            elif st and nv:
                pair = (st, nv)
            elif imm and nv:
                pair = (imm, nv)
            else:
                pair = (imm or st or nv, None)
            pa = tables[pair[0]]
            pb = tables[pair[1]] if pair[1] else None
            lab, conf = ops.vote(pa, [_GID[c] for c in CLASS_NAMES[pair[0]]], pb, [_GID[c] for c in CLASS_NAMES[pair[1]]] if pair[1] else None,
                                 tc, self.confidence_thresh)
            host = {k: v.cpu().numpy() for k, v in tables.items()}
            self.probs.append(host)
            for name, table in host.items():
                lazy = _LazyPredictions(name, table)
                if name.startswith("immune"):
                    getattr(self, name + "_pred").append(lazy)
                    self.immune_annotations.append(lazy)
                elif name == "struct":
                    self.struct_pred.append(lazy)
                    self.struct_annotations.append(lazy)
                else:
                    self.nerve_pred.append(lazy)
                    self.nerve_annotations.append(lazy)
            lab_h = lab.cpu().numpy().astype(np.int64)
            conf_h = conf.cpu().numpy()
            self.label_ids.append(lab_h)
            names = np.array(ops.GLOBAL_NAMES, dtype=object)
            self.annotations.append(names[lab_h].tolist())
            self.confidence.append([-1 if c == -1 else c for c in conf_h])    # int -1 marks a thresholded cell, as in model.py:507
            self._conf_arrays.append(conf_h)
        self.logger.log("Finished predicting cell types and tissue structures.")
        if self.extra_cell_types:
            self._find_extra_cell_types(min_samples=self.min_cells)
        self.cell_types = self._get_unique_cell_types()
        self.cell_types = np.delete(self.cell_types, np.where(self.cell_types == "Others"))
        self.cell_types = np.append(self.cell_types, "Others")
        self.colors = colors.get_colors(len(self.cell_types))     # model.py:459 (the legend PNG of model.py:461-462 is not drawn)
        self._annotations_all = None

    def merge_by_voting(self):
        """model.py:481-640.  predict() has already voted (HIP vote kernel over the probability tables); calling this afterwards,
        as external code following the reference might, leaves the result as is.  Before predict() it fails as the reference does."""
        if len(self.annotations) == 0:
            raise ValueError("No predictions to merge")

    @property
    def annotations_all(self):
        """model.py:464-478, built on first access (it copies every cell's pixel lists)."""
        if getattr(self, "_annotations_all", None) is None:
            out = []
            for i in range(len(self.annotations)):
                pos = self.preprocessor.cell_pos_dict[i]
                rows = []
                for j, key in enumerate(pos.keys()):
                    cell_type_int = np.where(self.cell_types == self.annotations[i][j])[0][0]
                    r, c = pos[key]
                    rows.append({"Cell ID": key, "Cell type": cell_type_int, "Confidence": self.confidence[i][j], "Row": r, "Column": c})
                out.append(rows)
            self._annotations_all = out
        return self._annotations_all

    # ---- extra cell types (model.py:642-675) ---------------------------------------------------------------------------------
    def _find_extra_cell_types(self, root_cell_type="Others", min_samples=10):
        """The cells the vote left as "Others", pooled over every image of the batch with their intensity rows, are embedded with UMAP
        (5 components, GPU: manifold.umap_embed) and clustered with HDBSCAN(min_cluster_size=min_samples) -- manifold.hdbscan (core
        distances and spanning tree on the GPU), or sklearn's host call with RIBCA_HDBSCAN=sklearn; cluster c becomes "Additional type c",
        noise stays "Others", and every pooled cell gets confidence -1.  With 10 or fewer such cells they all stay "Others".  Cell-sharded
        multi-rank runs: rank 0 clusters and broadcasts the label vector (one collective); every rank validates the HDBSCAN parameters
        first, so that none raises while another waits."""
        import time
        pooled = [(i, j) for i in range(len(self.annotations)) for j, name in enumerate(self.annotations[i]) if name == root_cell_type]
        if len(pooled) == 0:
            return
        if len(pooled) <= 10:
            self._apply_extra_labels(pooled, None)
            return
        from . import manifold
        backend = manifold.hdbscan_backend()
        # what fit() would raise, on every rank before the collective
        if backend == "sklearn":
            from sklearn.cluster import HDBSCAN
            HDBSCAN(min_cluster_size=min_samples)._validate_params()
        else:
            manifold.validate_hdbscan_params(min_samples)
        cluster = np.zeros(len(pooled), dtype=np.int64)
        t_embed = t_cluster = 0.0
        split = {"core": 0.0, "mst": 0.0, "tree": 0.0}
        if self.rank == 0:
            x = np.stack([self.preprocessor.intensity_full[i][j] for i, j in pooled])
            t0 = time.perf_counter()
            emb = manifold.umap_embed(x, n_components=5)
            t_embed = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            if backend == "sklearn":
                cluster = HDBSCAN(min_cluster_size=min_samples).fit(emb).labels_.astype(np.int64)
            else:
                cluster = manifold.hdbscan(emb, min_samples, timings=split)
            t_cluster = (time.perf_counter() - t0) * 1e3
        if self.world_size > 1:
            cluster = dist.broadcast_from_rank0(torch.from_numpy(cluster)).numpy()
        self._apply_extra_labels(pooled, cluster)
        n_clusters = int(cluster.max()) + 1 if len(cluster) else 0
        n_noise = int((cluster < 0).sum())
        self.extra_stats = {"pooled": len(pooled), "clusters": n_clusters, "noise": n_noise, "embed_ms": t_embed, "cluster_ms": t_cluster,
                            "backend": backend, "core_ms": split["core"], "mst_ms": split["mst"], "tree_ms": split["tree"]}
        self.logger.log("Extra cell types: {} pooled 'Others' cells, {} clusters found, {} cells left as noise; embed {:.1f} ms, cluster "
                        "{:.1f} ms ({}: core {:.1f}, mst {:.1f}, tree {:.1f}).".format(len(pooled), n_clusters, n_noise, t_embed, t_cluster,
                                                                                      backend, split["core"], split["mst"], split["tree"]))

    def _apply_extra_labels(self, pooled, cluster: Optional[np.ndarray]) -> None:
        """pooled[m] = (image, cell position) gets "Additional type {cluster[m]}" (label id len(GLOBAL_NAMES) + cluster[m]) or "Others"
        for noise / cluster None, and confidence -1 (the int of model.py, -1.0 in the float32 table behind export_annotations)."""
        base = len(ops.GLOBAL_NAMES)
        if cluster is not None and len(cluster) and cluster.max() >= 0:
            self.extra_names = [f"Additional type {c}" for c in range(int(cluster.max()) + 1)]
        else:
            self.extra_names = []
        for m, (i, j) in enumerate(pooled):
            c = -1 if cluster is None else int(cluster[m])
            if c >= 0:
                self.annotations[i][j] = self.extra_names[c]
                self.label_ids[i][j] = base + c
            else:
                self.annotations[i][j] = "Others"
                self.label_ids[i][j] = ops.OTHERS
            self.confidence[i][j] = -1
            if i < len(self._conf_arrays):
                self._conf_arrays[i][j] = np.float32(-1.0)

    def _get_unique_cell_types(self):
        seen = set()
        for per_image in self.annotations:
            seen.update(per_image)
        if self.tile_mode:
            # the reference's list covers every image of the batch (model.py:678-686): the union over the ranks, as an 18-entry presence
            # vector (the only exchange of a tile-per-rank run: control plane, 144 bytes)
            present = torch.tensor([1 if name in seen else 0 for name in ops.GLOBAL_NAMES], dtype=torch.int64)
            present = dist.all_reduce_sum(present)
            seen = {name for name, p in zip(ops.GLOBAL_NAMES, present.tolist()) if p > 0}
        return np.sort(np.array(list(seen)))

    def get_cell_type_names(self):
        txt = ""
        for i in range(len(self.cell_types)):
            txt += f"{i+1}: {self.cell_types[i]}"
            txt += "\n" if i % 3 == 2 else "  "
        return txt

    def export_annotations(self):
        """model.py:768-795: same header, columns, rounding and number formatting."""
        if len(self.annotations) == 0:
            if self.tile_mode and self.preprocessor._n_images > 0:
                return       # a rank that owns no image of the batch has nothing to write
            raise ValueError("No annotations to export")
        if self.rank != 0 and not self.tile_mode:
            return
        for i in range(len(self.annotations)):
            path = os.path.join(self.result_dir, f"{self.batch_id}_annotation_{self._image_number(i)}.csv")
            ids = self.preprocessor.cell_ids[i]
            x, y = self._centroids(i)
            rows, cols = np.round(y, 2), np.round(x, 2)
            regions = getattr(self, "tissue_regions", None)
            conf_txt = self._confidence_text(i)
            keys, labs, rl, cl = ids.tolist(), self.annotations[i], rows.tolist(), cols.tolist()
            with open(path, "w") as f:
                f.write("Cell Index,Cell Type,Confidence,Row,Column,Tissue Region\n")
                if regions is None:
                    f.write("".join([f"{k},{l},{c},{r},{cc},None\n" for k, l, c, r, cc in zip(keys, labs, conf_txt, rl, cl)]))
                else:
                    reg = regions[i]
                    f.write("".join([f"{k},{l},{c},{r},{cc},Region {reg[k]}\n" for k, l, c, r, cc in zip(keys, labs, conf_txt, rl, cl)]))
            self.logger.log(f"Exported annotations for image {i} to {path}")

    def _confidence_text(self, i: int) -> List[str]:
        """the ``Confidence`` column of local image i as export_annotations prints it, one string per cell"""
        conf = self.confidence[i]
        # The reference prints ``round(np.float32, 3)`` through an f-string (the float32 widened to double, e.g.
        # 0.5360000133514404) and the int -1 of a thresholded cell as "-1".  Same text, rounded and widened in one numpy call
        # instead of 100 k Python round() calls when the confidences are still the float32 table predict() produced.
        arr = self._conf_arrays[i] if i < len(getattr(self, "_conf_arrays", [])) and len(self._conf_arrays[i]) == len(conf) else None
        # ``confidence`` is public state (the reference's own _find_extra_cell_types edits it after predict()): the cached table is
        # only used while it still says the same thing
        if arr is not None and not np.array_equal(arr, np.asarray(conf, dtype=np.float32)):
            arr = None
        if arr is not None:
            return ["-1" if v == -1.0 else repr(v) for v in np.round(arr, 3).tolist()]
        return [f"{round(c, 3)}" for c in conf]

    def min_cells_per_image(self) -> int:
        """fewest cells in any image of the batch (what the reference's k-NN calls need to exceed); in tile-per-rank mode the minimum over
        every rank's images, so that all ranks take the same branches of the pipeline (main._pipeline)"""
        n = min((len(ids) for ids in self.preprocessor.cell_ids), default=0)
        return dist.all_reduce_min_int(n) if self.tile_mode else n

    def _image_number(self, i: int) -> int:
        """row of the batch CSV that local position i holds: i itself except in tile-per-rank mode (file names carry the batch-wide number)"""
        ids = self.preprocessor.image_ids
        return ids[i] if i < len(ids) else i

    def _writes_files(self) -> bool:
        """rank 0 writes everything in cell-sharded runs (every rank holds the same tables after the all-gather); in tile-per-rank mode
        every rank writes the files of its own images"""
        return self.rank == 0 or self.tile_mode

    def clear_tmp(self):
        for f in os.listdir(self.temp_dir):
            os.remove(os.path.join(self.temp_dir, f))
        os.rmdir(self.temp_dir)
        self.logger.log("Temporary files cleared")

    # ---- label painting (model.py:806-858) -------------------------------------------------------------------------
    def paint(self, image_idx: int):
        """Device tensors (H, W, 3) uint8 cell-type colours, (H, W, 3) uint8 confidence colours (silver where thresholded),
        (H, W) uint8 cell-type index + 1 -- what ``colorize`` writes as PNGs.  One gather kernel per image instead of the
        reference's per-cell fancy indexing."""
        pre = self.preprocessor
        ids = pre.cell_ids[image_idx]
        tidx = self._cell_type_ints(image_idx)
        palette = np.array(self.colors, dtype=np.uint8)
        conf = np.array([float(c) for c in self.confidence[image_idx]], dtype=np.float32)
        return ops.colorize(pre.masks_dev[image_idx], ids, palette[tidx], colors.confidence_colors(conf), (tidx + 1).astype(np.uint8))

    def colorize(self, from_script=False):
        if len(self.preprocessor.masks) == 0:
            raise ValueError("No masks to colorize")
        if len(self.annotations) == 0:
            raise ValueError("No annotations to colorize")
        from PIL import Image
        for i in range(len(self.preprocessor.masks)):
            type_rgb, conf_rgb, type_idx = (t.cpu().numpy() for t in self.paint(i))
            if not self._writes_files():
                continue
            num = self._image_number(i)
            Image.fromarray(type_rgb).save(os.path.join(self.result_dir, f"{self.batch_id}_colorized_annotation_{num}.png"))
            if not from_script:            # napari working file of the reference GUI (model.py:845-847), only inside its source tree
                gui_dir = "./src/multiplexed_image_annotator/cell_type_annotation/_working_dir_temp"
                if os.path.isdir(gui_dir):
                    Image.fromarray(type_idx).save(os.path.join(gui_dir, "output_img.png"))
            Image.fromarray(conf_rgb).save(os.path.join(self.result_dir, f"{self.batch_id}_confidence_{num}.png"))
            if self.n_regions > 0:             # model.py:823-855: region colours from the same palette, silver last
                pre = self.preprocessor
                ids = pre.cell_ids[i]
                region = np.array([self.tissue_regions[i][int(k)] for k in ids.tolist()], dtype=np.int64)
                palette = np.array(colors.get_colors(self.n_regions + 1), dtype=np.uint8)
                t_rgb, _, t_idx = ops.colorize(pre.masks_dev[i], ids, palette[region], palette[region], (region + 1).astype(np.uint8))
                Image.fromarray(t_rgb.cpu().numpy()).save(os.path.join(self.result_dir, f"{self.batch_id}_tissue_region_{num}.png"))
                if not from_script and os.path.isdir("./src/multiplexed_image_annotator/cell_type_annotation/_working_dir_temp"):
                    Image.fromarray(t_idx.cpu().numpy()).save("./src/multiplexed_image_annotator/cell_type_annotation/_working_dir_temp/output_img_2.png")

    # ---- what the analyses (analyses.py) read of the labels -------------------------------------------------------------
    def _label_names(self) -> List[str]:
        """name of every label id: the 18 global classes, then this run's extra cell types"""
        return list(ops.GLOBAL_NAMES) + list(getattr(self, "extra_names", []))

    def _cell_type_ints(self, image_idx: int) -> np.ndarray:
        types = {str(t): k for k, t in enumerate(self.cell_types)}
        gid_to_type = np.array([types.get(name, 0) for name in self._label_names()], dtype=np.int64)
        return gid_to_type[self.label_ids[image_idx]]

    # ---- per-cell-type plots (model.py:700-741, 861-912) ------------------------------------------------------------------------------
    HEATMAP_CELL = 24       # pixels per table cell of {batch_id}_*heatmap*.png
    HEATMAP_GAP = 1         # white pixels around every cell (the reference's linewidth=.5)
    PIE_CANVAS = 480        # side of the square the disc of {batch_id}_*cell-type_composition*.png is drawn in
    PIE_RADIUS = 200

    def _check_annotated(self, message: str) -> None:
        """the reference's ValueError before predict(); a rank of a tile-per-rank run that owns no image has nothing of its own and goes on"""
        if len(self.annotations) == 0 and not (self.tile_mode and self.preprocessor._n_images > 0):
            raise ValueError(message)

    def _type_sums(self, columns: bool, batch_wide: bool):
        """One ops.group_sums call per image over the groups ``self.cell_types`` (the batch-wide list on every rank): sums (I, T, C) and counts
        (I, T) as host arrays, the image number of each, the rows skipped per image (a name outside cell_types) and the milliseconds.  ``columns``
        False: one zero column (only the counts are wanted).  ``batch_wide`` in tile-per-rank mode: I covers every image of the batch -- one
        all-reduce in which each image's rows come from the rank that owns it and are +0.0 elsewhere, so they arrive as computed."""
        import time
        t0 = time.perf_counter()
        types = {str(t): k for k, t in enumerate(self.cell_types)}
        n_types = len(types)
        full = self.preprocessor.intensity_full
        width = 1
        if columns:
            width = next((a.shape[1] for a in full[:len(self.annotations)] if a is not None), len(self.channel_parser.markers))
        sums = np.zeros((len(self.annotations), n_types, width), dtype=np.float64)
        counts = np.zeros((len(self.annotations), n_types), dtype=np.int64)
        skipped = np.zeros(len(self.annotations), dtype=np.int64)
        dev = _lib.require_gpu()
        for i, names in enumerate(self.annotations):
            if len(names) == 0:
                continue
            ids = np.fromiter((types.get(name, -1) for name in names), dtype=np.int32, count=len(names))
            x = np.ascontiguousarray(full[i], dtype=np.float64) if columns else np.zeros((len(names), 1), dtype=np.float64)
            if x.shape != (len(names), width):
                raise ValueError(f"image {i}: {x.shape[0]} intensity rows of {x.shape[1]} channels for {len(names)} annotations of {width} channels")
            s, c, k = ops.group_sums(torch.from_numpy(x).to(dev), torch.from_numpy(ids).to(dev), n_types)
            sums[i], counts[i], skipped[i] = s.cpu().numpy(), c.cpu().numpy(), k
        numbers = [self._image_number(i) for i in range(len(self.annotations))]
        if batch_wide and self.tile_mode:
            n_batch = self.preprocessor._n_images
            buf = np.zeros((n_batch, n_types * (width + 1) + 1), dtype=np.float64)      # counts and skipped rows are exact in fp64 (< 2^53)
            for i, num in enumerate(numbers):
                buf[num, :n_types * width] = sums[i].reshape(-1)
                buf[num, n_types * width:-1] = counts[i]
                buf[num, -1] = skipped[i]
            buf = dist.all_reduce_sum(torch.from_numpy(buf)).numpy()
            sums = buf[:, :n_types * width].reshape(n_batch, n_types, width)
            counts = buf[:, n_types * width:-1].astype(np.int64)
            skipped = buf[:, -1].astype(np.int64)
            numbers = list(range(n_batch))
        return sums, counts, numbers, skipped, (time.perf_counter() - t0) * 1e3

    def generate_heatmap(self, integrate=False):
        """model.py:700-741: the mean intensity of every image channel (columns, labelled ``channel_parser.markers``) over the cells of every
        cell type present (rows: np.unique of the annotation names, of the batch with ``integrate`` or per image), as
        ``{batch_id}_Integrated_heatmap.png`` / ``{batch_id}_heatmap_{i}.png`` and, beside each, the table as ``.csv`` (cell_type, one
        column per marker, cells; 17 significant digits).  The means are ordered fp64 sums of ``preprocessor.intensity_full`` (ops.group_sums,
        one call per image; the images' sums added in image order) divided by the counts; ops.heatmap_raster paints the table, the labels and
        the colour bar are drawn on the host (plots.heatmap_figure).  Colours: colors.diverging_table (RdBu_r, not seaborn's vlag); any
        number of cell types draws (the reference's figsize is 0 inches high for fewer than four).  Returns None and records
        ``heatmap_stats``, one record per figure written by this rank.  Cell-sharded multi-rank runs: rank 0 computes and writes.
        Tile-per-rank: every rank writes its own images' figures; the integrated one is rank 0's, from one all-reduce every rank enters."""
        self._check_annotated("No annotations to generate heatmap")
        self.heatmap_stats = []
        if not self._computes_here():
            return None
        sums, counts, numbers, skipped, sums_ms = self._type_sums(columns=True, batch_wide=bool(integrate))
        if integrate:
            if self.rank == 0:
                self._write_heatmap(f"{self.batch_id}_Integrated_heatmap", self._add_in_order(sums), counts.sum(axis=0), int(skipped.sum()), sums_ms)
        else:
            for i, num in enumerate(numbers):
                self._write_heatmap(f"{self.batch_id}_heatmap_{num}", sums[i], counts[i], int(skipped[i]), sums_ms)
        return None

    def _write_heatmap(self, stem: str, sums: np.ndarray, counts: np.ndarray, skipped: int, sums_ms: float) -> None:
        import time
        from . import plots
        present = np.nonzero(counts > 0)[0]
        if len(present) == 0:
            self.logger.log(f"Heat map {stem}: no cells, nothing drawn")
            return
        present = present[np.argsort(np.array([str(self.cell_types[k]) for k in present]), kind="stable")]      # np.unique's order
        names = [str(self.cell_types[k]) for k in present]
        sums, counts = np.ascontiguousarray(sums[present]), np.ascontiguousarray(counts[present])
        width = sums.shape[1]
        markers = self._marker_names(width)
        dev = _lib.require_gpu()
        lut = colors.diverging_table()
        t0 = time.perf_counter()
        rect, vmin, vmax = ops.heatmap_raster(torch.from_numpy(sums).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(lut).to(dev),
                                              self.HEATMAP_CELL, self.HEATMAP_GAP)
        rect = rect.cpu().numpy()
        raster_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        fig, lay = plots.heatmap_figure(rect, lut, vmin, vmax, names, markers, self.HEATMAP_CELL)
        fig.save(os.path.join(self.result_dir, stem + ".png"))
        self._write_text(stem + ".csv", plots.heatmap_csv(names, markers, sums / counts[:, None].astype(np.float64), counts))
        draw_ms = (time.perf_counter() - t0) * 1e3
        stats = {"file": stem + ".png", "rows": len(names), "columns": width, "cells": int(counts.sum()), "skipped": int(skipped), "vmin": vmin,
                 "vmax": vmax, "rect": (lay["top"], lay["left"]), "sums_ms": sums_ms, "raster_ms": raster_ms, "draw_ms": draw_ms}
        self.heatmap_stats.append(stats)
        self.logger.log("Heat map {}: {} cell types x {} markers over {} cells ({} skipped), colour scale {:.4g} .. {:.4g}; sums {:.1f}, raster {:.1f}, "
                        "drawing {:.1f} ms.".format(stats["file"], len(names), width, stats["cells"], skipped, vmin, vmax, sums_ms, raster_ms, draw_ms))

    def cell_type_composition(self, reduction=True, integrate=False):
        """model.py:861-912: the share of every ``self.cell_types`` entry as a pie (wedges in that order and in ``self.colors``, from
        3 o'clock counter-clockwise as matplotlib's ax.pie; ops.pie_raster) with the reference's legend beside it
        (plots.legend_texts: with ``reduction=False`` it prints the raw count x 100, as the reference does), as
        ``{batch_id}_integrated_cell-type_composition.png`` / ``{batch_id}_cell-type_composition_{i}.png`` and a ``.csv`` (cell_type,
        cells, fraction) beside each.  The counts are those of ops.group_sums.  Returns None and records ``composition_stats``, one record
        per figure written by this rank; multi-rank runs as generate_heatmap."""
        self._check_annotated("No annotations to analyze")
        self.composition_stats = []
        if not self._computes_here():
            return None
        _, counts, numbers, skipped, sums_ms = self._type_sums(columns=False, batch_wide=bool(integrate))
        if integrate:
            if self.rank == 0:
                self._write_composition(f"{self.batch_id}_integrated_cell-type_composition", counts.sum(axis=0), reduction, int(skipped.sum()), sums_ms)
        else:
            for i, num in enumerate(numbers):
                self._write_composition(f"{self.batch_id}_cell-type_composition_{num}", counts[i], reduction, int(skipped[i]), sums_ms)
        return None

    def _write_composition(self, stem: str, counts: np.ndarray, reduction: bool, skipped: int, sums_ms: float) -> None:
        import time
        from . import plots
        names = [str(c) for c in self.cell_types]
        palette = np.array(self.colors, dtype=np.uint8).reshape(-1, 3)
        kept, rays = plots.pie_wedges(counts)
        t0 = time.perf_counter()
        if len(kept):
            dev = _lib.require_gpu()
            disc = ops.pie_raster(torch.from_numpy(rays).to(dev), torch.from_numpy(np.ascontiguousarray(palette[kept])).to(dev), self.PIE_CANVAS,
                                  self.PIE_RADIUS).cpu().numpy()
        else:      # no cell: no disc
            disc = np.full((self.PIE_CANVAS, self.PIE_CANVAS, 3), 255, dtype=np.uint8)
        raster_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        fig, lay = plots.pie_figure(disc, plots.legend_texts(names, counts, reduction), palette)
        fig.save(os.path.join(self.result_dir, stem + ".png"))
        self._write_text(stem + ".csv", plots.composition_csv(names, counts))
        draw_ms = (time.perf_counter() - t0) * 1e3
        stats = {"file": stem + ".png", "rows": len(names), "columns": 1, "wedges": int(len(kept)), "cells": int(counts.sum()), "skipped": int(skipped),
                 "vmin": None, "vmax": None, "rect": (lay["top"], lay["left"]), "sums_ms": sums_ms, "raster_ms": raster_ms, "draw_ms": draw_ms}
        self.composition_stats.append(stats)
        self.logger.log("Composition {}: {} cells in {} of {} cell types ({} skipped); counts {:.1f}, raster {:.1f}, drawing {:.1f} ms.".format(
            stats["file"], stats["cells"], len(kept), len(names), skipped, sums_ms, raster_ms, draw_ms))

    UMAP_CANVAS = (1200, 1600)      # rows, columns of {batch_id}_umap.png
    UMAP_RADIUS = 2

    def umap_visualization(self, *_a, **_k):
        """model.py:746-765: a 2-D UMAP of the intensity rows of every cell of the batch, coloured by cell type with the palette ``paint``
        uses, as ``{batch_id}_umap.png`` (1200 x 1600, filled discs in data order on white, no axes or legend: manifold.umap_embed with two
        components, then ops.scatter_raster) and ``{batch_id}_umap.csv`` (Image, Cell Index, Cell Type, UMAP 1, UMAP 2: the same points, for
        a plot with axes).  The spectral start runs on the GPU unless RIBCA_SPECTRAL=scipy; the embedding is seeded (RIBCA_UMAP_SEED), so
        two runs write the same bytes -- the reference's is not.  Returns the (n_cells, 2) float32 embedding and records ``umap_stats``.
        Cell-sharded multi-rank runs: rank 0 embeds, broadcasts the embedding (one collective) and writes.  Skipped with a log line, returning
        None: fewer than 4 cells, and tile-per-rank mode (no rank holds the other ranks' intensity rows)."""
        import time
        if len(self.annotations) == 0:
            raise ValueError("No annotations to visualize")
        if self.tile_mode:
            self.logger.log("umap_visualization: skipped (tile-per-rank mode: the intensity rows stay on the rank that owns the image)")
            return None
        from . import manifold
        backend = manifold.spectral_backend("gpu")      # validated on every rank before the collective
        rows = [(i, j, name) for i in range(len(self.annotations)) for j, name in enumerate(self.annotations[i])]
        n = len(rows)
        if n < 4:
            self.logger.log(f"umap_visualization: skipped ({n} cells: too few to embed)")
            return None
        seed = manifold.default_seed()
        emb = np.zeros((n, 2), dtype=np.float32)
        t: Dict = {}
        if self.rank == 0:
            x = np.concatenate([a for a in self.preprocessor.intensity_full[:len(self.annotations)] if a is not None], axis=0)
            assert len(x) == n
            emb = manifold.umap_embed(x, n_components=2, seed=seed, timings=t, spectral=backend)
        if self.world_size > 1:
            emb = dist.broadcast_from_rank0(torch.from_numpy(emb)).numpy()
        raster_ms, skipped = 0.0, 0
        if self._writes_files():
            from PIL import Image
            t0 = time.perf_counter()
            types = {str(c): k for k, c in enumerate(self.cell_types)}
            palette = np.array(self.colors, dtype=np.uint8)
            rgb = palette[np.array([types[name] for _, _, name in rows], dtype=np.int64)]
            h, w = self.UMAP_CANVAS
            dev = torch.device("cuda", torch.cuda.current_device())
            img, skipped = ops.scatter_raster(torch.from_numpy(emb).to(dev), torch.from_numpy(np.ascontiguousarray(rgb)).to(dev), h, w,
                                              ops.scatter_affine(emb, h, w), self.UMAP_RADIUS)
            Image.fromarray(img.cpu().numpy()).save(os.path.join(self.result_dir, f"{self.batch_id}_umap.png"))
            raster_ms = (time.perf_counter() - t0) * 1e3
            with open(os.path.join(self.result_dir, f"{self.batch_id}_umap.csv"), "w") as f:
                f.write("Image,Cell Index,Cell Type,UMAP 1,UMAP 2\n")
                for (i, j, name), (u, v) in zip(rows, emb.tolist()):
                    f.write(f"{self._image_number(i)},{int(self.preprocessor.cell_ids[i][j])},{name},{u:.9g},{v:.9g}\n")
        self.umap_stats = {"n": n, "seed": seed, "spectral_backend": t.get("spectral_backend", backend),
                           "spectral_iterations": t.get("spectral_iterations"), "spectral_spmm": t.get("spectral_spmm"),
                           "spectral_gpu_components": t.get("spectral_gpu_components", 0), "raster_ms": raster_ms,
                           "skipped_points": skipped, **{k + "_ms": t.get(k, 0.0) for k in ("knn", "fuzzy", "graph", "init", "sgd")}}
        s = self.umap_stats
        self.logger.log("UMAP plot: {} cells; knn {:.1f}, fuzzy {:.1f}, graph {:.1f}, init {:.1f} ({}, {} filter passes), sgd {:.1f}, raster {:.1f} ms; "
                        "seed {}.".format(n, s["knn_ms"], s["fuzzy_ms"], s["graph_ms"], s["init_ms"], s["spectral_backend"],
                                          s["spectral_iterations"], s["sgd_ms"], raster_ms, seed))
        return emb
