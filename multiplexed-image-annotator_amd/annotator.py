"""``Annotator``: drop-in for the reference orchestrator on its hot path (cell_type_annotation/model.py:90-919):
same constructor, ``preprocess()``, ``predict(batch_size)``, ``export_annotations()``, ``clear_tmp()``,
``get_cell_type_names()`` and the attributes downstream code reads (``annotations``, ``confidence``, ``annotations_all``,
``cell_types``, ``channel_parser``, ``preprocessor``, ``*_pred``).  Compute runs in the HIP library, the plots included:
``generate_heatmap()`` and ``cell_type_composition()`` reduce and rasterise on the GPU and write a CSV beside every PNG, and
``umap_visualization()`` embeds and draws there, so the reference's own call sequence (main.py:19-28) runs in full against this class.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, colors, dist, ops
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


class Annotator(object):
    def __init__(self, marker_list_path, image_path, device, main_dir='./', batch_id='', strict=True, infer=True, min_cells=-1,
                 normalize=True, blur=False, amax=1, confidence=0.25, cell_size=30, cell_type_confidence=None, n_jobs=0):
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
                                           cell_size, self.logger, n_jobs=n_jobs)
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
            return
        if ws > 1 and os.environ.get("RIBCA_NORM_SHARD") == "1":
            self.preprocessor.norm_shard = (rank, ws)
        self.preprocessor.transform(shard_fn=(lambda n: dist.shard_bounds(n, rank, ws)) if ws > 1 else None,
                                    gather_fn=(lambda t, n: dist.all_gather_rows(t, n)) if ws > 1 else None)
        self._n_images = self.preprocessor._n_images

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
            tab = self.preprocessor.cell_tables[i]
            conf = self.confidence[i]
            rows = np.round(tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64), 2)
            cols = np.round(tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64), 2)
            regions = getattr(self, "tissue_regions", None)
            # The reference prints ``round(np.float32, 3)`` through an f-string (the float32 widened to double, e.g.
            # 0.5360000133514404) and the int -1 of a thresholded cell as "-1".  Same text, rounded and widened in one numpy call
            # instead of 100 k Python round() calls when the confidences are still the float32 table predict() produced.
            arr = self._conf_arrays[i] if i < len(getattr(self, "_conf_arrays", [])) and len(self._conf_arrays[i]) == len(conf) else None
            # ``confidence`` is public state (the reference's own _find_extra_cell_types edits it after predict()): the cached table is
            # only used while it still says the same thing
            if arr is not None and not np.array_equal(arr, np.asarray(conf, dtype=np.float32)):
                arr = None
            if arr is not None:
                conf_txt = ["-1" if v == -1.0 else repr(v) for v in np.round(arr, 3).tolist()]
            else:
                conf_txt = [f"{round(c, 3)}" for c in conf]
            keys, labs, rl, cl = ids.tolist(), self.annotations[i], rows.tolist(), cols.tolist()
            with open(path, "w") as f:
                f.write("Cell Index,Cell Type,Confidence,Row,Column,Tissue Region\n")
                if regions is None:
                    f.write("".join([f"{k},{l},{c},{r},{cc},None\n" for k, l, c, r, cc in zip(keys, labs, conf_txt, rl, cl)]))
                else:
                    reg = regions[i]
                    f.write("".join([f"{k},{l},{c},{r},{cc},Region {reg[k]}\n" for k, l, c, r, cc in zip(keys, labs, conf_txt, rl, cl)]))
            self.logger.log(f"Exported annotations for image {i} to {path}")

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

    # ---- neighbourhood analysis (model.py:798-800 -> spatial_methods.py:13-130) -----------------------------------------
    def _label_names(self) -> List[str]:
        """name of every label id: the 18 global classes, then this run's extra cell types"""
        return list(ops.GLOBAL_NAMES) + list(getattr(self, "extra_names", []))

    def _cell_type_ints(self, image_idx: int) -> np.ndarray:
        types = {str(t): k for k, t in enumerate(self.cell_types)}
        gid_to_type = np.array([types.get(name, 0) for name in self._label_names()], dtype=np.int64)
        return gid_to_type[self.label_ids[image_idx]]

    def neighborhood_matrix(self, image_indices, n_neighbors=25) -> np.ndarray:
        """Counts of (cell type, neighbour cell type) over every cell's n_neighbors - 1 nearest other cells, summed over the images."""
        t = len(self.cell_types)
        acc = None
        for i in image_indices:
            tab = self.preprocessor.cell_tables[i]
            x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)      # np.mean(Column), np.mean(Row) of the reference
            y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
            acc = ops.knn_cooccurrence(x, y, self._cell_type_ints(i), t, n_neighbors, out=acc)
        if acc is None:      # a rank that owns no image of the batch (tile-per-rank mode forced on a batch smaller than the world)
            return np.zeros((t, t), dtype=np.float64)
        return acc.cpu().numpy().astype(np.float64)

    def neighborhood_analysis(self, n_neighbors=25, integrate=True, normalize=True):
        """Writes the same CSVs as the reference (``{batch_id}_integrated_neighborhood.csv`` or one ``{batch_id}_neighborhood_{i}.csv``
        per image) and, beside each, the reference's heat map of the matrix as ``.png`` (spatial_methods.py:51-55, 110-114: seaborn's default scaling,
        the matrix min .. max; ops.table_raster, colors.diverging_table, plots.heatmap_figure).  Records ``neighborhood_stats``, one record
        per figure written by this rank."""
        if len(self.annotations) == 0:
            raise ValueError("No annotations")
        self.neighborhood_stats = []
        groups = [list(range(self._n_images))] if integrate else [[i] for i in range(self._n_images)]
        for g, idx in enumerate(groups):
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
        counts and the list; ``perm_ms``: the permutations; ``draw_ms``: everything after them on the host -- z-scores, both CSVs, raster and PNG).  Cell-sharded
        multi-rank runs: rank 0 computes and writes.  Tile-per-rank: every rank does its own images; the integrated tensor takes one all-reduce
        every rank enters (counts are exact in fp64)."""
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
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
            return None
        seed = enrichment.default_seed()
        n_local = len(self.annotations)
        groups = [list(range(n_local))] if integrate else [[i] for i in range(n_local)]
        dev = _lib.require_gpu()
        for g, members in enumerate(groups):
            obs = torch.zeros((t, t), dtype=torch.int64, device=dev)
            perm = torch.zeros((p, t, t), dtype=torch.int64, device=dev)
            cells, knn_ms, perm_ms = 0, 0.0, 0.0
            for i in members:
                tab = self.preprocessor.cell_tables[i]
                x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
                y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
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
            both = torch.cat([obs.reshape(-1), perm.reshape(-1)]).cpu()
            if integrate and self.tile_mode:
                buf = dist.all_reduce_sum(torch.cat([both.to(torch.float64), torch.tensor([float(cells)], dtype=torch.float64)]))
                both, cells = buf[:-1].to(torch.int64), int(buf[-1].item())
            if integrate and self.rank != 0:
                continue
            both = both.numpy()
            observed, null = both[:t * t].reshape(t, t), both[t * t:].reshape(p, t, t)
            t0 = time.perf_counter()
            stats = enrichment.z_scores(observed, null)
            names = [str(c) for c in self.cell_types]
            stem = f"{self.batch_id}_integrated_neighborhood_enrichment" if integrate else f"{self.batch_id}_neighborhood_enrichment"
            tail = "" if integrate else f"_{self._image_number(members[0])}"
            with open(os.path.join(self.result_dir, stem + tail + ".csv"), "w") as f:
                f.write(enrichment.matrix_csv(names, stats["z"]))
            with open(os.path.join(self.result_dir, stem + "_table" + tail + ".csv"), "w") as f:
                f.write(enrichment.table_csv(names, observed, stats))
            lim = enrichment.colour_limit(stats["z"])
            fig = self._write_table_figure(stem + tail, stats["z"], -lim, lim)
            draw_ms = (time.perf_counter() - t0) * 1e3
            rec = {"file": fig["file"], "n": cells, "T": t, "P": p, "seed": seed, "neighbors": int(n_neighbors), "limit": lim, "rect": fig["rect"],
                   "knn_ms": knn_ms, "perm_ms": perm_ms, "draw_ms": draw_ms}
            self.enrichment_stats.append(rec)
            self.logger.log("Neighbourhood enrichment {}: {} cells, {} cell types, {} permutations (seed {}), |z| up to {:.4g}; kNN {:.1f}, "
                            "permutations {:.1f}, z-scores and drawing {:.1f} ms.".format(rec["file"], cells, t, p, seed, lim, knn_ms, perm_ms, draw_ms))
        return None

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
        written by this rank.  Cell-sharded multi-rank runs: rank 0 computes and writes.  Tile-per-rank: every rank does its own images; the
        integrated tensor takes one all-reduce every rank enters (counts are exact in fp64 below 2^53; a group that could pass that is refused
        before any collective)."""
        import time
        from . import cooccurrence, enrichment
        self._check_annotated("No annotations")
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        r = cooccurrence.check_radii(cooccurrence.default_radii(self.cell_size) if radii is None else radii, ops.RADIAL_MAX_BANDS)
        nb = len(r)
        if t > 254:
            raise ValueError(f"cooccurrence_by_distance handles at most 254 cell types, got {t}")
        wanted = None
        if anchors is not None:
            wanted = []
            for a in anchors:
                k = names.index(a) if isinstance(a, str) and a in names else a
                if isinstance(k, (str, bool)) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < t:
                    raise ValueError(f"anchor {a!r} is not one of the cell types {names}")
                wanted.append(int(k))
        self.cooccurrence_stats = []
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
            return None
        n_local = len(self.annotations)
        groups = [list(range(n_local))] if integrate else [[i] for i in range(n_local)]
        cap = ops.RADIAL_MAX_CELLS
        sizes = [len(self.preprocessor.cell_ids[i]) for i in range(n_local)]
        if any(n > cap for n in sizes):
            raise ValueError(f"cooccurrence_by_distance takes at most {cap} cells per image, got {max(sizes)}")
        # the same bound on every rank of a tile-per-rank run (each knows the number of images of the batch, not their sizes)
        worst = self.preprocessor._n_images * cap * (cap - 1) if integrate and self.tile_mode else max([sum(sizes[i] * (sizes[i] - 1) for i in g) for g in groups] + [0])
        if worst >= 2 ** 53:
            raise ValueError(f"cooccurrence_by_distance: a group of up to {worst} pairs does not count exactly in fp64 (2^53)")
        dev = _lib.require_gpu()
        for g, members in enumerate(groups):
            acc = torch.zeros((nb, t, t), dtype=torch.int64, device=dev)
            present = np.zeros(t, dtype=np.int64)
            cells, count_ms = 0, 0.0
            for i in members:
                tab = self.preprocessor.cell_tables[i]
                if len(tab) == 0:      # an image without cells has no pair
                    continue
                x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
                y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
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
                buf = dist.all_reduce_sum(torch.cat([torch.from_numpy(counts.reshape(-1).astype(np.float64)), torch.from_numpy(present.astype(np.float64)),
                                                     torch.tensor([float(cells)], dtype=torch.float64)])).numpy()
                counts, present, cells = buf[:nb * t * t].astype(np.int64).reshape(nb, t, t), buf[nb * t * t:-1].astype(np.int64), int(buf[-1])
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            stem = f"{self.batch_id}_integrated_cooccurrence" if integrate else f"{self.batch_id}_cooccurrence"
            tail = "" if integrate else f"_{self._image_number(members[0])}"
            files = [stem + tail + ".csv"]
            with open(os.path.join(self.result_dir, files[0]), "w") as f:
                f.write(cooccurrence.table_csv(names, r, counts))
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
        return None

    # ---- nearest cell of every type: how far is each cell from the nearest cell of type b (scimap's spatial_distance, spatstat's Gcross) ---------
    NEAREST_NULL_BYTES = 64 << 20      # the permutation counts of one call stay under this on the device; longer nulls go in ranges of permutations

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
        this rank.  Cell-sharded multi-rank runs: rank 0 computes and writes.  Tile-per-rank: every rank does its own images; the integrated
        counts take one all-reduce every rank enters (exact in fp64 below 2^53; a group that could pass that is refused before any
        collective)."""
        import time
        from PIL import Image
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
        wanted = None
        if targets is not None:
            wanted = []
            for a in targets:
                k = names.index(a) if isinstance(a, str) and a in names else a
                if isinstance(k, (str, bool)) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < t:
                    raise ValueError(f"target {a!r} is not one of the cell types {names}")
                wanted.append(int(k))
        n_local = len(self.annotations)
        cap = ops.NEAREST_MAX_CELLS
        sizes = [len(self.preprocessor.cell_ids[i]) for i in range(n_local)]
        if any(n > cap for n in sizes):
            raise ValueError(f"nearest_type_distances takes at most {cap} cells per image, got {max(sizes)}")
        groups = [list(range(n_local))] if integrate else [[i] for i in range(n_local)]
        # no count passes the cells of its group; the same bound on every rank of a tile-per-rank run (each knows the number of images, not their sizes)
        worst = self.preprocessor._n_images * cap if integrate and self.tile_mode else max([sum(sizes[i] for i in g) for g in groups] + [0])
        if worst >= 2 ** 53:
            raise ValueError(f"nearest_type_distances: a group of up to {worst} cells does not count exactly in fp64 (2^53)")
        self.nearest_stats = []
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
            return None
        seed = nearest.default_seed()
        r2 = r * r
        r_max = float(r[-1])
        lut = colors.viridis_table()
        per_call = max(1, self.NEAREST_NULL_BYTES // (8 * nb * t * t))
        for g, members in enumerate(groups):
            observed = np.zeros((nb, t, t), dtype=np.int64)
            null = np.zeros((p, nb, t, t), dtype=np.int64)
            present = np.zeros(t, dtype=np.int64)
            cells, distance_ms, perm_ms, draw_ms = 0, 0.0, 0.0, 0.0
            image_files = []
            for i in members:
                tab = self.preprocessor.cell_tables[i]
                ids = self.preprocessor.cell_ids[i]
                n = len(tab)
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                near2, arg = np.full((0, t), np.inf), np.full((0, t), -1, dtype=np.int32)
                if n:
                    x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
                    y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    near2_d, arg_d = ops.nearest_by_type(x, y, types, t)
                    near2, arg = near2_d.cpu().numpy(), arg_d.cpu().numpy()
                    t1 = time.perf_counter()
                    for q0 in range(0, p, per_call):      # the entry point is pure in the permutation index: the ranges are invisible
                        q = min(per_call, p - q0)
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
                with open(os.path.join(self.result_dir, image_files[-1]), "w") as f:
                    f.write(nearest.cells_csv(ids, types, names, near2, arg))
                for b in (wanted if wanted is not None else [k for k in range(t) if here[k] > 0]):
                    idx = nearest.distance_colour_index(near2[:, b], r_max)
                    rgb = lut[idx] if here[b] > 0 else np.tile(np.array(colors.SILVER, dtype=np.uint8), (n, 1))
                    painted = ops.colorize(self.preprocessor.masks_dev[i], ids, rgb, rgb, idx)[0].cpu().numpy()
                    image_files.append(f"{self.batch_id}_nearest_{cooccurrence.slug(names[b])}_{number}.png")
                    Image.fromarray(painted).save(os.path.join(self.result_dir, image_files[-1]))
                draw_ms += (time.perf_counter() - t0) * 1e3
            if integrate and self.tile_mode:
                buf = dist.all_reduce_sum(torch.cat([torch.from_numpy(observed.reshape(-1).astype(np.float64)),
                                                     torch.from_numpy(null.reshape(-1).astype(np.float64)),
                                                     torch.from_numpy(present.astype(np.float64)),
                                                     torch.tensor([float(cells)], dtype=torch.float64)])).numpy()
                no, nn = nb * t * t, p * nb * t * t
                observed, null = buf[:no].astype(np.int64).reshape(nb, t, t), buf[no:no + nn].astype(np.int64).reshape(p, nb, t, t)
                present, cells = buf[no + nn:-1].astype(np.int64), int(buf[-1])
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            stats = nearest.statistics(observed, null if p > 0 else None, present)
            stem = f"{self.batch_id}_integrated_nearest_table" if integrate else f"{self.batch_id}_nearest_table"
            tail = "" if integrate else f"_{self._image_number(members[0])}"
            files = [stem + tail + ".csv"]
            with open(os.path.join(self.result_dir, files[0]), "w") as f:
                f.write(nearest.table_csv(names, r, observed, present, stats))
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
        return None

    # ---- contact graph: which cells actually touch, read off the segmentation mask (histoCAT's neighbourhood analysis, steinbock's expansion graph) --
    CONTACT_NULL_BYTES = 64 << 20      # the permutation counts of one call stay under this on the device; longer nulls go in ranges of permutations

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
        written by this rank (``max_degree`` and ``slots`` over this rank's images).  Cell-sharded multi-rank runs: rank 0 computes and writes.
        Tile-per-rank: every rank does its own images; the integrated counts take one all-reduce every rank enters (exact in fp64 below 2^53; a
        group that could pass that is refused before any collective)."""
        import time
        from PIL import Image
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
        groups = [list(range(n_local))] if integrate else [[i] for i in range(n_local)]
        # no sum of pixel pairs passes pixels x offsets of its group; the same bound on every rank of a tile-per-rank run (each knows the number
        # of images of the batch, not their sizes: a mask holds fewer than 2^31 pixels)
        reach = contact.DISK_OFFSETS[d - 1]
        pixels = [int(self.preprocessor.masks_dev[i].numel()) for i in range(n_local)]
        worst = self.preprocessor._n_images * (2 ** 31) * reach if integrate and self.tile_mode else max([sum(pixels[i] for i in g) * reach for g in groups] + [0])
        if worst >= 2 ** 53:
            raise ValueError(f"contact_analysis: a group of up to {worst} pixel pairs does not count exactly in fp64 (2^53)")
        self.contact_stats = []
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
            return None
        seed = contact.default_seed()
        lut = colors.viridis_table()
        per_call = max(1, self.CONTACT_NULL_BYTES // (8 * t * t))
        dev = _lib.require_gpu()
        for g, members in enumerate(groups):
            edges = np.zeros((t, t), dtype=np.int64)
            weight = np.zeros((t, t), dtype=np.int64)
            null = np.zeros((p, t, t), dtype=np.int64)
            cells, n_edges, max_degree, slots, graph_ms, perm_ms, draw_ms = 0, 0, 0, 0, 0.0, 0.0, 0.0
            image_files = []
            for i in members:
                ids = self.preprocessor.cell_ids[i]
                mask = self.preprocessor.masks_dev[i]
                n = len(ids)
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                graph = ops.contact_graph(mask, ids, d)
                t1 = time.perf_counter()
                src, dst, pairs, degree = graph["src"], graph["dst"], graph["pairs"], graph["degree"]
                if p > 0 and len(src) > 0:
                    src_d, dst_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
                    for q0 in range(0, p, per_call):      # the entry point is pure in the permutation index: the ranges are invisible
                        q = min(per_call, p - q0)
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
                with open(os.path.join(self.result_dir, image_files[-3]), "w") as f:
                    f.write(contact.edges_csv(ids, types, names, src, dst, pairs))
                with open(os.path.join(self.result_dir, image_files[-2]), "w") as f:
                    f.write(contact.cells_csv(ids, types, names, src, dst, pairs, degree))
                idx = contact.degree_colour_index(degree)
                rgb = lut[idx].reshape(n, 3)
                painted = ops.colorize(mask, ids, rgb, rgb, idx)[0].cpu().numpy()
                Image.fromarray(painted).save(os.path.join(self.result_dir, image_files[-1]))
                draw_ms += (time.perf_counter() - t0) * 1e3
            if integrate and self.tile_mode:
                buf = dist.all_reduce_sum(torch.cat([torch.from_numpy(edges.reshape(-1).astype(np.float64)),
                                                     torch.from_numpy(weight.reshape(-1).astype(np.float64)),
                                                     torch.from_numpy(null.reshape(-1).astype(np.float64)),
                                                     torch.tensor([float(cells), float(n_edges)], dtype=torch.float64)])).numpy()
                tt = t * t
                edges, weight = buf[:tt].astype(np.int64).reshape(t, t), buf[tt:2 * tt].astype(np.int64).reshape(t, t)
                null, cells, n_edges = buf[2 * tt:-2].astype(np.int64).reshape(p, t, t), int(buf[-2]), int(buf[-1])
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            stats = None
            if p > 0:
                stats = enrichment.z_scores(edges, null) if n_edges > 0 else contact.nan_stats(t)
            stem = f"{self.batch_id}_integrated_contact" if integrate else f"{self.batch_id}_contact"
            tail = "" if integrate else f"_{self._image_number(members[0])}"
            files = [stem + "_table" + tail + ".csv"]
            with open(os.path.join(self.result_dir, files[0]), "w") as f:
                f.write(contact.table_csv(names, edges, weight, stats))
            share = contact.row_normalised(weight)
            top = float(share.max()) if share.size else 0.0
            fig = self._write_table_figure(stem + "_pairs" + tail, share, 0.0, top if top > 0.0 else 1.0)
            figures = [{"file": fig["file"], "what": "pairs", "limit": top, "rect": fig["rect"]}]
            files.append(fig["file"])
            if p > 0:
                files.append(stem + tail + ".csv")
                with open(os.path.join(self.result_dir, files[-1]), "w") as f:
                    f.write(enrichment.matrix_csv(names, stats["z"]))
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
        return None

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
        kernels alone (tools/time_consumers.py --morphology times those).  Cell-sharded multi-rank runs: rank 0 computes and
        writes.  Tile-per-rank: every rank does its own images; for the integrated group one all-reduce of the cell counts and one all-gather of the
        feature rows, which rank 0 orders by (image number, cell id), so its files are a single-rank run's."""
        import time
        from PIL import Image
        from . import morphology
        self._check_annotated("No annotations")
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        self.morphology_stats = []
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
            return None
        n_local = len(self.annotations)
        groups = [list(range(n_local))] if integrate else [[i] for i in range(n_local)]
        lut = colors.viridis_table()
        width = 3 + len(morphology.FEATURES)      # image number, cell id, cell type, the features: a row of the tile-per-rank exchange
        for g, members in enumerate(groups):
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
                with open(os.path.join(self.result_dir, image_files[-3]), "w") as f:
                    f.write(morphology.cells_csv(ids, types, names, feat))
                for name, idx in ((image_files[-2], morphology.diameter_colour_index(feat["equivalent_diameter"], self.cell_size)),
                                  (image_files[-1], morphology.coverage_colour_index(feat["patch_coverage"]))):
                    rgb = lut[idx].reshape(n, 3)
                    painted = ops.colorize(mask, ids, rgb, rgb, idx)[0].cpu().numpy()
                    Image.fromarray(painted).save(os.path.join(self.result_dir, name))
                rows.append(np.concatenate([np.full((n, 1), float(number)), ids.reshape(n, 1).astype(np.float64), types.reshape(n, 1).astype(np.float64),
                                            morphology.feature_matrix(feat)], axis=1))
                draw_ms += (time.perf_counter() - t0) * 1e3
            table = np.concatenate(rows, axis=0)
            if integrate and self.tile_mode:
                counts = np.zeros(self.world_size, dtype=np.float64)
                counts[self.rank] = len(table)
                counts = dist.all_reduce_sum(torch.from_numpy(counts)).numpy().astype(np.int64)
                cap = int(counts.max())
                send = np.zeros((cap, width), dtype=np.float64)
                send[:len(table)] = table
                full = dist.all_gather_rows(torch.from_numpy(send), cap * self.world_size).numpy() if cap else send      # equal shards of cap rows
                table = np.concatenate([full[r * cap:r * cap + int(counts[r])] for r in range(self.world_size)], axis=0)
                table = table[np.lexsort((table[:, 1], table[:, 0]))]      # by (image number, cell id): the order of a single-rank run
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            types = table[:, 2].astype(np.int64)
            feat = morphology.from_matrix(table[:, 3:])
            stem = f"{self.batch_id}_integrated_morphology" if integrate else f"{self.batch_id}_morphology"
            tail = "" if integrate else f"_{self._image_number(members[0])}"
            mid = "" if integrate else "_means"      # {batch_id}_morphology_{image number}.csv is the image's cell table
            files = [stem + "_summary" + tail + ".csv", stem + mid + tail + ".csv"]
            with open(os.path.join(self.result_dir, files[0]), "w") as f:
                f.write(morphology.summary_csv(names, morphology.summary(types, t, feat)))
            z = morphology.standardised_means(types, t, feat)
            with open(os.path.join(self.result_dir, files[1]), "w") as f:
                f.write(morphology.matrix_csv(names, z))
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
        return None

    # ---- cell intensities: the marker columns of the single-cell table, over each cell's own pixels (steinbock's measure intensities) ------------
    def cell_intensities(self, integrate=True, maps=True):
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
        its outputs back -- (tools/time_consumers.py --intensities times the kernel alone).  Multi-rank runs as cell_morphology: cell-sharded,
        rank 0 computes and writes; tile-per-rank, every rank does its own images, and the integrated group takes one all-reduce of the counts and
        one all-gather of the rows, which rank 0 orders by (image number, cell id), so its files are a single-rank run's."""
        import time
        from PIL import Image
        from . import intensities
        self._check_annotated("No annotations")
        t = len(self.cell_types)
        names = [str(c) for c in self.cell_types]
        self.intensity_stats = []
        self.intensity_mask = []
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
            return None
        n_local = len(self.annotations)
        groups = [list(range(n_local))] if integrate else [[i] for i in range(n_local)]
        lut = colors.viridis_table()
        stats = intensities.statistic_names()
        median = stats.index("median")
        full = self.preprocessor.intensity_full
        c_img = int(self.preprocessor.images_dev[0].shape[0]) if n_local else len(self.channel_parser.markers)
        markers = [str(m) for m in self.channel_parser.markers]
        markers = (markers + [f"channel {j}" for j in range(len(markers), c_img)])[:c_img]
        width = 4 + 3 * c_img      # image number, cell id, cell type, area, then the means, the medians and the window table: a row of the exchange
        for g, members in enumerate(groups):
            rows, image_files, kernel_ms, draw_ms, missing = [np.zeros((0, width))], [], 0.0, 0.0, 0
            for i in members:
                ids = np.asarray(self.preprocessor.cell_ids[i], dtype=np.int64)
                mask = self.preprocessor.masks_dev[i]
                image = self.preprocessor.images_dev[i]
                n = len(ids)
                if int(image.shape[0]) != c_img:
                    raise ValueError(f"image {self._image_number(i)} has {int(image.shape[0])} channels, the batch {c_img}")
                types = self._cell_type_ints(i) if n else np.zeros(0, dtype=np.int64)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                area, sums, order = ops.cell_intensities(image, mask, self.preprocessor.cell_ids_dev[i], self.preprocessor.cell_bbox_dev[i],
                                                         intensities.Q_NUM, intensities.Q_DEN)
                kernel_ms += (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                feat = intensities.features(area, sums, order, intensities.Q_NUM, intensities.Q_DEN)
                self.intensity_mask.append(feat[:, :, 0].copy())
                number = self._image_number(i)
                image_files.append(f"{self.batch_id}_intensities_{number}.csv")
                with open(os.path.join(self.result_dir, image_files[-1]), "w") as f:
                    f.write(intensities.cells_csv(ids, types, names, area, markers, stats, feat))
                if maps:
                    for c, marker in enumerate(markers):
                        image_files.append(f"{self.batch_id}_intensity_{intensities.file_slug(marker)}_{number}.png")
                        idx = intensities.colour_index(feat[:, c, 0])
                        rgb = lut[idx].reshape(n, 3)
                        painted = ops.colorize(mask, ids, rgb, rgb, idx)[0].cpu().numpy()
                        Image.fromarray(painted).save(os.path.join(self.result_dir, image_files[-1]))
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
                counts = np.zeros(self.world_size + 1, dtype=np.float64)      # the rows of every rank, then the images without a window table
                counts[self.rank], counts[-1] = len(table), missing
                counts = dist.all_reduce_sum(torch.from_numpy(counts)).numpy().astype(np.int64)
                missing, counts = int(counts[-1]), counts[:-1]
                cap = int(counts.max())
                send = np.zeros((cap, width), dtype=np.float64)
                send[:len(table)] = table
                gathered = dist.all_gather_rows(torch.from_numpy(send), cap * self.world_size).numpy() if cap else send      # equal shards of cap rows
                table = np.concatenate([gathered[r * cap:r * cap + int(counts[r])] for r in range(self.world_size)], axis=0)
                table = table[np.lexsort((table[:, 1], table[:, 0]))]      # by (image number, cell id): the order of a single-rank run
            if integrate and self.rank != 0:
                continue
            t0 = time.perf_counter()
            types = table[:, 2].astype(np.int64)
            means, medians, window = table[:, 4:4 + c_img], table[:, 4 + c_img:4 + 2 * c_img], table[:, 4 + 2 * c_img:]
            empty, streamed = int((table[:, 3] == 0).sum()), int((table[:, 3] > ops.INTENSITY_RESIDENT).sum())
            stem = f"{self.batch_id}_integrated_intensities" if integrate else f"{self.batch_id}_intensities"
            tail = "" if integrate else f"_{self._image_number(members[0])}"
            mid = "" if integrate else "_medians"      # {batch_id}_intensities_{image number}.csv is the image's cell table
            files = [stem + "_summary" + tail + ".csv", stem + mid + tail + ".csv"]
            with open(os.path.join(self.result_dir, files[0]), "w") as f:
                f.write(intensities.summary_csv(names, markers, intensities.type_summary(types, t, means, medians)))
            z = intensities.standardised_medians(types, t, means)
            with open(os.path.join(self.result_dir, files[1]), "w") as f:
                f.write(intensities.matrix_csv(names, markers, z))
            fig = self._write_table_figure(stem + mid + tail, z, -intensities.Z_LIMIT, intensities.Z_LIMIT, row_names=names, col_names=markers)
            files.append(fig["file"])
            if not missing:
                files.append(stem + "_vs_window" + tail + ".csv")
                with open(os.path.join(self.result_dir, files[-1]), "w") as f:
                    f.write(intensities.vs_window_csv(markers, intensities.vs_window(means, window)))
            draw_ms += (time.perf_counter() - t0) * 1e3
            cells = len(table)
            rec = {"file": files[0], "files": files, "image_files": image_files, "figure": {"file": fig["file"], "limit": intensities.Z_LIMIT, "rect": fig["rect"]},
                   "n": cells, "C": c_img, "T": t, "area_zero": empty, "streamed": streamed, "kernel_ms": kernel_ms, "draw_ms": draw_ms}
            self.intensity_stats.append(rec)
            self.logger.log("Cell intensities {}: {} cells, {} markers, {} cell types; {} cells without a pixel, {} above {} pixels (streaming form); "
                            "ops.cell_intensities with its copies {:.1f}, tables and drawing {:.1f} ms.".format(
                                files[0], cells, c_img, t, empty, streamed, ops.INTENSITY_RESIDENT, kernel_ms, draw_ms))
        return None

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
        and the permutations; ``draw_ms``: statistics, CSV, raster and PNG).  Cell-sharded multi-rank runs: rank 0 computes and writes.
        Tile-per-rank: every rank does its own images; the integrated table takes one all-reduce every rank enters, each image's numbers in
        that image's row and +0.0 elsewhere, so they arrive as computed and rank 0 writes the bytes of a single-rank run."""
        import time
        from . import autocorr
        full = self.preprocessor.intensity_full
        n_local = self._n_images
        if (len(full) == 0 or n_local == 0) and not (self.tile_mode and self.preprocessor._n_images > 0):
            raise ValueError("No intensities: call preprocess() first")
        p = int(n_perms)
        if p < 1:
            raise ValueError(f"n_perms must be at least 1, got {n_perms}")
        k = int(n_neighbors)
        tables = [None if full[i] is None else np.ascontiguousarray(full[i], dtype=np.float64) for i in range(n_local)]      # None: an image without cells
        width = next((t.shape[1] for t in tables if t is not None), len(self.channel_parser.markers))
        if width > ops.AUTOCORR_MAX_CHANNELS:
            raise ValueError(f"spatial_autocorrelation handles at most {ops.AUTOCORR_MAX_CHANNELS} channels, got {width}")
        for i, t in enumerate(tables):
            if t is None or len(t) < k:
                raise ValueError(f"image {self._image_number(i)} has {0 if t is None else len(t)} cells, fewer than n_neighbors = {k}")
            if t.ndim != 2 or t.shape[1] != width or len(t) != len(self.preprocessor.cell_tables[i]):
                raise ValueError(f"image {self._image_number(i)}: an intensity table of shape {t.shape} for {len(self.preprocessor.cell_tables[i])} "
                                 f"cells of {width} channels")
        self.autocorr_stats = []
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
            return None
        seed = autocorr.default_seed()
        markers = [str(m) for m in self.channel_parser.markers]
        markers = (markers + [f"channel {j}" for j in range(len(markers), width)])[:width]
        groups = [list(range(n_local))] if integrate else [[i] for i in range(n_local)]
        dev = _lib.require_gpu()
        one = (p + 1) * 2 * width      # per image: the observed and the permuted numerators, then the sums of squares, then the cells
        for members in groups:
            rows = np.zeros((len(members), one + width + 1), dtype=np.float64)
            knn_ms, perm_ms = 0.0, 0.0
            for r, i in enumerate(members):
                tab = self.preprocessor.cell_tables[i]
                x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
                y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
                n = len(tables[i])
                group = torch.zeros(n, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mean = ops.group_sums(torch.from_numpy(tables[i]).to(dev), group, 1)[0].cpu().numpy()[0] / float(n)
                z = tables[i] - mean
                rows[r, one:one + width] = ops.group_sums(torch.from_numpy(z * z).to(dev), group, 1)[0].cpu().numpy()[0]
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
            stem = f"{self.batch_id}_integrated_spatial_autocorr" if integrate else f"{self.batch_id}_spatial_autocorr_{self._image_number(members[0])}"
            with open(os.path.join(self.result_dir, stem + ".csv"), "w") as f:
                f.write(autocorr.table_csv(markers, cells, stats))
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
        return None

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
        from PIL import Image
        from . import cooccurrence, local_autocorr
        full = self.preprocessor.intensity_full
        n_local = self._n_images
        if (len(full) == 0 or n_local == 0) and not (self.tile_mode and self.preprocessor._n_images > 0):
            raise ValueError("No intensities: call preprocess() first")
        p = int(n_perms)
        if p < 1:
            raise ValueError(f"n_perms must be at least 1, got {n_perms}")
        k = int(n_neighbors)
        num_den = local_autocorr.alpha_fraction(alpha)
        tables = [None if full[i] is None else np.ascontiguousarray(full[i], dtype=np.float64) for i in range(n_local)]      # None: an image without cells
        width = next((t.shape[1] for t in tables if t is not None), len(self.channel_parser.markers))
        if width > ops.AUTOCORR_MAX_CHANNELS:
            raise ValueError(f"local_autocorrelation handles at most {ops.AUTOCORR_MAX_CHANNELS} channels, got {width}")
        names = [str(m) for m in self.channel_parser.markers]
        names = (names + [f"channel {j}" for j in range(len(names), width)])[:width]
        if markers is None:
            chosen = list(range(width))
        else:
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
        self.local_autocorr_stats = []
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
            return None
        seed = local_autocorr.default_seed()
        selected = [names[c] for c in chosen]
        dev = _lib.require_gpu()
        for i in range(n_local):
            tab = self.preprocessor.cell_tables[i]
            x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
            y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
            n = len(tables[i])
            group = torch.zeros(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mean = ops.group_sums(torch.from_numpy(tables[i]).to(dev), group, 1)[0].cpu().numpy()[0] / float(n)
            z = tables[i] - mean
            m2 = ops.group_sums(torch.from_numpy(z * z).to(dev), group, 1)[0].cpu().numpy()[0][chosen]
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
            ids = self.preprocessor.cell_ids[i]
            stem = f"{self.batch_id}_local_autocorr_{self._image_number(i)}"
            files = [stem + ".csv", stem + "_summary.csv"]
            with open(os.path.join(self.result_dir, files[0]), "w") as f:
                f.write(local_autocorr.table_csv(ids, selected, stats))
            with open(os.path.join(self.result_dir, files[1]), "w") as f:
                f.write(local_autocorr.summary_csv(selected, stats["class"]))
            for c, name in enumerate(selected):
                cls = np.ascontiguousarray(stats["class"][:, c])
                rgb = colors.LISA_COLORS[cls]
                painted = ops.colorize(self.preprocessor.masks_dev[i], ids, rgb, rgb, cls)[0].cpu().numpy()
                files.append(f"{stem}_{cooccurrence.slug(name)}.png")
                Image.fromarray(painted).save(os.path.join(self.result_dir, files[-1]))
            counts = local_autocorr.class_counts(stats["class"])
            rec = {"file": files[0], "files": files, "n": n, "C": len(chosen), "P": p, "seed": seed, "neighbors": k, "alpha": num_den,
                   "markers": selected, "significant": int(counts[:, 1:].sum()), "knn_ms": (t1 - t0) * 1e3, "perm_ms": (t2 - t1) * 1e3,
                   "draw_ms": (time.perf_counter() - t2) * 1e3}
            self.local_autocorr_stats.append(rec)
            self.logger.log("Local autocorrelation {}: {} cells, {} markers, {} permutations (seed {}), {} significant (cell, marker) pairs at alpha "
                            "{}/{}; centring, kNN and lags {:.1f}, permutations {:.1f}, statistics and drawing {:.1f} ms.".format(
                                files[0], n, len(chosen), p, seed, rec["significant"], num_den[0], num_den[1], rec["knn_ms"], rec["perm_ms"],
                                rec["draw_ms"]))
        return None

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
            tab = self.preprocessor.cell_tables[i]
            x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
            y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
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
            tab = self.preprocessor.cell_tables[i]
            x = tab[:, 5].astype(np.float64) / tab[:, 6].astype(np.float64)
            y = tab[:, 4].astype(np.float64) / tab[:, 6].astype(np.float64)
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

    @staticmethod
    def _add_in_order(tables: np.ndarray) -> np.ndarray:
        """the (T, C) tables of the images added from +0.0 in ascending image order"""
        total = np.zeros(tables.shape[1:], dtype=tables.dtype)
        for t in tables:
            total = total + t
        return total

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
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
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
        markers = [str(m) for m in self.channel_parser.markers]
        markers = (markers + [f"channel {j}" for j in range(len(markers), width)])[:width]
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
        with open(os.path.join(self.result_dir, stem + ".csv"), "w") as f:
            f.write(plots.heatmap_csv(names, markers, sums / counts[:, None].astype(np.float64), counts))
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
        if self.world_size > 1 and not self.tile_mode and self.rank != 0:
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
        with open(os.path.join(self.result_dir, stem + ".csv"), "w") as f:
            f.write(plots.composition_csv(names, counts))
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
