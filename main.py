#!/usr/bin/env python3
"""CLI with the reference's argument surface (reference main.py:56-112) on the MI355X hot path.

Runs marker parsing -> preprocess -> predict -> export_annotations -> tissue_region_analysis -> neighborhood_analysis ->
colorize, as the reference does (main.py:19-28), its two plotting steps included: the integrated cell-type heat map and the cell-type
composition pies are reduced and rasterised on the GPU and written with a CSV beside each PNG.  ``--min-cells N`` (N > 0) re-clusters the cells the vote left as "Others" into
"Additional type c" labels (GPU UMAP embedding + GPU HDBSCAN, as the reference's min_cells).  ``--enrichment-perms N`` (N > 0) adds the
permutation z-scores of the neighbourhood matrix (Annotator.neighborhood_enrichment); ``--cooccurrence-bands N`` (N > 0) the cell-type pair counts
and lifts in N distance bands of one cell size each (Annotator.cooccurrence_by_distance); ``--autocorr-perms N`` (N > 0) Moran's I and Geary's C
of every marker with an N-permutation null (Annotator.spatial_autocorrelation); ``--local-autocorr-perms N`` (N > 0) local Moran's I, Getis-Ord
Gi* and a hot-spot map per marker and image from N conditional permutations (Annotator.local_autocorrelation); ``--nearest-bands N`` (N > 0) the
distance of every cell to the nearest cell of each type and the cross-type G function at N radii of one cell size each, with ``--nearest-perms P``
(P > 0) against a P-permutation label null (Annotator.nearest_type_distances); ``--contact-distance D`` (1 <= D <= 8) the contact graph of the
segmentation mask -- which cells lie within D pixels of each other -- with its edge, cell and type-pair tables and a degree map per image, and with
``--contact-perms P`` (P > 0) the z-scores of the type pairs against a P-permutation label null (Annotator.contact_analysis); ``--morphology`` the
per-cell morphology table read off the mask -- area, axes, eccentricity, perimeter, Euler number, the share of the outline that faces other cells,
the share of the cell inside its classifier window -- with its per-type summary and two maps per image (Annotator.cell_morphology);
``--intensities`` the per-cell marker intensities over each cell's own pixels -- mean, std, min, quartiles, max of every channel -- with the per-type
summary, the standardised type medians and one map per marker and image (Annotator.cell_intensities); ``--localization B`` (B one of 1, 2, 3, 4, 6, 8)
where every marker sits in every cell -- its mean over the pixels at most B pixels below the cell's edge and over the rest, their contrast, the
inscribed radius -- with the per-type profile over seven depth shells, the summary and one contrast map per marker and image
(Annotator.marker_localization); ``--colocalization`` whether two markers sit on the same pixels of a cell -- Pearson's r of every marker
pair per cell, and for the pairs named with ``--coloc-pairs A:B,...`` the Manders overlap and fractions, the share of the cell above both gates
(``--coloc-threshold T``) and an r map per image -- over the markers ``--coloc-markers A,B,...`` (default: all, at most 32), with the per-type
summary and the matrices of the median r (Annotator.marker_colocalization); ``--expand-mask D`` (1 <= D <= 32) grows every label of the mask by D pixels on the GPU
before anything reads it -- for masks that outline nuclei -- and writes the grown mask and a per-cell expansion table, and with ``--intensities``
the intensity tables of the nucleus (core) and of the grown ring as well (Annotator(expand_mask=D)); ``--repair-mask A`` (A >= 1) repairs the mask on
the GPU before the expansion and before anything reads it -- the pieces of a torn label become labels of their own, pieces of fewer than A pixels are
dropped, holes are filled -- and writes the repaired mask and a per-component table (Annotator(repair_mask=A)); ``--outlines`` every cell of the mask
the run works on as a polygon with its id, area, cell type, colour and confidence, traced on the GPU, one GeoJSON file (the layout of QuPath's export)
and one per-cell CSV per image (Annotator.cell_outlines); ``--match-masks`` matches a second mask of every image -- ``--second-mask-path`` beside
``--mask-path``, or the column ``second_mask_path`` of ``--batch-csv``: nuclei beside whole cells, or another tool's segmentation -- to the cells on the
GPU: which object belongs to which cell, the nuclear fraction, the IoU of every pair and the agreement of the two masks at IoU 0.5 .. 0.95, with
``--match-intensities`` the marker intensities inside and outside the owned objects and with ``--match-save-masks`` the two compartment masks
(Annotator.mask_matching).  Multi-GPU: launch under ``python -m torch.distributed.run --nproc-per-node N main.py ...``.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Annotate cell types in multiplexed images (MI355X hot path)')
    ap.add_argument('--marker-list-path', type=str, required=True)
    ap.add_argument('--device', type=str, default='cuda')
    ap.add_argument('--main-dir', type=str, default='./')
    ap.add_argument('--batch-id', type=str, required=True)
    ap.add_argument('--strict', action='store_true')
    ap.add_argument('--infer', action='store_true', default=True)      # as in the reference: cannot be switched off here
    ap.add_argument('--no-infer', dest='infer', action='store_false', help='blank planes instead of marker imputation')
    ap.add_argument('--min-cells', type=int, default=-1)
    ap.add_argument('--n-regions', type=int, default=3)
    ap.add_argument('--normalize', action='store_true', default=True)
    ap.add_argument('--no-normalize', dest='normalize', action='store_false')
    ap.add_argument('--blur', type=float, default=0.3)
    ap.add_argument('--amax', type=float, default=99.8)
    ap.add_argument('--confidence', type=float, default=0.3)
    ap.add_argument('--cell-type-confidence', type=float, default=None)
    ap.add_argument('--bs', type=int, default=128)
    ap.add_argument('--cell-size', type=int, default=30)
    ap.add_argument('--n_jobs', type=int, default=0)
    ap.add_argument('--enrichment-perms', type=int, default=0,
                    help='label permutations of the neighbourhood-enrichment z-scores written beside the neighbourhood matrix (0 = off)')
    ap.add_argument('--autocorr-perms', type=int, default=0,
                    help="permutations of the null of Moran's I and Geary's C of every marker, Annotator.spatial_autocorrelation (0 = off)")
    ap.add_argument('--local-autocorr-perms', type=int, default=0,
                    help="conditional permutations of the per-cell local Moran's I / Getis-Ord Gi* and hot-spot maps, Annotator.local_autocorrelation (0 = off)")
    ap.add_argument('--cooccurrence-bands', type=int, default=0,
                    help='distance bands (one cell size wide each, at most 32) of the co-occurrence-by-distance table and figures (0 = off)')
    ap.add_argument('--nearest-bands', type=int, default=0,
                    help='radii (one cell size apart, at most 32) of the nearest-cell-of-every-type tables, maps and G figures (0 = off)')
    ap.add_argument('--nearest-perms', type=int, default=0,
                    help='label permutations of the null of the cross-type G function; read only with --nearest-bands > 0 (0 = no null)')
    ap.add_argument('--contact-distance', type=int, default=0,
                    help='reach in pixels (1 .. 8) within which two cell masks are in contact: edge, cell and type-pair tables and degree maps (0 = off)')
    ap.add_argument('--contact-perms', type=int, default=0,
                    help='label permutations of the null of the contact type pairs; read only with --contact-distance > 0 (0 = no null)')
    ap.add_argument('--morphology', action='store_true',
                    help='per-cell morphology table from the mask (shape, border, Euler number, patch coverage), per-type summary and two maps per image')
    ap.add_argument('--intensities', action='store_true',
                    help="per-cell marker intensities over the cell's own mask pixels (mean, std, min, quartiles, max), per-type summary and one map per marker and image")
    ap.add_argument('--localization', type=int, default=0,
                    help="width in pixels (1, 2, 3, 4, 6 or 8) of the edge compartment of the marker localisation table: per cell and marker the mean "
                         "below the cell's edge and inside, their contrast and the inscribed radius, per-type depth profile and one map per marker and image (0 = off)")
    ap.add_argument('--colocalization', action='store_true',
                    help="per-cell marker colocalisation over the cell's own mask pixels: Pearson's r of every marker pair, per-type summary and "
                         "the matrices of the median r; the other --coloc-* flags are read only with it")
    ap.add_argument('--coloc-markers', type=str, default=None,
                    help='comma-separated names of the 2 .. 32 markers to correlate (default: every marker of the list, at most 32)')
    ap.add_argument('--coloc-pairs', type=str, default=None,
                    help='comma-separated pairs A:B of those markers that also get the full statistics (r, Manders overlap, M1, M2, pixels above '
                         'both gates, Jaccard) and an r map per image')
    ap.add_argument('--coloc-threshold', type=float, default=0.15,
                    help='the gate of the Manders fractions on the normalised intensity scale, 0 <= T < 1 (0.15 = 15 %%)')
    ap.add_argument('--outlines', action='store_true',
                    help='every cell as a polygon with properties, traced on the GPU from the mask after repair and expansion: one GeoJSON file '
                         '(QuPath detections: id, area, cell type, colour, confidence) and one per-cell ring table per image')
    ap.add_argument('--match-masks', action='store_true',
                    help='match a second mask of every image (--second-mask-path, or the column second_mask_path of --batch-csv) to the cells: per-cell, '
                         'per-object and pair tables, a nuclear-fraction map, and the agreement of the two masks at IoU 0.5 .. 0.95')
    ap.add_argument('--second-mask-path', type=str, default=None, help='the second mask of --image-path; read only with --match-masks')
    ap.add_argument('--match-min-overlap', type=int, default=50,
                    help='percent (1 .. 100) of an object that must lie in its cell for the cell to own it; read only with --match-masks')
    ap.add_argument('--match-intensities', action='store_true',
                    help='with --match-masks: the per-cell marker intensities inside the owned objects and over the rest of the cell')
    ap.add_argument('--match-save-masks', action='store_true', help='with --match-masks: write the inner and outer compartment masks as .npy')
    ap.add_argument('--expand-mask', type=int, default=0,
                    help='grow every label of the mask by this many pixels (1 .. 32) on the GPU before anything reads it: for nuclear masks; writes the '
                         'expanded mask and a per-cell expansion table, and with --intensities the core and ring tables (0 = use the mask as it is)')
    ap.add_argument('--repair-mask', type=int, default=0,
                    help='repair the mask on the GPU before anything reads it: pieces of a torn label become labels of their own, pieces of fewer than '
                         'this many pixels are dropped, holes are filled; writes the repaired mask and a per-component table (0 = use the mask as it is)')
    grp = ap.add_mutually_exclusive_group(required=True)
    grp.add_argument('--image-path', type=str)
    grp.add_argument('--batch-csv', type=str)
    ap.add_argument('--mask-path', type=str)
    args = ap.parse_args(argv)
    if args.image_path and not args.mask_path:
        ap.error("--mask-path is required when using --image-path")
    if args.match_masks and args.image_path and not args.second_mask_path:
        ap.error("--match-masks needs --second-mask-path beside --mask-path (or the column second_mask_path in --batch-csv)")
    if not 1 <= args.match_min_overlap <= 100:
        ap.error("--match-min-overlap takes a percent of 1 .. 100")
    if not 0 <= args.contact_distance <= 8:
        ap.error("--contact-distance takes 0 (off) or a reach of 1 .. 8 pixels")
    if not 0 <= args.expand_mask <= 32:
        ap.error("--expand-mask takes 0 (off) or a distance of 1 .. 32 pixels")
    if args.localization not in (0, 1, 2, 3, 4, 6, 8):
        ap.error("--localization takes 0 (off) or an edge band of 1, 2, 3, 4, 6 or 8 pixels")
    if not 0 <= args.repair_mask <= 2 ** 31 - 1:
        ap.error("--repair-mask takes 0 (off) or a smallest area of 1 pixel or more")
    args.coloc = None      # the arguments of Annotator.marker_colocalization; None: nothing of it is read or written
    if args.colocalization:
        try:
            args.coloc = _coloc_arguments(args.marker_list_path, args.coloc_markers, args.coloc_pairs, args.coloc_threshold)
        except ValueError as e:
            ap.error(str(e))
    return args


def _coloc_arguments(marker_list_path, markers, pairs, threshold):
    """the keyword arguments of Annotator.marker_colocalization from the --coloc-* flags; ValueError for a threshold outside 0 <= T < 1, a
    marker the list does not hold (or holds twice, or named twice), fewer than 2 or more than 32 markers, a malformed or repeated pair"""
    import numpy as np
    from multiplexed_image_annotator_amd import colocalization
    if not 0.0 <= threshold < 1.0:
        raise ValueError("--coloc-threshold takes a gate T with 0 <= T < 1")
    listed = [str(m) for m in np.atleast_1d(np.loadtxt(marker_list_path, delimiter=',', dtype=str))]
    chosen = listed if markers is None else [m for m in markers.split(",")]
    for m in chosen:
        if listed.count(m) != 1 or chosen.count(m) != 1:
            raise ValueError(f"--coloc-markers: {m!r} is not one marker of {marker_list_path}, named once")
    if not 2 <= len(chosen) <= colocalization.MAX_MARKERS:
        raise ValueError(f"--colocalization correlates 2 to {colocalization.MAX_MARKERS} markers, got {len(chosen)}: select some with --coloc-markers")
    named = None if pairs is None else pairs.split(",")
    colocalization.parse_pairs(named, chosen)
    return dict(markers=None if markers is None else chosen, pairs=named, threshold=threshold)


def _setup():
    import __graft_entry__
    __graft_entry__.build()
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch
        import torch.distributed as dist
        if not dist.is_initialized():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            dist.init_process_group(os.environ.get("RIBCA_DIST_BACKEND", "nccl"))


def _check_expand_mask(expand_mask):
    """the ValueError of ImageProcessor(expand_mask=...), before anything is built or read"""
    from multiplexed_image_annotator_amd import ops
    return ops.check_expand_distance(expand_mask, "expand_mask", allow_zero=True)


def _check_repair_mask(repair_mask):
    """the ValueError of ImageProcessor(repair_mask=...), before anything is built or read"""
    from multiplexed_image_annotator_amd import repair
    return repair.check_min_area(repair_mask, "repair_mask", allow_zero=True)


def _pipeline(annotator, bs, n_regions, enrichment_perms=0, cooccurrence_bands=0, autocorr_perms=0, local_autocorr_perms=0, nearest_bands=0,
              nearest_perms=0, match=None, outlines=False, localization=0, coloc=None, expand_mask=0, morphology=False, intensities=False,
              contact_distance=0, contact_perms=0):
    """The call sequence of reference main.py:19-28 / 43-52: the CSV is exported ONCE, before the tissue-region analysis, so its
    "Tissue Region" column reads None exactly as the reference's does (RIBCA_EXPORT_REGIONS=1 opts in to a second export that
    carries the regions).  Two guards the reference lacks keep small images from raising inside its k-NN queries.  Its plotting
    calls (generate_heatmap(integrate=True), cell_type_composition()) draw on the GPU; the batch-wide pie is written beside the
    reference's per-image ones, as the heat map and the neighbourhood matrix of this sequence are the integrated ones."""
    p = annotator.channel_parser
    if not p.immune_base and not p.immune_extended and not p.immune_full and not p.struct and not p.nerve:
        raise ValueError("No panels are applied. Please check the marker list.")
    annotator.preprocess()
    annotator.predict(bs)
    annotator.generate_heatmap(integrate=True)
    annotator.export_annotations()
    n_cells = annotator.min_cells_per_image()
    if n_regions > 0 and n_cells >= 201:           # the reference's 201-neighbour query raises on smaller images
        annotator.tissue_region_analysis(n_regions)
        if os.environ.get("RIBCA_EXPORT_REGIONS") == "1":      # opt-in deviation: the reference's CSV never carries the regions
            annotator.export_annotations()
    if n_cells >= 25:                               # the reference's kNN (25 neighbours) raises on smaller images
        annotator.neighborhood_analysis(integrate=True, normalize=True)
        if enrichment_perms > 0:                    # not a step of the reference: the permutation z-scores of the same matrix
            annotator.neighborhood_enrichment(n_perms=enrichment_perms, integrate=True)
        if autocorr_perms > 0:                      # nor of this one: Moran's I and Geary's C of every marker over the same k-NN graph
            annotator.spatial_autocorrelation(n_perms=autocorr_perms, integrate=True)
        if local_autocorr_perms > 0:                # and WHERE each marker is structured: per-cell statistics and hot-spot maps, per image
            annotator.local_autocorrelation(n_perms=local_autocorr_perms)
    if cooccurrence_bands > 0:                      # nor is this one: which cell types meet at which distance (any number of cells)
        from multiplexed_image_annotator_amd import cooccurrence
        annotator.cooccurrence_by_distance(radii=cooccurrence.default_radii(annotator.cell_size, cooccurrence_bands), integrate=True)
    if nearest_bands > 0:                           # and how far every cell is from the nearest cell of each type (any number of cells)
        from multiplexed_image_annotator_amd import cooccurrence
        annotator.nearest_type_distances(radii=cooccurrence.default_radii(annotator.cell_size, nearest_bands), n_perms=max(nearest_perms, 0),
                                         integrate=True)
    if contact_distance > 0:                        # and which cells actually touch: the contact graph of the mask (any number of cells)
        annotator.contact_analysis(distance=contact_distance, n_perms=max(contact_perms, 0), integrate=True)
    if morphology:                                  # and what the cells themselves look like: the morphology table of the mask (any number of cells)
        annotator.cell_morphology(integrate=True)
    if intensities:                                 # and what they express: the marker intensities over each cell's own pixels (any number of cells)
        annotator.cell_intensities(integrate=True)
        if expand_mask > 0:                         # the mask was grown from nuclei: the same table over the nucleus and over the grown ring
            annotator.cell_intensities(integrate=True, maps=False, compartment="core")
            annotator.cell_intensities(integrate=True, maps=False, compartment="ring")
    if localization > 0:                            # and where in the cell they express it: rim or interior, per cell and marker (any number of cells)
        annotator.marker_localization(band=localization, integrate=True)
    if coloc is not None:                           # and whether two markers share the pixels of a cell: double positive, doublet or spill (any number of cells)
        annotator.marker_colocalization(integrate=True, **coloc)
    if match is not None:                           # and how a second mask of the same images -- nuclei, another tool's cells -- sits in the cells
        annotator.mask_matching(integrate=True, **match)
    if outlines:                                    # and the cells as objects a viewer can load: polygons with properties, per image
        annotator.cell_outlines()
    annotator.colorize(from_script=True)
    annotator.cell_type_composition()
    annotator.cell_type_composition(integrate=True)
    annotator.clear_tmp()


def run(marker_list_path, image_path, mask_path, device, main_dir, batch_id, bs, strict, infer, min_cells, n_regions, normalize, blur, amax,
        confidence, cell_size, cell_type_confidence, n_jobs, enrichment_perms=0, cooccurrence_bands=0, autocorr_perms=0, local_autocorr_perms=0,
        nearest_bands=0, nearest_perms=0, match=None, second_mask_path=None, outlines=False, localization=0, coloc=None, repair_mask=0, expand_mask=0,
        morphology=False, intensities=False, contact_distance=0, contact_perms=0):
    """reference main.py:9-36: one image + mask -> images.csv -> annotate; returns (intensity_dict, names) as the reference does."""
    import numpy as np
    _check_expand_mask(expand_mask)
    _check_repair_mask(repair_mask)
    _setup()
    from multiplexed_image_annotator_amd.annotator import Annotator
    path_ = os.path.join(main_dir, "images.csv")
    if int(os.environ.get("RANK", "0")) == 0:
        os.makedirs(main_dir, exist_ok=True)
        with open(path_, "w") as f:
            if match is not None and second_mask_path:
                f.write("image_path,mask_path,second_mask_path\n%s,%s,%s\n" % (image_path, mask_path, second_mask_path))
            else:
                f.write("image_path,mask_path\n%s,%s\n" % (image_path, mask_path))
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        dist.barrier()
    annotator = Annotator(marker_list_path, path_, device, main_dir, batch_id, strict, infer, min_cells, normalize, blur, amax, confidence,
                          cell_size, cell_type_confidence, n_jobs=n_jobs, expand_mask=expand_mask, repair_mask=repair_mask)
    _pipeline(annotator, bs, n_regions, enrichment_perms, cooccurrence_bands, autocorr_perms, local_autocorr_perms, nearest_bands, nearest_perms,
              expand_mask=expand_mask, morphology=morphology, intensities=intensities, contact_distance=contact_distance, contact_perms=contact_perms,
              outlines=outlines, match=match, localization=localization, coloc=coloc)
    intensity_dict = {}
    full = annotator.preprocessor.intensity_full[0]
    for i in range(len(full)):
        intensity_dict[i + 1] = full[i]
    intensity_dict[0] = np.zeros_like(full[0])
    names = annotator.get_cell_type_names()
    return intensity_dict, names


def batch_run(marker_list_path, image_path, device, main_dir, batch_id, bs, strict, infer, min_cells, n_regions, normalize, blur, amax,
              confidence, cell_size, cell_type_confidence, n_jobs=0, enrichment_perms=0, cooccurrence_bands=0, autocorr_perms=0,
              local_autocorr_perms=0, nearest_bands=0, nearest_perms=0, match=None, outlines=False, localization=0, coloc=None, repair_mask=0, expand_mask=0,
              morphology=False, intensities=False, contact_distance=0, contact_perms=0):
    """reference main.py:39-52: ``image_path`` is a CSV with columns image_path,mask_path (and second_mask_path for ``match``)."""
    _check_expand_mask(expand_mask)
    _check_repair_mask(repair_mask)
    _setup()
    from multiplexed_image_annotator_amd.annotator import Annotator
    annotator = Annotator(marker_list_path, image_path, device, main_dir, batch_id, strict, infer, min_cells, normalize, blur, amax,
                          confidence, cell_size, cell_type_confidence, n_jobs=n_jobs, expand_mask=expand_mask, repair_mask=repair_mask)
    _pipeline(annotator, bs, n_regions, enrichment_perms, cooccurrence_bands, autocorr_perms, local_autocorr_perms, nearest_bands, nearest_perms,
              expand_mask=expand_mask, morphology=morphology, intensities=intensities, contact_distance=contact_distance, contact_perms=contact_perms,
              outlines=outlines, match=match, localization=localization, coloc=coloc)


def main(argv=None):
    args = parse_args(argv)
    common = dict(marker_list_path=args.marker_list_path, device=args.device, main_dir=args.main_dir, batch_id=args.batch_id, bs=args.bs,
                  strict=args.strict, infer=args.infer, min_cells=args.min_cells, n_regions=args.n_regions, normalize=args.normalize,
                  blur=args.blur, amax=args.amax, confidence=args.confidence, cell_size=args.cell_size,
                  cell_type_confidence=args.cell_type_confidence, n_jobs=args.n_jobs, enrichment_perms=args.enrichment_perms,
                  cooccurrence_bands=args.cooccurrence_bands, autocorr_perms=args.autocorr_perms,
                  local_autocorr_perms=args.local_autocorr_perms, nearest_bands=args.nearest_bands, nearest_perms=args.nearest_perms,
                  contact_distance=args.contact_distance, contact_perms=args.contact_perms, morphology=args.morphology, intensities=args.intensities,
                  expand_mask=args.expand_mask, repair_mask=args.repair_mask, outlines=args.outlines, localization=args.localization,
                  coloc=args.coloc)
    if args.match_masks:      # the arguments of Annotator.mask_matching; None: nothing of it is read or written
        common["match"] = dict(min_overlap=args.match_min_overlap, intensities=args.match_intensities, save_masks=args.match_save_masks)
    if args.batch_csv:
        return batch_run(image_path=args.batch_csv, **common)
    return run(image_path=args.image_path, mask_path=args.mask_path, second_mask_path=args.second_mask_path, **common)


if __name__ == "__main__":
    main()
