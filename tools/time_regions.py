#!/usr/bin/env python3
"""Times the tissue-region step (Annotator.tissue_region_analysis, method "kmeans") both ways on the same count table: the GPU path
(regions.pca_project + regions.kmeans, csrc/regions.hip) and scikit-learn's PCA(0.99).fit_transform + KMeans(k).fit_predict, the host calls
kept behind RIBCA_REGIONS=sklearn.  Planted bands of cell-type mixes (synth.planted_bands), T = 13 cell types, k = 5 and 10.

    python tools/time_regions.py [--sizes 10000,50000,100000] [--types 13] [--ks 5,10] [--repeats 3] [--no-sklearn] [--out FILE]

One JSON line per (size, k) on stdout, appended to --out (default profiles/regions/time_regions.jsonl).  Every figure is the median of
--repeats runs; the first size is run once more beforehand and discarded (library load, code-object load).  The 201-NN counting that
precedes both paths is not part of either figure."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000,100000")
    ap.add_argument("--types", type=int, default=13)
    ap.add_argument("--ks", default="5,10")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions", "time_regions.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from multiplexed_image_annotator_amd import ops, regions, synth
    sizes = [int(s) for s in args.sizes.split(",")]
    ks = [int(s) for s in args.ks.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for i, n in enumerate([sizes[0]] + sizes):
        x, y, types, band = synth.planted_bands(n, args.types, 6, 11)
        counts = ops.knn_composition_counts(x, y, types, args.types)
        torch.cuda.synchronize()
        table = None
        for k in ks[:1] if i == 0 else ks:
            pca_ms, km_ms, iters = [], [], []
            for _ in range(1 if i == 0 else args.repeats):
                t0 = time.perf_counter()
                emb = regions.pca_project(counts, ops.TISSUE_NEIGHBOURHOODS)
                torch.cuda.synchronize()
                pca_ms.append((time.perf_counter() - t0) * 1e3)
                info = {}
                t0 = time.perf_counter()
                labels = regions.kmeans(emb, k, 0, timings=info)
                km_ms.append((time.perf_counter() - t0) * 1e3)
                iters.append(info["iterations"])
            rec = {"n": n, "types": args.types, "F": 8 * args.types, "d": int(emb.shape[1]), "k": k, "gpu_pca_ms": round(median(pca_ms), 2),
                   "gpu_kmeans_ms": round(median(km_ms), 2), "gpu_kmeans_init_ms": round(info["init_ms"], 2), "gpu_iterations": iters[-1],
                   "gpu_pca_ms_runs": [round(v, 2) for v in pca_ms], "gpu_kmeans_ms_runs": [round(v, 2) for v in km_ms]}
            if not args.no_sklearn and i > 0:
                from sklearn.cluster import KMeans
                from sklearn.decomposition import PCA
                from sklearn.metrics import adjusted_rand_score
                if table is None:
                    table = counts.cpu().numpy().astype(np.float64)
                    table /= table.sum(axis=2, keepdims=True)
                    table = table.reshape(n, -1)
                sp, sk, si = [], [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    ys = PCA(n_components=0.99).fit_transform(table)
                    sp.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    km = KMeans(n_clusters=k).fit(ys)
                    sk.append((time.perf_counter() - t0) * 1e3)
                    si.append(int(km.n_iter_))
                rec.update(sklearn_pca_ms=round(median(sp), 2), sklearn_kmeans_ms=round(median(sk), 2), sklearn_iterations=si,
                           sklearn_pca_ms_runs=[round(v, 2) for v in sp], sklearn_kmeans_ms_runs=[round(v, 2) for v in sk],
                           ari_gpu_vs_sklearn=round(float(adjusted_rand_score(km.labels_, labels)), 4),
                           host_threads=int(os.environ.get("OMP_NUM_THREADS") or 0))
            if i == 0:
                continue      # warm-up
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
