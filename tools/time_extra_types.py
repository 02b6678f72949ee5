#!/usr/bin/env python3
"""Stage timings of the extra-cell-types step (Annotator(min_cells > 0)): k-NN, fuzzy weights, host graph, spectral start (eigsh), SGD and
HDBSCAN, for planted pooled cells (8 Gaussian blobs + 5 % noise) at C = 15 markers.

    python tools/time_extra_types.py [--sizes 10000,50000,100000] [--dim 15] [--no-hdbscan] [--no-sklearn] [--repeats 3] [--out FILE]

One JSON line per size on stdout (and appended to --out).  The first size is run twice and the first run discarded (library load, kernel
code-object load).  HDBSCAN(min_cluster_size=50) is timed --repeats times on the same embedding both ways: manifold.hdbscan (core distances
and spanning tree on the GPU, tree code on the host; the median run's split is recorded) and sklearn's fit, the yardstick of the same run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000,100000")
    ap.add_argument("--dim", type=int, default=15)
    ap.add_argument("--no-hdbscan", action="store_true")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import __graft_entry__
    __graft_entry__.build()
    import umap_restatement as R
    from multiplexed_image_annotator_amd import manifold
    sizes = [int(s) for s in args.sizes.split(",")]
    for i, n in enumerate([sizes[0]] + sizes):
        per = np.array([300, 600, 900, 1200, 1500, 2000, 2500, 3000], dtype=np.float64)
        blob = np.maximum((per / per.sum() * n / 1.05).astype(int), 1)
        x, y = R.planted_blobs(0, dim=args.dim, sizes=tuple(blob.tolist()))
        t = {}
        t0 = time.perf_counter()
        emb = manifold.umap_embed(x, n_components=5, seed=0, timings=t)
        t["umap_total"] = (time.perf_counter() - t0) * 1e3
        rec = {"n": len(x), "dim": args.dim}
        for k, v in t.items():      # stage milliseconds; the spectral backend's name and its counts under their own names
            rec.update({k + "_ms": round(v, 2)} if isinstance(v, float) else {k: v})
        if not args.no_hdbscan:
            from sklearn.metrics import adjusted_rand_score
            runs = []
            for _ in range(1 if i == 0 else args.repeats):
                tt = {}
                t0 = time.perf_counter()
                lab = manifold.hdbscan(emb, 50, timings=tt)
                runs.append(((time.perf_counter() - t0) * 1e3, tt))
            runs.sort(key=lambda r: r[0])
            med = runs[len(runs) // 2]
            rec["hdbscan_gpu_ms"] = round(med[0], 1)
            rec["hdbscan_gpu_ms_runs"] = [round(r[0], 1) for r in runs]
            rec.update({f"hdbscan_gpu_{k}_ms": round(v, 1) for k, v in med[1].items()})
            rec["hdbscan_gpu_clusters"] = int(lab.max()) + 1
            rec["ari_blobs_gpu"] = round(float(adjusted_rand_score(y[y >= 0], lab[y >= 0])), 4)
            if not args.no_sklearn and i > 0:
                from sklearn.cluster import HDBSCAN
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import hdbscan_numpy
                sk = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    ref = HDBSCAN(min_cluster_size=50).fit(emb).labels_
                    sk.append(round((time.perf_counter() - t0) * 1e3, 1))
                sk.sort()
                rec["hdbscan_ms"] = sk[len(sk) // 2]
                rec["hdbscan_ms_runs"] = sk
                rec["hdbscan_clusters"] = int(ref.max()) + 1
                rec["ari_blobs"] = round(float(adjusted_rand_score(y[y >= 0], ref[y >= 0])), 4)
                rec["hdbscan_points_differ"] = int(hdbscan_numpy.best_renaming_mismatches(ref, lab))
        if i == 0:
            continue      # warm-up
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
