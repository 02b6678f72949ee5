#!/usr/bin/env python3
"""Times the spectral start of the UMAP embedding both ways on the same graph: scipy's eigsh exactly as manifold._spectral_component calls it (the
"scipy" backend) and manifold.spectral_component_gpu (csrc/spectral.hip).  The graph is the pruned fuzzy graph of planted blobs
(8 Gaussian blobs in 15-D plus 5 % uniform noise, sizes in the ratio 3:6:9:12:15:20:25:30), built by the pipeline's own GPU steps (knn_dense,
umap_fuzzy_weights, fuzzy_union, prune_graph).

    python tools/time_spectral.py [--sizes 10000,50000,100000] [--dims 2,5] [--repeats 3] [--no-quality] [--out FILE]

One JSON line per (size, dim) on stdout, appended to --out (default profiles/spectral/time_spectral.jsonl): the median milliseconds of
--repeats runs of either solver, the GPU solver's filter passes and SpMM column products, the largest residual ||S x - theta x|| of either
result (the same fp64 host product for both), and -- for dim 2 unless --no-quality -- the trustworthiness (5 neighbours, 3 000 sampled rows)
of the finished 2-D embedding from either start.  The first size is run once beforehand and discarded (library and code-object load)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIO = (3, 6, 9, 12, 15, 20, 25, 30)


def median(v):
    return sorted(v)[len(v) // 2]


def planted(n, seed=0, dim=15):
    import numpy as np
    rng = np.random.RandomState(seed)
    blob = int(round(n / 1.05))
    sizes = [blob * r // sum(RATIO) for r in RATIO]
    centres = rng.uniform(-10, 10, size=(len(sizes), dim))
    xs = [centres[c] + rng.randn(m, dim) for c, m in enumerate(sizes)]
    xs.append(rng.uniform(-14, 14, size=(n - sum(sizes), dim)))
    x = np.concatenate(xs).astype(np.float32)
    return x[rng.permutation(len(x))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000,100000")
    ap.add_argument("--dims", default="2,5")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral", "time_spectral.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import scipy.sparse
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from multiplexed_image_annotator_amd import _lib, manifold, ops
    dev = _lib.require_gpu()
    sizes = [int(s) for s in args.sizes.split(",")]
    dims = [int(s) for s in args.dims.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def residual(g, vec):
        deg = np.asarray(g.astype(np.float64).sum(axis=1)).ravel()
        d = scipy.sparse.diags(1.0 / np.sqrt(deg))
        s = d @ g.astype(np.float64) @ d
        vec = vec / np.linalg.norm(vec, axis=0)
        sv = s @ vec
        theta = np.einsum("ij,ij->j", vec, sv)
        return float(np.linalg.norm(sv - vec * theta, axis=0).max())

    for i, n in enumerate([sizes[0]] + sizes):
        x = planted(n)
        idx_d, dist_d = ops.knn_dense(torch.from_numpy(x).to(dev), 15)
        _, _, w_d = ops.umap_fuzzy_weights(idx_d, dist_d)
        n_epochs = manifold.default_epochs(n)
        g = manifold.prune_graph(manifold.fuzzy_union(idx_d.cpu().numpy(), w_d.cpu().numpy(), n), n_epochs)
        from scipy.sparse.csgraph import connected_components
        comps = int(connected_components(g, directed=False)[0])
        for dim in dims[:1] if i == 0 else dims:
            gpu_ms, info, vec = [], {}, None
            for _ in range(1 if i == 0 else args.repeats):
                info = {}
                t0 = time.perf_counter()
                vec = manifold.spectral_component_gpu(g, dim, info=info)
                gpu_ms.append((time.perf_counter() - t0) * 1e3)
            if i == 0:
                continue      # warm-up
            rec = {"n": n, "dim": dim, "nnz_per_row": round(g.nnz / n, 2), "components": comps, "gpu_ms": round(median(gpu_ms), 2),
                   "gpu_ms_runs": [round(v, 2) for v in gpu_ms], "gpu_iterations": info.get("iterations"), "gpu_spmm": info.get("spmm"),
                   "gpu_block": info.get("block"), "gpu_degrees": info.get("degrees"), "gpu_converged": vec is not None,
                   "gpu_residual": residual(g, vec) if vec is not None else None, "host_threads": int(os.environ.get("OMP_NUM_THREADS") or 0)}
            sc_ms, ref = [], None
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                ref = manifold._spectral_component(g, dim)
                sc_ms.append((time.perf_counter() - t0) * 1e3)
            rec.update(eigsh_ms=round(median(sc_ms), 2), eigsh_ms_runs=[round(v, 2) for v in sc_ms], eigsh_converged=ref is not None,
                       eigsh_residual=residual(g, ref) if ref is not None else None)
            if dim == 2 and not args.no_quality and comps == 1:
                from sklearn.manifold import trustworthiness
                sub = np.random.RandomState(1).choice(n, min(n, 3000), replace=False)
                for name in ("gpu", "scipy"):
                    vals = []
                    for seed in (0, 1, 2):
                        emb = manifold.umap_embed(x, n_components=2, seed=seed, spectral=name)
                        vals.append(round(float(trustworthiness(x[sub], emb[sub], n_neighbors=5)), 4))
                    rec[f"trust_{name}_start_seeds012"] = vals
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
