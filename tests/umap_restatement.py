"""Plain numpy / scipy restatement of the umap steps of the extra-cell-types path (include/ribca_hip.h: ribca_knn_dense,
ribca_umap_fuzzy_weights, ribca_umap_optimize; multiplexed_image_annotator_amd/manifold.py), written from their description:

- k-NN: fp32 sum of squared differences in dimension order, rows sorted by (distance, index), the row itself included;
- smooth_knn_dist (local_connectivity 1, bandwidth 1, target log2 k over neighbours 1..k-1, 64 bisection steps, tolerance 1e-5, floor 1e-3 x
  the row mean, or x the global mean for a row without a positive distance) and the membership weights;
- union P + P^T - P o P^T, pruning below max / n_epochs, epochs_per_sample;
- one Jacobi epoch of the layout SGD with the counter-based negative samples (splitmix64 of seed, epoch, edge, sample).

Vectorised, it runs a whole layout of a few thousand points on the CPU (restated_embed), which is what the quality thresholds of
tests/test_gpu_umap.py were calibrated on.
"""
import numpy as np
import scipy.sparse

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def knn(x, k):
    x = np.asarray(x, dtype=np.float32)
    n, dim = x.shape
    s = np.zeros((n, n), dtype=np.float32)
    for d in range(dim):
        e = x[None, :, d] - x[:, None, d]
        s += e * e
    order = np.argsort(s, axis=1, kind="stable")[:, :k]      # stable: equal distances stay in index order
    return order.astype(np.int32), np.sqrt(np.take_along_axis(s, order, axis=1))


def smooth_knn_dist(dist, n_iter=64):
    dist = np.asarray(dist, dtype=np.float32)
    n, k = dist.shape
    target = np.log2(k)
    pos = dist > 0
    first = np.argmax(pos, axis=1)
    rho = np.where(pos.any(axis=1), dist[np.arange(n), first], np.float32(0)).astype(np.float32)
    lo = np.zeros(n)
    hi = np.full(n, np.inf)
    mid = np.ones(n)
    done = np.zeros(n, dtype=bool)
    d = (dist[:, 1:] - rho[:, None]).astype(np.float32)
    for _ in range(n_iter):
        with np.errstate(over="ignore"):
            terms = np.where(d > 0, np.exp(-(d.astype(np.float64) / mid[:, None])), 1.0)
        psum = np.zeros(n)      # sequential fp64 sum, as the kernel adds
        for j in range(k - 1):
            psum = psum + terms[:, j]
        close = np.abs(psum - target) < 1e-5
        done |= close
        act = ~done
        up = act & (psum > target)
        dn = act & ~(psum > target)
        hi = np.where(up, mid, hi)
        mid = np.where(up, (lo + hi) / 2.0, mid)
        lo = np.where(dn, mid, lo)
        mid = np.where(dn, np.where(np.isinf(hi), mid * 2.0, (lo + hi) / 2.0), mid)
    sigma = mid.astype(np.float32)
    row_mean = dist.astype(np.float64).mean(axis=1)
    glob_mean = dist.astype(np.float64).mean()
    floor = np.where(rho > 0, 1e-3 * row_mean, 1e-3 * glob_mean)
    low = sigma.astype(np.float64) < floor
    sigma = np.where(low, floor.astype(np.float32), sigma).astype(np.float32)
    return sigma, rho


def membership(idx, dist, sigma, rho):
    n, k = idx.shape
    d = (dist - rho[:, None]).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = np.exp(-(d / sigma[:, None])).astype(np.float32)
    w = np.where((d <= 0) | (sigma[:, None] == 0), np.float32(1), v).astype(np.float32)
    w[idx == np.arange(n)[:, None]] = 0.0
    return w


def union(idx, w, n):
    k = idx.shape[1]
    p = scipy.sparse.csr_matrix((w.ravel(), (np.repeat(np.arange(n), k), idx.ravel())), shape=(n, n))
    p.eliminate_zeros()
    g = (p + p.T - p.multiply(p.T)).tocsr()
    g.eliminate_zeros()
    g.sort_indices()
    return g


def prune(g, n_epochs):
    g = g.copy()
    g.data[g.data < g.data.max() / float(n_epochs)] = 0
    g.eliminate_zeros()
    g.sort_indices()
    return g


def epochs_per_sample(w, n_epochs):
    ns = n_epochs * (w / w.max())
    return np.where(ns > 0, float(n_epochs) / np.maximum(ns.astype(np.float64), 1e-300), -1.0)


def rev_index(g):
    rows = np.repeat(np.arange(g.shape[0]), np.diff(g.indptr))
    pos = {(r, c): e for e, (r, c) in enumerate(zip(rows.tolist(), g.indices.tolist()))}
    return np.array([pos[(c, r)] for r, c in zip(rows.tolist(), g.indices.tolist())], dtype=np.int64)


def splitmix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def neg_samples(seed, epoch, e, p, n):
    """sample p of edge e in epoch `epoch`: (top 32 bits of splitmix64(splitmix64(splitmix64(splitmix64(seed) ^ epoch) ^ e) ^ p)) mod n"""
    key = splitmix64(splitmix64(np.uint64(seed)) ^ np.uint64(epoch))
    h = splitmix64(splitmix64(key ^ np.asarray(e, dtype=np.uint64)) ^ np.asarray(p, dtype=np.uint64))
    return ((h >> np.uint64(32)) % np.uint64(n)).astype(np.int64)


def _rdist(u, v):
    s = np.zeros(u.shape[0], dtype=np.float32)
    for d in range(u.shape[1]):
        e = u[:, d] - v[:, d]
        s = s + e * e
    return s


def _attract(d2, a, b):
    d = d2.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pb = np.exp(b * np.log(d))
        g = -2.0 * a * b * (pb / d) / (a * pb + 1.0)
    return np.where(d > 0, g, 0.0)


def _repulse(d2, a, b, gamma):
    d = d2.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = 2.0 * gamma * b / ((0.001 + d) * (a * np.exp(b * np.log(d)) + 1.0))
    return np.where(d > 0, g, 0.0)


def jacobi_epoch(emb, indptr, indices, rev, eps, state, epoch, n_epochs, a, b, seed, gamma=1.0, alpha0=1.0, neg_rate=5.0):
    """One epoch; emb (n, dim) fp32 is returned anew, state = [next_sample, next_neg] (fp64 per edge) is advanced in place."""
    n, dim = emb.shape
    nxt, nneg = state
    alpha = alpha0 * (1.0 - epoch / n_epochs)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    acc = np.zeros((n, dim))
    fe = float(epoch)
    sampled = nxt <= fe
    es = np.flatnonzero(sampled)
    v, k = rows[es], indices[es]
    diff = (emb[v] - emb[k]).astype(np.float32)
    g = _attract(_rdist(emb[v], emb[k]), a, b)
    np.add.at(acc, v, np.clip(g[:, None] * diff.astype(np.float64), -4, 4) * alpha)
    epsn = eps / neg_rate
    nn = np.zeros(len(eps), dtype=np.int64)
    nn[es] = ((fe - nneg[es]) / epsn[es]).astype(np.int64)
    nn = np.maximum(nn, 0)
    if nn.sum():
        ee = np.repeat(np.arange(len(eps)), nn)
        pp = np.arange(len(ee)) - np.repeat(np.cumsum(nn) - nn, nn)
        j = neg_samples(seed, epoch, ee, pp, n)
        vv = rows[ee]
        keep = j != vv
        ee, j, vv = ee[keep], j[keep], vv[keep]
        d2 = _rdist(emb[vv], emb[j])
        gr = _repulse(d2, a, b, gamma)
        diff = (emb[vv] - emb[j]).astype(np.float32)
        np.add.at(acc, vv, np.clip(gr[:, None] * diff.astype(np.float64), -4, 4) * alpha)
    # move_other: the head k of the mirrored edge (k -> v) moves v by -clip(g (x_k - x_v)) alpha
    ins = np.flatnonzero(sampled[rev])
    v, k = rows[ins], indices[ins]
    diff = (emb[k] - emb[v]).astype(np.float32)
    g = _attract(_rdist(emb[v], emb[k]), a, b)
    np.subtract.at(acc, v, np.clip(g[:, None] * diff.astype(np.float64), -4, 4) * alpha)
    new = (emb.astype(np.float64) + acc).astype(np.float32)
    nxt[es] += eps[es]
    nneg[es] += nn[es] * epsn[es]
    return new


def optimize(emb, indptr, indices, rev, eps, n_epochs_run, n_epochs, a, b, seed, **kw):
    state = [eps.astype(np.float64).copy(), (eps / kw.get("neg_rate", 5.0)).astype(np.float64)]
    for ep in range(n_epochs_run):
        emb = jacobi_epoch(emb, indptr, indices, rev, eps, state, ep, n_epochs, a, b, seed, **kw)
    return emb


def restated_embed(x, n_components=5, n_neighbors=15, seed=0):
    """the whole umap_embed on the CPU: restated GPU steps + the host steps of manifold.py"""
    from multiplexed_image_annotator_amd import manifold
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    k = min(n_neighbors, n - 1)
    idx, dist = knn(x, k)
    sigma, rho = smooth_knn_dist(dist)
    w = membership(idx, dist, sigma, rho)
    n_epochs = 500 if n <= 10000 else 200
    g = prune(union(idx, w, n), n_epochs)
    eps = epochs_per_sample(g.data, n_epochs)
    a, b = manifold.find_ab_params()
    emb = manifold.initial_embedding(g, n_components, seed)
    return optimize(emb, g.indptr, g.indices, manifold.reverse_edges(g), eps, n_epochs, n_epochs, a, b, seed)


def planted_blobs(seed=0, dim=15, sizes=(300, 600, 900, 1200, 1500, 2000, 2500, 3000), noise_frac=0.05, spread=1.0):
    """8 Gaussian blobs in dim-D plus uniform noise points: (x, labels) with label -1 for noise"""
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-10, 10, size=(len(sizes), dim))
    xs, ys = [], []
    for c, m in enumerate(sizes):
        xs.append(centres[c] + spread * rng.randn(m, dim))
        ys.append(np.full(m, c))
    n_noise = int(noise_frac * sum(sizes))
    xs.append(rng.uniform(-14, 14, size=(n_noise, dim)))
    ys.append(np.full(n_noise, -1))
    x = np.concatenate(xs).astype(np.float32)
    y = np.concatenate(ys)
    perm = rng.permutation(len(x))
    return x[perm], y[perm]
