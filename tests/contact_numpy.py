"""numpy restatement of the cell contact graph, written from the rules include/ribca_hip.h states for ribca_contact_table and
ribca_edge_perm_counts: which pixels belong to which cell, the ordered pixel pairs w(i, j) within the integer Euclidean reach d in two forms -- a
plain loop over the definition and one masked compare per offset -- the (n, S) table the entry point writes, the edge list, and the label null
over an edge list (the bijection of enrichment_numpy)."""
import numpy as np

import enrichment_numpy as EN


def offsets(d):
    """the (dr, dc) of the disk dr^2 + dc^2 <= d^2 without (0, 0)"""
    return [(dr, dc) for dr in range(-d, d + 1) for dc in range(-d, d + 1) if dr * dr + dc * dc <= d * d and (dr, dc) != (0, 0)]


def cell_image(mask, label_to_cell, n):
    """(H, W) int64: the cell of every pixel, -1 for no cell (label outside [0, L), or mapped outside [0, n))"""
    mask = np.asarray(mask).astype(np.int64)
    table = np.asarray(label_to_cell).astype(np.int64)
    inside = (mask >= 0) & (mask < len(table))
    cell = np.full(mask.shape, -1, dtype=np.int64)
    cell[inside] = table[mask[inside]]
    cell[(cell < 0) | (cell >= n)] = -1
    return cell


def pair_weights_loop(mask, label_to_cell, n, d):
    """{(i, j): w(i, j)} by the definition, one pixel pair at a time"""
    cell = cell_image(mask, label_to_cell, n)
    h, w = cell.shape
    out = {}
    for r in range(h):
        for c in range(w):
            i = int(cell[r, c])
            if i < 0:
                continue
            for dr, dc in offsets(d):
                rr, cc = r + dr, c + dc
                if 0 <= rr < h and 0 <= cc < w:
                    j = int(cell[rr, cc])
                    if j >= 0 and j != i:
                        out[(i, j)] = out.get((i, j), 0) + 1
    return out


def pair_weights(mask, label_to_cell, n, d):
    """the same by shifted arrays: one masked compare per offset, np.unique over a << 32 | b"""
    cell = cell_image(mask, label_to_cell, n)
    h, w = cell.shape
    codes = []
    for dr, dc in offsets(d):
        if abs(dr) >= h or abs(dc) >= w:      # an image thinner than the reach: the offset leaves it from every pixel
            continue
        a = cell[max(0, -dr):h - max(0, dr), max(0, -dc):w - max(0, dc)]
        b = cell[max(0, dr):h - max(0, -dr), max(0, dc):w - max(0, -dc)]
        hit = (a >= 0) & (b >= 0) & (a != b)
        codes.append((a[hit] << 32) | b[hit])
    codes = np.concatenate(codes) if codes else np.zeros(0, dtype=np.int64)
    keys, counts = np.unique(codes, return_counts=True)
    return {(int(k >> 32), int(k & 0xFFFFFFFF)): int(v) for k, v in zip(keys, counts)}


def edge_list(weights):
    """(src, dst int32, pairs int64) sorted by (src, dst)"""
    keys = sorted(weights)
    return (np.array([k[0] for k in keys], dtype=np.int32), np.array([k[1] for k in keys], dtype=np.int32),
            np.array([weights[k] for k in keys], dtype=np.int64))


def table(weights, n, slots):
    """(nbr (n, S) int32, pairs (n, S) int64, degree (n) int32) as ribca_contact_table writes them when every row fits"""
    nbr = np.full((n, slots), -1, dtype=np.int32)
    pairs = np.zeros((n, slots), dtype=np.int64)
    degree = np.zeros(n, dtype=np.int32)
    for (i, j) in sorted(weights):
        nbr[i, degree[i]] = j
        pairs[i, degree[i]] = weights[(i, j)]
        degree[i] += 1
    return nbr, pairs, degree


def edge_pair_counts(src, dst, labels, n_types):
    """(T, T) int64 over the directed edges; an end outside [0, n) or a label outside [0, T) is skipped"""
    src = np.asarray(src).astype(np.int64)
    dst = np.asarray(dst).astype(np.int64)
    labels = np.asarray(labels).astype(np.int64)
    n = len(labels)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    a, b = labels[src[ok]], labels[dst[ok]]
    good = (a >= 0) & (a < n_types) & (b >= 0) & (b < n_types)
    out = np.zeros((n_types, n_types), dtype=np.int64)
    np.add.at(out, (a[good], b[good]), 1)
    return out


def edge_perm_counts(src, dst, cell_type, n_types, seed, image, p0, n_perms):
    """(P, T, T) int64: permutation p0 + j gives cell i the label cell_type[sigma(i)]"""
    cell_type = np.asarray(cell_type)
    n = len(cell_type)
    return np.stack([edge_pair_counts(src, dst, cell_type[EN.sigma(n, seed, image, p0 + j)], n_types) for j in range(n_perms)])


def random_mask(h, w, cells, seed, radius=5.0):
    """(h, w) int32: every pixel within ``radius`` of a random centre carries the label 1 + the index of the nearest centre, the rest 0 -- discs
    that flatten against each other where they meet, with gaps elsewhere; a centre may end up without a pixel"""
    rng = np.random.RandomState(seed)
    cr, cc = rng.uniform(0, h, cells), rng.uniform(0, w, cells)
    rr, cols = np.mgrid[0:h, 0:w]
    d2 = (rr[None] - cr[:, None, None]) ** 2 + (cols[None] - cc[:, None, None]) ** 2
    near = d2.argmin(axis=0)
    return np.where(d2.min(axis=0) <= radius * radius, near + 1, 0).astype(np.int32)


def identity_table(mask):
    """label k -> cell k - 1, label 0 -> no cell: (table int32, n)"""
    top = max(int(np.asarray(mask).max()), 1)
    return np.arange(-1, top, dtype=np.int32), top


def planted_mask(seed=500):
    """240 x 240, a 20 x 20 grid of 12-px sites: 120 random sites hold an A | B domino of two touching 5 x 5 squares, every other site one
    jittered 5 x 5 square of type C or D.  Returns (mask int32 with labels 1 .. 520 in site order, labels (520) with A, B, C, D = 0 .. 3)."""
    rng = np.random.RandomState(seed)
    mask = np.zeros((240, 240), dtype=np.int32)
    domino = np.zeros(400, dtype=bool)
    domino[rng.choice(400, 120, replace=False)] = True
    labels = []
    for site in range(400):
        r0, c0 = 12 * (site // 20), 12 * (site % 20)
        if domino[site]:
            mask[r0 + 3:r0 + 8, c0 + 1:c0 + 6] = len(labels) + 1
            labels.append(0)
            mask[r0 + 3:r0 + 8, c0 + 6:c0 + 11] = len(labels) + 1
            labels.append(1)
        else:
            jr, jc = rng.randint(0, 8, 2)
            mask[r0 + jr:r0 + jr + 5, c0 + jc:c0 + jc + 5] = len(labels) + 1
            labels.append(2 + int(rng.randint(0, 2)))
    return mask, np.array(labels, dtype=np.int64)
