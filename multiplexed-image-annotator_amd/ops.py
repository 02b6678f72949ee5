"""Thin Python wrappers over the C ABI: one function per entry point of ``include/ribca_hip.h``.

Inputs and outputs are torch CUDA(HIP) tensors; nothing here computes on the CPU except tiny host-side
parameter preparation (Gaussian taps, index tables).  All calls enqueue on the current torch stream.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

PATCH = 40
OTHERS = 17
#: utils.py:143-146 key order (tie-break order of the vote); index = global class id, 17 = Others
VOTE_ORDER: List[str] = ["CD4 T cell", "CD8 T cell", "Dendritic cell", "B cell", "M1 macrophage cell", "M2 macrophage cell",
                         "Regulatory T cell", "Granulocyte cell", "Plasma cell", "Natural killer cell", "Mast cell",
                         "Stroma cell", "Smooth muscle", "Endothelial cell", "Epithelial cell", "Proliferating/tumor cell",
                         "Nerve cell"]
GLOBAL_NAMES: List[str] = VOTE_ORDER + ["Others"]

_BLOCK_TENSORS = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
                  "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"]


def _block_keys(prefix: str, depth: int) -> List[str]:
    """the 12 tensors of each timm Block, in blob order"""
    return [f"{prefix}{i}.{t}" for i in range(depth) for t in _BLOCK_TENSORS]


#: state-dict key order of the flat parameter blob (include/ribca_hip.h, ribca_vit_blob_len)
def blob_keys(depth: int) -> List[str]:
    return (["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"] + _block_keys("blocks.", depth)
            + ["norm.weight", "norm.bias", "head.weight", "head.bias"])


def gaussian_taps() -> np.ndarray:
    """27 fp64 weights for sigma = 1, 2, 3 (truncate 4.0), computed exactly as scipy.ndimage's
    ``_gaussian_kernel1d`` does (reference utils.py:265 -> skimage.filters.gaussian -> scipy): entry k of each
    segment is the normalised weight at distance k."""
    taps = np.concatenate([_gauss_weights(sigma) for sigma in (1, 2, 3)])
    assert taps.shape == (27,)
    return taps


_TAPS_DEV: Dict[int, torch.Tensor] = {}
_WS: Dict[int, torch.Tensor] = {}


def _taps(device) -> torch.Tensor:
    key = device.index or 0
    if key not in _TAPS_DEV:
        _TAPS_DEV[key] = torch.from_numpy(gaussian_taps()).to(device)
    return _TAPS_DEV[key]


def workspace(nbytes: int, device, slot: int = 0) -> torch.Tensor:
    """Grow-only scratch buffer per (device, slot) (caller-owned memory of the C ABI).  Work enqueued on different streams
    at the same time must use different slots."""
    key = (device.index or 0, slot)
    cur = _WS.get(key)
    if cur is None or cur.numel() < nbytes:
        _WS[key] = None
        cur = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _WS[key] = cur
    return cur


def _workspace_ptr(nbytes: int, device, slot: int = 0) -> int:
    """the address of ``nbytes`` on a 256-byte boundary inside the (device, slot) workspace, which keeps the memory alive"""
    return (workspace(nbytes + 256, device, slot).data_ptr() + 255) & ~255


def _scratch(nbytes: int, device) -> torch.Tensor:
    """The ``ws is None`` default of a wrapper: what the library's own ``*_ws_bytes`` query asks for.  Never empty, so that arguments the
    library refuses (query = 0) reach its range message and not its NULL check."""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _ws(ws: Optional[torch.Tensor], nbytes: int, device, who: str) -> torch.Tensor:
    """A wrapper's ``ws`` argument: ``_scratch(nbytes)`` for None, else the caller's buffer once it is what the library is handed -- bytes,
    contiguous, on ``device`` (its size is the library's to refuse)."""
    if ws is None:
        return _scratch(nbytes, device)
    if ws.dtype != torch.uint8 or ws.device != device or not ws.is_contiguous():
        raise ValueError(f"{who}: ws must be a contiguous uint8 tensor on the device of its inputs")
    return ws


def _u64(seed: int) -> int:
    """a Python int as the uint64_t seed of the ABI: wrapped, not refused"""
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _cell_table(ids, device=None):
    """The label -> cell table of the ascending mask labels ``ids`` (cell i = ids[i]) as int32 [max label + 1], -1 for a label that is no cell;
    label 0 is never one (the background; colorize paints labels > 0 only).  One entry, -1, for no ids.  On ``device``; the numpy array for None."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    table = np.full(int(ids.max()) + 1 if len(ids) else 1, -1, dtype=np.int32)
    table[ids] = np.arange(len(ids), dtype=np.int32)
    table[0] = -1
    return table if device is None else torch.from_numpy(table).to(device)


def _points(x, y, cell_type, device, who: str):
    """(x, y, labels) on the device as fp64, fp64 and int32 -- labels None for ``cell_type`` None -- after the check that they are n coordinates
    and n labels: the kernels read all three at every index below n"""
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(device)
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).to(device)
    td = None if cell_type is None else torch.from_numpy(np.ascontiguousarray(cell_type, dtype=np.int32)).to(device)
    if xd.dim() != 1 or yd.shape != xd.shape or (td is not None and td.shape != xd.shape):
        shapes = ", ".join(str(tuple(t.shape)) for t in (xd, yd, td) if t is not None)
        raise ValueError(f"{who} takes n coordinates" + (" and n labels" if td is not None else "") + f", got {shapes}")
    return xd, yd, td


def _radii2(radii) -> np.ndarray:
    """the radii squared once in fp64, a contiguous 1-D array: what the kernels compare fp64 squared distances with"""
    r = np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
    return np.ascontiguousarray(r * r)


def _counts_out(out: Optional[torch.Tensor], shape, device, who: str) -> torch.Tensor:
    """the ``out`` of an accumulating counter: zeros of ``shape`` for None, else the caller's tensor once it is what the kernel adds into"""
    if out is None:
        return torch.zeros(shape, dtype=torch.int64, device=device)
    if out.dtype != torch.int64 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{who}: out must be a contiguous int64 tensor of shape {tuple(shape)} on the device of its inputs")
    return out


# ------------------------------------------------------------------------------------------- pre-processing
def mask_minmax(mask: torch.Tensor) -> Tuple[int, int]:
    assert mask.dtype == torch.int32 and mask.is_cuda
    out = torch.empty(2, dtype=torch.int32, device=mask.device)
    check(lib().ribca_mask_minmax(ptr(mask), mask.numel(), ptr(out), stream_ptr()), "ribca_mask_minmax")
    mx, mn = out.tolist()
    return mx, mn


def _label_tables(mask: torch.Tensor) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """The per-label reduction of an (H, W) int32 device mask, left on the device: ti (5, L) int32 = rmin, rmax, cmin, cmax, count and tu (2, L)
    int64 = sum_r, sum_c for the labels 0 .. L - 1; None for a mask without a cell.  Negative labels are an error."""
    assert mask.dtype == torch.int32 and mask.is_cuda and mask.dim() == 2
    h, w = mask.shape
    if mask.numel() == 0:
        return None
    mx, mn = mask_minmax(mask)
    if mn < 0:
        raise ValueError("segmentation mask holds negative labels; cell ids must be 1..N with 0 = background")
    if mx <= 0:
        return None
    L = mx + 1
    ti = torch.empty((5, L), dtype=torch.int32, device=mask.device)
    tu = torch.empty((2, L), dtype=torch.int64, device=mask.device)
    check(lib().ribca_label_table(ptr(mask), h, w, L, ptr(ti), ptr(tu), stream_ptr()), "ribca_label_table")
    return ti, tu


def _no_cells(device) -> Tuple[torch.Tensor, torch.Tensor]:
    return torch.zeros(0, dtype=torch.int32, device=device), torch.zeros((0, 4), dtype=torch.int32, device=device)


def label_table(mask: torch.Tensor, with_device: bool = False):
    """(H, W) int32 device mask -> (ids ascending int64 [n], table int64 [n, 7]: rmin, rmax, cmin, cmax, sum_r, sum_c,
    count) on the host.  The per-label reduction runs on the GPU; the host only drops absent labels.  ``with_device``: additionally the
    device-resident (ids int32 [n], bbox int32 [n, 4]) the crop consumes, so that a caller that needs the host table anyway (CSV
    centroids) does not send the id list back up."""
    tables = _label_tables(mask)
    if tables is None:
        e = (np.zeros(0, np.int64), np.zeros((0, 7), np.int64))
        return e + _no_cells(mask.device) if with_device else e
    ti, tu = tables
    ti_h = ti.cpu().numpy().astype(np.int64)
    tu_h = tu.cpu().numpy()
    ids = np.flatnonzero(ti_h[4] > 0)
    table = np.stack([ti_h[0, ids], ti_h[1, ids], ti_h[2, ids], ti_h[3, ids], tu_h[0, ids], tu_h[1, ids], ti_h[4, ids]], axis=1)
    if with_device:
        ids_d = torch.nonzero(ti[4] > 0).flatten()
        return ids.astype(np.int64), table.astype(np.int64), ids_d.to(torch.int32), ti[:4].index_select(1, ids_d).t().contiguous()
    return ids.astype(np.int64), table.astype(np.int64)


def label_table_device(mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The same reduction with the result left ON THE DEVICE: (ids int32 [n] ascending, bbox int32 [n, 4]: rmin, rmax, cmin, cmax) --
    what ``extract_patches`` consumes.  Only the label range (two scalars) and the cell count cross PCIe; the sharded path uses it so
    that no rank bounces the id list through numpy between the label table and the crop (reference preprocess.py:159-211 builds the
    whole dict on the host)."""
    tables = _label_tables(mask)
    if tables is None:
        return _no_cells(mask.device)
    ti = tables[0]
    ids = torch.nonzero(ti[4] > 0).flatten()                       # ascending; the one host sync (its length)
    bbox = ti[:4].index_select(1, ids).t().contiguous()
    return ids.to(torch.int32), bbox


def channel_min(image: torch.Tensor) -> torch.Tensor:
    assert image.dtype == torch.float32 and image.is_cuda and image.dim() == 3
    c, h, w = image.shape
    out = torch.empty(c, dtype=torch.float32, device=image.device)
    check(lib().ribca_channel_min(ptr(image), c, h * w, ptr(out), stream_ptr()), "ribca_channel_min")
    return out


_RESIZE_PLANS: Dict[Tuple[int, int], Tuple[Optional[torch.Tensor], int, torch.Tensor]] = {}


def resize_plan(patch_size: int) -> Tuple[Optional[np.ndarray], int, np.ndarray]:
    """What ``skimage.transform.resize((C, ps, ps) -> (C, 40, 40), order=0, anti_aliasing=True)`` does per plane, as data:
    Gaussian taps at distance 0..R (sigma = (ps/40 - 1)/2 > 0 only when down-sampling; scipy's truncate-4 radius), and the 40
    nearest-neighbour source indices of ``scipy.ndimage.zoom(order=0, grid_mode=True)`` -- both computed with the same fp64
    operations as the libraries (reference call site preprocess.py:106)."""
    ps = int(patch_size)
    factor = np.divide(ps, PATCH)                              # skimage: factors = input_shape / output_shape
    sigma = max(0.0, float((factor - 1) / 2))
    taps, radius = None, 0
    if sigma > 0:
        radius = int(4.0 * sigma + 0.5)
        if radius > 0:
            taps = _gauss_weights(sigma)
    zoom = np.float64(ps) / np.float64(PATCH)                  # ndimage.zoom(grid_mode=True): input extent / output extent
    o = np.arange(PATCH, dtype=np.float64)
    cc = (o + 0.5) * zoom - 0.5                                # NI_ZoomShift: cc += 0.5; cc *= zoom; cc -= 0.5
    idx = np.floor(cc + 0.5).astype(np.int64)                  # order 0: start = floor(cc + 0.5)
    idx = np.clip(idx, 0, ps - 1)
    return taps, radius, idx.astype(np.int32)


def _resize_plan_dev(patch_size: int, device):
    key = (int(patch_size), device.index or 0)
    if key not in _RESIZE_PLANS:
        taps, radius, idx = resize_plan(patch_size)
        t = torch.from_numpy(np.ascontiguousarray(taps)).to(device) if taps is not None else None
        _RESIZE_PLANS[key] = (t, radius, torch.from_numpy(idx).to(device))
    return _RESIZE_PLANS[key]


def extract_patches(image: torch.Tensor, mask: torch.Tensor, chan_min: torch.Tensor, ids: torch.Tensor, bbox: torch.Tensor,
                    want_avg: bool = False, out: Optional[torch.Tensor] = None, patch_size: int = PATCH) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Soft-masked fp32 patches (n, C, 40, 40) for the given cells (ids int32 [n], bbox int32 [n, 4]).  ``patch_size`` =
    ``int(40 * cell_size / 30)`` (reference preprocess.py:78): windows of another size are resized to 40 x 40 as the
    reference does (preprocess.py:106)."""
    c, h, w = image.shape
    n = ids.numel()
    assert image.dtype == torch.float32 and mask.dtype == torch.int32 and ids.dtype == torch.int32 and bbox.dtype == torch.int32
    assert mask.shape == (h, w) and bbox.shape == (n, 4)
    if out is None:
        out = torch.empty((n, c, PATCH, PATCH), dtype=torch.float32, device=image.device)
    assert out.shape == (n, c, PATCH, PATCH) and out.dtype == torch.float32 and out.is_contiguous()
    avg = torch.empty((n, c), dtype=torch.float64, device=image.device) if want_avg else None
    if n and int(patch_size) == PATCH:
        check(lib().ribca_extract_patches(ptr(image), c, h, w, ptr(mask), ptr(chan_min), ptr(ids), ptr(bbox), ptr(_taps(image.device)), n,
                                          ptr(out), ptr(avg), stream_ptr()), "ribca_extract_patches")
    elif n:
        taps, radius, idx = _resize_plan_dev(patch_size, image.device)
        check(lib().ribca_extract_patches_scaled(ptr(image), c, h, w, ptr(mask), ptr(chan_min), ptr(ids), ptr(bbox), ptr(_taps(image.device)), n,
                                                 int(patch_size), ptr(taps), radius, ptr(idx), ptr(out), ptr(avg), stream_ptr()),
              "ribca_extract_patches_scaled")
    return out, avg


def colorize(mask: torch.Tensor, ids: np.ndarray, type_rgb: np.ndarray, conf_rgb: np.ndarray, type_idx: np.ndarray):
    """Paint every labelled pixel with its cell's colours (reference Annotator.colorize, model.py:806-858): ``ids`` ascending cell
    labels (n), per-cell ``type_rgb`` / ``conf_rgb`` (n, 3) uint8 and ``type_idx`` (n) uint8.  Returns device tensors (H, W, 3),
    (H, W, 3), (H, W) uint8."""
    assert mask.is_cuda and mask.dtype == torch.int32 and mask.dim() == 2
    n = len(ids)
    assert type_rgb.shape == (n, 3) and conf_rgb.shape == (n, 3) and type_idx.shape == (n,)
    h, w = mask.shape
    dev = mask.device
    tab_d = _cell_table(ids, dev)
    a = torch.from_numpy(np.ascontiguousarray(type_rgb, dtype=np.uint8)).to(dev) if n else torch.zeros((1, 3), dtype=torch.uint8, device=dev)
    b = torch.from_numpy(np.ascontiguousarray(conf_rgb, dtype=np.uint8)).to(dev) if n else torch.zeros((1, 3), dtype=torch.uint8, device=dev)
    c = torch.from_numpy(np.ascontiguousarray(type_idx, dtype=np.uint8)).to(dev) if n else torch.zeros((1,), dtype=torch.uint8, device=dev)
    out_t = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    out_c = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    out_i = torch.empty((h, w), dtype=torch.uint8, device=dev)
    mask_c = mask.contiguous()
    check(lib().ribca_colorize(ptr(mask_c), h * w, ptr(tab_d), tab_d.numel(), ptr(a), ptr(b), ptr(c), ptr(out_t), ptr(out_c), ptr(out_i),
                               stream_ptr()), "ribca_colorize")
    return out_t, out_c, out_i


def knn_cooccurrence(x: np.ndarray, y: np.ndarray, cell_type: np.ndarray, n_types: int, n_neighbors: int, out: Optional[torch.Tensor] = None,
                     device=None) -> torch.Tensor:
    """(n_types, n_types) int64 device tensor of (cell, neighbour) type pairs over each cell's n_neighbors - 1 nearest other cells
    (reference spatial_methods.neighborhood_analysis); accumulates into ``out`` when given."""
    dev = device or _lib.require_gpu()
    n = len(x)
    if n_neighbors > n:      # what scikit-learn's kneighbors raises inside the reference
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {n_neighbors}, n_samples_fit = {n}")
    xd, yd, td = _points(x, y, cell_type, dev, "knn_cooccurrence")
    out = _counts_out(out, (int(n_types), int(n_types)), xd.device, "knn_cooccurrence")
    check(lib().ribca_knn_cooccurrence(ptr(xd), ptr(yd), ptr(td), n, int(n_neighbors), int(n_types), ptr(out), stream_ptr()),
          "ribca_knn_cooccurrence")
    return out


def knn_neighbours(x: np.ndarray, y: np.ndarray, n_neighbors: int, device=None) -> torch.Tensor:
    """(n, n_neighbors - 1) int32 device tensor: every cell's nearest other cells in rank order -- the list ``knn_cooccurrence`` counts over
    (same fp64 search, ties towards the lower index, the cell itself dropped)."""
    dev = device or _lib.require_gpu()
    n = len(x)
    if n_neighbors > n:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {n_neighbors}, n_samples_fit = {n}")
    xd, yd, _ = _points(x, y, None, dev, "knn_neighbours")
    idx = torch.empty((n, max(int(n_neighbors) - 1, 0)), dtype=torch.int32, device=dev)
    check(lib().ribca_knn_neighbours(ptr(xd), ptr(yd), n, int(n_neighbors), ptr(idx), stream_ptr()), "ribca_knn_neighbours")
    return idx


NHOOD_MAX_TYPES = 64      # the LDS histogram of csrc/enrichment.hip
NHOOD_MAX_NEIGHBOURS = 31


def nhood_perm_counts_ws_bytes(n: int, n_perms: int) -> int:
    return int(lib().ribca_nhood_perm_counts_ws_bytes(int(n), int(n_perms)))


def nhood_perm_counts(idx: torch.Tensor, cell_type: np.ndarray, n_types: int, seed: int, image: int, p0: int, n_perms: int,
                      out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n_perms, n_types, n_types) int64 device tensor: the co-occurrence counts over the fixed (n, m) int32 device neighbour list ``idx`` under
    the label permutations p0 .. p0 + n_perms - 1 of (seed, image) -- cell i carries cell_type[sigma_p(i)]; include/ribca_hip.h states sigma.
    Accumulates into ``out`` when given (the images of a group).  Labels outside [0, n_types) raise before any launch."""
    if idx.dtype != torch.int32 or idx.dim() != 2:
        raise ValueError("nhood_perm_counts takes an (n, m) int32 neighbour list")
    labels = np.ascontiguousarray(cell_type, dtype=np.int32)
    n, m = idx.shape
    if labels.shape != (n,):
        raise ValueError(f"nhood_perm_counts: {labels.shape} labels for {n} cells")
    if n and (int(labels.min()) < 0 or int(labels.max()) >= int(n_types)):
        raise ValueError(f"nhood_perm_counts: labels must lie in [0, {int(n_types)}), got {int(labels.min())} .. {int(labels.max())}")
    idx = idx.contiguous()
    td = torch.from_numpy(labels).to(idx.device)
    shape = (max(int(n_perms), 0), max(int(n_types), 0), max(int(n_types), 0))
    out = _counts_out(out, shape, idx.device, "nhood_perm_counts")
    ws = _ws(ws, nhood_perm_counts_ws_bytes(n, n_perms), idx.device, "nhood_perm_counts")
    check(lib().ribca_nhood_perm_counts(ptr(idx), ptr(td), n, m, int(n_types), _u64(seed), int(image), int(p0), int(n_perms), ptr(out), ptr(ws),
                                        ws.numel(), stream_ptr()), "ribca_nhood_perm_counts")
    return out


RADIAL_MAX_BANDS = 32      # the thresholds csrc/cooccurrence.hip takes by value
RADIAL_MAX_CELLS = 1 << 21


def radial_pair_counts_ws_bytes(n: int, n_types: int, n_bands: int) -> int:
    return int(lib().ribca_radial_pair_counts_ws_bytes(int(n), int(n_types), int(n_bands)))


def radial_pair_counts(x: np.ndarray, y: np.ndarray, cell_type: np.ndarray, n_types: int, radii: Sequence[float], out: Optional[torch.Tensor] = None,
                       device=None) -> torch.Tensor:
    """(B, n_types, n_types) int64 device tensor: the ordered pairs of cells i != j by (band, type of i, type of j), band b holding the pairs with
    radii[b - 1] < distance <= radii[b] (band 0 from distance 0; beyond the last radius: not counted; a label outside [0, n_types) is skipped).
    ``radii`` in pixels, finite, non-negative and strictly increasing, at most RADIAL_MAX_BANDS of them; they are squared once in fp64 here and
    the kernel compares fp64 squared distances with them.  Accumulates into ``out`` when given (the images of a group)."""
    dev = device or _lib.require_gpu()
    xd, yd, td = _points(x, y, cell_type, dev, "radial_pair_counts")
    n = xd.numel()
    r2 = _radii2(radii)
    out = _counts_out(out, (len(r2), max(int(n_types), 0), max(int(n_types), 0)), xd.device, "radial_pair_counts")
    ws = _scratch(radial_pair_counts_ws_bytes(n, n_types, len(r2)), dev)
    check(lib().ribca_radial_pair_counts(ptr(xd), ptr(yd), ptr(td), n, int(n_types), r2.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(r2),
                                         ptr(out), ptr(ws), ws.numel(), stream_ptr()), "ribca_radial_pair_counts")
    return out


NEAREST_MAX_TYPES = 254           # csrc/nearest.hip: the distance table
NEAREST_PERM_MAX_TYPES = 64       # ... and the permutation counts
NEAREST_MAX_CELLS = 1 << 21


def nearest_by_type_ws_bytes(n: int, n_types: int) -> int:
    return int(lib().ribca_nearest_by_type_ws_bytes(int(n), int(n_types)))


def nearest_perm_counts_ws_bytes(n: int, n_types: int, n_perms: int) -> int:
    return int(lib().ribca_nearest_perm_counts_ws_bytes(int(n), int(n_types), int(n_perms)))


def nearest_by_type(x: np.ndarray, y: np.ndarray, cell_type: np.ndarray, n_types: int, ws: Optional[torch.Tensor] = None,
                    device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(near2, arg): (n, n_types) fp64 and int32 device tensors, per cell and cell type the squared distance to the nearest OTHER cell of that
    type (+inf where there is none) and the lowest index that attains it (-1 where there is none); a label outside [0, n_types) is never a
    target, its cell still has a row.  fp64 brute force, csrc/nearest.hip; include/ribca_hip.h states every comparison."""
    dev = device or _lib.require_gpu()
    xd, yd, td = _points(x, y, cell_type, dev, "nearest_by_type")
    n = xd.numel()
    near2 = torch.empty((n, max(int(n_types), 0)), dtype=torch.float64, device=dev)
    arg = torch.empty((n, max(int(n_types), 0)), dtype=torch.int32, device=dev)
    ws = _ws(ws, nearest_by_type_ws_bytes(n, n_types), xd.device, "nearest_by_type")
    check(lib().ribca_nearest_by_type(ptr(xd), ptr(yd), ptr(td), n, int(n_types), ptr(near2), ptr(arg), ptr(ws), ws.numel(), stream_ptr()),
          "ribca_nearest_by_type")
    return near2, arg


def nearest_perm_counts(x: np.ndarray, y: np.ndarray, cell_type: np.ndarray, n_types: int, radii: Sequence[float], seed: int, image: int, p0: int,
                        n_perms: int, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """(n_perms, B, n_types, n_types) int64 device tensor: under the label permutations p0 .. p0 + n_perms - 1 of (seed, image) -- the positions
    stay, cell i carries cell_type[sigma_p(i)], the sigma of ``nhood_perm_counts`` -- the cells of type a whose nearest other cell of type b lies
    in the band radii[k - 1] < distance <= radii[k] (band 0 from distance 0; beyond the last radius: not counted).  ``radii`` in pixels, squared
    once in fp64 here as ``radial_pair_counts`` squares them.  Accumulates into ``out`` when given (the images of a group)."""
    dev = device or _lib.require_gpu()
    xd, yd, td = _points(x, y, cell_type, dev, "nearest_perm_counts")
    n = xd.numel()
    r2 = _radii2(radii)
    out = _counts_out(out, (max(int(n_perms), 0), len(r2), max(int(n_types), 0), max(int(n_types), 0)), xd.device, "nearest_perm_counts")
    ws = _ws(ws, nearest_perm_counts_ws_bytes(n, n_types, n_perms), xd.device, "nearest_perm_counts")
    check(lib().ribca_nearest_perm_counts(ptr(xd), ptr(yd), ptr(td), n, int(n_types), r2.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(r2),
                                          _u64(seed), int(image), int(p0), int(n_perms), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
          "ribca_nearest_perm_counts")
    return out


CONTACT_MAX_REACH = 8             # csrc/contact.hip: the halo of a pixel tile
CONTACT_MAX_TYPES = 254           # the uint8 index image of colorize, as for the other cell-type steps
CONTACT_PERM_MAX_TYPES = 64       # the LDS histogram of the null
CONTACT_FIRST_SLOTS = 32          # slots per row of the first attempt; doubled while a row overflows
CONTACT_MAX_SLOTS = 1024
CONTACT_MAX_TABLE_BYTES = 2 << 30      # of nbr + pairs, 12 bytes per slot


def contact_table_ws_bytes(h: int, w: int, n: int, slots: int) -> int:
    return int(lib().ribca_contact_table_ws_bytes(int(h), int(w), int(n), int(slots)))


def edge_perm_counts_ws_bytes(n: int, n_perms: int) -> int:
    return int(lib().ribca_edge_perm_counts_ws_bytes(int(n), int(n_perms)))


def contact_table(mask: torch.Tensor, label_to_cell: torch.Tensor, n: int, d: int, slots: int, ws: Optional[torch.Tensor] = None):
    """(nbr (n, slots) int32, pairs (n, slots) int64, degree (n) int32, over (2) int32) device tensors of ribca_contact_table, one attempt at
    ``slots`` slots per row: with over[0] == 0 row i lists the cells in contact with cell i in ascending index order and the ordered pixel pairs
    within the reach ``d`` beside them; include/ribca_hip.h states the contract."""
    if mask.dtype != torch.int32 or mask.dim() != 2 or not mask.is_cuda or label_to_cell.dtype != torch.int32 or label_to_cell.dim() != 1:
        raise ValueError("contact_table takes an (H, W) int32 device mask and an (L) int32 label -> cell table")
    dev = mask.device
    mask, table = mask.contiguous(), label_to_cell.contiguous().to(dev)
    h, w = mask.shape
    rows, cols = max(int(n), 0), max(int(slots), 0)
    nbr = torch.empty((rows, cols), dtype=torch.int32, device=dev)
    pairs = torch.empty((rows, cols), dtype=torch.int64, device=dev)
    degree = torch.empty((rows,), dtype=torch.int32, device=dev)
    over = torch.empty((2,), dtype=torch.int32, device=dev)
    ws = _ws(ws, contact_table_ws_bytes(h, w, n, slots), dev, "contact_table")
    check(lib().ribca_contact_table(ptr(mask), h, w, ptr(table), table.numel(), int(n), int(d), int(slots), ptr(nbr), ptr(pairs), ptr(degree),
                                    ptr(over), ptr(ws), ws.numel(), stream_ptr()), "ribca_contact_table")
    return nbr, pairs, degree, over


def contact_graph(mask: torch.Tensor, ids: np.ndarray, d: int, first_slots: int = CONTACT_FIRST_SLOTS) -> Dict[str, np.ndarray]:
    """The contact graph of an (H, W) int32 device mask over the cells ``ids`` (ascending mask labels, cell i = ids[i]; the label -> cell table
    is built as ``colorize`` builds it, label 0 never a cell): two cells are in contact when pixels of theirs lie within ``d`` pixels (Euclidean,
    1 <= d <= 8).  Returns host arrays: the directed edge list ``src``, ``dst`` int32 and ``pairs`` int64 (the ordered pixel pairs within the
    reach) sorted by (src, dst), each contact in both directions, ``degree`` (n) int32, and ``slots`` = the row length that fitted.  The table
    starts at ``first_slots`` slots per cell and doubles while a row overflows; ValueError when that would pass 1024 slots or 2 GiB -- a
    background region labelled as a cell is the usual cause, and the message names its mask label."""
    assert mask.is_cuda and mask.dtype == torch.int32 and mask.dim() == 2
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    n = len(ids)
    if n == 0:
        return {"src": np.zeros(0, np.int32), "dst": np.zeros(0, np.int32), "pairs": np.zeros(0, np.int64), "degree": np.zeros(0, np.int32),
                "slots": int(first_slots)}
    tab_d = _cell_table(ids, mask.device)
    slots = int(first_slots)
    while True:
        nbr, pairs, degree, over = contact_table(mask, tab_d, n, d, slots)
        failed, lowest = over.tolist()
        if failed == 0:
            break
        why = (f"contact_graph: {failed} cell(s) touch more than {slots} others at reach {d}, the lowest of them mask label {int(ids[lowest])}; "
               "a background region labelled as a cell is the usual cause")
        if slots * 2 > CONTACT_MAX_SLOTS:
            raise ValueError(f"{why} (the table stops at {CONTACT_MAX_SLOTS} slots per cell)")
        if 12 * n * slots * 2 > CONTACT_MAX_TABLE_BYTES:
            raise ValueError(f"{why} (a table of {slots * 2} slots for {n} cells would pass 2 GiB)")
        slots *= 2
    nbr_h, pairs_h, deg_h = nbr.cpu().numpy(), pairs.cpu().numpy(), degree.cpu().numpy()
    keep = np.arange(slots)[None, :] < deg_h[:, None]      # row-major: sorted by (src, dst)
    src = np.repeat(np.arange(n, dtype=np.int32), deg_h)
    return {"src": src, "dst": np.ascontiguousarray(nbr_h[keep], dtype=np.int32), "pairs": np.ascontiguousarray(pairs_h[keep], dtype=np.int64),
            "degree": deg_h.astype(np.int32), "slots": slots}


def edge_perm_counts(src, dst, cell_type: np.ndarray, n_types: int, seed: int, image: int, p0: int, n_perms: int,
                     out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """(n_perms, n_types, n_types) int64 device tensor: the type pairs over the directed edges (src[e], dst[e]) -- int32 arrays or device
    tensors -- under the label permutations p0 .. p0 + n_perms - 1 of (seed, image): cell i carries cell_type[sigma_p(i)], the sigma of
    ``nhood_perm_counts``.  An edge with an end outside [0, n) or a label outside [0, n_types) is skipped.  Accumulates into ``out`` when given
    (the images of a group)."""
    dev = device or (src.device if isinstance(src, torch.Tensor) else _lib.require_gpu())
    sd = src.to(dev) if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src, dtype=np.int32)).to(dev)
    dd = dst.to(dev) if isinstance(dst, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int32)).to(dev)
    if sd.dtype != torch.int32 or dd.dtype != torch.int32 or sd.dim() != 1 or dd.shape != sd.shape:
        raise ValueError("edge_perm_counts takes two (E) int32 edge arrays")
    sd, dd = sd.contiguous(), dd.contiguous()
    labels = np.ascontiguousarray(cell_type, dtype=np.int32).reshape(-1)
    n = len(labels)
    td = torch.from_numpy(labels).to(dev)
    out = _counts_out(out, (max(int(n_perms), 0), max(int(n_types), 0), max(int(n_types), 0)), sd.device, "edge_perm_counts")
    ws = _ws(ws, edge_perm_counts_ws_bytes(n, n_perms), sd.device, "edge_perm_counts")
    check(lib().ribca_edge_perm_counts(ptr(sd), ptr(dd), sd.numel(), ptr(td), n, int(n_types), _u64(seed), int(image), int(p0), int(n_perms), ptr(out),
                                       ptr(ws), ws.numel(), stream_ptr()), "ribca_edge_perm_counts")
    return out


def mask_morphology_ws_bytes(h: int, w: int, n: int) -> int:
    return int(lib().ribca_mask_morphology_ws_bytes(int(h), int(w), int(n)))


def mask_morphology(mask: torch.Tensor, ids: np.ndarray, rect: Optional[np.ndarray] = None, ws: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
    """The morphology sums of an (H, W) int32 device mask over the cells ``ids`` (ascending mask labels, cell i = ids[i]; the label -> cell table
    is built as ``contact_graph`` and ``colorize`` build it, label 0 never a cell).  Returns host arrays: ``sums`` (n, 16) int64 -- area, raw
    moments, leaving pixel edges, perimeter classes, bit quads and the pixels inside the cell's row ``r0, r1, c0, c1`` of ``rect`` (n, 4) int32,
    0 without one -- and ``bbox`` (n, 4) int32; include/ribca_hip.h states the columns, morphology.features turns them into the table."""
    assert mask.is_cuda and mask.dtype == torch.int32 and mask.dim() == 2
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    n = len(ids)
    if n == 0:
        return {"sums": np.zeros((0, 16), np.int64), "bbox": np.zeros((0, 4), np.int32)}
    dev = mask.device
    tab_d = _cell_table(ids, dev)
    rect_d = None
    if rect is not None:
        rect = np.ascontiguousarray(rect, dtype=np.int32)
        if rect.shape != (n, 4):
            raise ValueError(f"mask_morphology takes one rectangle r0, r1, c0, c1 per cell, got {rect.shape} for {n} cells")
        rect_d = torch.from_numpy(rect).to(dev)
    mask = mask.contiguous()
    h, w = mask.shape
    sums = torch.empty((n, 16), dtype=torch.int64, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    ws = _ws(ws, mask_morphology_ws_bytes(h, w, n), dev, "mask_morphology")
    check(lib().ribca_mask_morphology(ptr(mask), h, w, ptr(tab_d), tab_d.numel(), n, ptr(rect_d), ptr(sums), ptr(bbox), ptr(ws), ws.numel(),
                                      stream_ptr()), "ribca_mask_morphology")
    return {"sums": sums.cpu().numpy(), "bbox": bbox.cpu().numpy()}


EXPAND_MAX_DISTANCE = 32          # csrc/expand.hip EX_D_MAX: the largest halo of a pixel tile
EXPAND_TILE = 32                  # csrc/expand.hip EX_TILE


def expand_labels_ws_bytes(h: int, w: int, distance: int) -> int:
    return int(lib().ribca_expand_labels_ws_bytes(int(h), int(w), int(distance)))


def check_expand_distance(distance, what: str = "distance", allow_zero: bool = False) -> int:
    """``distance`` as an int, ValueError unless it is an integer (no bool) in 1 .. EXPAND_MAX_DISTANCE, or 0 where that means "do not expand" """
    low = 0 if allow_zero else 1
    if isinstance(distance, bool) or not isinstance(distance, (int, np.integer)) or not low <= int(distance) <= EXPAND_MAX_DISTANCE:
        raise ValueError(f"{what} must be an integer from {low} to {EXPAND_MAX_DISTANCE} pixels, got {distance!r}")
    return int(distance)


def expand_labels(mask: torch.Tensor, distance: int, want_dist2: bool = False, ws: Optional[torch.Tensor] = None):
    """Grows the labels of an (H, W) int32 device mask by ``distance`` pixels, what skimage.segmentation.expand_labels does: a pixel <= 0 within
    Euclidean distance ``distance`` of a labelled pixel (> 0) takes the label of the nearest one -- the smallest label among those at exactly the
    smallest squared distance, not the one a scan meets first -- and every other pixel keeps its value.  Returns the grown mask, a new device
    tensor, and with ``want_dist2`` also the (H, W) int32 squared distance to that pixel: 0 on a labelled pixel, -1 where nothing was in reach
    (include/ribca_hip.h states the contract).  Does not synchronise."""
    if not torch.is_tensor(mask) or mask.dtype != torch.int32 or mask.dim() != 2 or not mask.is_cuda:
        raise ValueError("expand_labels takes an (H, W) int32 device mask")
    d = check_expand_distance(distance)
    mask = mask.contiguous()
    h, w = mask.shape
    dev = mask.device
    out = torch.empty_like(mask)
    dist2 = torch.empty_like(mask) if want_dist2 else None
    ws = _ws(ws, expand_labels_ws_bytes(h, w, d), dev, "expand_labels")
    check(lib().ribca_expand_labels(ptr(mask), h, w, d, ptr(out), ptr(dist2), ptr(ws), ws.numel(), stream_ptr()), "ribca_expand_labels")
    return (out, dist2) if want_dist2 else out


COMPONENTS_TILE = 32              # csrc/components.hip CC_TILE


def mask_components_ws_bytes(h: int, w: int) -> int:
    return int(lib().ribca_mask_components_ws_bytes(int(h), int(w)))


def _device_mask(mask, who: str) -> torch.Tensor:
    if not torch.is_tensor(mask) or mask.dtype != torch.int32 or mask.dim() != 2 or not mask.is_cuda or mask.numel() == 0:
        raise ValueError(f"{who} takes a non-empty (H, W) int32 device mask")
    return mask.contiguous()


def mask_components(mask: torch.Tensor, ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The connected components of an (H, W) int32 device mask: pixels of one label > 0 at 8-connectivity, the pixels <= 0 (the background) at
    4-connectivity.  Returns ``root`` (H, W) int32, for every pixel the raster index of the first pixel of its component, and ``stats``
    (H W, 4) int32, at the row of every root the component's area, whether it touches the image border, and the smallest and largest label > 0
    that is 4-adjacent to it (0, 0 without one); every other row is 0 (include/ribca_hip.h states the contract).  Does not synchronise."""
    mask = _device_mask(mask, "mask_components")
    h, w = mask.shape
    root = torch.empty_like(mask)
    stats = torch.empty((h * w, 4), dtype=torch.int32, device=mask.device)
    ws = _ws(ws, mask_components_ws_bytes(h, w), mask.device, "mask_components")
    check(lib().ribca_mask_components(ptr(mask), h, w, ptr(root), ptr(stats), ptr(ws), ws.numel(), stream_ptr()), "ribca_mask_components")
    return root, stats


def relabel(root: torch.Tensor, new_label: torch.Tensor) -> torch.Tensor:
    """``new_label[root]`` as a new (H, W) int32 device tensor: ``root`` as mask_components gives it, ``new_label`` H W int32 values on the
    device, read at the raster index of every component's first pixel.  Does not synchronise."""
    root = _device_mask(root, "relabel")
    h, w = root.shape
    if not torch.is_tensor(new_label) or new_label.dtype != torch.int32 or new_label.numel() != h * w or new_label.device != root.device:
        raise ValueError("relabel takes one int32 label per pixel of root, on its device")
    new_label = new_label.contiguous()
    out = torch.empty_like(root)
    check(lib().ribca_mask_relabel(ptr(root), ptr(new_label), h, w, ptr(out), stream_ptr()), "ribca_mask_relabel")
    return out


def _component_rows(mask: torch.Tensor, root: torch.Tensor, stats: torch.Tensor):
    """the compacted rows of mask_components on the host: (index of the roots on the device, roots, the mask's value there, stats rows), ascending"""
    idx = torch.nonzero(stats[:, 0] > 0).reshape(-1)
    roots = idx.cpu().numpy().astype(np.int64)
    labels = mask.reshape(-1).index_select(0, idx).cpu().numpy().astype(np.int64)
    rows = stats.index_select(0, idx).cpu().numpy().astype(np.int64)
    return idx, roots, labels, rows


def repair_labels(mask: torch.Tensor, min_area: int):
    """Repairs an (H, W) int32 device mask by the rules of repair.py: of the pieces of a torn label the largest keeps the label and the others
    become labels of their own above the largest one, pieces of fewer than ``min_area`` pixels become background, and holes -- enclosed background
    bordered by one label -- are filled.  Two runs of mask_components with the decisions taken on the host over the component rows between
    them.  Returns (the repaired mask, a new device tensor whose background is 0; the (n, 7) int64 component rows in the order of
    repair.COLUMNS, one per foreground component of the mask as read; the record of repair.stats, its ``repair_ms`` left at 0 for the caller's clock).  Synchronises."""
    from . import repair
    mask = _device_mask(mask, "repair_labels")
    a = repair.check_min_area(min_area)
    h, w = mask.shape
    dev = mask.device
    root, stats = mask_components(mask)
    idx, roots, labels, rows = _component_rows(mask, root, stats)
    fg = labels > 0
    action, new_id = repair.decide(roots[fg], labels[fg], rows[fg, 0], a)
    new = np.zeros(len(roots), dtype=np.int32)
    new[fg] = new_id
    table = torch.zeros(h * w, dtype=torch.int32, device=dev)
    table[idx] = torch.from_numpy(new).to(dev)
    mid = relabel(root, table)
    root2, stats2 = mask_components(mid)
    idx2, _, labels2, rows2 = _component_rows(mid, root2, stats2)
    new2, hole, left = repair.fill(labels2, rows2[:, 1], rows2[:, 2], rows2[:, 3])
    table.zero_()
    table[idx2] = torch.from_numpy(new2.astype(np.int32)).to(dev)
    out = relabel(root2, table)
    comps = repair.rows(roots[fg], labels[fg], rows[fg, 0], action, new_id, w, new2[hole], rows2[hole, 0])
    record = repair.stats(comps, a, int(hole.sum()), int(rows2[hole, 0].sum()), int(left.sum()))
    return out, comps, record


OUTLINES_TILE = 32                # csrc/outlines.hip OL_TILE
OUTLINES_SPARE_ROWS = 1024        # rows of the first attempt beyond two per cell
RING_COLUMNS = ("cell", "start", "vertices", "edges", "area2", "saddles")


def mask_rings_ws_bytes(h: int, w: int, n: int) -> int:
    return int(lib().ribca_mask_rings_ws_bytes(int(h), int(w), int(n)))


def mask_rings(mask: torch.Tensor, ids: np.ndarray, ws: Optional[torch.Tensor] = None, first_cap: Optional[int] = None) -> Dict[str, np.ndarray]:
    """The outlines of the cells ``ids`` (ascending mask labels, cell i = ids[i]; the label -> cell table is built as ``contact_graph`` builds
    it, label 0 never a cell) of an (H, W) int32 device mask as closed rings of lattice vertices, traced on the GPU (csrc/outlines.hip;
    include/ribca_hip.h states the lattice, the saddle rule and the ring row).  Returns host arrays: ``rings`` (R, 6) int64 -- cell, start,
    vertices, edges, area2, saddles (RING_COLUMNS) -- sorted by (cell, start); ``first`` (R + 1) int64, the prefix sum of the vertex counts;
    ``vertices`` (first[R], 2) int32 = [r, c], the vertices of ring k at which the direction changes from first[k] on, the start first, in the
    order of the ring (exterior rings clockwise on the screen, holes counter-clockwise); and ``calls``, how often ribca_mask_rings ran: once
    with room for ``first_cap`` rings (None: 2 n + 1024), a second time with the exact number when the mask has more.  RibcaError when a ring the first kernel reported
    does not trace again.  Synchronises."""
    mask = _device_mask(mask, "mask_rings")
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    n = len(ids)
    empty = {"rings": np.zeros((0, 6), np.int64), "first": np.zeros(1, np.int64), "vertices": np.zeros((0, 2), np.int32), "calls": 0}
    if n == 0:
        return empty
    dev = mask.device
    h, w = mask.shape
    tab_d = _cell_table(ids, dev)
    ws = _ws(ws, mask_rings_ws_bytes(h, w, n), dev, "mask_rings")
    total = torch.empty(1, dtype=torch.int64, device=dev)
    cap, calls = (2 * n + OUTLINES_SPARE_ROWS if first_cap is None else max(int(first_cap), 1)), 0
    while True:
        rings = torch.empty((cap, 6), dtype=torch.int64, device=dev)
        check(lib().ribca_mask_rings(ptr(mask), h, w, ptr(tab_d), tab_d.numel(), n, cap, ptr(rings), ptr(total), ptr(ws), ws.numel(), stream_ptr()),
              "ribca_mask_rings")
        calls += 1
        found = int(total.item())
        if found <= cap:
            break
        if calls == 2:
            raise _lib.RibcaError(f"ribca_mask_rings: {found} rings after a call that counted {cap}")
        cap = found
    if found == 0:
        empty["calls"] = calls
        return empty
    rings = rings[:found]
    order = torch.argsort(rings[:, 0] * ((h + 1) * (w + 1)) + rings[:, 1])      # (cell, start): no two rings of a cell share a start
    rings = rings.index_select(0, order).contiguous()
    first = torch.zeros(found + 1, dtype=torch.int64, device=dev)
    first[1:] = torch.cumsum(rings[:, 2], 0)
    vertices = torch.empty((int(first[-1].item()), 2), dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().ribca_mask_ring_vertices(ptr(mask), h, w, ptr(tab_d), tab_d.numel(), n, ptr(rings), found, ptr(first), ptr(vertices), ptr(bad),
                                         stream_ptr()), "ribca_mask_ring_vertices")
    if int(bad.item()) != 0:
        raise _lib.RibcaError(f"ribca_mask_ring_vertices: {int(bad.item())} of {found} rings did not trace again")
    return {"rings": rings.cpu().numpy(), "first": first.cpu().numpy(), "vertices": vertices.cpu().numpy(), "calls": calls}


OVERLAP_FIRST_SLOTS = 8           # a cell overlaps one or two objects of a second segmentation of the same image


def mask_overlap_ws_bytes(h: int, w: int, n: int, slots: int) -> int:
    return int(lib().ribca_mask_overlap_ws_bytes(int(h), int(w), int(n), int(slots)))


def _two_masks(mask_a, mask_b, who: str):
    if (not torch.is_tensor(mask_a) or not torch.is_tensor(mask_b) or mask_a.dtype != torch.int32 or mask_b.dtype != torch.int32 or mask_a.dim() != 2
            or not mask_a.is_cuda or mask_b.device != mask_a.device or tuple(mask_b.shape) != tuple(mask_a.shape)):
        raise ValueError(f"{who} takes two (H, W) int32 masks of one shape on one device")
    a = mask_a.contiguous()
    return a, (a if mask_b is mask_a else mask_b.contiguous())


def _table_arg(table, device, who: str) -> torch.Tensor:
    if not torch.is_tensor(table) or table.dtype != torch.int32 or table.dim() != 1:
        raise ValueError(f"{who} takes (L) int32 label tables")
    return table.contiguous().to(device)


def mask_overlap(mask_a: torch.Tensor, tab_a: torch.Tensor, n: int, mask_b: torch.Tensor, tab_b: torch.Tensor, m: int, slots: int,
                 ws: Optional[torch.Tensor] = None):
    """(partner (n, slots) int32, inter (n, slots) int64, degree (n) int32, area_a (n) int32, area_b (m) int32, over (2) int32) device tensors of
    ribca_mask_overlap, one attempt at ``slots`` slots per row: with over[0] == 0 row i lists the objects of ``mask_b`` that share pixels with
    cell i of ``mask_a`` in ascending index order and the shared pixels beside them; ``tab_a`` maps the labels of ``mask_a`` to the cells
    0 .. n - 1 and ``tab_b`` those of ``mask_b`` to the objects 0 .. m - 1; include/ribca_hip.h states the contract."""
    mask_a, mask_b = _two_masks(mask_a, mask_b, "mask_overlap")
    dev = mask_a.device
    tab_a, tab_b = _table_arg(tab_a, dev, "mask_overlap"), _table_arg(tab_b, dev, "mask_overlap")
    h, w = mask_a.shape
    rows, objs, cols = max(int(n), 0), max(int(m), 0), max(int(slots), 0)
    partner = torch.empty((rows, cols), dtype=torch.int32, device=dev)
    inter = torch.empty((rows, cols), dtype=torch.int64, device=dev)
    degree = torch.empty((rows,), dtype=torch.int32, device=dev)
    area_a = torch.empty((rows,), dtype=torch.int32, device=dev)
    area_b = torch.empty((objs,), dtype=torch.int32, device=dev)
    over = torch.empty((2,), dtype=torch.int32, device=dev)
    ws = _ws(ws, mask_overlap_ws_bytes(h, w, n, slots), dev, "mask_overlap")
    check(lib().ribca_mask_overlap(ptr(mask_a), ptr(mask_b), h, w, ptr(tab_a), tab_a.numel(), int(n), ptr(tab_b), tab_b.numel(), int(m), int(slots),
                                   ptr(partner), ptr(inter), ptr(degree), ptr(area_a), ptr(area_b), ptr(over), ptr(ws), ws.numel(), stream_ptr()),
          "ribca_mask_overlap")
    return partner, inter, degree, area_a, area_b, over


def _label_areas(mask: torch.Tensor, ids: np.ndarray) -> np.ndarray:
    """the pixels of every label of ``ids`` in the mask, for the side of overlap_pairs that has a partner mask without a single object"""
    tables = _label_tables(mask) if len(ids) else None
    if tables is None:
        return np.zeros(len(ids), np.int32)
    count = tables[0][4].cpu().numpy()
    inside = ids < len(count)
    out = np.zeros(len(ids), np.int32)
    out[inside] = count[ids[inside]]
    return out


def overlap_pairs(mask_a: torch.Tensor, ids_a, mask_b: torch.Tensor, ids_b, first_slots: int = OVERLAP_FIRST_SLOTS) -> Dict[str, np.ndarray]:
    """The pixels every (cell, object) pair of two (H, W) int32 device masks shares: the cells are the labels ``ids_a`` of ``mask_a`` (ascending,
    cell i = ids_a[i]), the objects the labels ``ids_b`` of ``mask_b``; both label -> index tables are built as ``contact_graph`` builds its one,
    label 0 never a cell or an object.  Returns host arrays: ``cell``, ``obj`` int32 and ``inter`` int64, one entry per pair that shares a pixel,
    sorted by (cell, obj); ``degree`` (n) int32, the objects a cell overlaps; ``area_a`` (n) and ``area_b`` (m) int32; and ``slots``, the row
    length that fitted.  The table starts at ``first_slots`` slots per cell and doubles while a row overflows; ValueError when that would pass
    1024 slots or 2 GiB -- a background region labelled as a cell is the usual cause, and the message names its mask label.  Without cells or
    without objects there are no pairs and ribca_mask_overlap is not called: the areas of the other side come from the label table."""
    mask_a, mask_b = _two_masks(mask_a, mask_b, "overlap_pairs")
    ids_a, ids_b = np.asarray(ids_a, dtype=np.int64).reshape(-1), np.asarray(ids_b, dtype=np.int64).reshape(-1)
    n, m = len(ids_a), len(ids_b)
    if n == 0 or m == 0:
        return {"cell": np.zeros(0, np.int32), "obj": np.zeros(0, np.int32), "inter": np.zeros(0, np.int64), "degree": np.zeros(n, np.int32),
                "area_a": _label_areas(mask_a, ids_a), "area_b": _label_areas(mask_b, ids_b), "slots": int(first_slots)}
    dev = mask_a.device
    tab_a, tab_b = _cell_table(ids_a, dev), _cell_table(ids_b, dev)
    slots = int(first_slots)
    while True:
        partner, inter, degree, area_a, area_b, over = mask_overlap(mask_a, tab_a, n, mask_b, tab_b, m, slots)
        failed, lowest = over.tolist()
        if failed == 0:
            break
        why = (f"overlap_pairs: {failed} cell(s) overlap more than {slots} objects of the second mask, the lowest of them mask label "
               f"{int(ids_a[lowest])}; a background region labelled as a cell is the usual cause")
        if slots * 2 > CONTACT_MAX_SLOTS:
            raise ValueError(f"{why} (the table stops at {CONTACT_MAX_SLOTS} slots per cell)")
        if 12 * n * slots * 2 > CONTACT_MAX_TABLE_BYTES:
            raise ValueError(f"{why} (a table of {slots * 2} slots for {n} cells would pass 2 GiB)")
        slots *= 2
    part_h, inter_h, deg_h = partner.cpu().numpy(), inter.cpu().numpy(), degree.cpu().numpy()
    keep = np.arange(slots)[None, :] < deg_h[:, None]      # row-major: sorted by (cell, obj)
    return {"cell": np.repeat(np.arange(n, dtype=np.int32), deg_h), "obj": np.ascontiguousarray(part_h[keep], dtype=np.int32),
            "inter": np.ascontiguousarray(inter_h[keep], dtype=np.int64), "degree": deg_h.astype(np.int32),
            "area_a": area_a.cpu().numpy().astype(np.int32), "area_b": area_b.cpu().numpy().astype(np.int32), "slots": slots}


def mask_compartments(mask_a: torch.Tensor, ids_a, mask_b: torch.Tensor, ids_b, owner) -> Tuple[torch.Tensor, torch.Tensor]:
    """``mask_a`` split by the objects of ``mask_b`` its cells own: ``owner`` (m) holds for every object of ``ids_b`` the index of its cell in
    ``ids_a`` or -1.  Returns two new (H, W) int32 device tensors: ``inner`` keeps the label of ``mask_a`` on the pixels of a cell that lie in
    an object the cell owns, ``outer`` on the other pixels of a cell; both are 0 elsewhere (include/ribca_hip.h states the contract).  Without
    cells both are 0; without objects ``outer`` is the cells of ``mask_a``.  Does not synchronise."""
    mask_a, mask_b = _two_masks(mask_a, mask_b, "mask_compartments")
    ids_a, ids_b = np.asarray(ids_a, dtype=np.int64).reshape(-1), np.asarray(ids_b, dtype=np.int64).reshape(-1)
    owner = np.ascontiguousarray(np.asarray(owner, dtype=np.int32).reshape(-1))
    n, m = len(ids_a), len(ids_b)
    if len(owner) != m:
        raise ValueError(f"mask_compartments takes one owner per object, got {len(owner)} for {m} objects")
    dev = mask_a.device
    h, w = mask_a.shape
    tab_a = _cell_table(ids_a, dev)
    if n == 0 or m == 0:      # no object owns anything: the kernel's answer with one object that is nobody's
        tab_b, owner, m = torch.full((1,), -1, dtype=torch.int32, device=dev), np.full(1, -1, np.int32), 1
        n = max(n, 1)          # tab_a of no cells is one entry of -1: no pixel is a cell
    else:
        tab_b = _cell_table(ids_b, dev)
    owner_d = torch.from_numpy(owner).to(dev)
    inner, outer = torch.empty_like(mask_a), torch.empty_like(mask_a)
    check(lib().ribca_mask_compartments(ptr(mask_a), ptr(mask_b), h, w, ptr(tab_a), tab_a.numel(), n, ptr(tab_b), tab_b.numel(), m, ptr(owner_d),
                                        ptr(inner), ptr(outer), stream_ptr()), "ribca_mask_compartments")
    return inner, outer


INTENSITY_SMALL_BOX = 1024       # csrc/intensities.hip IN_SMALL_BOX: a clipped box of at most this many pixels is one wave's
INTENSITY_RESIDENT = 4096         # csrc/intensities.hip IN_RESIDENT: in a larger box, a cell of more pixels takes the streaming form
INTENSITY_MAX_CHANNELS = 64
INTENSITY_MAX_QUANTILES = 8


def cell_intensities(image: torch.Tensor, mask: torch.Tensor, ids, bbox, q_num: Sequence[int] = (0, 1, 2, 3, 4), q_den: int = 4,
                     out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """Per cell and channel the exact sums and order statistics over the cell's own pixels: ``image`` (C, H, W) fp32 and ``mask`` (H, W) int32 on
    the device, ``ids`` (n) the mask label of every cell and ``bbox`` (n, 4) its box ``rmin, rmax, cmin, cmax`` (inclusive; host arrays or
    device tensors, e.g. ImageProcessor.cell_ids_dev / cell_bbox_dev).  Returns host arrays ``area`` (n) int32, ``sums`` (n, C, 2) fp64
    ``[sum, ssd]`` and ``order`` (n, C, Q, 2) fp32, the order statistics that bracket the quantiles ``q_num[k] / q_den`` (include/ribca_hip.h
    states the summation order and the ranks; intensities.features turns them into the table).  ``out``: device tensors to fill instead
    (returned as they are, no copy back, no synchronise)."""
    assert image.is_cuda and image.dtype == torch.float32 and image.dim() == 3
    assert mask.is_cuda and mask.dtype == torch.int32 and mask.dim() == 2 and tuple(mask.shape) == tuple(image.shape[1:])
    dev = image.device
    q = np.ascontiguousarray(np.asarray(q_num, dtype=np.int32).reshape(-1))
    c, h, w = (int(v) for v in image.shape)
    ids_d = ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1)))
    bbox_d = bbox if torch.is_tensor(bbox) else torch.from_numpy(np.ascontiguousarray(np.asarray(bbox, dtype=np.int32).reshape(-1, 4)))
    ids_d = ids_d.to(device=dev, dtype=torch.int32).contiguous()
    bbox_d = bbox_d.to(device=dev, dtype=torch.int32).contiguous()
    n = ids_d.numel()
    if tuple(bbox_d.shape) != (n, 4):
        raise ValueError(f"cell_intensities takes one box rmin, rmax, cmin, cmax per cell, got {tuple(bbox_d.shape)} for {n} cells")
    if out is None:
        area = torch.empty((n,), dtype=torch.int32, device=dev)
        sums = torch.empty((n, c, 2), dtype=torch.float64, device=dev)
        order = torch.empty((n, c, len(q), 2), dtype=torch.float32, device=dev)
    else:
        area, sums, order = out
        assert area.is_contiguous() and sums.is_contiguous() and order.is_contiguous()
        assert area.dtype == torch.int32 and sums.dtype == torch.float64 and order.dtype == torch.float32
        assert area.numel() == n and sums.numel() == n * c * 2 and order.numel() == n * c * len(q) * 2
    if n:
        check(lib().ribca_cell_intensities(ptr(image.contiguous()), c, h, w, ptr(mask.contiguous()), ptr(ids_d), ptr(bbox_d), n,
                                           q.ctypes.data_as(ctypes.c_void_p), len(q), int(q_den), ptr(area), ptr(sums), ptr(order), stream_ptr()),
              "ribca_cell_intensities")
    if out is not None:
        return out
    return area.cpu().numpy(), sums.cpu().numpy(), order.cpu().numpy()


DEPTH_MAX_DISTANCE = 32           # csrc/localization.hip LO_D_MAX: the largest halo of a pixel tile
DEPTH_TILE = 32                   # csrc/localization.hip LO_TILE
SHELLS_MAX = 8                    # csrc/localization.hip LO_S_MAX: the accumulators a partial's owner keeps in registers


def mask_depth_ws_bytes(h: int, w: int, distance: int) -> int:
    return int(lib().ribca_mask_depth_ws_bytes(int(h), int(w), int(distance)))


def mask_depth(mask: torch.Tensor, distance: int, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The depth of every labelled pixel of an (H, W) int32 device mask below the edge of its own cell: the squared Euclidean distance to the
    nearest pixel inside the image that carries another value -- background or another cell --, -1 where that is more than ``distance`` pixels
    away, 0 on the background (<= 0).  A cell cut by the image border is measured from its visible edge only (include/ribca_hip.h states the
    contract).  Returns a new (H, W) int32 device tensor.  Does not synchronise."""
    if not torch.is_tensor(mask) or mask.dtype != torch.int32 or mask.dim() != 2 or not mask.is_cuda:
        raise ValueError("mask_depth takes an (H, W) int32 device mask")
    if isinstance(distance, bool) or not isinstance(distance, (int, np.integer)) or not 1 <= int(distance) <= DEPTH_MAX_DISTANCE:
        raise ValueError(f"distance must be an integer from 1 to {DEPTH_MAX_DISTANCE} pixels, got {distance!r}")
    d = int(distance)
    mask = mask.contiguous()
    h, w = mask.shape
    depth2 = torch.empty_like(mask)
    ws = _ws(ws, mask_depth_ws_bytes(h, w, d), mask.device, "mask_depth")
    check(lib().ribca_mask_depth(ptr(mask), h, w, d, ptr(depth2), ptr(ws), ws.numel(), stream_ptr()), "ribca_mask_depth")
    return depth2


def cell_shell_sums(image: torch.Tensor, mask: torch.Tensor, depth2: torch.Tensor, ids, bbox, edges2: Sequence[int],
                    out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """Per cell the pixels, and per cell and channel the exact fp64 sum, of every depth shell: ``image`` (C, H, W) fp32, ``mask`` and ``depth2``
    (H, W) int32 on the device (``depth2`` from ``mask_depth``), ``ids`` (n) and ``bbox`` (n, 4) as for ``cell_intensities``, ``edges2`` the
    S - 1 strictly increasing positive squared shell edges (2 <= S <= SHELLS_MAX).  A pixel is in shell #{j : depth2 > edges2[j]}, in the last
    one when its depth2 is -1.  Returns host arrays ``count`` (n, S) int32, ``deepest`` (n) int32 -- the largest depth2 of the cell, -1 when
    one of its pixels is -1, 0 for a cell without a pixel -- and ``sums`` (n, C, S) fp64 (include/ribca_hip.h states the summation order;
    localization.features turns them into the table).  ``out``: device tensors to fill instead (returned as they are, no copy back, no
    synchronise)."""
    assert image.is_cuda and image.dtype == torch.float32 and image.dim() == 3
    assert mask.is_cuda and mask.dtype == torch.int32 and mask.dim() == 2 and tuple(mask.shape) == tuple(image.shape[1:])
    assert depth2.is_cuda and depth2.dtype == torch.int32 and tuple(depth2.shape) == tuple(mask.shape)
    dev = image.device
    e2 = np.ascontiguousarray(np.asarray(edges2, dtype=np.int32).reshape(-1))
    s = len(e2) + 1
    c, h, w = (int(v) for v in image.shape)
    ids_d = ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1)))
    bbox_d = bbox if torch.is_tensor(bbox) else torch.from_numpy(np.ascontiguousarray(np.asarray(bbox, dtype=np.int32).reshape(-1, 4)))
    ids_d = ids_d.to(device=dev, dtype=torch.int32).contiguous()
    bbox_d = bbox_d.to(device=dev, dtype=torch.int32).contiguous()
    n = ids_d.numel()
    if tuple(bbox_d.shape) != (n, 4):
        raise ValueError(f"cell_shell_sums takes one box rmin, rmax, cmin, cmax per cell, got {tuple(bbox_d.shape)} for {n} cells")
    if out is None:
        count = torch.empty((n, s), dtype=torch.int32, device=dev)
        deepest = torch.empty((n,), dtype=torch.int32, device=dev)
        sums = torch.empty((n, c, s), dtype=torch.float64, device=dev)
    else:
        count, deepest, sums = out
        assert count.is_contiguous() and deepest.is_contiguous() and sums.is_contiguous()
        assert count.dtype == torch.int32 and deepest.dtype == torch.int32 and sums.dtype == torch.float64
        assert count.numel() == n * s and deepest.numel() == n and sums.numel() == n * c * s
    if n:
        check(lib().ribca_cell_shell_sums(ptr(image.contiguous()), c, h, w, ptr(mask.contiguous()), ptr(depth2.contiguous()), ptr(ids_d), ptr(bbox_d), n,
                                          e2.ctypes.data_as(ctypes.c_void_p), s, ptr(count), ptr(deepest), ptr(sums), stream_ptr()),
              "ribca_cell_shell_sums")
    if out is not None:
        return out
    return count.cpu().numpy(), deepest.cpu().numpy(), sums.cpu().numpy()


COLOC_RESIDENT = 4096             # csrc/colocalization.hip CO_RESIDENT: a cell of more pixels takes the streaming form
COLOC_MAX_MARKERS = 32            # csrc/colocalization.hip CO_K_MAX: a gate word is 32 bits
COLOC_CHUNK_BYTES = 1 << 30       # the device outputs of one launch of cell_coloc stay within this; more cells go in consecutive chunks


def cell_coloc(image: torch.Tensor, mask: torch.Tensor, ids, bbox, chan: Sequence[int], thr: Sequence[float],
               out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """Per cell the second-order sums of K selected channels over the cell's own pixels: ``image`` (C, H, W) fp32 and ``mask`` (H, W) int32 on
    the device, ``ids`` (n) and ``bbox`` (n, 4) as for ``cell_intensities`` (host arrays or device tensors), ``chan`` K distinct channel indices
    (2 <= K <= COLOC_MAX_MARKERS, any order) and ``thr`` one finite gate per selected channel on the image's own scale (a pixel is above its
    gate when ``value > thr``, strictly).  Returns host arrays ``area`` (n) int32, ``both`` (n, P) int32 -- the pixels above both gates of every
    pair (k, l), k <= l, in the order (0,0), (0,1) .. (0,K-1), (1,1) .., P = K (K + 1) / 2 of them --, ``sums`` (n, K) fp64, ``cross`` (n, P) fp64 -- the centred cross products -- and
    ``gated`` (n, K, K) fp64 -- ``gated[:, k, l]`` the sum of channel k over the pixels where channel l is above its gate (include/ribca_hip.h
    states the summation order; colocalization.features turns them into the coefficients).  The cells go in consecutive chunks whose device
    outputs stay within COLOC_CHUNK_BYTES; every cell is worked alone, so the result does not depend on the chunking.  ``out``: device tensors
    to fill instead (returned as they are, no copy back, no synchronise)."""
    assert image.is_cuda and image.dtype == torch.float32 and image.dim() == 3
    assert mask.is_cuda and mask.dtype == torch.int32 and mask.dim() == 2 and tuple(mask.shape) == tuple(image.shape[1:])
    dev = image.device
    ch = np.ascontiguousarray(np.asarray(chan, dtype=np.int32).reshape(-1))
    gates = np.ascontiguousarray(np.asarray(thr, dtype=np.float32).reshape(-1))
    k = len(ch)
    if len(gates) != k:
        raise ValueError(f"cell_coloc takes one gate per selected channel, got {len(gates)} for {k} channels")
    p = k * (k + 1) // 2
    c, h, w = (int(v) for v in image.shape)
    ids_d = ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1)))
    bbox_d = bbox if torch.is_tensor(bbox) else torch.from_numpy(np.ascontiguousarray(np.asarray(bbox, dtype=np.int32).reshape(-1, 4)))
    ids_d = ids_d.to(device=dev, dtype=torch.int32).contiguous()
    bbox_d = bbox_d.to(device=dev, dtype=torch.int32).contiguous()
    n = ids_d.numel()
    if tuple(bbox_d.shape) != (n, 4):
        raise ValueError(f"cell_coloc takes one box rmin, rmax, cmin, cmax per cell, got {tuple(bbox_d.shape)} for {n} cells")
    image, mask = image.contiguous(), mask.contiguous()
    per_cell = 4 + 4 * p + 8 * k + 8 * p + 8 * k * k      # bytes of the five outputs
    step = max(1, COLOC_CHUNK_BYTES // per_cell)

    def launch(lo, hi, area, both, sums, cross, gated):
        check(lib().ribca_cell_coloc(ptr(image), c, h, w, ptr(mask), ptr(ids_d[lo:hi]), ptr(bbox_d[lo:hi]), hi - lo,
                                     ch.ctypes.data_as(ctypes.c_void_p), gates.ctypes.data_as(ctypes.c_void_p), k, ptr(area), ptr(both), ptr(sums),
                                     ptr(cross), ptr(gated), stream_ptr()), "ribca_cell_coloc")

    if out is not None:
        area, both, sums, cross, gated = out
        assert all(x.is_cuda and x.is_contiguous() for x in out)
        assert area.dtype == torch.int32 and both.dtype == torch.int32 and all(x.dtype == torch.float64 for x in (sums, cross, gated))
        assert area.numel() == n and both.numel() == n * p and sums.numel() == n * k and cross.numel() == n * p and gated.numel() == n * k * k
        both2, sums2, cross2, gated2 = both.view(n, p), sums.view(n, k), cross.view(n, p), gated.view(n, k * k)
        for lo in range(0, n, step):      # the caller's tensors hold every cell: a chunk is a slice of rows of each
            hi = min(lo + step, n)
            launch(lo, hi, area.view(n)[lo:hi], both2[lo:hi], sums2[lo:hi], cross2[lo:hi], gated2[lo:hi])
        return out
    host = (np.empty((n,), np.int32), np.empty((n, p), np.int32), np.empty((n, k), np.float64), np.empty((n, p), np.float64),
            np.empty((n, k, k), np.float64))
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        m = hi - lo
        dev_out = (torch.empty((m,), dtype=torch.int32, device=dev), torch.empty((m, p), dtype=torch.int32, device=dev),
                   torch.empty((m, k), dtype=torch.float64, device=dev), torch.empty((m, p), dtype=torch.float64, device=dev),
                   torch.empty((m, k, k), dtype=torch.float64, device=dev))
        launch(lo, hi, *dev_out)
        for dst, src in zip(host, dev_out):
            dst[lo:hi] = src.cpu().numpy()
    return host


AUTOCORR_MAX_CHANNELS = 64      # csrc/autocorr.hip
AUTOCORR_MAX_NEIGHBOURS = 31


def autocorr_observed_ws_bytes(n: int, c: int) -> int:
    return int(lib().ribca_autocorr_observed_ws_bytes(int(n), int(c)))


def autocorr_perm_ws_bytes(n: int, c: int, n_perms: int) -> int:
    return int(lib().ribca_autocorr_perm_ws_bytes(int(n), int(c), int(n_perms)))


def _autocorr_args(what: str, z: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if z.dtype != torch.float64 or z.dim() != 2 or idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != z.shape[0]:
        raise ValueError(f"{what} takes an (n, C) float64 table of centred values and an (n, m) int32 neighbour list")
    if idx.device != z.device:
        raise ValueError(f"{what}: the table and the neighbour list must be on the same device")
    if not bool(torch.isfinite(z).all()):
        raise ValueError(f"{what}: the table holds values that are not finite")
    return z.contiguous(), idx.contiguous()


def autocorr_observed(z: torch.Tensor, idx: torch.Tensor, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(2, C) fp64 device tensor: the numerators of Moran's I (row 0: the sum over the cells of z[i] times the sum of its neighbours' z) and of
    Geary's C (row 1: the sum of the squared differences to the neighbours) of every column of the (n, C) fp64 device table ``z`` of CENTRED
    values over the fixed (n, m) int32 device neighbour list ``idx``.  A pure function of its inputs: include/ribca_hip.h states the order of
    every addition.  Values that are not finite raise before any launch."""
    z, idx = _autocorr_args("autocorr_observed", z, idx)
    n, c = z.shape
    out = torch.empty((2, c), dtype=torch.float64, device=z.device)
    ws = _ws(ws, autocorr_observed_ws_bytes(n, c), z.device, "autocorr_observed")
    check(lib().ribca_autocorr_observed(ptr(z), ptr(idx), n, c, idx.shape[1], ptr(out), ptr(ws), ws.numel(), stream_ptr()), "ribca_autocorr_observed")
    return out


def autocorr_perm(z: torch.Tensor, idx: torch.Tensor, seed: int, image: int, p0: int, n_perms: int, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n_perms, 2, C) fp64 device tensor: the numerators of ``autocorr_observed`` under the permutations p0 .. p0 + n_perms - 1 of (seed, image)
    -- cell i carries the whole row z[sigma_p(i)], one bijection for all channels (the sigma of ``nhood_perm_counts``, keyed the same way).
    Slice j depends on (z, idx, seed, image, p0 + j) alone."""
    z, idx = _autocorr_args("autocorr_perm", z, idx)
    n, c = z.shape
    out = torch.empty((max(int(n_perms), 0), 2, c), dtype=torch.float64, device=z.device)
    ws = _ws(ws, autocorr_perm_ws_bytes(n, c, n_perms), z.device, "autocorr_perm")
    check(lib().ribca_autocorr_perm(ptr(z), ptr(idx), n, c, idx.shape[1], _u64(seed), int(image), int(p0), int(n_perms), ptr(out), ptr(ws), ws.numel(),
                                    stream_ptr()), "ribca_autocorr_perm")
    return out


def local_perm_counts_ws_bytes(n: int, c: int, n_perms: int) -> int:
    return int(lib().ribca_local_perm_counts_ws_bytes(int(n), int(c), int(n_perms)))


def local_lag(z: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """(n, C) fp64 device tensor: per cell and channel the sum of the neighbours' values of the (n, C) fp64 device table ``z`` of CENTRED values
    over the (n, m) int32 device neighbour list ``idx``, added in list order (csrc/local_autocorr.hip).  Values that are not finite raise
    before any launch."""
    z, idx = _autocorr_args("local_lag", z, idx)
    n, c = z.shape
    lag = torch.empty((n, c), dtype=torch.float64, device=z.device)
    check(lib().ribca_local_lag(ptr(z), ptr(idx), n, c, idx.shape[1], ptr(lag), stream_ptr()), "ribca_local_lag")
    return lag


def local_perm_counts(z: torch.Tensor, idx: torch.Tensor, lag: torch.Tensor, seed: int, image: int, p0: int, n_perms: int,
                      ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ge, le), two (n, C) int64 device tensors: how many of the conditional permutations p0 .. p0 + n_perms - 1 of (seed, image) -- cell i
    keeps its row, the others move around it with the sigma of ``nhood_perm_counts`` -- give cell i a neighbour sum at or above / at or below
    ``lag`` (the output of ``local_lag``).  Counts of adjoining ranges of permutations add up entry by entry."""
    z, idx = _autocorr_args("local_perm_counts", z, idx)
    n, c = z.shape
    if lag.dtype != torch.float64 or tuple(lag.shape) != (n, c) or lag.device != z.device:
        raise ValueError("local_perm_counts takes the (n, C) float64 lag of local_lag on the device of z")
    lag = lag.contiguous()
    ge = torch.empty((n, c), dtype=torch.int32, device=z.device)      # the library's uint32, widened below: a count may reach 2^31
    le = torch.empty((n, c), dtype=torch.int32, device=z.device)
    ws = _ws(ws, local_perm_counts_ws_bytes(n, c, n_perms), z.device, "local_perm_counts")
    check(lib().ribca_local_perm_counts(ptr(z), ptr(idx), ptr(lag), n, c, idx.shape[1], _u64(seed), int(image), int(p0), int(n_perms), ptr(ge), ptr(le),
                                        ptr(ws), ws.numel(), stream_ptr()), "ribca_local_perm_counts")
    return ge.to(torch.int64) & 0xFFFFFFFF, le.to(torch.int64) & 0xFFFFFFFF


TISSUE_NEIGHBOURHOODS = (10, 20, 30, 50, 75, 100, 150, 200)       # spatial_methods.py:155


def knn_composition_counts(x: np.ndarray, y: np.ndarray, cell_type: np.ndarray, n_types: int, sizes: Sequence[int] = TISSUE_NEIGHBOURHOODS,
                           device=None) -> torch.Tensor:
    """(n, len(sizes), n_types) int16 device tensor: for every cell and every neighbourhood size the number of cells of each type among
    its nearest other cells (every row sums to its size) -- the integers behind ``knn_compositions``, left on the device for the
    tissue-region step (regions.pca_project)."""
    dev = device or _lib.require_gpu()
    n = len(x)
    if max(sizes) + 1 > n:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {max(sizes) + 1}, n_samples_fit = {n}")
    xd, yd, td = _points(x, y, cell_type, dev, "knn_composition_counts")
    sd = torch.tensor(list(sizes), dtype=torch.int32, device=dev)
    counts = torch.empty((n, len(sizes), n_types), dtype=torch.int16, device=dev)
    check(lib().ribca_knn_compositions(ptr(xd), ptr(yd), ptr(td), n, int(n_types), ptr(sd), len(sizes), ptr(counts), stream_ptr()),
          "ribca_knn_compositions")
    return counts


def knn_compositions(x: np.ndarray, y: np.ndarray, cell_type: np.ndarray, n_types: int, sizes: Sequence[int] = TISSUE_NEIGHBOURHOODS,
                     device=None) -> np.ndarray:
    """(n, len(sizes) * n_types) float64: for every cell and every neighbourhood size the fraction of each cell type among its
    nearest other cells -- the ``compositions`` matrix of the reference's tissue_region_partition (spatial_methods.py:158-176).
    The k-NN search and the counting run on the GPU; the division count / size is done here in fp64 as numpy does it there."""
    n = len(x)
    c = knn_composition_counts(x, y, cell_type, n_types, sizes, device).cpu().numpy().astype(np.float64)
    c /= c.sum(axis=2, keepdims=True)
    return c.reshape(n, len(sizes) * n_types)


# ------------------------------------------------------------------------------------------- tissue regions (PCA + k-means, csrc/regions.hip)
def region_gram_ws_bytes(n: int, f: int) -> int:
    return int(lib().ribca_region_gram_ws_bytes(n, f))


def region_gram(counts: torch.Tensor, ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Column sums (F) and Gram matrix (F, F) of the (n, F) int16 device count table, exact int64."""
    counts = counts.contiguous()
    n, f = counts.shape
    colsum = torch.empty(f, dtype=torch.int64, device=counts.device)
    gram = torch.empty((f, f), dtype=torch.int64, device=counts.device)
    ws = _ws(ws, region_gram_ws_bytes(n, f), counts.device, "region_gram")
    check(lib().ribca_region_gram(ptr(counts), n, f, ptr(colsum), ptr(gram), ptr(ws), ws.numel(), stream_ptr()), "ribca_region_gram")
    return colsum, gram


def region_project(counts: torch.Tensor, size_col: torch.Tensor, mean: torch.Tensor, comps: torch.Tensor) -> torch.Tensor:
    """y (n, d) fp64 = (counts / size_col - mean) @ comps.T with every output summed over the columns in ascending order."""
    counts = counts.contiguous()
    n, f = counts.shape
    d = comps.shape[0]
    y = torch.empty((n, d), dtype=torch.float64, device=counts.device)
    check(lib().ribca_region_project(ptr(counts), n, f, ptr(size_col.contiguous()), ptr(mean.contiguous()), ptr(comps.contiguous()), d, ptr(y),
                                     stream_ptr()), "ribca_region_project")
    return y


def kmeans_trials_ws_bytes(n: int, n_cand: int) -> int:
    return int(lib().ribca_kmeans_trials_ws_bytes(n, n_cand))


def kmeans_trials(y: torch.Tensor, cand: torch.Tensor, closest: Optional[torch.Tensor],
                  ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One k-means++ step on y (n, d) fp64: (L, n) min(closest, d2 to candidate row cand[t]) and (L) potentials (fixed-order sums)."""
    n, d = y.shape
    m = int(cand.numel())
    cand_d2 = torch.empty((m, n), dtype=torch.float64, device=y.device)
    pot = torch.empty(m, dtype=torch.float64, device=y.device)
    ws = _ws(ws, kmeans_trials_ws_bytes(n, m), y.device, "kmeans_trials")
    check(lib().ribca_kmeans_trials(ptr(y), n, d, ptr(cand), m, ptr(closest), ptr(cand_d2), ptr(pot), ptr(ws), ws.numel(), stream_ptr()),
          "ribca_kmeans_trials")
    return cand_d2, pot


def kmeans_assign(y: torch.Tensor, centres: torch.Tensor, labels: torch.Tensor, mind2: Optional[torch.Tensor], changed: torch.Tensor) -> None:
    """labels (n) int32 in place: the centre with the least (d2, index); mind2 (n) fp64; changed (1) int32 = labels that moved."""
    n, d = y.shape
    check(lib().ribca_kmeans_assign(ptr(y), n, d, ptr(centres), centres.shape[0], ptr(labels), ptr(mind2), ptr(changed), stream_ptr()),
          "ribca_kmeans_assign")


def kmeans_update_ws_bytes(n: int, d: int, k: int) -> int:
    return int(lib().ribca_kmeans_update_ws_bytes(n, d, k))


def kmeans_update(y: torch.Tensor, labels: torch.Tensor, centres_old: torch.Tensor, centres_new: torch.Tensor, sums: torch.Tensor,
                  counts: torch.Tensor, changed: Optional[torch.Tensor], stat: torch.Tensor, ws: torch.Tensor) -> None:
    """The M step in the fixed summation order (include/ribca_hip.h): sums, counts, centres_new and stat (1 + 2 k) are written."""
    n, d = y.shape
    check(lib().ribca_kmeans_update(ptr(y), n, d, ptr(labels), centres_old.shape[0], ptr(centres_old), ptr(centres_new), ptr(sums), ptr(counts),
                                    ptr(changed), ptr(stat), ptr(ws), ws.numel(), stream_ptr()), "ribca_kmeans_update")


def kmeans_finalize(sums: torch.Tensor, counts: torch.Tensor, centres_old: torch.Tensor, centres_new: torch.Tensor,
                    changed: Optional[torch.Tensor], stat: torch.Tensor) -> None:
    k, d = sums.shape
    check(lib().ribca_kmeans_finalize(ptr(sums), ptr(counts), k, d, ptr(centres_old), ptr(centres_new), ptr(changed), ptr(stat), stream_ptr()),
          "ribca_kmeans_finalize")


def kmeans_relocate(y: torch.Tensor, labels: torch.Tensor, far_rows: torch.Tensor, empty_ids: torch.Tensor, sums: torch.Tensor,
                    counts: torch.Tensor) -> None:
    """scikit-learn's empty-cluster rule on the sums: row far_rows[m] moves from its cluster's sum to empty cluster empty_ids[m]."""
    n, d = y.shape
    check(lib().ribca_kmeans_relocate(ptr(y), n, d, sums.shape[0], ptr(labels), ptr(far_rows), ptr(empty_ids), int(far_rows.numel()), ptr(sums),
                                      ptr(counts), stream_ptr()), "ribca_kmeans_relocate")


# ------------------------------------------------------------------------------------------- umap embedding (extra cell types)
def knn_dense(x: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact k nearest rows of the (n, dim) fp32 device matrix x, the row itself included: (n, k) int32 indices and (n, k) fp32
    Euclidean distances, each row sorted by (distance, index)."""
    x = x.contiguous()
    n, dim = x.shape
    idx = torch.empty((n, k), dtype=torch.int32, device=x.device)
    dist = torch.empty((n, k), dtype=torch.float32, device=x.device)
    check(lib().ribca_knn_dense(ptr(x), n, dim, int(k), ptr(idx), ptr(dist), stream_ptr()), "ribca_knn_dense")
    return idx, dist


def umap_fuzzy_weights(idx: torch.Tensor, dist: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """umap's smooth_knn_dist + compute_membership_strengths over a knn_dense table: sigma (n), rho (n), weights (n, k), fp32."""
    n, k = idx.shape
    sigma = torch.empty(n, dtype=torch.float32, device=idx.device)
    rho = torch.empty(n, dtype=torch.float32, device=idx.device)
    w = torch.empty((n, k), dtype=torch.float32, device=idx.device)
    check(lib().ribca_umap_fuzzy_weights(ptr(idx.contiguous()), ptr(dist.contiguous()), n, k, ptr(sigma), ptr(rho), ptr(w), stream_ptr()),
          "ribca_umap_fuzzy_weights")
    return sigma, rho, w


def umap_optimize_ws_bytes(n: int, dim: int, nnz: int) -> int:
    """workspace of umap_optimize (include/ribca_hip.h): the sampling state of every edge and the positions after an epoch"""
    return int(lib().ribca_umap_optimize_ws_bytes(n, dim, nnz))


def umap_optimize(emb: torch.Tensor, indptr: torch.Tensor, indices: torch.Tensor, rev: torch.Tensor, eps: torch.Tensor, a: float, b: float,
                  n_epochs: int, seed: int, gamma: float = 1.0, alpha0: float = 1.0, neg_rate: float = 5.0,
                  ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """n_epochs of umap's layout SGD on emb (n, dim <= 8) fp32 in place (deterministic Jacobi epochs, hashed negative samples)."""
    n, dim = emb.shape
    nnz = int(indices.numel())
    ws = _ws(ws, umap_optimize_ws_bytes(n, dim, nnz), emb.device, "umap_optimize")
    check(lib().ribca_umap_optimize(ptr(emb), n, dim, ptr(indptr), ptr(indices), ptr(rev), ptr(eps), float(a), float(b), float(gamma),
                                    float(alpha0), float(neg_rate), int(n_epochs), _u64(seed), ptr(ws), ws.numel(), stream_ptr()), "ribca_umap_optimize")
    return emb


# ------------------------------------------------------------------------------------------- spectral start (csrc/spectral.hip)
def _f64(t: torch.Tensor, cols: Optional[int] = None) -> torch.Tensor:
    if t.dtype != torch.float64 or t.dim() != 2 or not t.is_cuda:
        raise ValueError("the spectral primitives take 2-D float64 device tensors")
    if cols is not None and t.shape[1] != cols:
        raise ValueError(f"expected {cols} columns, got {t.shape[1]}")
    return t


def spectral_spmm(indptr: torch.Tensor, indices: torch.Tensor, weights: torch.Tensor, dinv: torch.Tensor, x: torch.Tensor,
                  out: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 0.0, gamma: float = 0.0,
                  z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (n, m) fp64 = alpha (S x) + beta x + gamma z with S = D^-1/2 A D^-1/2 of the symmetric CSR graph (int64 indptr, int32 indices, fp32
    weights, fp64 dinv = 1 / sqrt(degree)); every row one sequential sum in CSR order (include/ribca_hip.h).  out may be z, never x."""
    n, m = _f64(x).shape
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or weights.dtype != torch.float32 or dinv.dtype != torch.float64:
        raise ValueError("spectral_spmm takes int64 indptr, int32 indices, float32 weights and float64 dinv")
    if indptr.numel() != n + 1 or dinv.numel() != n or indices.numel() != weights.numel():
        raise ValueError("spectral_spmm: the graph does not match x")
    if out is None:
        out = torch.empty_like(x)
    if z is not None:
        _f64(z, m)
    if _f64(out, m).shape[0] != n or (z is not None and z.shape[0] != n):
        raise ValueError("spectral_spmm: x, z and out differ in shape")
    check(lib().ribca_spectral_spmm(ptr(indptr), ptr(indices), ptr(weights), int(indices.numel()), ptr(dinv), n, m, ptr(x), float(alpha), float(beta),
                                    float(gamma), ptr(z), ptr(out), stream_ptr()), "ribca_spectral_spmm")
    return out


def spectral_gram_ws_bytes(n: int, p: int, q: int) -> int:
    return int(lib().ribca_spectral_gram_ws_bytes(n, p, q))


def spectral_gram(u: torch.Tensor, v: torch.Tensor, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(p, q) fp64 device tensor u^T v, summed in chunks of 1024 rows in ascending order, then over the chunks in ascending order."""
    n, p = _f64(u).shape
    if _f64(v).shape[0] != n:
        raise ValueError("spectral_gram: u and v differ in rows")
    q = v.shape[1]
    g = torch.empty((p, q), dtype=torch.float64, device=u.device)
    ws = _ws(ws, spectral_gram_ws_bytes(n, p, q), u.device, "spectral_gram")
    check(lib().ribca_spectral_gram(ptr(u), ptr(v), n, p, q, ptr(g), ptr(ws), ws.numel(), stream_ptr()), "ribca_spectral_gram")
    return g


def spectral_combine(u: torch.Tensor, c: torch.Tensor, out: Optional[torch.Tensor] = None, add: bool = False) -> torch.Tensor:
    """out (n, m) = u (n, p) c (p, m), a sequential sum over p; ``add`` starts every sum at out's own value instead of 0."""
    n, p = _f64(u).shape
    m = _f64(c).shape[1]
    if c.shape[0] != p:
        raise ValueError("spectral_combine: u and c do not match")
    if out is None:
        if add:
            raise ValueError("spectral_combine: add needs out")
        out = torch.empty((n, m), dtype=torch.float64, device=u.device)
    if _f64(out, m).shape[0] != n:
        raise ValueError("spectral_combine: out has the wrong shape")
    check(lib().ribca_spectral_combine(ptr(u), n, p, ptr(c), m, 1 if add else 0, ptr(out), stream_ptr()), "ribca_spectral_combine")
    return out


# ------------------------------------------------------------------------------------------- scatter plot (csrc/scatter.hip)
SCATTER_MARGIN = 0.05


def scatter_affine(points: np.ndarray, height: int, width: int, margin: float = SCATTER_MARGIN) -> Tuple[float, float, float, float]:
    """(ax, bx, ay, by) in fp64: column = ax x + bx sends [min x - margin span, max x + margin span] to [0, width - 1], row = ay y + by sends
    the same range of y to [height - 1, 0] (y grows upwards, as in a plot).  A span of 0 counts as 1; non-finite rows are left out."""
    pts = np.asarray(points, dtype=np.float64)
    pts = pts[np.isfinite(pts).all(axis=1)]
    if len(pts) == 0:
        return 1.0, 0.0, -1.0, float(height - 1)
    out = []
    for c, size, flip in ((0, width, False), (1, height, True)):
        lo, hi = float(pts[:, c].min()), float(pts[:, c].max())
        span = hi - lo if hi > lo else 1.0
        lo, hi = lo - margin * span, hi + margin * span
        a = (size - 1) / (hi - lo)
        out += [-a, a * hi] if flip else [a, -a * lo]
    return tuple(out)


def scatter_raster(points: torch.Tensor, rgb: torch.Tensor, height: int, width: int, affine: Sequence[float], radius: int = 2,
                   ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, int]:
    """(height, width, 3) uint8 device image of the (n, 2) fp32 device points as filled discs in their (n, 3) uint8 colours on white, later
    points over earlier ones, and the number of points skipped (centre not finite or off the canvas).  include/ribca_hip.h states the pixels."""
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 2 or rgb.dtype != torch.uint8 or rgb.shape != (points.shape[0], 3):
        raise ValueError("scatter_raster takes (n, 2) float32 points and (n, 3) uint8 colours")
    ax, bx, ay, by = (float(v) for v in affine)
    out = torch.empty((int(height), int(width), 3), dtype=torch.uint8, device=points.device)
    ws = _ws(ws, lib().ribca_scatter_raster_ws_bytes(int(height), int(width)), points.device, "scatter_raster")
    skipped = ctypes.c_int64(0)
    n = points.shape[0]
    check(lib().ribca_scatter_raster(ptr(points) if n else None, ptr(rgb) if n else None, n, ax, bx, ay, by, int(height), int(width), int(radius),
                                     ptr(out), ctypes.byref(skipped), ptr(ws), ws.numel(), stream_ptr()), "ribca_scatter_raster")
    return out, int(skipped.value)


# ------------------------------------------------------------------------------------------- per-cell-type statistics (csrc/celltype_stats.hip)
GROUP_SUM_ROWS = 1024      # R of the summation tree (include/ribca_hip.h; kSumChunk of csrc/ribca_scratch.h)
GROUP_SUM_MAX_COLUMNS = 1024
GROUP_SUM_MAX_GROUPS = 256


def group_sums_ws_bytes(n: int, c: int, groups: int) -> int:
    return int(lib().ribca_group_sums_ws_bytes(int(n), int(c), int(groups)))


def group_sums(x: torch.Tensor, group: torch.Tensor, groups: int, ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """sums (groups, c) fp64 and counts (groups) int64 device tensors of the rows of the (n, c) fp64 device matrix x by their (n) int32 group
    id, and the number of rows whose id lies outside [0, groups) (ignored).  The sums are a pure function of the inputs: include/ribca_hip.h
    states the summation tree."""
    if x.dtype != torch.float64 or x.dim() != 2 or group.dtype != torch.int32 or group.shape != (x.shape[0],):
        raise ValueError("group_sums takes an (n, c) float64 matrix and (n) int32 group ids")
    x, group = x.contiguous(), group.contiguous()
    n, c = x.shape
    sums = torch.empty((max(int(groups), 0), c), dtype=torch.float64, device=x.device)
    counts = torch.empty(max(int(groups), 0), dtype=torch.int64, device=x.device)
    ws = _ws(ws, group_sums_ws_bytes(n, c, groups), x.device, "group_sums")
    skipped = ctypes.c_int64(0)
    check(lib().ribca_group_sums(ptr(x) if n else None, ptr(group) if n else None, n, c, int(groups), ptr(sums), ptr(counts), ctypes.byref(skipped),
                                 ptr(ws), ws.numel(), stream_ptr()), "ribca_group_sums")
    return sums, counts, int(skipped.value)


def heatmap_raster(sums: torch.Tensor, counts: torch.Tensor, lut: torch.Tensor, cell: int, gap: int,
                   ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, float, float]:
    """(T cell, C cell, 3) uint8 device image of the (T, C) table of means sums / counts through the (256, 3) uint8 look-up table, and the
    vmin, vmax of its colour scale (NaN, NaN when every count is 0).  include/ribca_hip.h states the pixels."""
    if sums.dtype != torch.float64 or sums.dim() != 2 or counts.dtype != torch.int64 or counts.shape != (sums.shape[0],) or \
            lut.dtype != torch.uint8 or lut.shape != (256, 3):
        raise ValueError("heatmap_raster takes (T, C) float64 sums, (T) int64 counts and a (256, 3) uint8 table")
    sums, counts, lut = sums.contiguous(), counts.contiguous(), lut.contiguous()
    t, c = sums.shape
    out = torch.empty((t * max(int(cell), 0), c * max(int(cell), 0), 3), dtype=torch.uint8, device=sums.device)
    ws = _ws(ws, lib().ribca_heatmap_raster_ws_bytes(t, c, int(cell), int(gap)), sums.device, "heatmap_raster")
    vmin, vmax = ctypes.c_double(0.0), ctypes.c_double(0.0)
    check(lib().ribca_heatmap_raster(ptr(sums), ptr(counts), t, c, ptr(lut), int(cell), int(gap), ptr(out), ctypes.byref(vmin), ctypes.byref(vmax),
                                     ptr(ws), ws.numel(), stream_ptr()), "ribca_heatmap_raster")
    return out, float(vmin.value), float(vmax.value)


def table_raster(values: torch.Tensor, lut: torch.Tensor, cell: int, gap: int, vmin: float, vmax: float) -> torch.Tensor:
    """(R cell, C cell, 3) uint8 device image of the (R, C) fp64 device table through the (256, 3) uint8 look-up table on the colour scale
    vmin .. vmax the caller gives (values clamped to it, NaN silver, the middle entry when vmin == vmax).  include/ribca_hip.h states the pixels."""
    if values.dtype != torch.float64 or values.dim() != 2 or lut.dtype != torch.uint8 or lut.shape != (256, 3):
        raise ValueError("table_raster takes an (R, C) float64 table and a (256, 3) uint8 table of colours")
    values, lut = values.contiguous(), lut.contiguous()
    r, c = values.shape
    out = torch.empty((r * max(int(cell), 0), c * max(int(cell), 0), 3), dtype=torch.uint8, device=values.device)
    check(lib().ribca_table_raster(ptr(values), r, c, ptr(lut), int(cell), int(gap), float(vmin), float(vmax), ptr(out), stream_ptr()), "ribca_table_raster")
    return out


def pie_raster(rays: torch.Tensor, rgb: torch.Tensor, size: int, radius: int) -> torch.Tensor:
    """(size, size, 3) uint8 device image: a disc of the given radius around the pixel (size // 2, size // 2) cut into m + 1 wedges by the
    (m, 2) fp64 device rays (cos, sin; ascending angle), wedge w in rgb[w] ((m + 1, 3) uint8), white outside.  include/ribca_hip.h states the
    pixels."""
    if rays.dtype != torch.float64 or rays.dim() != 2 or rays.shape[1] != 2 or rgb.dtype != torch.uint8 or rgb.shape != (rays.shape[0] + 1, 3):
        raise ValueError("pie_raster takes (m, 2) float64 rays and (m + 1, 3) uint8 colours")
    rays, rgb = rays.contiguous(), rgb.contiguous()
    m = rays.shape[0]
    out = torch.empty((max(int(size), 0), max(int(size), 0), 3), dtype=torch.uint8, device=rgb.device)
    check(lib().ribca_pie_raster(ptr(rays) if m else None, m, ptr(rgb), int(size), int(radius), ptr(out), stream_ptr()), "ribca_pie_raster")
    return out


# ------------------------------------------------------------------------------------------- HDBSCAN (extra cell types)
def core_distance_ws_bytes(n: int, dim: int, min_samples: int) -> int:
    return int(lib().ribca_core_distance_ws_bytes(n, dim, min_samples))


def core_distance(x: torch.Tensor, min_samples: int, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """core2 (n) fp32: the min_samples-th smallest squared distance of every row of the (n, dim <= 64) fp32 device matrix x, the row itself
    counted (include/ribca_hip.h: fp32 sums of squared differences in dimension order)."""
    x = x.contiguous()
    n, dim = x.shape
    core2 = torch.empty(n, dtype=torch.float32, device=x.device)
    ws = _ws(ws, core_distance_ws_bytes(n, dim, int(min_samples)), x.device, "core_distance")
    check(lib().ribca_core_distance(ptr(x), n, dim, int(min_samples), ptr(core2), ptr(ws), ws.numel(), stream_ptr()), "ribca_core_distance")
    return core2


def mreach_mst_ws_bytes(n: int) -> int:
    """workspace of mreach_mst (include/ribca_hip.h): the control words and ten per-point / per-label arrays"""
    return int(lib().ribca_mreach_mst_ws_bytes(n))


def mreach_mst(x: torch.Tensor, core2: torch.Tensor, ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The minimum spanning tree of the mutual-reachability graph of x (n, dim <= 64) under the total order (mreach2, min(i, j), max(i, j)):
    u < v (n - 1) int32 and w = sqrt(mreach2) (n - 1) fp32, in a reproducible order."""
    x = x.contiguous()
    n, dim = x.shape
    m = max(n - 1, 0)
    u = torch.empty(m, dtype=torch.int32, device=x.device)
    v = torch.empty(m, dtype=torch.int32, device=x.device)
    w = torch.empty(m, dtype=torch.float32, device=x.device)
    ws = _ws(ws, mreach_mst_ws_bytes(n), x.device, "mreach_mst")
    check(lib().ribca_mreach_mst(ptr(x), n, dim, ptr(core2.contiguous()), ptr(u), ptr(v), ptr(w), ptr(ws), ws.numel(), stream_ptr()),
          "ribca_mreach_mst")
    return u, v, w


# ------------------------------------------------------------------------------------------- whole-image normalisation
def _gauss_weights(sigma: float) -> np.ndarray:
    """Taps at distance 0..R of scipy.ndimage.gaussian_filter(sigma, truncate=4.0), computed as scipy computes them."""
    sd = float(sigma)
    radius = int(4.0 * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:])


def gaussian_filter_f32(x: torch.Tensor, sigma: float, tmp: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                        mode: str = "reflect") -> torch.Tensor:
    """scipy.ndimage.gaussian_filter(x, sigma) on (C, H, W) fp32 planes: axis 0 pass then axis 1 pass, bit-identical."""
    assert x.dtype == torch.float32 and x.is_cuda and x.dim() == 3
    c, h, w = x.shape
    taps = torch.from_numpy(_gauss_weights(sigma)).to(x.device)
    r = taps.numel() - 1
    tmp = torch.empty_like(x) if tmp is None else tmp
    out = torch.empty_like(x) if out is None else out
    md = {"reflect": 0, "nearest": 1}[mode]
    check(lib().ribca_gauss1d(ptr(x), ptr(tmp), c, h, w, 0, ptr(taps), r, md, stream_ptr()), "ribca_gauss1d")
    check(lib().ribca_gauss1d(ptr(tmp), ptr(out), c, h, w, 1, ptr(taps), r, md, stream_ptr()), "ribca_gauss1d")
    return out


def _order_statistics(x: torch.Tensor, ranks: np.ndarray) -> np.ndarray:
    """Exact k-th smallest value (0-based rank per plane) of non-negative fp32 planes (C, H, W) by a 3-pass radix select
    (11 + 11 + 10 key bits).  The histograms are built on the GPU; the host only walks 2048-bin prefix sums."""
    c = x.shape[0]
    hw = x.shape[1] * x.shape[2]
    dev = x.device
    hist = torch.empty((c, 2048), dtype=torch.int32, device=dev)
    prefix = np.zeros(c, dtype=np.uint32)
    remaining = np.asarray(ranks, dtype=np.int64).copy()
    mask_hi = 0
    for shift, bits in ((21, 11), (10, 11), (0, 10)):
        pre_d = torch.from_numpy(prefix.view(np.int32).copy()).to(dev)
        check(lib().ribca_radix_hist(ptr(x), c, hw, ptr(pre_d), mask_hi, shift, bits, ptr(hist), stream_ptr()), "ribca_radix_hist")
        h = hist.cpu().numpy().astype(np.int64)
        cum = np.cumsum(h, axis=1)
        for p in range(c):
            b = int(np.searchsorted(cum[p], remaining[p], side="right"))
            remaining[p] -= cum[p, b - 1] if b > 0 else 0
            prefix[p] |= np.uint32(b << shift)
        mask_hi |= ((1 << bits) - 1) << shift
    return prefix.view(np.float32).copy()


def _numpy_quantile_impl():
    """numpy's own linear-quantile helpers (index, gamma, lerp): the percentile threshold of ``_normalize`` must round exactly
    as ``np.percentile`` does.  They live in a private module that exists since NumPy 2.0 (the version this package is
    validated against); anything else fails loudly instead of silently diverging from the reference."""
    try:
        from numpy.lib import _function_base_impl as fb
        for name in ("_QuantileMethods", "_get_indexes", "_get_gamma", "_lerp"):
            getattr(fb, name)
    except (ImportError, AttributeError) as e:
        raise _lib.RibcaError(f"normalize_image needs NumPy >= 2.0 quantile internals (found numpy {np.__version__}): {e}") from e
    return fb


def _percentile_plan(n: int, amax):
    """The two sorted-array indexes np.percentile(x, amax) (method 'linear', fp32 data of n values) interpolates between,
    and its fp32 interpolation weight -- obtained by running numpy's own index/gamma helpers, so dtypes and rounding are
    numpy's whatever its version.  Returns (prev, next, gamma) with prev == next and gamma None when no interpolation."""
    fb = _numpy_quantile_impl()
    q = np.asanyarray(np.true_divide(amax, np.float32(100)))     # np.percentile divides by a.dtype.type(100) for float data
    virtual = np.asanyarray(fb._QuantileMethods["linear"]["get_virtual_index"](n, q))
    if np.issubdtype(virtual.dtype, np.integer):
        return int(virtual), int(virtual), None
    prev, nxt = fb._get_indexes(np.empty((0,), dtype=np.float32), virtual, n)
    gamma = fb._get_gamma(virtual, prev, fb._QuantileMethods["linear"])
    return int(prev) % n, int(nxt) % n, gamma


def _percentile_like_numpy(n: int, amax, lo_hi_getter):
    """np.percentile of one fp32 plane given a callable returning its exact order statistics (prev, next)."""
    fb = _numpy_quantile_impl()
    prev, nxt, gamma = _percentile_plan(n, amax)
    a, b = lo_hi_getter(np.array([prev]), np.array([nxt]))
    return np.float32(a) if gamma is None else fb._lerp(np.float32(a), np.float32(b), gamma)


def normalize_image(raw, blur=0, amax=100, u16_bits: bool = False) -> torch.Tensor:
    """ImageProcessor._normalize (reference preprocess.py:214-239) on the GPU, bit-identical to the CPU path.
    ``raw``: (C, H, W) numpy array or torch tensor of any real dtype; returns a fp32 CUDA tensor in [-1, 1].
    ``u16_bits``: a torch.int16 tensor holds uint16 pixel BITS (how a device-resident uint16 image is carried, torch having no
    uint16 arithmetic); without the flag int16 data is signed and converted by value like every other dtype."""
    fb = _numpy_quantile_impl()
    dev = _lib.require_gpu()
    if isinstance(raw, np.ndarray):
        if raw.dtype == np.uint16:
            src = torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to(dev)
            img = torch.empty(raw.shape, dtype=torch.float32, device=dev)
            check(lib().ribca_u16_to_f32(ptr(src), ptr(img), src.numel(), stream_ptr()), "ribca_u16_to_f32")
        else:
            img = torch.from_numpy(raw.astype(np.float32)).to(dev)
    elif raw.dtype == torch.uint16 or (raw.dtype == torch.int16 and u16_bits):     # uint16 pixels already resident on the device
        src = raw.to(dev).contiguous()
        if src.dtype == torch.uint16:
            src = src.view(torch.int16)
        img = torch.empty(tuple(raw.shape), dtype=torch.float32, device=dev)
        check(lib().ribca_u16_to_f32(ptr(src), ptr(img), src.numel(), stream_ptr()), "ribca_u16_to_f32")
    else:
        img = raw.to(device=dev, dtype=torch.float32).contiguous().clone()
    c, h, w = img.shape
    hw = h * w
    tmp = torch.empty_like(img)
    bg = gaussian_filter_f32(img, 20, tmp=tmp)
    check(lib().ribca_bg_subtract(ptr(img), ptr(bg), img.numel(), 125.0, stream_ptr()), "ribca_bg_subtract")
    if blur:
        blurred = gaussian_filter_f32(img, blur, tmp=tmp, out=bg)
        img, bg = blurred, img
    mx_d = torch.empty(c, dtype=torch.float32, device=dev)
    check(lib().ribca_plane_max(ptr(img), c, hw, ptr(mx_d), stream_ptr()), "ribca_plane_max")
    mx = mx_d.cpu().numpy()
    mode = np.zeros(c, np.int32)                 # 0: no positive pixel -> plane of -1
    clip = np.full(c, np.inf, np.float32)
    denom = np.ones(c, np.float32)
    sel = np.flatnonzero(mx > 0)
    if sel.size:
        prev, nxt, gamma = _percentile_plan(hw, amax)
        planes = img[torch.from_numpy(sel).to(dev)] if sel.size < c else img
        lo = _order_statistics(planes, np.full(sel.size, prev))
        hi = lo if nxt == prev else _order_statistics(planes, np.full(sel.size, nxt))
        for j, p in enumerate(sel):
            t = np.float32(lo[j]) if gamma is None else fb._lerp(np.float32(lo[j]), np.float32(hi[j]), gamma)
            m = np.float32(mx[p])
            if t > 20:                            # preprocess.py:234-235
                clip[p] = t
                m = min(m, np.float32(t))
            mode[p] = 1
            denom[p] = max(25, m)                 # preprocess.py:238
    # one named tensor per argument: a temporary would be returned to the caching allocator (and its block handed to the next
    # .to(dev)) before the kernel that reads it is enqueued
    mode_d = torch.from_numpy(mode).to(dev)
    clip_d = torch.from_numpy(clip).to(dev)
    denom_d = torch.from_numpy(denom).to(dev)
    check(lib().ribca_norm_finalize(ptr(img), c, hw, ptr(mode_d), ptr(clip_d), ptr(denom_d), stream_ptr()), "ribca_norm_finalize")
    return img


# ------------------------------------------------------------------------------------------- ViT
def decision_distance(pa: torch.Tensor, others_a: Optional[int], pb: Optional[torch.Tensor], others_b: Optional[int],
                      thresholds: Sequence[float]) -> torch.Tensor:
    """How far (in probability) each cell is from the nearest boundary of the vote (reference model.py:481-633): the smaller of the top-2
    margin among the candidate classes and the distance of the best candidate from every quantity it is compared with -- the models'
    "Others" probabilities, the confidence threshold, the per-type thresholds in force.  Conservative (a threshold that does not bind
    for a cell still counts): it decides which cells Annotator.predict re-evaluates at full precision and which it reports as inside the
    arithmetic's noise floor.  ``others_x`` = column of "Others" in table x (None: the table has none)."""
    def split(p, o):
        if o is None:
            return p, None
        keep = [i for i in range(p.shape[1]) if i != o]
        return p[:, keep], p[:, o]
    va, oa = split(pa, others_a)
    cand, oth = [va], [oa] if oa is not None else []
    if pb is not None:
        vb, ob = split(pb, others_b)
        cand.append(vb)
        if ob is not None:
            oth.append(ob)
    v = torch.cat(cand, dim=1)
    top = torch.topk(v, min(2, v.shape[1]), dim=1).values
    best = top[:, 0]
    dist_ = (top[:, 0] - top[:, -1]) if v.shape[1] > 1 else torch.full_like(best, 2.0)
    for o in oth:
        dist_ = torch.minimum(dist_, (best - o).abs())
    for t in thresholds:
        if t is not None and t >= 0:
            dist_ = torch.minimum(dist_, (best - float(t)).abs())
    return dist_


class VitModel:
    """One packed classifier on one device (replaces a timm ``VisionTransformer`` instance of reference
    model.py:188-234).  ``state_dict`` uses the timm key names of the reference checkpoints."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device=None):
        device = device or _lib.require_gpu()
        self.device = torch.device(device)
        d = state_dict["cls_token"].shape[-1]
        c = state_dict["patch_embed.proj.weight"].shape[1]
        k = state_dict["head.weight"].shape[0]
        depth = 0
        while f"blocks.{depth}.norm1.weight" in state_dict:
            depth += 1
        if state_dict["pos_embed"].shape[1] != 101 or tuple(state_dict["patch_embed.proj.weight"].shape[2:]) != (4, 4):
            raise ValueError("expected a 40x40 / patch-4 ViT (101 tokens)")
        self.D, self.C, self.K, self.depth = int(d), int(c), int(k), depth
        blob = torch.cat([state_dict[key].detach().to(torch.float32).reshape(-1) for key in blob_keys(depth)]).to(self.device)
        want = lib().ribca_vit_blob_len(self.D, self.C, self.K, depth)
        if blob.numel() != want:
            raise ValueError(f"state dict has {blob.numel()} parameters, expected {want}")
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().ribca_vit_create(ptr(blob), blob.numel(), self.D, self.C, self.K, depth, stream_ptr(), ctypes.byref(handle)),
                  "ribca_vit_create")
            torch.cuda.current_stream().synchronize()  # the blob may be freed once packing has finished
        self._h = handle
        self.flops_per_cell = float(lib().ribca_vit_flops_per_cell(self._h))
        self.probe_fast_minus_full = 0.0
        self.probe_logit_delta = 0.0
        self.probe_predicted_dp = 0.0
        self.fast_ok = True
        #: fast level of the handle (ribca_vit_set_fast_level): 2 = with the per-cell kernel's MX products, 1 = every other MX product only;
        #: 0 once the probe has refused both (``fast_ok`` False).  predicted worst |dp| per level the probe tried: ``probe_level_dp``
        self.fast_level = self._set_fast_level(2)
        self.probe_level_dp: Dict[int, float] = {}
        if lib().ribca_mx_enabled(self.D) and os.environ.get("RIBCA_MARGIN_PROBE", "1") != "0":
            self._calibrate_margin()

    # ---- whether a model's weights tolerate the MX arithmetic is measured, not assumed (round 6) ---------------------------------------
    PROBE_CELLS = 64
    #: largest |dp| of a real cell over 0.25 x the probe's logit-difference move: <= 2.75 in 64 (family, head, seed, classifier) cases over
    #: 6000 real cells each (profiles/r6/probe_vs_real.txt); 3 is what the rule assumes
    PROBE_FACTOR = 3.0
    #: the fast (MX) forward is used only where the predicted worst |fast - full precision| stays below RECHECK_MARGIN / PROBE_DIVISOR
    PROBE_DIVISOR = 2.5

    def _set_fast_level(self, level: int) -> int:
        """select the handle's fast level; returns the level in effect (1 where the model has no per-cell MX kernel)"""
        try:
            fn = lib().ribca_vit_set_fast_level
        except AttributeError:      # an A/B library older than the entry point (RIBCA_LIB): one fast level
            return 1
        got = int(fn(self._h, int(level)))
        if got < 0:
            check(1, "ribca_vit_set_fast_level")
        return got

    def _calibrate_margin(self) -> None:
        """What the margin-gated re-evaluation rests on is |fast - full precision| staying well inside RECHECK_MARGIN for every cell (a cell
        the fast path places outside the margin then cannot cross a boundary at full precision), and what the 1e-3 confidence tolerance
        rests on is the same distance staying a fraction of it.  On the uniform synthetic family with the audit's soft head the distance is
        1-3e-5 over 2000 real cells; a sharper head (the bench's head_gain 4) or weights with heavy tails, LayerNorm gains two decades apart
        and massive-activation channels -- what trained ViTs have (synth.make_vit_state_dict_heavy) -- move the block-scaled correction
        products by 1-6e-4.  So it is MEASURED once per model, at load time, on a fixed synthetic probe (PROBE_CELLS patches: background
        -1, sparse positive signal; the same cells whatever the image, the rank or the chunk, so a cell's treatment never depends on
        where it was computed).  The statistic is saturation-free: delta = the largest move of a LOGIT DIFFERENCE, log p_i - log p_top,
        between the two forwards (a probe cell whose softmax is saturated hides any move of its probabilities: the probability form of
        this probe under-predicted real cells by up to 100 x); a probability then moves by at most p (1 - p) delta <= delta / 4.  Over 64
        cases (two weight families x two head gains x four seeds x the four MX-capable classifiers) the largest |dp| of 6000 real cells
        was 0.18 ... 2.75 x delta / 4 (tools/probe_vs_real.py, profiles/r6/probe_vs_real.txt), so the predicted worst case is
        PROBE_FACTOR x delta / 4 and a model is accepted while that stays below RECHECK_MARGIN / 2.5 = 4e-4 (delta <= 5.3e-4): every
        accepted case measured <= 2.5e-4.  A model beyond the bar runs EVERY product at three fp16 passes (``fast_ok`` False: the
        precise forward for all cells, slower, nothing to re-evaluate).  Costs two 64-cell forwards per model.

        Levels: a model whose handle has the per-cell kernel's MX products (fast level 2) is probed with them first; if that misses the bar
        the probe is repeated at level 1 (the per-cell kernel at three fp16 passes, fc1 / fc2 still MX) before the model is given up to the
        precise forward -- one more 64-cell forward, only for a model that fails level 2."""
        g = torch.Generator().manual_seed(0x5249424341)
        u = torch.rand((self.PROBE_CELLS, self.C, PATCH, PATCH), generator=g, dtype=torch.float32) * 2.0 - 1.0
        x = torch.where(u > 0.1, u, torch.full_like(u, -1.0)).to(self.device)
        with torch.cuda.device(self.device):
            src = list(range(self.C))
            full = self._forward(x, src, chunk_cells=self.PROBE_CELLS, precise=True).double()
            lp = torch.log(full.clamp_min(1e-300))
            top = full.argmax(1, keepdim=True)
            for level in ((2, 1) if self.fast_level == 2 else (1,)):
                self.fast_level = self._set_fast_level(level)
                fast = self._forward(x, src, chunk_cells=self.PROBE_CELLS, precise=False, force_fast=True).double()
                self.probe_fast_minus_full = float((fast - full).abs().max().item())       # (informational: the probability form)
                ok = (fast > 1e-30) & (full > 1e-30)
                lf = torch.log(fast.clamp_min(1e-300))
                d = ((lf - lf.gather(1, top)) - (lp - lp.gather(1, top))).abs()
                self.probe_logit_delta = float(d[ok].max().item()) if bool(ok.any()) else 0.0
                self.probe_predicted_dp = self.PROBE_FACTOR * 0.25 * self.probe_logit_delta
                self.probe_level_dp[level] = self.probe_predicted_dp
                self.fast_ok = self.probe_predicted_dp <= float(type(self).RECHECK_MARGIN) / self.PROBE_DIVISOR
                if self.fast_ok:
                    break
        if not self.fast_ok:
            self.fast_level = 0

    @property
    def recheck_margin(self) -> float:
        """cells whose fast result lies this close to a decision boundary are re-evaluated at full operand precision"""
        return float(type(self).RECHECK_MARGIN)

    @property
    def uses_mx(self) -> bool:
        """True where this model's forward really runs the MX products (the width allows them AND the probe accepted the weights)"""
        return bool(lib().ribca_mx_enabled(self.D)) and self.fast_ok

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().ribca_vit_destroy(h)
            except Exception:
                pass
            self._h = None

    # Cells whose fast (MX) result lies this close to a decision boundary are re-evaluated with three fp16 passes per product.  The MX
    # pair moves softmax outputs by 2-4e-5 against the fp16x3 path (measured; 1e-4 class with every product in that form, emulated):
    # 1e-3 leaves an order of magnitude, and is the north star's own confidence tolerance.  It is the FLOOR of the margin: the margin a
    # model actually uses is ``recheck_margin`` (calibrated on the model's own weights at load time, _calibrate_margin).
    RECHECK_MARGIN = 1.0e-3

    #: width -> multiple of the caller's chunk_cells a forward of that width uses (RIBCA_CHUNK_SCALE=<n> overrides it for every width: A/B)
    CHUNK_SCALE = {576: 4}

    #: the scaled chunk never exceeds this many cells (the workspace of a 576-wide forward is ~ 3.9 MB per cell and there is one per segment
    #: stream: 4096 cells x 3 streams = 48 GB of the 288; a caller that asks for more than this itself gets what it asked for, unscaled)
    MAX_SCALED_CHUNK = 4096

    def chunk_scale(self) -> int:
        env = os.environ.get("RIBCA_CHUNK_SCALE")
        return max(1, int(env)) if env else self.CHUNK_SCALE.get(self.D, 1)

    def effective_chunk(self, chunk_cells: int) -> int:
        """cells per launch sequence a forward of this width really uses for a caller's ``chunk_cells`` (bench.py reports it per model)"""
        c = max(1, int(chunk_cells))
        return max(c, min(c * self.chunk_scale(), self.MAX_SCALED_CHUNK))

    def predict_proba(self, patches: torch.Tensor, src_chan: Sequence[int], chunk_cells: int = 1024, ws_slot: int = 0,
                      streams: int = 1, recheck: Optional[Sequence[float]] = None) -> torch.Tensor:
        """``_forward`` plus, where this width runs the MX pair, the full-precision re-evaluation of the cells near a decision boundary:
        ``recheck`` = the thresholds the caller will compare confidences with (``[]``: only the top-2 margin counts; ``None``: no
        re-evaluation).  A cell is re-evaluated when its two best classes are closer than RECHECK_MARGIN or its best probability is
        within RECHECK_MARGIN of a threshold -- a property of the cell's own fast result, so results stay independent of chunking.
        ``self.last_recheck`` = {"cells": re-evaluated, "undecidable": of those, still within 2e-4 of a boundary afterwards}."""
        probs = self._forward(patches, src_chan, chunk_cells, ws_slot, streams, precise=False)
        self.last_recheck = {"cells": 0, "undecidable": 0}
        if recheck is None or probs.shape[0] == 0 or not self.uses_mx:      # (every product already at three fp16 passes: nothing to re-evaluate)
            return probs

        def near(p, eps):
            top = torch.topk(p, min(2, p.shape[1]), dim=1).values
            m = (top[:, 0] - top[:, -1]) < eps if p.shape[1] > 1 else torch.zeros(p.shape[0], dtype=torch.bool, device=p.device)
            for t in recheck:
                if t is not None and t > 0:
                    m |= (top[:, 0] - float(t)).abs() < eps
            return m

        idx = torch.nonzero(near(probs, self.recheck_margin)).flatten()
        if idx.numel():
            again = self._forward(patches.index_select(0, idx), src_chan, chunk_cells, ws_slot, 1, precise=True)
            probs.index_copy_(0, idx, again)
            self.last_recheck = {"cells": int(idx.numel()), "undecidable": int(near(again, 2.0e-4).sum().item())}
        return probs

    def _forward(self, patches: torch.Tensor, src_chan: Sequence[int], chunk_cells: int = 1024, ws_slot: int = 0,
                 streams: int = 1, precise: bool = False, force_fast: bool = False) -> torch.Tensor:
        """softmax(model(x), dim=1) for full-channel patches (n, C_img, 40, 40); ``src_chan[c]`` = image channel of model
        channel c or -1 for a blank plane (reference preprocess.py:110-120, model.py:397-406).

        ``streams`` > 1 splits the cells into that many contiguous segments and enqueues each on its own HIP stream (own
        workspace slot): cells are independent, so one segment's launch gaps, tile tails and store bursts overlap another
        segment's MFMA work.  The result is identical to the single-stream run (every cell sees the same arithmetic)."""
        assert patches.is_cuda and patches.dtype == torch.float32 and patches.dim() == 4 and patches.shape[2:] == (PATCH, PATCH)
        if len(src_chan) != self.C:
            raise ValueError(f"model expects {self.C} channels, got an index list of {len(src_chan)}")
        n, c_img = patches.shape[0], patches.shape[1]
        if any(s >= c_img or s < -1 for s in src_chan):
            raise ValueError("channel index out of range")
        probs = torch.empty((n, self.K), dtype=torch.float32, device=patches.device)
        if n == 0:
            return probs
        # force_fast: the MX products even where the probe refused this model's weights (tests and audits measure what the rule protects from)
        fwd = lib().ribca_vit_forward_precise if (precise or not (self.fast_ok or force_fast)) else lib().ribca_vit_forward
        # callers size chunks for the ensemble (1024 cells = 103 424 GEMM rows); the 576-wide classifier's launches are then 4.7 rounds of
        # workgroups and lose a twentieth each to the partial last round plus a fixed 39 us of ramp (profiles/r5/mx_rounds.txt): it takes
        # CHUNK_SCALE times the caller's chunk (same-box sweep, profiles/r5/chunk_streams_full.txt: 39.3-39.9 -> 40.4-41.3 k cells/s at 4 x;
        # the narrower classifiers measured flat or slightly worse).  Results do not depend on the chunk size (test_classifier_bitwise_repeatable).
        chunk = max(1, min(self.effective_chunk(chunk_cells), n))
        src = torch.tensor(list(src_chan), dtype=torch.int32, device=patches.device)
        nbytes = lib().ribca_vit_workspace_bytes(self._h, chunk)
        patches = patches.contiguous()
        n_chunks = (n + chunk - 1) // chunk
        nseg = max(1, min(int(streams), n_chunks))
        if nseg == 1:
            aligned = _workspace_ptr(nbytes, patches.device, ws_slot)
            check(fwd(self._h, ptr(patches), c_img, ptr(src), n, ptr(probs), aligned, nbytes, chunk, stream_ptr()), "ribca_vit_forward")
            return probs
        main = torch.cuda.current_stream(patches.device)
        ready = torch.cuda.Event()
        ready.record(main)
        side = _side_streams(patches.device, nseg)
        for i, st in enumerate(side):
            c0, c1 = n_chunks * i // nseg, n_chunks * (i + 1) // nseg
            lo, hi = c0 * chunk, min(c1 * chunk, n)
            if hi <= lo:
                continue
            aligned = _workspace_ptr(nbytes, patches.device, (ws_slot + 1) * 64 + i)
            st.wait_event(ready)
            with torch.cuda.stream(st):
                check(fwd(self._h, ptr(patches[lo:hi]), c_img, ptr(src), hi - lo, ptr(probs[lo:hi]), aligned, nbytes, chunk, stream_ptr()),
                      "ribca_vit_forward")
            done = torch.cuda.Event()
            done.record(st)
            main.wait_event(done)
        return probs


_SIDE: Dict[Tuple[int, int], "torch.cuda.Stream"] = {}


def _side_streams(device, n: int):
    out = []
    for i in range(n):
        key = (device.index or 0, i)
        if key not in _SIDE:
            _SIDE[key] = torch.cuda.Stream(device=device)
        out.append(_SIDE[key])
    return out


def mae_blob_keys(enc_depth: int, dec_depth: int) -> List[str]:
    return (["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"] + _block_keys("blocks.", enc_depth)
            + ["norm.weight", "norm.bias", "decoder_embed.weight", "decoder_embed.bias", "mask_token", "decoder_pos_embed"]
            + _block_keys("decoder_blocks.", dec_depth) + ["decoder_norm.weight", "decoder_norm.bias", "decoder_pred.weight", "decoder_pred.bias"])


class MaeModel:
    """Packed marker imputer on one device (replaces the ``MaskedAutoencoderViT`` inside the reference's
    ``MarkerImputer``, markerImputer.py:258-287); ``state_dict`` = the ``["model"]`` entry of a ``*_impute.pth`` checkpoint."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device=None):
        device = device or _lib.require_gpu()
        self.device = torch.device(device)
        self.L = int(state_dict["pos_embed"].shape[1]) - 1
        enc = dec = 0
        while f"blocks.{enc}.norm1.weight" in state_dict:
            enc += 1
        while f"decoder_blocks.{dec}.norm1.weight" in state_dict:
            dec += 1
        if state_dict["cls_token"].shape[-1] != 768 or state_dict["mask_token"].shape[-1] != 512 or \
                tuple(state_dict["patch_embed.proj.weight"].shape) != (768, 1, 40, 40):
            raise ValueError("expected the reference imputer geometry (768/512 wide, one 40x40 tile per token)")
        blob = torch.cat([state_dict[k].detach().to(torch.float32).reshape(-1) for k in mae_blob_keys(enc, dec)]).to(self.device)
        if blob.numel() != lib().ribca_mae_blob_len(self.L, enc, dec):
            raise ValueError("imputer state dict does not match (L, depths)")
        self._h = self._create(blob, enc, dec)
        self.probe_plane_delta = 0.0
        self.fast_ok = True
        # the imputer's fast path (folded blocks, 768-wide encoder on the MX kernel) has no full-precision twin inside one handle: where the
        # environment leaves the choice open, a second handle on the round-2 path (three fp16 passes everywhere) is the yardstick of a load-time
        # probe, as for the classifiers (VitModel._calibrate_margin)
        if os.environ.get("RIBCA_MARGIN_PROBE", "1") != "0" and os.environ.get("RIBCA_MAE_FOLD") is None:
            self._probe(blob, enc, dec)

    def _create(self, blob, enc, dec, fold: Optional[int] = None):
        """``fold`` None: the library's choice (RIBCA_MAE_FOLD in the environment at this call); 1 / 0: the folded / the fp16x3 path"""
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            if fold is None:
                check(lib().ribca_mae_create(ptr(blob), blob.numel(), self.L, enc, dec, stream_ptr(), ctypes.byref(handle)), "ribca_mae_create")
            else:
                check(lib().ribca_mae_create_path(ptr(blob), blob.numel(), self.L, enc, dec, int(fold), stream_ptr(), ctypes.byref(handle)),
                      "ribca_mae_create_path")
            torch.cuda.current_stream().synchronize()
        return handle

    #: the fast imputer is kept while its imputed pixels (values in [-1, 1]) stay this close to the fp16x3 imputer's on the probe: the uniform
    #: family measures 8e-5 on real cells, which moves the classifier's confidences behind it by 2e-6 (tests/test_gpu_e2e.py, config-5 audit)
    PROBE_LIMIT = 1.0e-3
    PROBE_CELLS = 64

    def _probe(self, blob, enc, dec) -> None:
        drop = self._create(blob, enc, dec, fold=0)      # the yardstick; whichever handle `drop` names when the probe ends (or fails) goes
        try:
            g = torch.Generator().manual_seed(0x5249424342)
            u = torch.rand((self.PROBE_CELLS, self.L, PATCH, PATCH), generator=g, dtype=torch.float32) * 2.0 - 1.0
            x = torch.where(u > 0.1, u, torch.full_like(u, -1.0))
            x[:, self.L - 1] = -1.0                      # the last marker missing, as in BASELINE config 5
            present = list(range(self.L - 1))
            a, b = x.to(self.device).contiguous(), x.to(self.device).contiguous()
            with torch.cuda.device(self.device):
                self._impute_with(self._h, a, present, self.PROBE_CELLS)
                self._impute_with(drop, b, present, self.PROBE_CELLS)
                self.probe_plane_delta = float((a[:, self.L - 1] - b[:, self.L - 1]).abs().max().item())
            self.fast_ok = self.probe_plane_delta <= self.PROBE_LIMIT
            if not self.fast_ok:      # these weights do not tolerate the MX products: every product at three fp16 passes
                self._h, drop = drop, self._h
        finally:
            lib().ribca_mae_destroy(drop)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().ribca_mae_destroy(h)
            except Exception:
                pass
            self._h = None

    #: a cell is <= 16 token rows here against 101 in a classifier: callers that size chunks for the classifiers (Annotator, bench.py) hand the
    #: imputer this many times their chunk, so that its GEMMs see a comparable row count (50 000 cells: 0.489 s at 1024, 0.464 s at 4096;
    #: profiles/r5/ab_mae_fold.txt).  Results do not depend on the chunk size (tests/test_gpu_e2e.py::test_config5_full_size_properties).
    CHUNK_FACTOR = 4

    def impute(self, patches: torch.Tensor, present: Sequence[int], chunk_cells: int = 1024) -> torch.Tensor:
        """In place: every channel of ``patches`` (n, L, 40, 40) not listed in ``present`` is replaced by its prediction."""
        return self._impute_with(self._h, patches, present, chunk_cells)

    def _impute_with(self, handle, patches: torch.Tensor, present: Sequence[int], chunk_cells: int) -> torch.Tensor:
        assert patches.is_cuda and patches.dtype == torch.float32 and patches.is_contiguous() and tuple(patches.shape[1:]) == (self.L, PATCH, PATCH)
        n = patches.shape[0]
        pres = sorted(int(c) for c in present)
        if n == 0:
            return patches
        chunk = max(1, min(int(chunk_cells), n))
        nbytes = lib().ribca_mae_workspace_bytes(handle, chunk, len(pres))
        if nbytes <= 0:
            raise ValueError("need at least one present and one missing channel")
        aligned = _workspace_ptr(nbytes, patches.device)
        arr = (ctypes.c_int32 * len(pres))(*pres)
        check(lib().ribca_mae_impute(handle, ptr(patches), arr, len(pres), n, aligned, nbytes, chunk, stream_ptr()), "ribca_mae_impute")
        return patches


def resolve_channels(channel_index: Sequence[int], c_img: int) -> List[int]:
    """Reference channel-select semantics (preprocess.py:110-120): the FIRST -1 becomes a blank plane, every further -1
    stays in a numpy fancy index and therefore picks the LAST image channel."""
    out, seen_blank = [], False
    for ci in channel_index:
        if ci == -1 and not seen_blank:
            out.append(-1)
            seen_blank = True
        elif ci == -1:
            out.append(c_img - 1)
        else:
            out.append(int(ci))
    return out


# ------------------------------------------------------------------------------------------- vote
def vote(p_a: torch.Tensor, map_a: Sequence[int], p_b: Optional[torch.Tensor], map_b: Optional[Sequence[int]],
         type_conf: Sequence[float], conf: float) -> Tuple[torch.Tensor, torch.Tensor]:
    n = p_a.shape[0]
    dev = p_a.device
    label = torch.empty(n, dtype=torch.int8, device=dev)
    out_conf = torch.empty(n, dtype=torch.float32, device=dev)
    ma = torch.tensor(list(map_a), dtype=torch.int8, device=dev)
    mb = torch.tensor(list(map_b), dtype=torch.int8, device=dev) if p_b is not None else None
    tc = torch.tensor([float(np.float32(v)) for v in type_conf], dtype=torch.float32, device=dev)
    pa_c = p_a.contiguous()                                   # named: only tensors that outlive the call cross the ABI
    pb_c = p_b.contiguous() if p_b is not None else None
    check(lib().ribca_vote(ptr(pa_c), pa_c.shape[1], ptr(ma), ptr(pb_c) if pb_c is not None else None,
                           pb_c.shape[1] if pb_c is not None else 0, ptr(mb), ptr(tc), float(np.float32(conf)), n, ptr(label),
                           ptr(out_conf), stream_ptr()), "ribca_vote")
    return label, out_conf


# ------------------------------------------------------------------------------------------- profiling
def prof_enable(on: bool) -> None:
    lib().ribca_prof_enable(1 if on else 0)


def prof_read() -> Dict[str, Tuple[float, int]]:
    ms = (ctypes.c_double * 10)()
    cnt = (ctypes.c_int64 * 10)()
    lib().ribca_prof_read(ms, cnt)
    return {lib().ribca_prof_name(i).decode(): (ms[i], cnt[i]) for i in range(10)}
