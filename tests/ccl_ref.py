"""CPU restatement of the lesion-node kernels (csrc/ccl.hip) in plain numpy, and of reference
src/lesion_gnn/datasets/nodes/lesions.py:147-176 in torch on top of it.

The label contract: nonzero pixels are foreground whatever their value; 0 is the background, even
when there is none; components are numbered 1, 2, ... in raster order of their first pixel
(scipy.ndimage.label's numbering). Pinned by hand-written known answers and against scipy in
tests/test_ccl_ref.py.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import oracle.pyg_ref as ref


def _roots(fg: np.ndarray, connectivity: int) -> np.ndarray:
    """Per pixel the smallest flat index of its component (background: -1). Hook-and-jump: every
    round each root adopts the smallest root among its members' neighbours, then all pointers
    jump to their roots; ends when no edge joins two roots."""
    H, W = fg.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    pairs = [(idx[:, 1:], idx[:, :-1], fg[:, 1:] & fg[:, :-1]),
             (idx[1:, :], idx[:-1, :], fg[1:, :] & fg[:-1, :])]
    if connectivity == 8:
        pairs += [(idx[1:, 1:], idx[:-1, :-1], fg[1:, 1:] & fg[:-1, :-1]),
                  (idx[1:, :-1], idx[:-1, 1:], fg[1:, :-1] & fg[:-1, 1:])]
    elif connectivity != 4:
        raise ValueError("connectivity must be 4 or 8")
    a = np.concatenate([p[0][p[2]] for p in pairs])
    b = np.concatenate([p[1][p[2]] for p in pairs])
    parent = np.arange(H * W, dtype=np.int64)
    while a.size:
        ra, rb = parent[a], parent[b]
        live = ra != rb
        if not live.any():
            break
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    parent[~fg.reshape(-1)] = -1
    return parent.reshape(H, W)


def label(image: np.ndarray, connectivity: int = 8) -> tuple[int, np.ndarray]:
    """(nlabel, labels (H, W) int64): label = 1 + rank of the component's root among the roots."""
    image = np.asarray(image)
    fg = image != 0
    root = _roots(fg, connectivity).reshape(-1)
    is_root = root == np.arange(root.size)
    rank = np.cumsum(is_root)  # 1-based at the roots
    labels = np.where(root >= 0, rank[np.maximum(root, 0)], 0).astype(np.int64)
    return int(is_root.sum()) + 1, labels.reshape(image.shape)


def stats(labels: np.ndarray, nlabel: int) -> tuple[np.ndarray, np.ndarray]:
    """(stats (nlabel, 5) int32: left, top, width, height, area; centroids (nlabel, 2) fp64:
    integer coordinate sums divided by the area). A label without a pixel gets zeros."""
    H, W = labels.shape
    lab = labels.reshape(-1)
    y, x = np.divmod(np.arange(H * W, dtype=np.int64), W)
    area = np.bincount(lab, minlength=nlabel).astype(np.int64)
    sx = np.zeros(nlabel, dtype=np.int64)
    sy = np.zeros(nlabel, dtype=np.int64)
    np.add.at(sx, lab, x)
    np.add.at(sy, lab, y)
    big = np.iinfo(np.int64).max
    x0, y0 = np.full(nlabel, big), np.full(nlabel, big)
    x1, y1 = np.full(nlabel, -1, dtype=np.int64), np.full(nlabel, -1, dtype=np.int64)
    np.minimum.at(x0, lab, x)
    np.minimum.at(y0, lab, y)
    np.maximum.at(x1, lab, x)
    np.maximum.at(y1, lab, y)
    has = area > 0
    out = np.zeros((nlabel, 5), dtype=np.int32)
    out[has, 0] = x0[has]
    out[has, 1] = y0[has]
    out[has, 2] = (x1 - x0 + 1)[has]
    out[has, 3] = (y1 - y0 + 1)[has]
    out[:, 4] = area
    cent = np.zeros((nlabel, 2), dtype=np.float64)
    cent[has, 0] = sx[has].astype(np.float64) / area[has].astype(np.float64)
    cent[has, 1] = sy[has].astype(np.float64) / area[has].astype(np.float64)
    return out, cent


def connected_components_with_stats(image: np.ndarray, connectivity: int = 8):
    nlabel, labels = label(image, connectivity)
    st, cent = stats(labels, nlabel)
    return nlabel, labels, st, cent


def label_pool(logits: torch.Tensor, size: tuple[int, int]) -> torch.Tensor:
    """Reference lesions.py:150-153 for one image: (K, Hin, Win) -> (H, W) uint8."""
    am = torch.argmax(logits, dim=0, keepdim=True)[None].float()
    return F.adaptive_max_pool2d(am, output_size=size)[0, 0].byte()


def lesion_nodes_ref(label_map: torch.Tensor, features: torch.Tensor, label: int,
                     reduce: str = "mean", dtype: torch.dtype | None = None):
    """Reference lesions.py:150-176 on the CPU: label_map (1, K, Horg, Worg) logits, features
    (1, C, H, W) already reinterpolated (:147-148 is the caller's) -> (pos fp64 [n, 2], x
    [n, C + 1], y). dtype: evaluate the pooling in this precision (float64 for the error bound)."""
    label_map = torch.argmax(label_map, dim=1, keepdim=True)
    Horg = label_map.shape[-2]
    label_map = F.adaptive_max_pool2d(label_map.float(), output_size=features.shape[2:])
    connected_map = label_map.squeeze().byte().numpy()
    H = label_map.shape[-2]
    nlabel, cc, _, centroids = connected_components_with_stats(connected_map, connectivity=8)
    centroids = centroids * Horg / H
    features = torch.cat([features, label_map], dim=1)
    if dtype is not None:
        features = features.to(dtype)
    x = ref.extract_features_by_cc(torch.from_numpy(cc), features, nlabel, reduce=reduce)
    return torch.from_numpy(centroids), x, torch.tensor([label])
