"""The images the connected-component tests label (tests/test_gpu_ccl.py), each for a way a
parallel labelling can go wrong, and the inputs of the lesion-node pipeline tests."""
from __future__ import annotations

import numpy as np
import torch

SIZES = [(1, 1), (1, 70), (70, 1), (2, 2), (33, 31), (37, 53), (64, 64), (65, 63), (130, 257),
         (512, 512)]
NOISE = [0.05, 0.3, 0.41, 0.6, 0.9]  # 0.41: near the 8-connected percolation point


def _serpentine(H, W):
    """Every other row filled, joined alternately at the right and left end: one component whose
    chain of merges runs through every row."""
    img = np.zeros((H, W), dtype=np.uint8)
    img[::2] = 1
    for i, y in enumerate(range(1, H - 1, 2)):
        img[y, W - 1 if i % 2 == 0 else 0] = 1
    return img


def _spiral(H, W):
    """A one-pixel square spiral from the top-left corner inwards, one background pixel between
    its laps."""
    img = np.zeros((H, W), dtype=np.uint8)
    y = x = 0
    dy, dx = 0, 1
    img[0, 0] = 1

    def free(yy, xx):
        return not (0 <= yy < H and 0 <= xx < W) or not img[yy, xx]

    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and not img[ny, nx] and free(ny + dy, nx + dx):
                y, x = ny, nx
                img[y, x] = 1
                break
            dy, dx = dx, -dy  # turn right
        else:
            return img


def _combs(H, W):
    """Two combs wound into each other: one hangs from the top row, one stands on the bottom
    row, their teeth alternate two columns apart and stop two rows short of the other's spine."""
    img = np.zeros((H, W), dtype=np.uint8)
    img[0] = 1
    img[H - 1] = 1
    img[:max(H - 2, 1), 0::4] = 1
    img[min(2, H - 1):, 2::4] = 1
    return img


def _diagonals(H, W):
    img = np.zeros((H, W), dtype=np.uint8)
    i = np.arange(min(H, W))
    img[i, i] = 1
    img[i, W - 1 - i] = 1
    return img


def _rings(H, W):
    y, x = np.mgrid[:H, :W]
    d = np.minimum(np.minimum(y, x), np.minimum(H - 1 - y, W - 1 - x))
    return (d % 2 == 0).astype(np.uint8)


def images(H: int, W: int) -> dict[str, np.ndarray]:
    """name -> (H, W) uint8 image."""
    y, x = np.mgrid[:H, :W]
    out = {
        "zeros": np.zeros((H, W), dtype=np.uint8),
        "ones": np.ones((H, W), dtype=np.uint8),
        "checkerboard": ((y + x) % 2 == 0).astype(np.uint8),
        "dots": ((y % 2 == 0) & (x % 2 == 0)).astype(np.uint8),
        "rows": (y % 2 == 0).astype(np.uint8) + np.zeros((H, W), dtype=np.uint8),
        "columns": (x % 2 == 0).astype(np.uint8) + np.zeros((H, W), dtype=np.uint8),
        "serpentine": _serpentine(H, W),
        "spiral": _spiral(H, W),
        "combs": _combs(H, W),
        "diagonals": _diagonals(H, W),
        "rings": _rings(H, W),
    }
    for k, p in enumerate(NOISE):
        rng = np.random.default_rng(1000 * k + 7 * H + W)
        out[f"noise{p}"] = (rng.random((H, W)) < p).astype(np.uint8)
    out["classes"] = np.random.default_rng(H * 31 + W).integers(0, 5, (H, W)).astype(np.uint8)
    return out


def blob_classes(H: int, W: int, n: int, seed: int) -> torch.Tensor:
    """(H, W) int64 class map: background 0 and n axis-aligned blobs of classes 1..4 (later blobs
    overwrite earlier ones, so shapes and touching classes occur)."""
    gen = torch.Generator().manual_seed(seed)
    cls = torch.zeros(H, W, dtype=torch.int64)
    for _ in range(n):
        h = int(torch.randint(1, max(2, H // 8), (1,), generator=gen))
        w = int(torch.randint(1, max(2, W // 8), (1,), generator=gen))
        y0 = int(torch.randint(0, H - h + 1, (1,), generator=gen))
        x0 = int(torch.randint(0, W - w + 1, (1,), generator=gen))
        cls[y0:y0 + h, x0:x0 + w] = int(torch.randint(1, 5, (1,), generator=gen))
    return cls


def logits_of(classes: torch.Tensor, K: int, seed: int) -> torch.Tensor:
    """(1, K, H, W) fp32 logits whose argmax is `classes`: uniform [0, 1) noise, + 8 at the
    class."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.rand(1, K, *classes.shape, generator=gen)
    return z + 8.0 * torch.nn.functional.one_hot(classes, K).permute(2, 0, 1)[None].float()
