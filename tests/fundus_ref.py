"""Numpy restatement of the fundus preprocessing chain (lesion_gnn_amd/datasets/fundus.py): one
function per step, exact integers on the pixel path (int64), Python doubles for the size rule,
float64 for the normalised output. It restates the reference's FundusAutocrop ->
LongestMaxSize -> PadIfNeeded(BORDER_CONSTANT) -> Normalize -> ToTensorV2 with OpenCV's 8-bit
INTER_LINEAR / INTER_NEAREST written out; the restated arithmetic is the contract.
tests/test_fundus_ref.py holds known answers for this file itself.
"""
from __future__ import annotations

import numpy as np


def box(image: np.ndarray, threshold: float = 25.0) -> tuple[int, int, int, int]:
    """Step 1: (x_min, x_max, y_min, y_max) of the pixels with red > threshold; (0, W, 0, H) when
    there is none, or the lit pixels share one column or one row."""
    H, W = image.shape[:2]
    ys, xs = np.nonzero(image[:, :, 0].astype(np.float64) > float(threshold))
    if ys.size == 0:
        return 0, W, 0, H
    x_min, x_max, y_min, y_max = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    if x_min == x_max or y_min == y_max:
        return 0, W, 0, H
    return x_min, x_max, y_min, y_max


def crop(image: np.ndarray, b: tuple[int, int, int, int]) -> np.ndarray:
    """image[y_min:y_max, x_min:x_max]: the upper bounds are exclusive."""
    x_min, x_max, y_min, y_max = b
    return image[y_min:y_max, x_min:x_max]


def _rint(v: float) -> int:
    return int(np.rint(np.float64(v)))  # half to even


def new_size(h: int, w: int, S: int) -> tuple[int, int]:
    """Step 2: (new_h, new_w) of LongestMaxSize(S), each at least 1."""
    scale = S / float(max(h, w))
    return max(1, _rint(h * scale)), max(1, _rint(w * scale))


def linear_taps(dst: int, src: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One axis of step 3: per destination index the first source index and the two int
    coefficients (sum 2048)."""
    sc = 1.0 / (dst / src)
    s = np.empty(dst, np.int64)
    a0 = np.empty(dst, np.int64)
    a1 = np.empty(dst, np.int64)
    for d in range(dst):
        f = np.float32((d + 0.5) * sc - 0.5)
        i = int(np.floor(f))
        f = np.float32(f - np.float32(i))
        if i < 0:
            i, f = 0, np.float32(0)
        if i >= src - 1:
            i, f = src - 1, np.float32(0)
        s[d] = i
        a0[d] = int(np.rint(np.float32((np.float32(1) - f) * np.float32(2048))))
        a1[d] = int(np.rint(np.float32(f * np.float32(2048))))
    return s, a0, a1


def resize_linear(src: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    """Step 3: 8-bit INTER_LINEAR of an (h, w, C) uint8 image, in integers."""
    h, w = src.shape[:2]
    sx, a0, a1 = linear_taps(new_w, w)
    sy, b0, b1 = linear_taps(new_h, h)
    sx1, sy1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    S = src.astype(np.int64)
    # horizontal pass for every source row, then the vertical one
    t = S[:, sx] * a0[None, :, None] + S[:, sx1] * a1[None, :, None]
    t0, t1 = t[sy], t[sy1]
    out = (((b0[:, None, None] * (t0 >> 4)) >> 16) + ((b1[:, None, None] * (t1 >> 4)) >> 16)
           + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def nearest_index(dst: int, src: int) -> np.ndarray:
    sc = 1.0 / (dst / src)
    return np.array([min(int(np.floor(d * sc)), src - 1) for d in range(dst)], np.int64)


def resize_nearest(src: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    """Step 4: INTER_NEAREST of an (h, w) label mask."""
    h, w = src.shape[:2]
    return src[nearest_index(new_h, h)][:, nearest_index(new_w, w)]


def pad_offsets(new_h: int, new_w: int, S: int) -> tuple[int, int]:
    """Step 5: (pad_top, pad_left) of PadIfNeeded, centre; the remainder goes below and right."""
    return int((S - new_h) / 2.0), int((S - new_w) / 2.0)


def pad(img: np.ndarray, S: int) -> np.ndarray:
    new_h, new_w = img.shape[:2]
    top, left = pad_offsets(new_h, new_w, S)
    out = np.zeros((S, S) + img.shape[2:], img.dtype)
    out[top:top + new_h, left:left + new_w] = img
    return out


def norm_constants(mean, std) -> tuple[np.ndarray, np.ndarray]:
    """m_c = float32(mean_c * 255), r_c = float32(1 / (std_c * 255)), as float64 values."""
    m = np.array([np.float32(float(v) * 255.0) for v in mean], np.float64)
    r = np.array([np.float32(1.0 / (float(v) * 255.0)) for v in std], np.float64)
    return m, r


def normalize(u8: np.ndarray, mean, std) -> np.ndarray:
    """Step 6: (S, S, 3) uint8 -> (3, S, S) float64, (v - m_c) * r_c."""
    m, r = norm_constants(mean, std)
    return ((u8.astype(np.float64) - m) * r).transpose(2, 0, 1)


def preprocess(image: np.ndarray, S: int, mean, std, threshold: float = 25.0,
               mask: np.ndarray | None = None) -> dict:
    """The whole chain for one image: box, geom, uint8 (S, S, 3), image (3, S, S) float64, mask
    (S, S) or None."""
    b = box(image, threshold)
    c = crop(image, b)
    h, w = c.shape[:2]
    new_h, new_w = new_size(h, w, S)
    u8 = pad(resize_linear(c, new_h, new_w), S)
    top, left = pad_offsets(new_h, new_w, S)
    out = {"box": np.array(b, np.int32),
           "geom": np.array([b[0], b[2], w, h, new_w, new_h, left, top], np.int32),
           "uint8": u8, "image": normalize(u8, mean, std), "mask": None}
    if mask is not None:
        out["mask"] = pad(resize_nearest(crop(mask, b), new_h, new_w), S)
    return out
