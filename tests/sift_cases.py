"""Inputs of the SIFT tests: seeded smooth textures (filtered noise at two scales, scaled to uint8;
not symmetric shapes, which create exact ties), a constant image, a batch with the constant image
in the middle, and two Gaussian blobs with known centres. The oracle's result per case is computed
once and shared (`oracle`)."""
from __future__ import annotations

import functools

import numpy as np

from tests import sift_ref

# (height, width): 44 x 52 ends in an 11 x 13 octave (repeated reflection, one interior row),
# 37 x 41 halves odd sizes, 96 x 128 has four octaves
TEXTURE_SIZES = ((48, 64), (44, 52), (37, 41), (96, 128))
SIGMAS = (1.6, 1.2, 0.8)  # 0.8: the 0.01 floor of the base blur, a 3-tap kernel
NUM_KEYPOINTS = (16, 10000)  # the selection cuts / fewer than asked
BLOBS = ((3.0, 30.3, 22.6), (5.0, 31.5, 24.25))  # (s, centre x, centre y) on a 48 x 64 field


def _smooth(rng, H: int, W: int, s: float) -> np.ndarray:
    return sift_ref.blur(rng.standard_normal((H, W)), s)


@functools.lru_cache(maxsize=None)
def texture(H: int, W: int, seed: int = 0, channels: int = 3) -> np.ndarray:
    """uint8 (H, W, channels) or (H, W) for channels == 0."""
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    planes = []
    for _ in range(max(channels, 1)):
        t = _smooth(rng, H, W, 1.2) + 3.0 * _smooth(rng, H, W, 2.5)
        t = (t - t.min()) / (t.max() - t.min())
        planes.append(np.rint(t * 255.0).astype(np.uint8))
    out = np.stack(planes, axis=-1) if channels else planes[0]
    out.setflags(write=False)
    return out


def constant(H: int = 48, W: int = 64, value: int = 97) -> np.ndarray:
    return np.full((H, W, 3), value, dtype=np.uint8)


def batch3() -> np.ndarray:
    """Three 48 x 64 images, the constant one in the middle: an empty segment."""
    return np.stack([texture(48, 64, 1), constant(), texture(48, 64, 2)])


def blob(s: float, cx: float, cy: float, H: int = 48, W: int = 64) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    g = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s))
    return np.rint(20.0 + 200.0 * g).astype(np.uint8)


# the cases the stage and end-to-end tests run: (name, image, sigma)
def cases():
    out = [(f"texture{H}x{W}", texture(H, W), 1.6) for H, W in TEXTURE_SIZES]
    out.append(("texture48x64_sigma1.2", texture(48, 64), 1.2))
    out.append(("texture48x64_sigma0.8", texture(48, 64), 0.8))
    out.append(("texture37x41_gray", texture(37, 41, 3, channels=0), 1.6))
    return out


CASE_NAMES = [c[0] for c in cases()]


def case(name: str):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def oracle(name: str, num_keypoints: int = 10000) -> dict:
    """The oracle's whole chain for a case, computed once per process; do not modify."""
    _, image, sigma = case(name)
    return sift_ref.extract(image, num_keypoints, sigma)
