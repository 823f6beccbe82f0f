"""Fundus image preprocessing on the GPU: the chain every image-consuming path of the reference
applies to a decoded photograph, `FundusAutocrop -> LongestMaxSize -> PadIfNeeded(BORDER_CONSTANT)
-> Normalize -> ToTensorV2` (fundus-datamodules/src/fundus_datamodules/base.py:93-120,
`FundusDataModule.get_transforms`; utils/autocrop.py:28-45 holds the crop rule;
src/lesion_gnn/datasets/nodes/lesions.py:132-141 spells the same chain out).

A batch of uint8 RGB images already on the GPU goes in, possibly of different sizes; the
network-ready `[B, 3, S, S]` float32 batch comes out, and optionally the `[B, S, S, 3]` uint8 image
before the normalisation (what `SiftExtractor.nodes_from_batch` takes) and the resized label mask.
The output shape depends only on `S` and nothing is read back to the host, so the call works
inside a HIP-graph capture. Two HIP entries do the work (csrc/fundus.hip): lgnn_fundus_bbox reads
every pixel once for the crop box, lgnn_fundus_preprocess derives the sizes from the box on the
device and writes the outputs.

The arithmetic is integer: OpenCV's 8-bit INTER_LINEAR (and INTER_NEAREST for the mask)
restated, with tests/fundus_ref.py as its statement in numpy. Agreement with OpenCV and
albumentations themselves is not pinned. The augmentations of
`get_transforms(data_aug=True)` and image decoding on the GPU are out of scope.
"""
from __future__ import annotations

import dataclasses
from pathlib import Path

import torch

# timm.data.constants, written out (timm is not a dependency)
IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


class FundusAutocrop:
    """Reference FundusAutocrop (utils/autocrop.py): the box of the pixels whose red channel
    exceeds `threshold`."""

    def __init__(self, threshold: float = 25.0):
        self.threshold = float(threshold)

    def boxes(self, images) -> torch.Tensor:
        """images: (B, H, W, 3) uint8 on the GPU, or a list of (H_b, W_b, 3) -> (B, 4) int32 on
        the device: (x_min, x_max, y_min, y_max) per image, the whole image (0, W, 0, H) when the
        mask is empty or one pixel wide or high. The crop is image[y_min:y_max, x_min:x_max]:
        the upper bounds are exclusive, as in the reference, so the last lit row and column are
        dropped."""
        from .. import ops

        return ops.fundus_bbox(images, self.threshold)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(threshold={self.threshold})"


@dataclasses.dataclass
class FundusBatch:
    """What `FundusPreprocess.__call__` returns."""

    image: torch.Tensor         # [B, 3, S, S] fp32, normalised
    uint8: torch.Tensor | None  # [B, S, S, 3] uint8, before the normalisation
    mask: torch.Tensor | None   # [B, S, S] uint8, nearest-neighbour labels, padding 0
    boxes: torch.Tensor         # [B, 4] int32 (x_min, x_max, y_min, y_max)
    geom: torch.Tensor          # [B, 8] int32 (x_min, y_min, w, h, new_w, new_h, pad_left, pad_top)

    def to_original(self, pos: torch.Tensor, index) -> torch.Tensor:
        """(x, y) positions in the preprocessed frame (pixel d's centre at d) -> float64 (x, y)
        in the source image's pixels: the resize's own mapping src = (d - pad + 0.5) * (w /
        new_w) - 0.5, plus the crop's corner. pos [n, 2]; index: the image of every position
        ([n] integers on the device) or one image (int). Plain torch arithmetic on the device
        from `geom`, e.g. for carrying node centroids back to the photograph."""
        g = self.geom[index].to(torch.float64)
        if g.dim() == 1:
            g = g[None]
        p = pos.to(torch.float64)
        origin, crop, new, pad = g[:, 0:2], g[:, 2:4], g[:, 4:6], g[:, 6:8]
        return (p - pad + 0.5) * (crop / new) - 0.5 + origin


class FundusPreprocess:
    """The non-augmenting transform of the reference's `FundusDataModule.get_transforms` for a
    batch: autocrop, resize the longer side to `img_size`, pad to a square, normalise.

    Where the resized side `rint(side * img_size / max(h, w))` would be 0 (a crop more than
    2 * img_size times longer than wide), the reference raises inside OpenCV; here the side is
    clamped to 1.
    """

    def __init__(self, img_size, normalization_mean=IMAGENET_DEFAULT_MEAN,
                 normalization_std=IMAGENET_DEFAULT_STD, threshold: float = 25.0):
        if isinstance(img_size, (tuple, list)):
            if len(img_size) != 2 or img_size[0] != img_size[1]:
                # the reference's chain then gives an output shape that varies with the crop
                raise ValueError(f"img_size must be an int or a square pair, got {img_size}")
            img_size = img_size[0]
        self.img_size = int(img_size)
        if self.img_size < 2:
            raise ValueError(f"img_size must be at least 2, got {img_size}")
        self.normalization_mean = tuple(float(v) for v in normalization_mean)
        self.normalization_std = tuple(float(v) for v in normalization_std)
        if len(self.normalization_mean) != 3 or len(self.normalization_std) != 3 or \
                not all(s > 0 for s in self.normalization_std):
            raise ValueError("normalization_mean and normalization_std are three numbers each, "
                             "every std positive")
        self.autocrop = FundusAutocrop(threshold)

    @torch.no_grad()
    def __call__(self, images, masks=None, return_uint8: bool = False) -> FundusBatch:
        """images: a (B, H, W, 3) uint8 GPU tensor, or a list of (H_b, W_b, 3) uint8 GPU tensors
        of different sizes; masks: (B, H, W) uint8 or a list of (H_b, W_b), or None. Four
        launches per 16 images, no host read."""
        from .. import ops

        boxes = self.autocrop.boxes(images)
        image, u8, mask, geom = ops.fundus_preprocess(
            images, boxes, self.img_size, self.normalization_mean, self.normalization_std,
            masks=masks, want_uint8=return_uint8)
        return FundusBatch(image=image, uint8=u8, mask=mask, boxes=boxes, geom=geom)

    def from_paths(self, paths, return_uint8: bool = False) -> FundusBatch:
        """Decode the images at `paths` with PIL (RGB) and preprocess them as one batch."""
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError(
                "FundusPreprocess.from_paths decodes the images with PIL, which is not "
                "installed: decode them yourself and pass the uint8 tensors to "
                "__call__(images)") from e
        import numpy as np

        images = []
        for path in paths:
            path = Path(path)
            try:
                with Image.open(path) as im:
                    array = np.array(im.convert("RGB"), dtype=np.uint8)
            except OSError as e:
                raise RuntimeError(f"Could not read image {path}") from e
            images.append(torch.from_numpy(array).to("cuda"))
        return self(images, return_uint8=return_uint8)

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}(img_size={self.img_size}, "
                f"normalization_mean={self.normalization_mean}, "
                f"normalization_std={self.normalization_std}, "
                f"threshold={self.autocrop.threshold})")
