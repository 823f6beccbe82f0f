"""SIFT-node extraction (reference src/lesion_gnn/datasets/nodes/sift.py): the configuration
(:11-14, `SiftNodesConfig`) and the extractor (:17-70, `SiftExtractor`).

The reference calls `cv2.SIFT_create(nfeatures=num_keypoints, contrastThreshold=0,
sigma=sigma).detectAndCompute` on the host. Here the image is a uint8 tensor on the GPU and the
whole chain runs in HIP (csrc/sift.hip): the gray conversion, the doubled base image and the
Gaussian and DoG levels of every octave in fp32 (lgnn_sift_pyramid); the 26-neighbour extrema in
(octave, layer, row, column) order (lgnn_sift_count, lgnn_sift_candidates); refinement,
orientation peaks, duplicate removal and the cut at the `num_keypoints`-th largest response, in
float64 (lgnn_sift_keypoints, lgnn_sift_gather); and the 4 x 4 x 8 descriptors
(lgnn_sift_descriptors). It is OpenCV's algorithm with its defaults nOctaveLayers = 3 and
edgeThreshold = 10, restated: tests/sift_ref.py states it in numpy, and agreement with OpenCV
itself is not pinned. Two differences from OpenCV's output are deliberate: the
keypoints come ordered by response (descending, then by octave, layer, row, column), and the
per-keypoint arithmetic is float64 where OpenCV's is float32.

`nodes_from_image` takes one image, `nodes_from_batch` a batch of one size with launch counts and
host reads (two: the candidate total and the node offsets) that do not depend on the batch size;
`__call__` decodes a file with PIL and does what `nodes_from_image` does. Masks, user-provided keypoints
and other SIFT settings are out of scope.
"""
from __future__ import annotations

import dataclasses
import warnings
from pathlib import Path

import torch


@dataclasses.dataclass(kw_only=True)
class SiftNodesConfig:
    num_keypoints: int
    sigma: float


@dataclasses.dataclass
class SiftNodes:
    """The graph of one image before its edges exist: the attributes of the reference's
    `Data(x, pos, score, y, name)` (sift.py:59-65), plus the edge slots KNNGraph, RadiusGraph and
    GaussianDistance fill."""

    x: torch.Tensor      # [n, 128] fp32: descriptors, integers in 0..255
    pos: torch.Tensor    # [n, 2] fp64 (x, y) in the image's pixels
    score: torch.Tensor  # [n] fp64: the keypoints' responses
    y: torch.Tensor      # tensor([label])
    name: str | None = None
    edge_index: torch.Tensor | None = None
    edge_attr: torch.Tensor | None = None


@dataclasses.dataclass
class SiftNodesBatch:
    """The SIFT nodes of B images, flat (`SiftExtractor.nodes_from_batch`): image b owns the rows
    [ptr[b], ptr[b + 1]). `batch[b]` is that image's `SiftNodes`, holding views into the batch;
    `to_store()` hands the tensors to a `GraphStore` as they are."""

    x: torch.Tensor      # [sum n, 128] fp32
    pos: torch.Tensor    # [sum n, 2] fp64
    score: torch.Tensor  # [sum n] fp64
    y: torch.Tensor      # [B] int64, on the host like SiftNodes.y
    ptr: torch.Tensor    # [B + 1] int64 on the device
    names: list | None = None
    ptr_host: torch.Tensor | None = None  # the host copy nodes_from_batch read

    def __post_init__(self):
        if self.ptr_host is None:
            self.ptr_host = self.ptr.cpu()

    def __len__(self) -> int:
        return self.ptr_host.numel() - 1

    def __getitem__(self, b: int) -> SiftNodes:
        b = range(len(self))[b]
        lo, hi = int(self.ptr_host[b]), int(self.ptr_host[b + 1])
        return SiftNodes(x=self.x[lo:hi], pos=self.pos[lo:hi], score=self.score[lo:hi],
                         y=self.y[b:b + 1], name=None if self.names is None else self.names[b])

    def to_store(self):
        from ..memory import GraphStore

        return GraphStore.from_tensors(self.x, self.pos, self.y, self.ptr_host)


class SiftExtractor:
    """Reference SiftExtractor (sift.py:17-70) on the GPU."""

    def __init__(self, num_keypoints: int, sigma: float):
        """Extract SIFT keypoints from an image.

        Args:
            num_keypoints (int): number of keypoints to extract
            sigma (float): sigma for SIFT's Gaussian filter
        """
        self.num_keypoints = num_keypoints
        self.sigma = sigma

    def __call__(self, img_path: Path, label: int) -> SiftNodes:
        """Decode the image at img_path (RGB, as the reference's imread + cvtColor gives) and
        return `nodes_from_image` of it, named by the file's stem."""
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError(
                "SiftExtractor.__call__ decodes the image with PIL, which is not installed: "
                "decode it yourself and pass the uint8 tensor to nodes_from_image(image, label, "
                "name)") from e
        import numpy as np

        img_path = Path(img_path)
        try:
            with Image.open(img_path) as im:
                array = np.array(im.convert("RGB"), dtype=np.uint8)
        except OSError as e:
            raise RuntimeError(f"Could not read image {img_path}") from e
        image = torch.from_numpy(array).to("cuda")
        return self._extract(image[None], [label], [img_path.stem], shown=[img_path])[0]

    def nodes_from_image(self, image: torch.Tensor, label: int,
                         name: str | None = None) -> SiftNodes:
        """image (H, W, 3) or (H, W) uint8 on the GPU -> its SIFT nodes: the `num_keypoints`
        strongest keypoints (all of them, with a warning, when there are fewer; ties at the cut
        are kept), strongest first."""
        if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3):
            raise ValueError("image must be a (H, W, 3) or (H, W) uint8 tensor")
        return self._extract(image[None], [label], None if name is None else [name],
                             shown=[name])[0]

    def nodes_from_batch(self, images: torch.Tensor, labels, names=None) -> SiftNodesBatch:
        """`nodes_from_image` for B images of one size at once: images (B, H, W, 3) or (B, H, W)
        uint8 on the GPU, labels the B graph labels, names B names or None. Image b's rows are
        exactly what `nodes_from_image` gives for it alone. The launch count does not depend on
        B, and the host reads the device twice: the candidate total and the B + 1 node offsets,
        which size the outputs."""
        return self._extract(images, labels, names, shown=names)

    @torch.no_grad()
    def _extract(self, images: torch.Tensor, labels, names, shown) -> SiftNodesBatch:
        """shown: what the warnings call each image (its path, its name, else its index)."""
        from ... import _lib, ops

        if images.dtype != torch.uint8:
            raise ValueError(f"images must be uint8, got {images.dtype}")
        if images.dim() not in (3, 4) or (images.dim() == 4 and images.size(3) != 3):
            raise ValueError("images must be (B, H, W, 3) or (B, H, W)")
        _lib.require_gpu(images)
        if torch.compiler.is_compiling() or torch.cuda.is_current_stream_capturing():
            raise NotImplementedError(
                "SiftExtractor sizes its outputs from the data (host reads): not available under "
                "torch.compile or HIP-graph capture")
        B, H, W = images.shape[:3]
        if B < 1 or H < 2 or W < 2:
            raise ValueError("images must hold at least one image of at least 2 x 2 pixels")
        if not self.sigma > 0:
            raise ValueError(f"sigma must be positive, got {self.sigma}")
        if int(self.num_keypoints) < 1:
            raise ValueError(f"num_keypoints must be at least 1, got {self.num_keypoints}")
        y = torch.as_tensor(labels, dtype=torch.int64, device="cpu").reshape(-1)
        if y.numel() != B:
            raise ValueError(f"{y.numel()} labels for {B} images")
        if names is not None:
            names = list(names)
            if len(names) != B:
                raise ValueError(f"{len(names)} names for {B} images")
        pyramid = ops.sift_pyramid(images, self.sigma)
        cand = ops.sift_candidates(pyramid)  # host read 1: the candidate total
        kf, ki, ptr, ptr_host = ops.sift_keypoints(pyramid, cand, self.sigma,
                                                   int(self.num_keypoints))  # host read 2
        x = ops.sift_descriptors(pyramid, kf, ki)
        for b, n in enumerate((ptr_host[1:] - ptr_host[:-1]).tolist()):
            who = shown[b] if shown is not None and shown[b] is not None else b
            if n == 0:
                warnings.warn(f"Image {who} has no keypoints.")
            elif n < self.num_keypoints:
                warnings.warn(f"Image {who} has less than {self.num_keypoints} keypoints.")
        # the fp32 fields as fp64, like the reference's np.array of Python floats
        return SiftNodesBatch(x=x, pos=kf[:, :2].double(), score=kf[:, 4].double(), y=y, ptr=ptr,
                              names=names, ptr_host=ptr_host)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(num_keypoints={self.num_keypoints}, sigma={self.sigma})"
