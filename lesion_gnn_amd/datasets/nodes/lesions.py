"""Lesion-node extraction (reference src/lesion_gnn/datasets/nodes/lesions.py): the
configuration (:22-71: the feature sources, `FeaturesReduction`, `LesionsNodesConfig`) and the
extractor from the segmentation output on (:147-177).

The front of `LesionsExtractor.__call__` (:111-145: image loading, the fundus segmentation model,
a timm encoder from the HF hub) needs network weights and image data and is out of scope
(DESIGN.md §7). What follows it starts from two tensors and runs on HIP kernels:
`nodes_from_maps` pools the argmax of the segmentation logits to the feature size
(lgnn_label_pool), labels its connected components and takes their centroids (lgnn_ccl,
lgnn_ccl_stats: `connected_components_with_stats`, in place of OpenCV on the host), and pools
the features per component (`extract_features_by_cc`, :88-93, lgnn_cc_pool) into the d_in =
encoder channels + 1 node features. `nodes_from_batch` does the same for a batch of images in one
pass (lgnn_label_pool_batch, lgnn_ccl_batch, lgnn_ccl_stats_batch) and pools the features where
`reinterpolation` would put them without interpolating them first (lgnn_cc_pool_resample).
"""
from __future__ import annotations

import dataclasses
from enum import Enum

import torch


@dataclasses.dataclass(kw_only=True)
class SegmentationEncoderFeatures:
    layer: int


@dataclasses.dataclass(kw_only=True)
class SegmentationDecoderFeatures:
    pass


@dataclasses.dataclass(kw_only=True)
class TimmEncoderFeatures:
    timm_model: str
    layer: int


FeatureSource = SegmentationEncoderFeatures | SegmentationDecoderFeatures | TimmEncoderFeatures


class FeaturesReduction(str, Enum):
    MEAN = "mean"
    MAX = "max"


@dataclasses.dataclass(kw_only=True)
class LesionsNodesConfig:
    feature_source: FeatureSource
    features_reduction: FeaturesReduction = FeaturesReduction.MEAN
    reinterpolation: tuple[int, int] | None = None
    compile: bool = True


def extract_features_by_cc(cc: torch.Tensor, features: torch.Tensor, nlabel: int,
                           reduce: str | FeaturesReduction = "mean") -> torch.Tensor:
    """Reference lesions.py:88-93. cc (H, W) int64 component labels (OpenCV
    connectedComponents), features (1, C, H, W) fp32 on the GPU -> [max(cc) + 1, C]: the mean
    (or max) feature of each component's pixels (torch_scatter.scatter(features.view(C, H*W).T,
    cc.flatten(), 0, reduce)); nlabel == 1 -> features.mean((2, 3)), the (1, C) global mean.
    One HIP launch pair (lgnn_cc_pool) reading the channel-major map once; the output size is
    read from the device (one host sync, as max(cc) + 1 is in torch_scatter)."""
    from ... import ops

    reduce = FeaturesReduction(reduce).value
    if features.dim() != 4 or features.size(0) != 1:
        raise ValueError("features must be (1, C, H, W)")
    C, H, W = features.shape[1:]
    if cc.numel() != H * W:
        raise ValueError("cc must be (H, W) like the feature map")
    f = features.reshape(C, H * W)
    if nlabel == 1:
        return ops.cc_pool(f, torch.zeros_like(cc), 1, reduce_max=False).view(1, C)
    size = int(cc.max().item()) + 1
    return ops.cc_pool(f, cc, size, reduce_max=(reduce == "max"))


def connected_components_with_stats(image: torch.Tensor, connectivity: int = 8):
    """cv2.connectedComponentsWithStats on the GPU (reference lesions.py:158-160): image (H, W),
    nonzero = foreground, cast as the reference's `.byte()` does -> (nlabel: int, cc (H, W)
    int64, stats (nlabel, 5) int32: left, top, width, height, area, centroids (nlabel, 2) fp64:
    x, y), tensors on the device. Label 0 is the background; components are numbered in raster
    order of their first pixel (scipy.ndimage.label's order; OpenCV's may be a permutation of
    it). One host read: nlabel, which sizes the outputs."""
    from ... import ops

    if image.dim() != 2:
        raise ValueError("image must be (H, W)")
    img = image if image.dtype == torch.uint8 else image.to(torch.uint8)
    cc, num = ops.ccl(img, connectivity)
    nlabel = int(num.item())
    stats, centroids = ops.ccl_stats(cc, nlabel, validate=False)
    return nlabel, cc, stats, centroids


@dataclasses.dataclass
class LesionNodes:
    """The graph of one image before its edges exist: the attributes of the reference's
    `Data(pos, y, name, x)` (lesions.py:174-176) that KNNGraph, RadiusGraph and GaussianDistance
    read and write."""

    pos: torch.Tensor  # [n, 2] fp64 (x, y) in the coordinates of the segmentation output
    x: torch.Tensor    # [n, C + 1] fp32: pooled features, then the pooled class
    y: torch.Tensor    # tensor([label])
    name: str | None = None
    edge_index: torch.Tensor | None = None
    edge_attr: torch.Tensor | None = None


@dataclasses.dataclass
class LesionNodesBatch:
    """The lesion nodes of B images, flat (`LesionsExtractor.nodes_from_batch`): image b owns the
    rows [ptr[b], ptr[b + 1]). `batch[b]` is that image's `LesionNodes`, holding views into the
    batch; `to_store()` hands the tensors to a `GraphStore` as they are."""

    x: torch.Tensor    # [sum n, C + 1] fp32
    pos: torch.Tensor  # [sum n, 2] fp64
    y: torch.Tensor    # [B] int64, on the host like LesionNodes.y
    ptr: torch.Tensor  # [B + 1] int64 on the device
    names: list | None = None
    ptr_host: torch.Tensor | None = None  # the host copy nodes_from_batch read

    def __post_init__(self):
        if self.ptr_host is None:
            self.ptr_host = self.ptr.cpu()

    def __len__(self) -> int:
        return self.ptr_host.numel() - 1

    def __getitem__(self, b: int) -> LesionNodes:
        b = range(len(self))[b]
        lo, hi = int(self.ptr_host[b]), int(self.ptr_host[b + 1])
        return LesionNodes(pos=self.pos[lo:hi], x=self.x[lo:hi], y=self.y[b:b + 1],
                           name=None if self.names is None else self.names[b])

    def to_store(self):
        from ..memory import GraphStore

        return GraphStore.from_tensors(self.x, self.pos, self.y, self.ptr_host)


class LesionsExtractor:
    """Reference LesionsExtractor (lesions.py:96-186) from the segmentation output on:
    `nodes_from_maps` is lines 147-176 on the GPU, `nodes_from_batch` the same for a batch of
    images in one pass. The segmentation model, the timm encoder and image loading are not part
    of this package, so `__call__` raises."""

    def __init__(self, config: LesionsNodesConfig):
        self.feature_source = config.feature_source
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.features_reduction = FeaturesReduction(config.features_reduction)
        self.reinterpolation = config.reinterpolation
        # config.compile wraps the scatter in torch.compile in the reference; the HIP launches
        # here have nothing to compile, so it is accepted and ignored

    def __call__(self, img_path, label: int):
        raise NotImplementedError(
            "LesionsExtractor.__call__ needs the fundus segmentation model and image loading, "
            "which are outside this package: run them and pass their outputs to "
            "nodes_from_maps(label_map, features, label, name)")

    @torch.no_grad()
    def nodes_from_maps(self, label_map: torch.Tensor, features: torch.Tensor, label: int,
                        name: str | None = None) -> LesionNodes:
        """label_map (1, K, Horg, Worg) fp32 segmentation logits and features (1, C, h, w) fp32,
        both on the GPU -> the image's lesion nodes (the background's included, as in the
        reference): one node per connected component of the nonzero classes at the feature
        resolution, its centroid scaled back by Horg / H and its mean / max feature with the
        class appended."""
        from ... import _lib, ops

        _lib.require_gpu(label_map, features)
        if label_map.dim() != 4 or label_map.size(0) != 1:
            raise ValueError("label_map must be (1, K, H, W)")
        if features.dim() != 4 or features.size(0) != 1:
            raise ValueError("features must be (1, C, H, W)")
        if self.reinterpolation is not None:
            features = torch.nn.functional.interpolate(
                features, size=self.reinterpolation, mode="bilinear", align_corners=False)
        Horg = label_map.size(2)
        C, H, W = features.shape[1:]
        classes = ops.label_pool(label_map[0], (H, W))
        nlabel, cc, _, centroids = connected_components_with_stats(classes, connectivity=8)
        limit = _lib.LGNN_CC_POOL_MAX_SEGMENTS
        if nlabel > limit:
            raise ValueError(f"{nlabel} components (background included) exceed the {limit} "
                             "segments lgnn_cc_pool takes")
        # (centroids * Horg) / H as numpy rounds it: a tensor divisor, since torch divides a GPU
        # tensor by a Python number as a product with the rounded reciprocal
        centroids = (centroids * Horg) / torch.full_like(centroids, H)
        # pooling is per channel, so the class channel is pooled on its own instead of through a
        # copy of the whole feature map with one channel appended (reference :169)
        reduce_max = self.features_reduction == FeaturesReduction.MAX and nlabel > 1
        lab = cc.reshape(-1)
        x = torch.cat([
            ops.cc_pool(features.reshape(C, H * W), lab, nlabel, reduce_max, validate=False),
            ops.cc_pool(classes.reshape(1, H * W).float(), lab, nlabel, reduce_max,
                        validate=False)], dim=1)
        return LesionNodes(pos=centroids, x=x, y=torch.tensor([label]), name=name)

    @torch.no_grad()
    def nodes_from_batch(self, label_maps: torch.Tensor, features: torch.Tensor, labels,
                         names=None) -> LesionNodesBatch:
        """`nodes_from_maps` for B images at once: label_maps (B, K, Horg, Worg) fp32 logits,
        features (B, C, h, w) fp32, both on the GPU, labels the B graph labels, names B names or
        None. The features are not interpolated to `reinterpolation`: the pooling samples them
        there as it reads (lgnn_cc_pool_resample), so no (B, C, H, W) tensor exists. The launch
        count does not depend on B, and the host reads the device once: the B + 1 node offsets,
        which size the outputs."""
        from ... import _lib, ops

        _lib.require_gpu(label_maps, features)
        if label_maps.dim() != 4:
            raise ValueError("label_maps must be (B, K, H, W)")
        if features.dim() != 4:
            raise ValueError("features must be (B, C, h, w)")
        B = label_maps.size(0)
        if features.size(0) != B:
            raise ValueError(f"label_maps holds {B} images, features {features.size(0)}")
        y = torch.as_tensor(labels, dtype=torch.int64, device="cpu").reshape(-1)
        if y.numel() != B:
            raise ValueError(f"{y.numel()} labels for {B} images")
        if names is not None:
            names = list(names)
            if len(names) != B:
                raise ValueError(f"{len(names)} names for {B} images")
        Horg = label_maps.size(2)
        C = features.size(1)
        H, W = self.reinterpolation if self.reinterpolation is not None else features.shape[2:]
        classes = ops.label_pool_batch(label_maps, (H, W))
        cc, _, ptr = ops.ccl_batch(classes, connectivity=8)
        ptr_host = ptr.cpu()  # the one host read
        sizes = ptr_host[1:] - ptr_host[:-1]
        limit = _lib.LGNN_CC_POOL_MAX_SEGMENTS
        if int(sizes.max()) > limit:
            b = int(sizes.argmax())
            raise ValueError(f"image {b}: {int(sizes[b])} components (background included) "
                             f"exceed the {limit} segments lgnn_cc_pool_resample takes")
        total, nmax = int(ptr_host[-1]), int(sizes.max())
        _, centroids = ops.ccl_stats_batch(cc, ptr, total, validate=False)
        # the same tensor divisor as nodes_from_maps
        centroids = (centroids * Horg) / torch.full_like(centroids, H)
        reduce_max = self.features_reduction == FeaturesReduction.MAX
        cls = classes.view(B, 1, H, W).float()

        def pool(f, c, lab, p, n, mx, rmax):
            return torch.cat([
                ops.cc_pool_resample(f, lab, p, n, rmax, max_nodes=mx, validate=False),
                ops.cc_pool_resample(c, lab, p, n, rmax, max_nodes=mx, validate=False)], dim=1)

        x = pool(features, cls, cc, ptr, total, nmax, reduce_max)
        lone = torch.nonzero(sizes == 1).reshape(-1)
        if reduce_max and lone.numel():
            # an image that is all background has one node, which the reference gives the mean
            # (nlabel == 1 in extract_features_by_cc), also under MAX
            idx = lone.to(x.device)
            sub_ptr = torch.arange(lone.numel() + 1, dtype=torch.int64).to(x.device)
            x[ptr_host[lone].to(x.device)] = pool(features[idx], cls[idx], cc[idx], sub_ptr,
                                                  lone.numel(), 1, False)
        return LesionNodesBatch(x=x, pos=centroids, y=y, ptr=ptr, names=names, ptr_host=ptr_host)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(feature_source={self.feature_source})"
