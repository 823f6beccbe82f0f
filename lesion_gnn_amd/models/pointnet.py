"""PointNet++ graph classifier — reference src/lesion_gnn/models/pointnet.py (SAModule,
GlobalSAModule, PointNet, PointNetModelConfig, PointNetLightning): two set-abstraction levels
(farthest point sampling, radius neighbourhoods, PointNetConv with a max aggregation), a global
max pool and an MLP head, over the lesions' positions and features; no edge_index.

forward(x, pos, batch) is the drop-in boundary `self.model(data.x, data.pos, data.batch)`. FPS,
the radius search, the split first layer of each PointNetConv, BatchNorm + ReLU, the max
aggregations and the dropout masks are HIP kernels; the Linears run on the dense GEMMs.

Kept quirks of the reference:
- the output is log_softmax(logits). With the CE criterion the loss is the same (log_softmax is
  idempotent); with a regression criterion the single output column is identically 0, so the
  model predicts grade 0 and receives no gradient — as the reference does.
- pos is cast to x's dtype before anything else (the reference's FIXME), so the geometry runs on
  fp32-rounded positions (widened to fp64 for exact, reproducible selections).
- FPS starts at a random point of each graph (`SAModule.random_start = True`, torch_cluster's
  default); tests and reproducible evaluation set it to False.

One forward makes three host reads: the graph sizes (both levels' sample counts and offsets
follow on the host) and the pair count of each of the two radius searches. The shapes depend on
the data, so compile=True and HIP-graph capture of the step raise; so do SyncBN
(`set_sync_bn`) and a forward in a torch.distributed group of more than one rank (out of scope).
"""
from __future__ import annotations

import dataclasses

import torch
import torch.nn as nn

from .. import _lib, cluster, dropout
from ..conv import DenseMLP, PointNetConv, dropout_state, global_max_pool
from ..utils.placeholder import Placeholder
from .base import BaseModelConfig, BaseModule


def _eager_single_process(what: str, x: torch.Tensor) -> None:
    """The contexts this model is not built for, each refused by name."""
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(
            f"{what} under torch.distributed is not supported: its BatchNorms use per-replica "
            "statistics and nothing shards its batches or reduces its gradients")
    if torch.compiler.is_compiling() or (x.is_cuda and torch.cuda.is_current_stream_capturing()):
        raise NotImplementedError(
            f"{what} sizes its outputs from the data (host reads): not available under "
            "torch.compile or HIP-graph capture")


class SAModule(nn.Module):
    """Set abstraction: FPS at `ratio`, neighbours within `radius` (at most 64, the first in
    index order), PointNetConv(nn). Returns (x, pos, batch) of the centroids, in FPS selection
    order. sets / out_sets: the graphs of the input rows and of the centroids when the caller
    already has them (cluster.sets_of / cluster.sampled); else read here (one more host read)."""

    random_start = True

    def __init__(self, ratio: float, radius: float, nn: nn.Module) -> None:
        super().__init__()
        self.ratio = ratio
        self.r = radius
        self.conv = PointNetConv(nn, add_self_loops=False)

    def forward(self, x: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor,
                sets: cluster.Sets | None = None, out_sets: cluster.Sets | None = None):
        _eager_single_process("SAModule", x)
        _lib.require_gpu(x, pos, batch)
        pos = pos.to(x.dtype)
        if sets is None:
            sets = cluster.sets_of(pos, batch, None)
        if out_sets is None:
            out_sets = cluster.sampled(sets, self.ratio)
        pos64 = pos.to(torch.float64)
        idx = cluster.fps_sets(pos64, sets, out_sets, None, self.random_start)
        pg = cluster.radius_sets(pos64, pos64[idx], sets, out_sets, self.r, 64)
        pos_dst = pos[idx]
        x = self.conv((x, None), (pos, pos_dst), pg)
        return x, pos_dst, batch[idx]


class GlobalSAModule(nn.Module):
    def __init__(self, nn: nn.Module) -> None:
        super().__init__()
        self.nn = nn

    def forward(self, x: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor,
                num_graphs: int | None = None) -> torch.Tensor:
        x = self.nn(torch.cat([x, pos.to(x.dtype)], dim=1))
        return global_max_pool(x, batch, num_graphs)


class PointNet(nn.Module):
    def __init__(self, input_features: int, pos_dim: int, num_classes: int):
        super().__init__()
        # input channels account for both `pos` and the node features
        self.sa1_module = SAModule(0.5, 0.2, DenseMLP([input_features + pos_dim, 64, 64, 128]))
        self.sa2_module = SAModule(0.25, 0.4, DenseMLP([128 + pos_dim, 128, 128, 256]))
        self.sa3_module = GlobalSAModule(DenseMLP([256 + pos_dim, 256, 512, 1024]))
        self.mlp = DenseMLP([1024, 512, 256, num_classes], dropout=0.5, norm=None)
        self._dropout_key = repr(0.5)
        # the head's dropout generator (lesion_gnn_amd.dropout; not in state_dict)
        self.register_buffer("_dropout_rng", dropout_state(self), persistent=False)

    def set_sync_bn(self, group, global_count: int | None = None) -> None:
        raise NotImplementedError("PointNet: SyncBatchNorm is not supported (its BatchNorm "
                                  "statistics are per replica)")

    def forward(self, x: torch.Tensor, pos: torch.Tensor, batch: torch.Tensor,
                num_graphs: int | None = None) -> torch.Tensor:
        _eager_single_process("PointNet", x)
        _lib.require_gpu(x, pos, batch)
        sets0 = cluster.sets_of(x, batch, num_graphs)  # the graph sizes: one host read
        sets1 = cluster.sampled(sets0, self.sa1_module.ratio)
        sets2 = cluster.sampled(sets1, self.sa2_module.ratio)
        B = sets0.num_graphs
        masks, p = None, self.mlp.dropout[0]
        if self.training and p > 0.0 and B > 0:  # both head masks in one launch, layer order
            masks = dropout.masks(self._dropout_rng, self.mlp.mask_shapes(B),
                                  dropout.key(self, p))
        x, pos, batch = self.sa1_module(x, pos, batch, sets0, sets1)
        x, pos, batch = self.sa2_module(x, pos, batch, sets1, sets2)
        x = self.sa3_module(x, pos, batch, B)
        return self.mlp(x, masks).log_softmax(dim=-1)


@dataclasses.dataclass(kw_only=True)
class PointNetModelConfig(BaseModelConfig):
    input_features: Placeholder[int] = dataclasses.field(default_factory=Placeholder, init=False)
    pos_dim: int
    compile: bool = False
    name: str = dataclasses.field(default="PointNet", init=False)


class PointNetModule(BaseModule):
    """Reference PointNetLightning (pointnet.py)."""

    def __init__(self, config: PointNetModelConfig):
        super().__init__(config)
        if config.compile:
            raise NotImplementedError(
                "PointNet: compile=True is not supported — FPS and the radius search size their "
                "outputs from the data (host reads), which torch.compile cannot trace")
        self.model = PointNet(
            input_features=config.input_features.value,
            pos_dim=config.pos_dim,
            num_classes=1 if self.is_regression else config.num_classes.value,
        )

    def _model_logits(self, data) -> torch.Tensor:
        return self.model(data.x, data.pos, data.batch, getattr(data, "num_graphs", None))
