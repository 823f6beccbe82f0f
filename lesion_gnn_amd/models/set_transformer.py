"""SetTransformer graph classifier — reference src/lesion_gnn/models/set_transformer.py:16-107
(SetTransformer, SetTransformerModelConfig, SetTransformerLightning): the lesions of an image as
an unordered set, no edges.

forward(x, batch) is the drop-in boundary `self.model(data.x, data.batch)` (reference :102):
in_proj -> ISAB x E -> PMA -> SAB x D -> flatten (concat) or mean over the seed rows -> out_proj.
The reference pads every set to the longest (to_dense_batch) and masks; here each set is the
contiguous row range Batch.ptr delimits and every attention block is one HIP autograd node
(ops.mab). The reference's quirk is kept: out_proj is Linear(inner_dim, num_classes) even with
concat=True, so concat works with num_seed_points = 1 only; its Lightning wrapper never passes
`concat`, so it stays True (mirrored by SetTransformerModule).

One difference: for a graph without nodes the reference returns NaN logits (a softmax over no
keys); this model returns finite ones (the attention output of an empty set is zero).
"""
from __future__ import annotations

import dataclasses

import torch
import torch.nn as nn

from .. import ops
from ..conv import (InducedSetAttentionBlock, PoolingByMultiheadAttention, SetAttentionBlock,
                    _pool_graph, _set_masks, dropout_state)
from ..utils.placeholder import Placeholder
from .base import BaseModelConfig, BaseModule


class SetTransformer(nn.Module):
    def __init__(self, input_features: int, inner_dim: int, num_classes: int,
                 num_inducing_points: int = 1, num_seed_points: int = 1,
                 num_encoder_blocks: int = 1, num_decoder_blocks: int = 1, heads: int = 1,
                 concat: bool = True, layer_norm: bool = False, dropout: float = 0.0) -> None:
        super().__init__()
        self.concat = concat
        self.num_seed_points = num_seed_points
        self.in_proj = nn.Linear(input_features, inner_dim)
        self.encoders = nn.ModuleList(
            [InducedSetAttentionBlock(inner_dim, num_inducing_points, heads, layer_norm, dropout)
             for _ in range(num_encoder_blocks)])
        self.pma = PoolingByMultiheadAttention(inner_dim, num_seed_points, heads, layer_norm,
                                               dropout)
        self.decoders = nn.ModuleList([SetAttentionBlock(inner_dim, heads, layer_norm, dropout)
                                       for _ in range(num_decoder_blocks)])
        self.out_proj = nn.Linear(inner_dim, num_classes)
        self.dropout = float(dropout)
        self._dropout_key = repr(self.dropout)
        # the attention-dropout generator (lesion_gnn_amd.dropout; not in state_dict), seeded by
        # the generator state and this model's initial weights
        self.register_buffer("_dropout_rng", dropout_state(self), persistent=False)

    def reset_parameters(self):
        self.in_proj.reset_parameters()
        for encoder in self.encoders:
            encoder.reset_parameters()
        self.pma.reset_parameters()
        for decoder in self.decoders:
            decoder.reset_parameters()
        self.out_proj.reset_parameters()

    def forward(self, x: torch.Tensor, batch: torch.Tensor,
                num_graphs: int | None = None) -> torch.Tensor:
        g = _pool_graph(x, batch, num_graphs)
        gptr, B, S, M = g.gptr, g.num_graphs, self.num_seed_points, x.size(0)
        # every attention-dropout mask of this forward in one launch, sites in execution order
        masks = _set_masks(self, [(b, (M, gptr, B)) for b in self.encoders]
                           + [(self.pma, (M, gptr, B))]
                           + [(b, (B * S, None, B, S)) for b in self.decoders])
        x = ops.linear_auto(x, self.in_proj.weight, self.in_proj.bias)
        for encoder in self.encoders:
            x = encoder(x, gptr, B, masks=masks.pop(0))
        x = self.pma(x, gptr, B, masks=masks.pop(0))
        for decoder in self.decoders:
            x = decoder(x, None, B, S, masks=masks.pop(0))
        x = x.view(B, -1) if self.concat else ops.set_readout(x, None, B, S, True)
        return ops.linear_auto(x, self.out_proj.weight, self.out_proj.bias)


@dataclasses.dataclass(kw_only=True)
class SetTransformerModelConfig(BaseModelConfig):
    input_features: Placeholder[int] = dataclasses.field(default_factory=Placeholder, init=False)
    inner_dim: int
    num_inducing_points: int
    num_seed_points: int
    num_encoder_blocks: int
    num_decoder_blocks: int
    heads: int
    layer_norm: bool
    dropout: float
    compile: bool = False
    name: str = dataclasses.field(default="SetTransformer", init=False)


class SetTransformerModule(BaseModule):
    """Reference SetTransformerLightning (set_transformer.py:84-107)."""

    def __init__(self, config: SetTransformerModelConfig):
        super().__init__(config)
        model = SetTransformer(
            input_features=config.input_features.value,
            inner_dim=config.inner_dim,
            num_classes=1 if self.is_regression else config.num_classes.value,
            num_inducing_points=config.num_inducing_points,
            num_seed_points=config.num_seed_points,
            num_encoder_blocks=config.num_encoder_blocks,
            num_decoder_blocks=config.num_decoder_blocks,
            heads=config.heads,
            layer_norm=config.layer_norm,
            dropout=config.dropout,
        )
        self.model = torch.compile(model, dynamic=True) if config.compile else model

    def _model_logits(self, data) -> torch.Tensor:
        return self.model(data.x, data.batch, getattr(data, "num_graphs", None))
