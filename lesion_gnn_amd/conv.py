"""Message-passing layers with PyG 2.5.1 constructor signatures and state_dict keys, computed by
the HIP kernels of liblgnn.so.

GCNConv  — PyG GCNConv(in, out): keys `lin.weight`, `bias` (added conv)
GINConv  — PyG GINConv(nn, eps=0): keys `nn.*`, `eps` (reference gin.py:23)
GraphConv — PyG GraphConv(in, out): keys `lin_rel.*`, `lin_root.weight` (DRGNet,
           reference models/drgnet.py:30-33,55)
global_mean_pool / global_add_pool — reference gin.py:33 / gat.py:56 (+ add)
PointNetConv, DenseMLP (PyG MLP with ReLU), global_max_pool — reference models/pointnet.py
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib, dropout, ops
from .graph import Graph, as_graph


def glorot_(t: torch.Tensor) -> None:
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-a, a)


class GCNConv(nn.Module):
    """out = D^-1/2 (A + I) D^-1/2 X W^T + b (gcn_norm with add_remaining_self_loops)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        glorot_(self.lin.weight)

    def forward(self, x: torch.Tensor, edge_index, act: int = _lib.LGNN_ACT_NONE) -> torch.Tensor:
        g = as_graph(edge_index, x.size(0))
        return ops.node_linear(x, self.lin.weight, self.bias, g, "gcn", 0.0, act)


class GraphConv(nn.Module):
    """out_i = lin_rel(sum_{j->i} w_ji x_j) + lin_root(x_i) (aggr 'add', no self loops), with the
    optional per-edge weight of the reference's GaussianDistance transform (drgnet.py:55, :103).

    The weighted aggregation runs in the HIP segmented-sum kernel (lgnn_spmm, transpose CSR in
    the backward) on whichever side of lin_rel has a width divisible by 4 — A(X) W^T == A(X W^T)
    — so DRGNet's wide input layer (d_in 1025) aggregates its `hidden` outputs and the final
    GraphConv(hidden, 1) its inputs; the two Linears run on the tile kernels or the library GEMM
    (ops.linear_auto)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin_rel = nn.Linear(in_channels, out_channels, bias=True)
        self.lin_root = nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, x: torch.Tensor, edge_index, edge_weight: torch.Tensor | None = None,
                elu: bool = False) -> torch.Tensor:
        """elu=True returns ELU(out) with the sum of the two branches and the activation as one
        HIP launch (ops.add_elu) and the bias inside a Linear kernel on every route, so that no
        torch elementwise op stands between the lgnn ops (DRGNet: eager and compiled then run the
        same kernels)."""
        _lib.require_gpu(x)
        g = as_graph(edge_index, x.size(0))
        if edge_weight is None and g.adj_values is not None:  # weighted adj_t (ToSparseTensor)
            edge_weight = g.adj_values
        kind = g.weighted(edge_weight) if edge_weight is not None else "gin"
        K, N = self.in_channels, self.out_channels
        if elu and not (K % 4 == 0 and (N % 4 != 0 or K <= N)) and N % 4 == 0:
            # lin_rel's bias rides on lin_root's kernel (the aggregation comes after lin_rel here)
            root = ops.linear_auto(x, self.lin_root.weight, self.lin_rel.bias)
            return ops.add_elu(ops.spmm(ops.linear_auto(x, self.lin_rel.weight), g, kind), root)
        root = ops.linear_auto(x, self.lin_root.weight)
        if K % 4 == 0 and (N % 4 != 0 or K <= N):
            rel = ops.linear_auto(ops.spmm(x, g, kind), self.lin_rel.weight, self.lin_rel.bias)
        elif N % 4 == 0:
            rel = ops.spmm(ops.linear_auto(x, self.lin_rel.weight), g, kind) + self.lin_rel.bias
        else:  # neither width divisible by 4: zero-pad the input columns for the aggregation
            pad = (-K) % 4
            agg = ops.spmm(torch.nn.functional.pad(x, (0, pad)), g, kind)[:, :K]
            rel = ops.linear_auto(agg, self.lin_rel.weight, self.lin_rel.bias)
        return ops.add_elu(rel, root) if elu else rel + root


class BatchNorm(nn.Module):
    """torch_geometric.nn.norm.BatchNorm: torch.nn.BatchNorm1d wrapped as `.module` (state_dict
    keys `module.{weight,bias,running_mean,running_var,num_batches_tracked}`)."""

    def __init__(self, in_channels: int, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.module = nn.BatchNorm1d(in_channels, eps=eps, momentum=momentum)


class MLP(nn.Module):
    """Parameter container with PyG MLP(channel_list, act="ELU", dropout=p) structure
    (norm="batch_norm", plain_last=True): `lins.{i}`, `norms.{i}.module`. The 3-entry form of the
    reference GIN (gin.py:23) is computed by the fused GINConv kernel chain."""

    def __init__(self, channel_list: list[int], dropout: float = 0.0):
        super().__init__()
        if len(channel_list) != 3:
            raise ValueError("the fused GIN MLP supports channel_list [d1, d2, d3] (reference "
                             "gin.py:23 uses [d1, d2, d2])")
        self.channel_list = list(channel_list)
        self.dropout = float(dropout)
        self._dropout_key = repr(self.dropout)
        self.lins = nn.ModuleList([nn.Linear(a, b) for a, b in
                                   zip(channel_list[:-1], channel_list[1:])])
        self.norms = nn.ModuleList([BatchNorm(channel_list[1])])


class GINConv(nn.Module):
    """PyG GINConv(nn, eps=0, train_eps=False): nn((1 + eps) x_i + sum_{j->i} x_j), with `nn` a
    2-layer MLP with BatchNorm + ELU (reference gin.py:23); keys `nn.*` and the `eps` buffer."""

    def __init__(self, mlp: MLP, eps: float = 0.0):
        super().__init__()
        self.nn = mlp
        self.initial_eps = float(eps)  # train_eps=False: eps stays at its initial value
        self.register_buffer("eps", torch.full((1,), float(eps)))
        self.sync_group = None  # torch.distributed group for SyncBN (None: per-replica stats)
        self.sync_count = None  # fixed global node count under SyncBN (None: all-reduced)

    def _mask(self, x: torch.Tensor, mask):
        """The MLP's dropout mask: the model's (drawn with its other masks in one launch), else
        one drawn here from the device's global generator; None when dropout is inactive."""
        mlp = self.nn
        if mask is not None or mlp.dropout == 0.0 or not self.training:
            return mask if (mlp.dropout > 0.0 and self.training) else None
        return dropout.masks(dropout.global_state(x.device),
                             [(x.size(0), mlp.channel_list[1])], dropout.key(mlp, mlp.dropout))[0]

    def forward(self, x: torch.Tensor, edge_index, act: int = _lib.LGNN_ACT_NONE,
                mask: torch.Tensor | None = None) -> torch.Tensor:
        g = as_graph(edge_index, x.size(0))
        mlp = self.nn
        bn = mlp.norms[0].module
        mask = self._mask(x, mask)
        return ops.gin_conv(x, mlp.lins[0].weight, mlp.lins[0].bias, bn, mlp.lins[1].weight,
                            mlp.lins[1].bias, g, self.initial_eps, mask, act, self.sync_group,
                            self.sync_count)

    def stack_spec(self, x: torch.Tensor, act: int, mask: torch.Tensor | None = None) -> dict:
        """This conv's weights, BatchNorm, eps and dropout mask for ops.gin_stack."""
        mlp = self.nn
        mask = self._mask(x, mask)
        return dict(W1=mlp.lins[0].weight, b1=mlp.lins[0].bias, bn=mlp.norms[0].module,
                    W2=mlp.lins[1].weight, b2=mlp.lins[1].bias, eps=self.initial_eps, mask=mask,
                    act=act, group=self.sync_group, sync_count=self.sync_count)

    def head_fusable(self, x: torch.Tensor) -> bool:
        mlp = self.nn
        return ops.gin_conv_head_eligible(x, mlp.lins[0].weight, mlp.lins[1].weight)

    def forward_head(self, x: torch.Tensor, g, act: int, W_out: torch.Tensor,
                     b_out: torch.Tensor, mean: bool, mask: torch.Tensor | None = None
                     ) -> torch.Tensor:
        """forward(x) followed by global pool + out_proj (W_out, b_out) in one autograd node
        (ops.gin_conv_head): the model's last conv and readout. Returns the logits."""
        mlp = self.nn
        bn = mlp.norms[0].module
        mask = self._mask(x, mask)
        return ops.gin_conv_head(x, mlp.lins[0].weight, mlp.lins[0].bias, bn, mlp.lins[1].weight,
                                 mlp.lins[1].bias, W_out, b_out, g, self.initial_eps, mask, act,
                                 self.sync_group, self.sync_count, mean)


class GATConv(nn.Module):
    """PyG 2.5.1 GATConv(in, out, heads, dropout) with concat=True, negative_slope=0.2,
    add_self_loops=True, bias=True (reference gat.py:31). state_dict: `lin.weight`, `att_src`,
    `att_dst` [1, H, C], `bias` [H*C]."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, dropout: float = 0.0,
                 negative_slope: float = 0.2):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.negative_slope, self.dropout = negative_slope, dropout
        self._dropout_key = repr(float(dropout))
        self.lin = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels))
        glorot_(self.lin.weight)
        glorot_(self.att_src)
        glorot_(self.att_dst)

    def mask_shape(self, g) -> tuple:
        """The attention-dropout mask: one multiplier per (target-CSR slot, head)."""
        return (g.csr("gat").col.numel(), self.heads)

    def _mask(self, x: torch.Tensor, g, mask):
        if self.dropout == 0.0 or not self.training:
            return None
        if mask is not None:
            return mask
        return dropout.masks(dropout.global_state(x.device), [self.mask_shape(g)],
                             dropout.key(self, self.dropout))[0]

    def forward(self, x: torch.Tensor, edge_index, act: int = _lib.LGNN_ACT_NONE,
                bf16: bool = False, mask: torch.Tensor | None = None,
                planes: tuple | None = None) -> torch.Tensor:
        """planes: (lin.weight's, its transpose's) split-3 planes from ops.s3_weight_bundle."""
        g = as_graph(edge_index, x.size(0))
        mask = self._mask(x, g, mask)
        return ops.gat_conv(x, self.lin.weight, self.att_src, self.att_dst, self.bias, g,
                            self.heads, self.negative_slope, mask, act, bf16, planes)

    def forward_head(self, x: torch.Tensor, g, act: int, W_out: torch.Tensor,
                     b_out: torch.Tensor, mean: bool, bf16: bool = False,
                     mask: torch.Tensor | None = None, planes: tuple | None = None
                     ) -> torch.Tensor:
        """forward(x) followed by global pool + out_proj (W_out, b_out) in one autograd node
        (ops.gat_conv_head): the model's last conv and readout. Returns the logits."""
        mask = self._mask(x, g, mask)
        return ops.gat_conv_head(x, self.lin.weight, self.att_src, self.att_dst, self.bias,
                                 W_out, b_out, g, self.heads, self.negative_slope, mask, act,
                                 bf16, mean, planes)


def global_mean_pool(x: torch.Tensor, batch: torch.Tensor, size: int | None = None,
                     graph: Graph | None = None) -> torch.Tensor:
    g = graph if graph is not None else _pool_graph(x, batch, size)
    return ops.segment_pool(x, g, mean=True)


def global_add_pool(x: torch.Tensor, batch: torch.Tensor, size: int | None = None,
                    graph: Graph | None = None) -> torch.Tensor:
    g = graph if graph is not None else _pool_graph(x, batch, size)
    return ops.segment_pool(x, g, mean=False)


def global_max_pool(x: torch.Tensor, batch: torch.Tensor, size: int | None = None,
                    graph: Graph | None = None) -> torch.Tensor:
    """PyG global_max_pool; a graph without nodes gives a zero row (PyG's scatter fill)."""
    g = graph if graph is not None else _pool_graph(x, batch, size)
    return ops.segment_max(x, g.gptr.to(torch.int64), g.num_graphs)


def _pool_graph(x: torch.Tensor, batch: torch.Tensor, size: int | None) -> Graph:
    _lib.require_gpu(x, batch)
    empty = torch.empty(2, 0, dtype=torch.int64, device=x.device)
    return Graph(empty, x.size(0), batch, size)


# ----------------------------------------------------------------------------------------------
# PointNet++: PyG 2.5.1 MLP (act="relu", norm="batch_norm" or None, plain_last=True) and
# PointNetConv(local_nn, aggr="max") as the reference's SAModule / GlobalSAModule use them.
# ----------------------------------------------------------------------------------------------


class DenseMLP(nn.Module):
    """PyG MLP(channel_list, dropout=p, act="relu", norm="batch_norm" | None, plain_last=True) for
    any channel list: every layer but the last is Linear -> BatchNorm -> ReLU -> dropout, the
    last a plain Linear. Keys `lins.{i}.{weight,bias}`, `norms.{i}.module.*` (norm=None: no norm
    keys, as PyG's Identity entries). The Linears run on the dense GEMMs (ops.linear_auto), norm +
    ReLU + dropout mask in one launch (ops.bn_act_rows). dropout: one probability or one per
    hidden layer."""

    def __init__(self, channel_list: list[int], dropout: float | list[float] = 0.0,
                 norm: str | None = "batch_norm"):
        super().__init__()
        if len(channel_list) < 2:
            raise ValueError("channel_list needs at least an input and an output width")
        if norm not in ("batch_norm", None):
            raise NotImplementedError(f"norm={norm!r}: only 'batch_norm' and None")
        hidden = len(channel_list) - 2
        if isinstance(dropout, (int, float)):
            dropout = [float(dropout)] * hidden
        if len(dropout) != hidden:
            raise ValueError("one dropout probability per hidden layer")
        self.channel_list = list(channel_list)
        self.dropout = [float(p) for p in dropout]
        self.lins = nn.ModuleList([nn.Linear(a, b) for a, b in
                                   zip(channel_list[:-1], channel_list[1:])])
        self.norms = nn.ModuleList([BatchNorm(c) if norm else nn.Identity()
                                    for c in channel_list[1:-1]])

    def mask_shapes(self, rows: int) -> list:
        """The shape of each hidden layer's dropout mask over `rows` rows (layers with p = 0
        included: their entry is not drawn)."""
        return [(rows, c) for c in self.channel_list[1:-1]]

    def forward(self, x: torch.Tensor | None, masks: list | None = None,
                z0: torch.Tensor | None = None, sums0: torch.Tensor | None = None
                ) -> torch.Tensor:
        """masks: per hidden layer its dropout keep-mask (or None), drawn by the owning model —
        without them an active dropout draws from the per-device generator. z0 (with sums0, its
        BatchNorm column sums): the first Linear's output when the caller computed it
        (PointNetConv's split first layer); x is then unused."""
        last = len(self.lins) - 1
        for i, lin in enumerate(self.lins):
            z = z0 if i == 0 and z0 is not None else ops.linear_auto(x, lin.weight, lin.bias)
            if i == last:
                return z
            p = self.dropout[i]
            mask = masks[i] if masks is not None else None
            if mask is None and p > 0.0 and self.training:
                mask = dropout.masks(dropout.global_state(z.device), [tuple(z.shape)], p)[0]
            norm = self.norms[i]
            x = ops.bn_act_rows(z, norm.module if isinstance(norm, BatchNorm) else None,
                                self.training, _lib.LGNN_ACT_RELU,
                                mask if self.training else None,
                                sums0 if i == 0 and z0 is not None else None)


class PointNetConv(nn.Module):
    """PyG PointNetConv(local_nn, global_nn=None, add_self_loops=False), aggr='max':
    out_i = max_{j in N(i)} local_nn(cat[x_j, pos_j - pos_i]), 0 where N(i) is empty. Keys
    `local_nn.*`.

    local_nn's first Linear is never applied per edge: with W1 = [Wx | Wp],
    cat[x_j, pos_j - pos_i] W1^T + b1 = U[j] - V[i] for U = cat[x, pos] W1^T + b1 (one row per
    point) and V = pos_dst Wp^T (one row per centroid); the per-edge rows are their gathered
    difference (ops.edge_sub), and dW1, db1, dx come from the node-level dU and dV. The rest of
    local_nn runs over the E rows, then the max over each centroid's rows (ops.segment_max).

    forward(x, pos, edge_index): x = the points' features or (x, x_dst) (x_dst is unused without
    a global_nn), pos = (pos, pos_dst), edge_index = a cluster.PairGraph (radius_sets) or PyG's
    [2, E] = [point j; centroid i] sorted by i, then j."""

    def __init__(self, local_nn: DenseMLP | None = None, global_nn: nn.Module | None = None,
                 add_self_loops: bool = False):
        super().__init__()
        if global_nn is not None:
            raise NotImplementedError("PointNetConv: global_nn is not supported (the reference "
                                      "passes none)")
        if add_self_loops:
            raise NotImplementedError("PointNetConv: add_self_loops=True is not supported (the "
                                      "reference's SAModule passes False)")
        if not isinstance(local_nn, DenseMLP):
            raise NotImplementedError("PointNetConv: local_nn must be a conv.DenseMLP")
        self.local_nn = local_nn

    def forward(self, x, pos, edge_index) -> torch.Tensor:
        from .cluster import PairGraph

        x = x[0] if isinstance(x, (tuple, list)) else x
        if x is None:
            raise NotImplementedError("PointNetConv: x=None (positions only) is not supported")
        pos, pos_dst = pos if isinstance(pos, (tuple, list)) else (pos, pos)
        _lib.require_gpu(x, pos, pos_dst)
        pg = edge_index if isinstance(edge_index, PairGraph) else \
            PairGraph.from_edge_index(edge_index, x.size(0), pos_dst.size(0))
        lin = self.local_nn.lins[0]
        dims = pos.size(1)
        if lin.in_features != x.size(1) + dims:
            raise ValueError("local_nn's input width must be x's channels + pos's dimension")
        pos, pos_dst = pos.to(x.dtype), pos_dst.to(x.dtype)
        U = ops.linear_auto(torch.cat([x, pos], dim=1), lin.weight, lin.bias)
        V = ops.linear_auto(pos_dst, lin.weight[:, x.size(1):])
        z, sums = ops.edge_sub(U, V, pg)
        msg = self.local_nn(None, z0=z, sums0=sums)
        return ops.segment_max(msg, pg.rowoff, pg.num_queries)


class SortAggregation(nn.Module):
    """PyG 2.5.1 SortAggregation(k) (reference models/drgnet.py:37, :59): per graph, rows sorted
    by the last channel (descending, stable), top k kept (zero rows when fewer), elements equal
    to min(x) - 1 zeroed; [ΣN, D] -> [B, k * D]. HIP: lgnn_sort_pool_fwd / _bwd."""

    def __init__(self, k: int):
        super().__init__()
        self.k = int(k)

    def forward(self, x: torch.Tensor, index: torch.Tensor | None = None,
                ptr: torch.Tensor | None = None, dim_size: int | None = None, dim: int = -2,
                graph: Graph | None = None) -> torch.Tensor:
        if dim not in (-2, 0) or x.dim() != 2:
            raise ValueError("SortAggregation: x must be [num_nodes, channels], dim=-2")
        if graph is None:
            if index is None:
                raise ValueError("SortAggregation needs the batch index (or a Graph)")
            graph = _pool_graph(x, index, dim_size)
        return ops.sort_pool(x, graph, self.k)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(k={self.k})"


# ----------------------------------------------------------------------------------------------
# Set attention: PyG 2.5.1 torch_geometric/nn/aggr/utils.py + set_transformer.py on ragged sets
# (the rows of a set are contiguous, delimited by Batch.ptr; nothing is padded or masked).
# The nn.MultiheadAttention / nn.Linear / nn.LayerNorm members are parameter containers with
# PyG's state_dict keys; their forward is never called (ops.mab runs the HIP kernels).
# ----------------------------------------------------------------------------------------------


def _ragged_self_mask_numel(ptr: torch.Tensor, heads: int) -> int:
    """heads * sum_g n_g^2: the attention-dropout mask of a SetAttentionBlock over ragged sets.
    The size depends on the set sizes, so it is read from the device (one synchronisation):
    eager mode only."""
    if torch.compiler.is_compiling() or torch.cuda.is_current_stream_capturing():
        raise NotImplementedError(
            "attention dropout of a SetAttentionBlock over ragged sets sizes its mask from the "
            "set sizes (a host read): not available under torch.compile or graph capture")
    n = (ptr[1:] - ptr[:-1]).to(torch.int64)
    return int((n * n).sum().item()) * heads


def draw_attention_masks(state: torch.Tensor, numels: list, key: str) -> list:
    """One flat dropout mask per attention site (site j from stream j of its launch, the sites in
    execution order), lgnn.h's LGNN_MAX_MASKS per launch."""
    out = []
    for i in range(0, len(numels), dropout.MAX_MASKS):
        out += dropout.masks(state, [(n,) for n in numels[i:i + dropout.MAX_MASKS]], key)
    return out


class MultiheadAttentionBlock(nn.Module):
    """PyG MultiheadAttentionBlock(channels, heads, layer_norm, dropout): keys `attn.*`, `lin.*`,
    `layer_norm1.*`, `layer_norm2.*`. forward(x, y, form): x the query rows, y the key rows (None:
    y is x), form the ops.AttnForm saying which rows belong to which set."""

    sites = 1  # attention-dropout sites of one forward

    def __init__(self, channels: int, heads: int = 1, layer_norm: bool = True,
                 dropout: float = 0.0):
        super().__init__()
        self.channels, self.heads, self.dropout = channels, heads, float(dropout)
        self.attn = nn.MultiheadAttention(channels, heads, batch_first=True, dropout=dropout)
        self.lin = nn.Linear(channels, channels)
        self.layer_norm1 = nn.LayerNorm(channels) if layer_norm else None
        self.layer_norm2 = nn.LayerNorm(channels) if layer_norm else None
        self._dropout_key = repr(self.dropout)

    def reset_parameters(self):
        self.attn._reset_parameters()
        self.lin.reset_parameters()
        if self.layer_norm1 is not None:
            self.layer_norm1.reset_parameters()
            self.layer_norm2.reset_parameters()

    def params(self) -> list:
        ln = [None] * 4 if self.layer_norm1 is None else [
            self.layer_norm1.weight, self.layer_norm1.bias, self.layer_norm2.weight,
            self.layer_norm2.bias]
        return [self.attn.in_proj_weight, self.attn.in_proj_bias, self.attn.out_proj.weight,
                self.attn.out_proj.bias, self.lin.weight, self.lin.bias] + ln

    def mask_numel(self, form: ops.AttnForm, Mq: int, Mk: int):
        n = ops.set_attn_mask_numel(form, self.heads, Mq, Mk)
        return n if n is not None else _ragged_self_mask_numel(form.qptr, self.heads)

    def forward(self, x: torch.Tensor, y: torch.Tensor | None, form: ops.AttnForm,
                mask: torch.Tensor | None = None) -> torch.Tensor:
        if mask is None and self.training and self.dropout > 0.0:
            # a lone block: its mask from the per-device generator (a model draws all of its
            # forward's masks in one launch and passes them in)
            k = x if y is None else y
            mask = draw_attention_masks(dropout.global_state(x.device),
                                        [self.mask_numel(form, x.size(0), k.size(0))],
                                        dropout.key(self, self.dropout))[0]
        return ops.mab(x, y, self.params(), form, self.heads, mask)

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}({self.channels}, heads={self.heads}, "
                f"layer_norm={self.layer_norm1 is not None}, dropout={self.dropout})")


def _set_form(ptr, num_sets: int, rows: int) -> tuple:
    """(ptr, rows per set) of a row layout: ragged by ptr, or `rows` rows per set."""
    return (ptr, 0) if ptr is not None else (None, int(rows))


class SetAttentionBlock(nn.Module):
    """PyG SetAttentionBlock: mab(x, x) per set. Key prefix `mab.`. The sets are ragged (ptr,
    Batch.ptr as int32) or hold `rows` rows each (ptr None)."""

    sites = 1

    def __init__(self, channels: int, heads: int = 1, layer_norm: bool = True,
                 dropout: float = 0.0):
        super().__init__()
        self.mab = MultiheadAttentionBlock(channels, heads, layer_norm, dropout)

    def reset_parameters(self):
        self.mab.reset_parameters()

    def form(self, ptr, num_sets: int, rows: int = 0) -> ops.AttnForm:
        p, r = _set_form(ptr, num_sets, rows)
        return ops.AttnForm(p, r, False, p, r, num_sets)

    def mask_numels(self, M: int, ptr, num_sets: int, rows: int = 0) -> list:
        return [self.mab.mask_numel(self.form(ptr, num_sets, rows), M, M)]

    def forward(self, x, ptr=None, num_sets: int | None = None, rows: int = 0, masks=None):
        return self.mab(x, None, self.form(ptr, num_sets, rows),
                        masks[0] if masks is not None else None)


class InducedSetAttentionBlock(nn.Module):
    """PyG InducedSetAttentionBlock: h = mab1(ind, x) (the same m inducing rows query every set),
    out = mab2(x, h). Keys `ind`, `mab1.*`, `mab2.*`."""

    sites = 2

    def __init__(self, channels: int, num_induced_points: int, heads: int = 1,
                 layer_norm: bool = True, dropout: float = 0.0):
        super().__init__()
        self.ind = nn.Parameter(torch.empty(1, num_induced_points, channels))
        self.mab1 = MultiheadAttentionBlock(channels, heads, layer_norm, dropout)
        self.mab2 = MultiheadAttentionBlock(channels, heads, layer_norm, dropout)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.ind)
        self.mab1.reset_parameters()
        self.mab2.reset_parameters()

    def forms(self, ptr, num_sets: int, rows: int = 0):
        p, r = _set_form(ptr, num_sets, rows)
        m = self.ind.size(1)
        return (ops.AttnForm(None, m, True, p, r, num_sets),
                ops.AttnForm(p, r, False, None, m, num_sets))

    def mask_numels(self, M: int, ptr, num_sets: int, rows: int = 0) -> list:
        f1, f2 = self.forms(ptr, num_sets, rows)
        m = self.ind.size(1)
        return [self.mab1.mask_numel(f1, m, M), self.mab2.mask_numel(f2, M, num_sets * m)]

    def forward(self, x, ptr=None, num_sets: int | None = None, rows: int = 0, masks=None):
        m1, m2 = masks if masks is not None else (None, None)
        if masks is None and self.training and self.mab1.dropout > 0.0:
            # a lone block: its masks from the per-device generator
            m1, m2 = draw_attention_masks(dropout.global_state(x.device),
                                          self.mask_numels(x.size(0), ptr, num_sets, rows),
                                          dropout.key(self.mab1, self.mab1.dropout))
        p, r = _set_form(ptr, num_sets, rows)
        return ops.isab(x, self.ind.view(self.ind.size(1), -1), self.mab1.params(),
                        self.mab2.params(), p, r, num_sets, self.mab1.heads, m1, m2)


class PoolingByMultiheadAttention(nn.Module):
    """PyG PoolingByMultiheadAttention: mab(seed, relu(lin(x))), S rows per set. Keys `lin.*`,
    `seed`, `mab.*`. Output [num_sets * S, channels], set g at rows [g * S, (g + 1) * S)."""

    sites = 1

    def __init__(self, channels: int, num_seed_points: int = 1, heads: int = 1,
                 layer_norm: bool = True, dropout: float = 0.0):
        super().__init__()
        self.lin = nn.Linear(channels, channels)
        self.seed = nn.Parameter(torch.empty(1, num_seed_points, channels))
        self.mab = MultiheadAttentionBlock(channels, heads, layer_norm, dropout)
        self.reset_parameters()

    def reset_parameters(self):
        self.lin.reset_parameters()
        glorot_(self.seed)
        self.mab.reset_parameters()

    def form(self, ptr, num_sets: int, rows: int = 0) -> ops.AttnForm:
        p, r = _set_form(ptr, num_sets, rows)
        return ops.AttnForm(None, self.seed.size(1), True, p, r, num_sets)

    def mask_numels(self, M: int, ptr, num_sets: int, rows: int = 0) -> list:
        return [self.mab.mask_numel(self.form(ptr, num_sets, rows), self.seed.size(1), M)]

    def forward(self, x, ptr=None, num_sets: int | None = None, rows: int = 0, masks=None):
        x = ops.res_norm(None, ops.linear_auto(x, self.lin.weight, self.lin.bias),
                         _lib.LGNN_ACT_RELU)
        return self.mab(self.seed.view(self.seed.size(1), -1), x, self.form(ptr, num_sets, rows),
                        masks[0] if masks is not None else None)


class SetTransformerAggregation(nn.Module):
    """PyG 2.5.1 SetTransformerAggregation (the readout of the reference's
    GAT(num_st_seed_points=...), gat.py:33-43): SAB x E over each set -> PMA (S seed rows per set)
    -> SAB x D over those rows -> [B, S * channels] (concat) or the mean over the S rows. A set
    with no rows gives a zero output row (what PyG's nan_to_num leaves). Keys `encoders.i.mab.*`,
    `pma.*`, `decoders.i.mab.*`. `index` must be sorted (PyG Batch order)."""

    def __init__(self, channels: int, num_seed_points: int = 1, num_encoder_blocks: int = 1,
                 num_decoder_blocks: int = 1, heads: int = 1, concat: bool = True,
                 layer_norm: bool = False, dropout: float = 0.0):
        super().__init__()
        self.channels, self.num_seed_points, self.heads = channels, num_seed_points, heads
        self.concat, self.layer_norm, self.dropout = concat, layer_norm, float(dropout)
        self.encoders = nn.ModuleList([SetAttentionBlock(channels, heads, layer_norm, dropout)
                                       for _ in range(num_encoder_blocks)])
        self.pma = PoolingByMultiheadAttention(channels, num_seed_points, heads, layer_norm,
                                               dropout)
        self.decoders = nn.ModuleList([SetAttentionBlock(channels, heads, layer_norm, dropout)
                                       for _ in range(num_decoder_blocks)])
        self._dropout_key = repr(self.dropout)
        self.register_buffer("_dropout_rng", dropout_state(self), persistent=False)

    def reset_parameters(self):
        for m in (*self.encoders, self.pma, *self.decoders):
            m.reset_parameters()

    def forward(self, x: torch.Tensor, index: torch.Tensor | None = None,
                ptr: torch.Tensor | None = None, dim_size: int | None = None, dim: int = -2, *,
                graph: Graph | None = None) -> torch.Tensor:
        if dim not in (-2, 0) or x.dim() != 2:
            raise ValueError("SetTransformerAggregation: x must be [num_nodes, channels], dim=-2")
        if graph is None:
            if index is None:
                raise ValueError("SetTransformerAggregation needs the batch index (or a Graph)")
            graph = _pool_graph(x, index, dim_size)
        gptr, B, S, M = graph.gptr, graph.num_graphs, self.num_seed_points, x.size(0)
        masks = _set_masks(self, [(b, (M, gptr, B)) for b in self.encoders]
                           + [(self.pma, (M, gptr, B))]
                           + [(b, (B * S, None, B, S)) for b in self.decoders])
        for blk in self.encoders:
            x = blk(x, gptr, B, masks=masks.pop(0))
        x = self.pma(x, gptr, B, masks=masks.pop(0))
        for blk in self.decoders:
            x = blk(x, None, B, S, masks=masks.pop(0))
        return ops.set_readout(x, gptr, B, S, not self.concat)

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}({self.channels}, num_seed_points="
                f"{self.num_seed_points}, heads={self.heads}, layer_norm={self.layer_norm}, "
                f"dropout={self.dropout})")


def dropout_state(module: nn.Module) -> torch.Tensor:
    """A module's attention-dropout generator state, seeded as the models' (from the default
    generator's state and the module's initial parameters, without drawing)."""
    return dropout.new_state(salt=dropout.param_salt(module))


def _set_masks(owner: nn.Module, blocks: list) -> list:
    """Per block of `blocks` [(block, mask_numels arguments)] the list of its attention-dropout
    masks (None when dropout is inactive), all drawn from owner._dropout_rng with one launch per
    LGNN_MAX_MASKS sites, site j of a launch from stream j, the sites in execution order."""
    if owner.dropout == 0.0 or not owner.training:
        return [None] * len(blocks)
    numels = []
    for blk, args in blocks:
        numels += blk.mask_numels(*args)
    flat = draw_attention_masks(owner._dropout_rng, numels, dropout.key(owner, owner.dropout))
    out = []
    for blk, _ in blocks:
        out.append(flat[:blk.sites])
        flat = flat[blk.sites:]
    return out
