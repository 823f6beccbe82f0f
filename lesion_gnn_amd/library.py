"""torch.library registration of the HIP ops: the `torch.compile(model, dynamic=True)` path.

The reference wraps its models in `torch.compile(model, dynamic=True)` when the config asks for
it (src/lesion_gnn/models/gin.py:56, gat.py:84, drgnet.py:103; configs/config.py:64 sets
compile=True for the GAT run). Under Dynamo every op of this package dispatches here instead of
to its eager `torch.autograd.Function` (ops.py): each HIP op is a `torch.library.custom_op` in
namespace `lgnn` with
  * a real (CUDA-key, i.e. HIP) implementation that calls the op's plain forward / backward
    function of ops.py (`<op>_fwd` / `<op>_bwd`), the one the eager autograd.Function calls, and
    returns fields of its saved record by name; the `_bwd` ops rebuild that record from their
    named arguments and the op's plan function,
  * a fake (meta) implementation giving output shapes from symbolic input shapes (dynamic=True),
    path-dependent ones from the same plan function,
  * `register_autograd` wiring its backward to a second custom op (`lgnn::<op>_bwd`).
The graph structure is built by `lgnn::graph_build` / `lgnn::batch_ptr` / `lgnn::weighted_csr`,
so a compiled model's FX graph holds only `lgnn` ops: no graph break, and nothing for Inductor to
generate (every kernel is already a hand-written fused HIP kernel).

A graph's CSR travels between ops as one `list[Tensor]` bundle (`GPARTS` order below); an absent
member is a 0-element uint8 tensor (`_none`). SyncBatchNorm (a torch.distributed all-reduce in the
middle of GINConv) is not supported under compile and raises.
"""
from __future__ import annotations

import types
from typing import Optional

import torch
from torch import Tensor
from torch.library import custom_op

from . import _lib, ops
from .graph import Csr

GPARTS = ("rowptr", "col", "w", "tptr", "tidx", "tw", "tmap", "tile_open", "err", "batch", "gptr")


def _none(dev) -> Tensor:
    return torch.empty(0, dtype=torch.uint8, device=dev)


def _is_none(t: Tensor | None) -> bool:
    return t is None or (t.dtype == torch.uint8 and t.numel() == 0)


def _opt(t: Tensor) -> Tensor | None:
    return None if _is_none(t) else t


def _enc(t: Tensor | None, dev) -> Tensor:
    return _none(dev) if t is None else t


class TGraph:
    """The graph view the eager op bodies read (csr(kind), tile_open(kind), batch, gptr,
    num_graphs), rebuilt from a GPARTS bundle inside a custom op's real implementation."""

    def __init__(self, parts: list[Tensor], kind: str = ""):
        p = dict(zip(GPARTS, parts))
        self.batch = _opt(p["batch"])
        self.gptr = _opt(p["gptr"])
        self.num_graphs = self.gptr.numel() - 1 if self.gptr is not None else None
        self.num_nodes = p["rowptr"].numel() - 1 if not _is_none(p["rowptr"]) else (
            self.batch.numel() if self.batch is not None else 0)
        self._kind = kind
        self._csr = None
        if not _is_none(p["rowptr"]):
            self._csr = Csr(rowptr=p["rowptr"], col=p["col"], w=p["w"], tptr=p["tptr"],
                            tidx=p["tidx"], tw=p["tw"], tmap=_opt(p["tmap"]),
                            tile_open=_opt(p["tile_open"]), err=p["err"])

    def csr(self, kind: str) -> Csr:
        if self._csr is None:
            raise RuntimeError(f"graph bundle carries no CSR (asked for {kind!r})")
        return self._csr

    def csr_planes(self, kind: str, planes=None) -> tuple[Csr, bool]:
        return self.csr(kind), False  # built by its own op: the caller splits the planes

    def tile_open(self, kind: str) -> Tensor:
        return self.csr(kind).tile_open


def gparts(graph, kind: str | None) -> list[Tensor]:
    """GPARTS bundle of a (traced) Graph for one CSR kind (None: pool-only, batch + gptr)."""
    dev = graph.device
    c = graph.csr(kind) if kind is not None else None
    vals = [None] * 9 if c is None else [c.rowptr, c.col, c.w, c.tptr, c.tidx, c.tw, c.tmap,
                                         c.tile_open, c.err]
    return [_enc(t, dev) for t in vals] + [_enc(graph.batch, dev), _enc(graph.gptr, dev)]


# ----------------------------------------------------------------------------------------------
# graph structure
# ----------------------------------------------------------------------------------------------


@custom_op("lgnn::graph_build", mutates_args=(), device_types="cuda")
def graph_build(edge_index: Tensor, num_nodes: int, kind: str) -> list[Tensor]:
    """lgnn_graph_build for one kind: [rowptr, col, w, tptr, tidx, tw, tmap, tile_open, err]."""
    from .graph import Graph

    g = Graph(edge_index, num_nodes)
    c = g.csr(kind)
    dev = edge_index.device
    return [c.rowptr, c.col, c.w, c.tptr, c.tidx, c.tw, _enc(c.tmap, dev),
            _enc(c.tile_open, dev), c.err]


@graph_build.register_fake
def _(edge_index, num_nodes, kind):
    return _graph_build_fake(edge_index, num_nodes, kind)


@custom_op("lgnn::graph_build_b", mutates_args=(), device_types="cuda")
def graph_build_b(edge_index: Tensor, num_nodes: int, kind: str, batch: Tensor,
                  num_graphs: int) -> list[Tensor]:
    """graph_build with the batch vector: the graph offsets (Batch.ptr) ride along with the
    build's first launch (no separate lgnn_batch_ptr launch): [graph_build's nine, gptr]."""
    from .graph import Graph

    g = Graph(edge_index, num_nodes, batch, num_graphs)
    c = g.csr(kind)
    dev = edge_index.device
    return [c.rowptr, c.col, c.w, c.tptr, c.tidx, c.tw, _enc(c.tmap, dev),
            _enc(c.tile_open, dev), c.err, g.gptr]


@graph_build_b.register_fake
def _(edge_index, num_nodes, kind, batch, num_graphs):
    return _graph_build_fake(edge_index, num_nodes, kind) + [
        batch.new_empty(num_graphs + 1, dtype=torch.int32)]


def _graph_build_fake(edge_index, num_nodes, kind):
    n = num_nodes
    cap = edge_index.shape[1] + n
    i32 = dict(dtype=torch.int32)
    f32 = dict(dtype=torch.float32)
    e = edge_index
    return [e.new_empty(n + 1, **i32), e.new_empty(cap, **i32), e.new_empty(cap, **f32),
            e.new_empty(n + 1, **i32), e.new_empty(cap, **i32), e.new_empty(cap, **f32),
            e.new_empty(cap if kind == "gat" else 0, **(i32 if kind == "gat" else
                                                       dict(dtype=torch.uint8))),
            e.new_empty((n + 63) // 64 + _lib.LGNN_TILE_OPEN_EXTRA if kind == "gcn" else 0,
                        **(i32 if kind == "gcn" else dict(dtype=torch.uint8))),
            e.new_empty(1, **i32)]


@custom_op("lgnn::batch_ptr", mutates_args=(), device_types="cuda")
def batch_ptr(batch: Tensor, num_graphs: int) -> Tensor:
    """lgnn_batch_ptr: Batch.ptr (int32 [B + 1]) from the sorted batch vector."""
    from . import _lib

    gptr = torch.empty(num_graphs + 1, dtype=torch.int32, device=batch.device)
    _lib.call("lgnn_batch_ptr", batch, batch.numel(), num_graphs, gptr,
              _lib.stream(batch.device))
    return gptr


@batch_ptr.register_fake
def _(batch, num_graphs):
    return batch.new_empty(num_graphs + 1, dtype=torch.int32)


@custom_op("lgnn::weighted_csr", mutates_args=(), device_types="cuda")
def weighted_csr(edge_index: Tensor, edge_weight: Tensor, num_nodes: int,
                 w_like: Tensor) -> list[Tensor]:
    """Per-edge weights gathered into the CSR pair's slots (Graph.weighted): [w, tw]."""
    n = num_nodes
    bad = ((edge_index < 0) | (edge_index >= n)).any(0)
    perm = torch.argsort(edge_index[1].masked_fill(bad, n), stable=True)
    tperm = torch.argsort(edge_index[0].masked_fill(bad, n), stable=True)
    w = edge_weight.detach().to(torch.float32)
    cw, ctw = torch.zeros_like(w_like), torch.zeros_like(w_like)
    cw[: w.numel()] = w[perm]
    ctw[: w.numel()] = w[tperm]
    return [cw, ctw]


@weighted_csr.register_fake
def _(edge_index, edge_weight, num_nodes, w_like):
    return [torch.empty_like(w_like), torch.empty_like(w_like)]


# ----------------------------------------------------------------------------------------------
# node linear (aggregate + Linear + bias + act), dense (library) linear, spmm
# ----------------------------------------------------------------------------------------------


def _grad_list(ts, dev) -> list[Tensor]:
    return [_enc(t, dev) for t in ts]


@custom_op("lgnn::node_linear", mutates_args=(), device_types="cuda")
def node_linear(x: Tensor, W: Tensor, b: Optional[Tensor], g: list[Tensor], kind: str,
                self_scale: float, act: int) -> Tensor:
    return ops.node_linear_fwd(x, W, b, TGraph(g, kind) if kind else None, kind, self_scale, act)[0]


@node_linear.register_fake
def _(x, W, b, g, kind, self_scale, act):
    return x.new_empty(x.shape[0], W.shape[0], dtype=torch.float32)


@custom_op("lgnn::node_linear_bwd", mutates_args=(), device_types="cuda")
def node_linear_bwd(dy: Tensor, x: Tensor, W: Tensor, y: Tensor, has_b: bool, g: list[Tensor],
                    kind: str, self_scale: float, act: int, want_dx: bool) -> list[Tensor]:
    sv = ops.LinearSaved(x=x.contiguous(), W=W.contiguous(), y=y,
                         graph=TGraph(g, kind) if kind else None, kind=kind, self_scale=self_scale,
                         act=act, has_b=has_b)
    return _grad_list(ops.node_linear_bwd(sv, dy, want_dx), x.device)


@node_linear_bwd.register_fake
def _(dy, x, W, y, has_b, g, kind, self_scale, act, want_dx):
    return [torch.empty_like(x) if want_dx else _none(x.device), torch.empty_like(W),
            W.new_empty(W.shape[0]) if has_b else _none(x.device)]


def _node_linear_setup(ctx, inputs, output):
    x, W, b, g, kind, self_scale, act = inputs
    ctx.save_for_backward(x, W, output, *g)
    ctx.meta = (b is not None, kind, self_scale, act)


def _node_linear_backward(ctx, dy):
    x, W, y, *g = ctx.saved_tensors
    has_b, kind, self_scale, act = ctx.meta
    dx, dW, db = torch.ops.lgnn.node_linear_bwd(dy, x, W, y, has_b, g, kind, self_scale, act,
                                                ctx.needs_input_grad[0])
    return _opt(dx), dW, _opt(db), [None] * len(g), None, None, None


node_linear.register_autograd(_node_linear_backward, setup_context=_node_linear_setup)


@custom_op("lgnn::s3_weight_planes_multi", mutates_args=(), device_types="cuda")
def s3_weight_planes_multi(Ws: list[Tensor], transposed: list[bool], bf16: bool) -> Tensor:
    """ops.s3_weight_bundle: every split-3 weight operand of a step in one flat buffer."""
    return ops.s3_bundle_raw(Ws, transposed, bf16)


@s3_weight_planes_multi.register_fake
def _(Ws, transposed, bf16):
    n = sum(ops._s3_bundle_sizes([tuple(W.shape) for W in Ws], transposed, bf16))
    return Ws[0].new_empty(n, dtype=torch.int16)


@custom_op("lgnn::dense_linear", mutates_args=(), device_types="cuda")
def dense_linear(x: Tensor, W: Tensor, b: Optional[Tensor], bf16: bool,
                 wp: Optional[Tensor]) -> Tensor:
    return ops.dense_linear_fwd(x, W, b, bf16, wp)[0]


@dense_linear.register_fake
def _(x, W, b, bf16, wp=None):
    return x.new_empty(x.shape[0], W.shape[0], dtype=torch.float32)


@custom_op("lgnn::dense_linear_bwd", mutates_args=(), device_types="cuda")
def dense_linear_bwd(dy: Tensor, x: Tensor, W: Tensor, has_b: bool, bf16: bool,
                     want_dx: bool) -> list[Tensor]:
    plan = ops.dense_plan(W.shape[0], bf16)
    # the MFMA kernels round an fp32 x themselves (as the eager path hands it over)
    sv = ops.DenseSaved(x=x.to(torch.bfloat16) if plan.x_bf16 else x.contiguous(), W=W.contiguous(),
                        wt=None, bf16=bf16, has_b=has_b, plan=plan)
    return _grad_list(ops.dense_linear_bwd(sv, dy, want_dx), x.device)


@dense_linear_bwd.register_fake
def _(dy, x, W, has_b, bf16, want_dx):
    return [torch.empty_like(x) if want_dx else _none(x.device), torch.empty_like(W),
            W.new_empty(W.shape[0]) if has_b else _none(x.device)]


def _dense_setup(ctx, inputs, output):
    x, W, b, bf16, _wp = inputs
    ctx.save_for_backward(x, W)
    ctx.meta = (b is not None, bf16)


def _dense_backward(ctx, dy):
    x, W = ctx.saved_tensors
    has_b, bf16 = ctx.meta
    dx, dW, db = torch.ops.lgnn.dense_linear_bwd(dy, x, W, has_b, bf16, ctx.needs_input_grad[0])
    return _opt(dx), dW, _opt(db), None, None


dense_linear.register_autograd(_dense_backward, setup_context=_dense_setup)


@custom_op("lgnn::spmm", mutates_args=(), device_types="cuda")
def spmm(x: Tensor, g: list[Tensor], self_scale: float, transpose: bool) -> Tensor:
    """Y = A X (+ self_scale X) over the bundle's target CSR, or over its transpose."""
    c = TGraph(g).csr("")
    if transpose:
        return ops.spmm_raw(c.tptr, c.tidx, c.tw, self_scale, ops._f32c(x))
    return ops.spmm_raw(c.rowptr, c.col, c.w, self_scale, ops._f32c(x))


@spmm.register_fake
def _(x, g, self_scale, transpose):
    return torch.empty_like(x)


def _spmm_setup(ctx, inputs, output):
    x, g, self_scale, transpose = inputs
    ctx.save_for_backward(*g)
    ctx.meta = (self_scale, transpose)


def _spmm_backward(ctx, dy):
    self_scale, transpose = ctx.meta
    g = list(ctx.saved_tensors)
    return torch.ops.lgnn.spmm(dy, g, self_scale, not transpose), [None] * len(g), None, None


spmm.register_autograd(_spmm_backward, setup_context=_spmm_setup)


# ----------------------------------------------------------------------------------------------
# pooling (+ out_proj)
# ----------------------------------------------------------------------------------------------


@custom_op("lgnn::pool_head", mutates_args=(), device_types="cuda")
def pool_head(x: Tensor, Wout: Tensor, bout: Tensor, g: list[Tensor],
              mean: bool) -> list[Tensor]:
    pooled, logits = ops.pool_head_fwd(ops._f32c(x), TGraph(g), mean, ops._f32c(Wout),
                                       ops._f32c(bout))
    return [logits, pooled]


@pool_head.register_fake
def _(x, Wout, bout, g, mean):
    B = g[GPARTS.index("gptr")].shape[0] - 1
    return [x.new_empty(B, Wout.shape[0]), x.new_empty(B, x.shape[1])]


@custom_op("lgnn::pool_head_bwd", mutates_args=(), device_types="cuda")
def pool_head_bwd(dlogits: Tensor, pooled: Tensor, Wout: Tensor, g: list[Tensor], mean: bool,
                  num_nodes: int, want_dx: bool) -> list[Tensor]:
    dp, dWo, dbo = ops.pool_head_bwd(ops._f32c(dlogits), pooled, Wout)
    dx = ops.pool_bwd(dp, TGraph(g), mean, num_nodes) if want_dx else None
    return _grad_list([dx, dWo, dbo], pooled.device)


@pool_head_bwd.register_fake
def _(dlogits, pooled, Wout, g, mean, num_nodes, want_dx):
    dx = pooled.new_empty(num_nodes, pooled.shape[1]) if want_dx else _none(pooled.device)
    return [dx, torch.empty_like(Wout), Wout.new_empty(Wout.shape[0])]


def _pool_head_setup(ctx, inputs, output):
    x, Wout, bout, g, mean = inputs
    ctx.save_for_backward(output[1], Wout, *g)
    ctx.meta = (mean, x.shape[0])


def _pool_head_backward(ctx, grads):
    pooled, Wout, *g = ctx.saved_tensors
    mean, M = ctx.meta
    dx, dWo, dbo = torch.ops.lgnn.pool_head_bwd(grads[0], pooled, Wout, g, mean, M,
                                                ctx.needs_input_grad[0])
    return _opt(dx), dWo, dbo, [None] * len(g), None


pool_head.register_autograd(_pool_head_backward, setup_context=_pool_head_setup)


@custom_op("lgnn::segment_pool", mutates_args=(), device_types="cuda")
def segment_pool(x: Tensor, g: list[Tensor], mean: bool) -> Tensor:
    return ops.pool_head_fwd(ops._f32c(x), TGraph(g), mean)[0]


@segment_pool.register_fake
def _(x, g, mean):
    return x.new_empty(g[GPARTS.index("gptr")].shape[0] - 1, x.shape[1])


@custom_op("lgnn::segment_pool_bwd", mutates_args=(), device_types="cuda")
def segment_pool_bwd(dp: Tensor, g: list[Tensor], mean: bool, num_nodes: int) -> Tensor:
    return ops.pool_bwd(ops._f32c(dp), TGraph(g), mean, num_nodes)


@segment_pool_bwd.register_fake
def _(dp, g, mean, num_nodes):
    return dp.new_empty(num_nodes, dp.shape[1])


def _segpool_setup(ctx, inputs, output):
    x, g, mean = inputs
    ctx.save_for_backward(*g)
    ctx.meta = (mean, x.shape[0])


def _segpool_backward(ctx, dp):
    mean, M = ctx.meta
    g = list(ctx.saved_tensors)
    return torch.ops.lgnn.segment_pool_bwd(dp, g, mean, M), [None] * len(g), None


segment_pool.register_autograd(_segpool_backward, setup_context=_segpool_setup)


# ----------------------------------------------------------------------------------------------
# dropout (lesion_gnn_amd.dropout): masks from the device generator, the mask product
# ----------------------------------------------------------------------------------------------


@custom_op("lgnn::dropout_masks", mutates_args=("state",), device_types="cuda",
           tags=(torch.Tag.nondeterministic_seeded,))
def dropout_masks(state: Tensor, numels: list[int], thr: int, scale: float) -> Tensor:
    """lgnn_dropout_masks: every mask in one flat fp32 tensor (lesion_gnn_amd.dropout layout),
    the state's counter advanced. Tagged nondeterministic_seeded so the compiler neither merges
    two calls nor recomputes one in the backward (the backward needs the forward's masks)."""
    from .dropout import dropout_masks_raw

    return dropout_masks_raw(state, list(numels), thr, scale)


@dropout_masks.register_fake
def _(state, numels, thr, scale):
    tot = 0
    for n in numels:
        tot += (n + 3) // 4 * 4
    return state.new_empty(tot, dtype=torch.float32)


@custom_op("lgnn::mask_mul", mutates_args=(), device_types="cuda")
def mask_mul(x: Tensor, m: Tensor) -> Tensor:
    """lgnn_mask_mul: x * m (dropout between convs)."""
    from .dropout import _mul

    return _mul(x, m)


@mask_mul.register_fake
def _(x, m):
    return torch.empty_like(x)


def _mask_mul_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])


def _mask_mul_backward(ctx, grad):
    (m,) = ctx.saved_tensors
    return torch.ops.lgnn.mask_mul(grad, m), None


mask_mul.register_autograd(_mask_mul_backward, setup_context=_mask_mul_setup)


# ----------------------------------------------------------------------------------------------
# GATConv
# ----------------------------------------------------------------------------------------------


@custom_op("lgnn::gat_conv", mutates_args=(), device_types="cuda")
def gat_conv(x: Tensor, W: Tensor, att_src: Tensor, att_dst: Tensor, bias: Optional[Tensor],
             g: list[Tensor], heads: int, slope: float, mask: Optional[Tensor], act: int,
             bf16: bool, wp: Optional[Tensor], wpt: Optional[Tensor]) -> list[Tensor]:
    """[Y, XP, a_s, a_d, alpha] (the eager _GATConv forward and what it saves)."""
    Y, sv = ops.gat_conv_fwd(x, W, att_src, att_dst, bias, TGraph(g, "gat"), heads, slope, mask,
                             act, bf16, wp)
    return [Y, sv.XP, sv.a_s, sv.a_d, sv.alpha]


@gat_conv.register_fake
def _(x, W, att_src, att_dst, bias, g, heads, slope, mask, act, bf16, wp=None, wpt=None):
    M, HC = x.shape[0], W.shape[0]
    cap = g[GPARTS.index("col")].shape[0]
    return [x.new_empty(M, HC), x.new_empty(M, HC), x.new_empty(M, heads),
            x.new_empty(M, heads), x.new_empty(cap, heads)]


@custom_op("lgnn::gat_conv_bwd", mutates_args=(), device_types="cuda")
def gat_conv_bwd(dY: Tensor, x: Tensor, W: Tensor, att_src: Tensor, att_dst: Tensor,
                 XP: Tensor, a_s: Tensor, a_d: Tensor, alpha: Tensor, Y: Tensor,
                 mask: Optional[Tensor], g: list[Tensor], heads: int, slope: float, act: int,
                 bf16: bool, has_bias: bool, want_dx: bool,
                 wpt: Optional[Tensor]) -> list[Tensor]:
    sv = _gat_saved(x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, mask, g, heads, slope, act,
                    bf16, has_bias, wpt)
    # the attention / bias gradients are ONE reduction buffer [att_src | att_dst | bias]
    # (outputs of a custom op may not alias each other): returned whole and split into views by
    # the autograd formula below, instead of three copies
    return _grad_list(ops.gat_conv_bwd(sv, dY, want_dx), x.device)


def _gat_saved(x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, mask, g, heads, slope, act, bf16,
               has_bias, wpt):
    """ops.GatSaved from the named arguments of a GAT backward op."""
    return ops.GatSaved(x=x.contiguous(), W=W.contiguous(), att_src=att_src.reshape(-1),
                        att_dst=att_dst.reshape(-1), XP=XP, a_s=a_s, a_d=a_d, alpha=alpha, Y=Y,
                        mask=mask, wt=None, wpt=wpt, graph=TGraph(g, "gat"), heads=heads,
                        slope=slope, act=act, bf16=bf16, has_bias=has_bias,
                        plan=ops.gat_plan(W.shape[1], W.shape[0], bf16))


@gat_conv_bwd.register_fake
def _(dY, x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, mask, g, heads, slope, act, bf16,
      has_bias, want_dx, wpt=None):
    dev = x.device
    return [torch.empty_like(x) if want_dx else _none(dev), torch.empty_like(W),
            W.new_empty(3 * W.shape[0])]


def _gat_setup(ctx, inputs, output):
    x, W, att_src, att_dst, bias, g, heads, slope, mask, act, bf16, _wp, wpt = inputs
    Y, XP, a_s, a_d, alpha = output
    ctx.save_for_backward(x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y,
                          _enc(mask, x.device), _enc(wpt, x.device), *g)
    ctx.meta = (heads, slope, act, bf16, bias is not None)


def _gat_backward(ctx, grads):
    x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, mask, wpt, *g = ctx.saved_tensors
    heads, slope, act, bf16, has_bias = ctx.meta
    dx, dW, red = torch.ops.lgnn.gat_conv_bwd(
        grads[0], x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, _opt(mask), g, heads, slope,
        act, bf16, has_bias, ctx.needs_input_grad[0], _opt(wpt))
    HC = W.shape[0]
    da_s = red[:HC].view(att_src.shape)
    da_d = red[HC:2 * HC].view(att_dst.shape)
    db = red[2 * HC:] if has_bias else None
    return (_opt(dx), dW, da_s, da_d, db, [None] * len(g), None, None, None, None, None, None,
            None)


gat_conv.register_autograd(_gat_backward, setup_context=_gat_setup)


@custom_op("lgnn::gat_conv_head", mutates_args=(), device_types="cuda")
def gat_conv_head(x: Tensor, W: Tensor, att_src: Tensor, att_dst: Tensor, bias: Optional[Tensor],
                  W_out: Tensor, b_out: Tensor, g: list[Tensor], heads: int, slope: float,
                  mask: Optional[Tensor], act: int, bf16: bool, mean: bool,
                  wp: Optional[Tensor], wpt: Optional[Tensor]) -> list[Tensor]:
    """The GAT model's last conv + global pool + out_proj as one node (ops._GATConvHead):
    [logits, Y, XP, a_s, a_d, alpha, pooled]."""
    logits, sv = ops.gat_head_fwd(x, W, att_src, att_dst, bias, W_out, b_out, TGraph(g, "gat"),
                                  heads, slope, mask, act, bf16, mean, wp)
    c = sv.conv
    return [logits, c.Y, c.XP, c.a_s, c.a_d, c.alpha, sv.pooled]


@gat_conv_head.register_fake
def _(x, W, att_src, att_dst, bias, W_out, b_out, g, heads, slope, mask, act, bf16, mean,
      wp=None, wpt=None):
    M, HC = x.shape[0], W.shape[0]
    cap = g[GPARTS.index("col")].shape[0]
    B = g[GPARTS.index("gptr")].shape[0] - 1
    return [x.new_empty(B, W_out.shape[0]), x.new_empty(M, HC), x.new_empty(M, HC),
            x.new_empty(M, heads), x.new_empty(M, heads), x.new_empty(cap, heads),
            x.new_empty(B, HC)]


@custom_op("lgnn::gat_conv_head_bwd", mutates_args=(), device_types="cuda")
def gat_conv_head_bwd(dlogits: Tensor, x: Tensor, W: Tensor, att_src: Tensor, att_dst: Tensor,
                      XP: Tensor, a_s: Tensor, a_d: Tensor, alpha: Tensor, Y: Tensor,
                      mask: Optional[Tensor], pooled: Tensor, W_out: Tensor, g: list[Tensor],
                      heads: int, slope: float, act: int, bf16: bool, has_bias: bool, mean: bool,
                      want_dx: bool, wpt: Optional[Tensor]) -> list[Tensor]:
    """[dx, dW, red (= [datt_src | datt_dst | dbias]), dW_out, db_out]: the readout's backward
    formed inside the edge kernel's load (lgnn_gat_bwd_edge_pool), no dH tensor."""
    conv = _gat_saved(x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, mask, g, heads, slope, act,
                      bf16, has_bias, wpt)
    sv = ops.HeadSaved(conv, pooled, W_out, mean)
    return _grad_list(ops.gat_head_bwd(sv, dlogits, want_dx), x.device)


@gat_conv_head_bwd.register_fake
def _(dlogits, x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, mask, pooled, W_out, g, heads,
      slope, act, bf16, has_bias, mean, want_dx, wpt=None):
    dev = x.device
    return [torch.empty_like(x) if want_dx else _none(dev), torch.empty_like(W),
            W.new_empty(3 * W.shape[0]), torch.empty_like(W_out), W_out.new_empty(W_out.shape[0])]


def _gat_head_setup(ctx, inputs, output):
    (x, W, att_src, att_dst, bias, W_out, b_out, g, heads, slope, mask, act, bf16, mean, _wp,
     wpt) = inputs
    _logits, Y, XP, a_s, a_d, alpha, pooled = output
    ctx.save_for_backward(x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, _enc(mask, x.device),
                          pooled, W_out, _enc(wpt, x.device), *g)
    ctx.meta = (heads, slope, act, bf16, bias is not None, mean)


def _gat_head_backward(ctx, grads):
    (x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, mask, pooled, W_out, wpt,
     *g) = ctx.saved_tensors
    heads, slope, act, bf16, has_bias, mean = ctx.meta
    dx, dW, red, dWo, dbo = torch.ops.lgnn.gat_conv_head_bwd(
        grads[0], x, W, att_src, att_dst, XP, a_s, a_d, alpha, Y, _opt(mask), pooled, W_out, g,
        heads, slope, act, bf16, has_bias, mean, ctx.needs_input_grad[0], _opt(wpt))
    HC = W.shape[0]
    da_s = red[:HC].view(att_src.shape)
    da_d = red[HC:2 * HC].view(att_dst.shape)
    db = red[2 * HC:] if has_bias else None
    return (_opt(dx), dW, da_s, da_d, db, dWo, dbo, [None] * len(g), None, None, None, None,
            None, None, None, None)


gat_conv_head.register_autograd(_gat_head_backward, setup_context=_gat_head_setup)


# ----------------------------------------------------------------------------------------------
# GINConv (MLP with BatchNorm; running statistics mutated in place)
# ----------------------------------------------------------------------------------------------


def _bn_stub(gamma, beta, running_mean, running_var, nbt, bn_eps, momentum):
    track = running_mean is not None
    return types.SimpleNamespace(
        weight=gamma, bias=beta, affine=gamma is not None, track_running_stats=track,
        running_mean=running_mean, running_var=running_var, num_batches_tracked=nbt,
        eps=bn_eps, momentum=None if momentum < 0 else momentum)


@custom_op("lgnn::gin_conv", mutates_args=(), device_types="cuda")
def gin_conv(x: Tensor, W1: Tensor, b1: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor],
             W2: Tensor, b2: Tensor, running_mean: Optional[Tensor],
             running_var: Optional[Tensor], g: list[Tensor], training: bool, eps: float,
             bn_eps: float, mask: Optional[Tensor], act: int) -> list[Tensor]:
    """[H, S or none, Z1, A1, mean, invstd, scale, shift, sums or none] (the eager _GINConv
    forward). Functional: in training the BatchNorm running statistics are NOT updated here —
    lgnn::bn_running_update does it from the returned batch sums (a mutating op cannot carry an
    autograd formula); in eval the running statistics are read."""
    rm, rv = (None, None) if training else (running_mean, running_var)
    bn = _bn_stub(gamma, beta, rm, rv, None, bn_eps, 0.1)
    H, sums, sv = ops.gin_conv_fwd(x, W1, b1, W2, b2, TGraph(g, "gin"), bn, training, eps, mask,
                                   act)
    return [H, _none(x.device) if sv.plan.gathered else sv.S, sv.Z1, sv.A1, sv.mean, sv.invstd,
            sv.scale, sv.shift, _enc(sums, x.device)]


@custom_op("lgnn::bn_running_update", mutates_args=("running_mean", "running_var", "nbt"),
           device_types="cuda")
def bn_running_update(running_mean: Tensor, running_var: Tensor, nbt: Optional[Tensor],
                      sums: Tensor, count: int, bn_eps: float, momentum: float) -> None:
    """BatchNorm1d running statistics from a batch's (sum z, sum z^2) (lgnn_bn_finalize in
    training mode), torch semantics (unbiased variance; momentum < 0: cumulative average)."""
    bn = _bn_stub(None, None, running_mean, running_var, nbt, bn_eps, momentum)
    ops.bn_finalize(sums, float(count), bn, True, running_mean.numel(), running_mean.device)


@bn_running_update.register_fake
def _(running_mean, running_var, nbt, sums, count, bn_eps, momentum):
    return None


@gin_conv.register_fake
def _(x, W1, b1, gamma, beta, W2, b2, running_mean, running_var, g, training, eps, bn_eps,
      mask, act):
    M, N1 = x.shape[0], W1.shape[0]
    gathered = ops.gin_plan(W1.shape[1], N1, W2.shape[0]).gathered
    S = _none(x.device) if gathered else torch.empty_like(x)
    sums = x.new_empty(2 * N1, dtype=torch.float64) if training else _none(x.device)
    return [x.new_empty(M, W2.shape[0]), S, x.new_empty(M, N1), x.new_empty(M, N1)] + \
        [x.new_empty(N1) for _ in range(4)] + [sums]


@custom_op("lgnn::gin_conv_bwd", mutates_args=(), device_types="cuda")
def gin_conv_bwd(dH: Tensor, S: Tensor, Z1: Tensor, A1: Tensor, H: Tensor, W1: Tensor,
                 W2: Tensor, mean: Tensor, invstd: Tensor, scale: Tensor, shift: Tensor,
                 mask: Optional[Tensor], g: list[Tensor], training: bool, count: int,
                 act: int, affine: bool, gathered: bool, eps: float,
                 want_dx: bool) -> list[Tensor]:
    plan = ops.gin_plan(W1.shape[1], W1.shape[0], W2.shape[0])
    assert plan.gathered == gathered, "GIN path switches changed between forward and backward"
    sv = ops.GinSaved(S=S.contiguous(), Z1=Z1, A1=A1, H=H, W1=W1.contiguous(), W2=W2.contiguous(),
                      mean=mean, invstd=invstd, scale=scale, shift=shift, mask=mask,
                      graph=TGraph(g, "gin"), self_scale=1.0 + eps, training=training,
                      count=float(count), group=None, act=act, affine=affine, plan=plan)
    return _grad_list(ops.gin_conv_bwd(sv, dH, want_dx), H.device)


@gin_conv_bwd.register_fake
def _(dH, S, Z1, A1, H, W1, W2, mean, invstd, scale, shift, mask, g, training, count, act,
      affine, gathered, eps, want_dx):
    dev = H.device
    N1 = W1.shape[0]
    dx = S.new_empty(S.shape[0], W1.shape[1]) if want_dx else _none(dev)
    dgb = [W1.new_empty(N1), W1.new_empty(N1)] if affine else [_none(dev), _none(dev)]
    return [dx, torch.empty_like(W1), W1.new_empty(N1)] + dgb + \
        [torch.empty_like(W2), W2.new_empty(W2.shape[0])]


def _gin_setup(ctx, inputs, output):
    (x, W1, b1, gamma, beta, W2, b2, running_mean, running_var, g, training, eps, bn_eps,
     mask, act) = inputs
    H, S, Z1, A1, mean, invstd, scale, shift, _sums = output
    gathered = _is_none(S)
    ctx.save_for_backward(x if gathered else S, Z1, A1, H, W1, W2, mean, invstd, scale, shift,
                          _enc(mask, x.device), *g)
    ctx.meta = (training, x.shape[0], act, gamma is not None, gathered, eps)


def _gin_backward(ctx, grads):
    S, Z1, A1, H, W1, W2, mean, invstd, scale, shift, mask, *g = ctx.saved_tensors
    training, count, act, affine, gathered, eps = ctx.meta
    dx, dW1, db1, dg, dbt, dW2, db2 = torch.ops.lgnn.gin_conv_bwd(
        grads[0], S, Z1, A1, H, W1, W2, mean, invstd, scale, shift, _opt(mask), g, training,
        count, act, affine, gathered, eps, ctx.needs_input_grad[0])
    return (_opt(dx), dW1, db1, _opt(dg), _opt(dbt), dW2, db2, None, None,
            [None] * len(g), None, None, None, None, None)


gin_conv.register_autograd(_gin_backward, setup_context=_gin_setup)


# ----------------------------------------------------------------------------------------------
# the fused GCN model body
# ----------------------------------------------------------------------------------------------


def _gcn_plan(params, L):
    return ops.gcn_plan([tuple(params[2 * l].shape) for l in range(L + 1)], L)


@custom_op("lgnn::gcn_stack", mutates_args=(), device_types="cuda")
def gcn_stack(x: Tensor, g: list[Tensor], mean: bool, L: int,
              params: list[Tensor]) -> list[Tensor]:
    """[logits, pooled, H_0..H_L, S_1..S_L, planes_t or none] (the eager _GCNStack forward)."""
    # the op's planes output is one fresh buffer: the planes, then the Â^T room
    logits, sv = ops.gcn_stack_fwd(x, TGraph(g, "gcn"), mean, L, params, want_dx=True,
                               adjt_after_planes=True)
    hs = sv.hs
    ss = [s if s.data_ptr() != x.data_ptr() and all(s.data_ptr() != h.data_ptr() for h in hs)
          else s.clone() for s in sv.ss]
    return [logits, sv.pooled] + hs + ss + [_enc(sv.planes_t, x.device)]


@gcn_stack.register_fake
def _(x, g, mean, L, params):
    B = g[GPARTS.index("gptr")].shape[0] - 1
    M = x.shape[0]
    Ws = [params[2 * l] for l in range(L + 1)]
    hs = [x.new_empty(M, W.shape[0]) for W in Ws]
    ss = [x.new_empty(M, Ws[l + 1].shape[1]) for l in range(L)]
    planes = (x.new_empty(ops.bwd_planes_numel(L, M), dtype=torch.int16)
              if _gcn_plan(params, L).keeps_planes else _none(x.device))
    return [x.new_empty(B, params[2 + 2 * L].shape[0]), x.new_empty(B, Ws[-1].shape[0])] + hs + \
        ss + [planes]


@custom_op("lgnn::gcn_stack_bwd", mutates_args=(), device_types="cuda")
def gcn_stack_bwd(dlogits: Tensor, x: Tensor, pooled: Tensor, hs: list[Tensor],
                  ss: list[Tensor], params: list[Tensor], planes_t: Tensor, g: list[Tensor],
                  mean: bool, L: int, want_dx: bool) -> list[Tensor]:
    """[dx or none, dparams...]

    The graph's tile_open (in g) is written here although the op declares no mutation: the fused
    backward's barrier words and partial-slot skip words (include/lgnn.h LGNN_SLOT_FLAG0) are
    scratch set and consumed inside this one call, and the next graph build zeroes them; the tile
    flags proper, the only part of tile_open other ops read, are left unchanged."""
    sv = ops.GcnSaved(x=x.contiguous(), pooled=pooled, hs=hs, ss=ss,
                      params=[p.contiguous() for p in params], planes_t=_opt(planes_t), adjt=None,
                      graph=TGraph(g, "gcn"), mean=mean, L=L, plan=_gcn_plan(params, L))
    dx, grads = ops.gcn_stack_bwd(sv, dlogits, want_dx)
    return _grad_list([dx] + grads, x.device)


@gcn_stack_bwd.register_fake
def _(dlogits, x, pooled, hs, ss, params, planes_t, g, mean, L, want_dx):
    return [torch.empty_like(x) if want_dx else _none(x.device)] + \
        [torch.empty_like(p) for p in params]


def _gcn_setup(ctx, inputs, output):
    x, g, mean, L, params = inputs
    logits, pooled, *rest = output
    hs, ss, planes = rest[:L + 1], rest[L + 1:2 * L + 1], rest[2 * L + 1]
    ctx.save_for_backward(x, pooled, planes, *hs, *ss, *params, *g)
    ctx.meta = (mean, L, len(params), len(g))


def _gcn_backward(ctx, grads):
    mean, L, npar, ng = ctx.meta
    x, pooled, planes, *rest = ctx.saved_tensors
    hs, ss = rest[:L + 1], rest[L + 1:2 * L + 1]
    params = rest[2 * L + 1:2 * L + 1 + npar]
    g = rest[2 * L + 1 + npar:]
    out = torch.ops.lgnn.gcn_stack_bwd(grads[0], x, pooled, list(hs), list(ss), list(params),
                                       planes, list(g), mean, L, ctx.needs_input_grad[0])
    return _opt(out[0]), [None] * ng, None, None, list(out[1:])


gcn_stack.register_autograd(_gcn_backward, setup_context=_gcn_setup)


# ----------------------------------------------------------------------------------------------
# SortAggregation
# ----------------------------------------------------------------------------------------------


@custom_op("lgnn::sort_pool", mutates_args=(), device_types="cuda")
def sort_pool(x: Tensor, g: list[Tensor], k: int) -> list[Tensor]:
    """[out, rank, fill]"""
    out, sv = ops.sort_pool_fwd(x, TGraph(g), k)
    return [out, sv.rank, sv.fill]


@sort_pool.register_fake
def _(x, g, k):
    B = g[GPARTS.index("gptr")].shape[0] - 1
    return [x.new_empty(B, k * x.shape[1]), x.new_empty(x.shape[0], dtype=torch.int32),
            x.new_empty(1)]


@custom_op("lgnn::sort_pool_bwd", mutates_args=(), device_types="cuda")
def sort_pool_bwd(dout: Tensor, x: Tensor, rank: Tensor, fill: Tensor, g: list[Tensor],
                  k: int) -> Tensor:
    sv = ops.SortSaved(x=x.contiguous(), rank=rank, fill=fill, graph=TGraph(g), k=k)
    return ops.sort_pool_bwd(sv, dout)


@sort_pool_bwd.register_fake
def _(dout, x, rank, fill, g, k):
    return torch.empty_like(x)


def _sort_setup(ctx, inputs, output):
    x, g, k = inputs
    ctx.save_for_backward(x, output[1], output[2], *g)
    ctx.k = k


def _sort_backward(ctx, grads):
    x, rank, fill, *g = ctx.saved_tensors
    return (torch.ops.lgnn.sort_pool_bwd(grads[0], x, rank, fill, list(g), ctx.k),
            [None] * len(g), None)


sort_pool.register_autograd(_sort_backward, setup_context=_sort_setup)


# ----------------------------------------------------------------------------------------------
# ELU(a + b): GraphConv's two branches and the activation after it
# ----------------------------------------------------------------------------------------------


@custom_op("lgnn::add_elu", mutates_args=(), device_types="cuda")
def add_elu(a: Tensor, b: Tensor) -> Tensor:
    return ops.add_act_fwd(a, b)


@add_elu.register_fake
def _(a, b):
    return torch.empty_like(a, memory_format=torch.contiguous_format)


@custom_op("lgnn::add_elu_bwd", mutates_args=(), device_types="cuda")
def add_elu_bwd(dy: Tensor, y: Tensor) -> Tensor:
    return ops.add_act_bwd(dy.contiguous(), y)


@add_elu_bwd.register_fake
def _(dy, y):
    return torch.empty_like(y)


def _add_elu_setup(ctx, inputs, output):
    ctx.save_for_backward(output)


def _add_elu_backward(ctx, grad):
    dz = torch.ops.lgnn.add_elu_bwd(grad, ctx.saved_tensors[0])
    return dz, dz


add_elu.register_autograd(_add_elu_backward, setup_context=_add_elu_setup)


# ----------------------------------------------------------------------------------------------
# DRGNet head
# ----------------------------------------------------------------------------------------------


@custom_op("lgnn::drgnet_head", mutates_args=(), device_types="cuda")
def drgnet_head(x: Tensor, k: int, params: list[Tensor], mask: Optional[Tensor]) -> list[Tensor]:
    """[logits, a1, sel, a2, h] (ops.drgnet_head_fwd and what it saves)."""
    logits, sv = ops.drgnet_head_fwd(x, k, tuple(params), mask)
    return [logits, sv.a1, sv.sel, sv.a2, sv.h]


@drgnet_head.register_fake
def _(x, k, params, mask):
    B, D, c0, c1, H, dense, C = ops.drgnet_head_dims(x, k, params, mask)
    return [x.new_empty(B, C), x.new_empty(B, k // 2, c0),
            x.new_empty(B, k // 2, (c0 + 15) // 16, dtype=torch.int16), x.new_empty(B, dense),
            x.new_empty(B, H)]


@custom_op("lgnn::drgnet_head_bwd", mutates_args=(), device_types="cuda")
def drgnet_head_bwd(dlogits: Tensor, x: Tensor, k: int, params: list[Tensor],
                    mask: Optional[Tensor], a1: Tensor, sel: Tensor, a2: Tensor,
                    h: Tensor) -> list[Tensor]:
    """[dx, the eight parameter gradients]"""
    sv = ops.DrgHeadSaved(x.contiguous(), k, tuple(p.contiguous() for p in params), mask, a1, sel,
                          a2, h)
    dx, dparams = ops.drgnet_head_bwd(sv, dlogits.contiguous())
    return [dx] + dparams


@drgnet_head_bwd.register_fake
def _(dlogits, x, k, params, mask, a1, sel, a2, h):
    return [torch.empty_like(x)] + [torch.empty_like(p) for p in params]


def _head_setup(ctx, inputs, output):
    x, k, params, mask = inputs
    ctx.save_for_backward(x, *output[1:], *params, *([] if mask is None else [mask]))
    ctx.k, ctx.npar = k, len(params)


def _head_backward(ctx, grads):
    x, a1, sel, a2, h, *rest = ctx.saved_tensors
    params, mask = rest[:ctx.npar], (rest[ctx.npar] if len(rest) > ctx.npar else None)
    out = torch.ops.lgnn.drgnet_head_bwd(grads[0], x, ctx.k, list(params), mask, a1, sel, a2, h)
    return out[0], None, list(out[1:]), None


drgnet_head.register_autograd(_head_backward, setup_context=_head_setup)


def gparts_empty(dev) -> list[Tensor]:
    return [_none(dev) for _ in GPARTS]


# ----------------------------------------------------------------------------------------------
# Set attention: MultiheadAttentionBlock as one op, the residual / activation / LayerNorm kernel,
# the set readout
# ----------------------------------------------------------------------------------------------


def _mab_params(wb: list[Tensor], ln: list[Tensor]) -> list:
    return list(wb) + (list(ln) if len(ln) else [None] * 4)


def _mab_rows(x, qptr, q_rows, num_sets):
    return x.shape[0] if qptr is not None else num_sets * q_rows


@custom_op("lgnn::mab", mutates_args=(), device_types="cuda")
def mab(x: Tensor, y: Optional[Tensor], wb: list[Tensor], ln: list[Tensor],
        qptr: Optional[Tensor], kptr: Optional[Tensor], q_rows: int, q_shared: bool, k_rows: int,
        num_sets: int, heads: int, mask: Optional[Tensor]) -> list[Tensor]:
    """[out, *ops.MAB_SAVED] (absent members as 0-element uint8 tensors)."""
    form = ops.AttnForm(qptr, q_rows, q_shared, kptr, k_rows, num_sets)
    out, sv = ops.mab_fwd(x, y, _mab_params(wb, ln), form, heads, mask)
    return [out] + [_enc(getattr(sv, n), x.device) for n in ops.MAB_SAVED]


@mab.register_fake
def _(x, y, wb, ln, qptr, kptr, q_rows, q_shared, k_rows, num_sets, heads, mask):
    C = wb[0].shape[1]
    R = _mab_rows(x, qptr, q_rows, num_sets)
    return [x.new_empty(R, C)] + _mab_saved_fake(x, y, C, R, heads, len(ln) > 0, mask, num_sets)


@custom_op("lgnn::mab_bwd", mutates_args=(), device_types="cuda")
def mab_bwd(dout: Tensor, x: Tensor, y: Optional[Tensor], wb: list[Tensor], ln: list[Tensor],
            saved: list[Tensor], qptr: Optional[Tensor], kptr: Optional[Tensor], q_rows: int,
            q_shared: bool, k_rows: int, num_sets: int, heads: int, mask: Optional[Tensor],
            want_dx: bool, want_dy: bool) -> list[Tensor]:
    """[dx, dy, the six weight / bias gradients, the four LayerNorm gradients] (absent: empty)."""
    form = ops.AttnForm(qptr, q_rows, q_shared, kptr, k_rows, num_sets)
    sv = ops.MabSaved(x.contiguous(), y.contiguous() if y is not None else None,
                      [p.contiguous() if p is not None else None for p in _mab_params(wb, ln)],
                      form, heads, mask, *[_opt(t) for t in saved])
    dx, dy, dps = ops.mab_bwd(sv, dout, want_dx, want_dy)
    return _grad_list([dx, dy] + dps, x.device)


@mab_bwd.register_fake
def _(dout, x, y, wb, ln, saved, qptr, kptr, q_rows, q_shared, k_rows, num_sets, heads, mask,
      want_dx, want_dy):
    none = lambda: x.new_empty(0, dtype=torch.uint8)  # noqa: E731
    return [torch.empty_like(x) if want_dx else none(),
            torch.empty_like(y) if (y is not None and want_dy) else none()] + \
        [torch.empty_like(p) for p in wb] + \
        ([torch.empty_like(p) for p in ln] if len(ln) else [none() for _ in range(4)])


def _mab_setup(ctx, inputs, output):
    x, y, wb, ln, qptr, kptr, q_rows, q_shared, k_rows, num_sets, heads, mask = inputs
    ts = [x, y, qptr, kptr, mask]
    ctx.present = [t is not None for t in ts]
    ctx.counts = (len(wb), len(ln))
    ctx.save_for_backward(*[t for t in ts if t is not None], *wb, *ln, *output[1:])
    ctx.meta = (q_rows, q_shared, k_rows, num_sets, heads)


def _mab_backward(ctx, grads):
    st = list(ctx.saved_tensors)
    x, y, qptr, kptr, mask = [st.pop(0) if p else None for p in ctx.present]
    nwb, nln = ctx.counts
    wb, ln, saved = st[:nwb], st[nwb:nwb + nln], st[nwb + nln:]
    q_rows, q_shared, k_rows, num_sets, heads = ctx.meta
    need = ctx.needs_input_grad
    g = torch.ops.lgnn.mab_bwd(grads[0], x, y, wb, ln, saved, qptr, kptr, q_rows, q_shared,
                               k_rows, num_sets, heads, mask, need[0], need[1] and y is not None)
    return (_opt(g[0]), _opt(g[1]), list(g[2:2 + nwb]), list(g[8:8 + nln]) if nln else [],
            None, None, None, None, None, None, None, None)


mab.register_autograd(_mab_backward, setup_context=_mab_setup)


@custom_op("lgnn::res_norm", mutates_args=(), device_types="cuda")
def res_norm(a: Optional[Tensor], b: Tensor, act: int, gamma: Optional[Tensor],
             beta: Optional[Tensor], a_rows: int, eps: float) -> list[Tensor]:
    """[y, mean, rstd]"""
    y, sv = ops.res_norm_fwd(a, a_rows, b, act, gamma, beta, eps)
    return [y, _enc(sv.mean, b.device), _enc(sv.rstd, b.device)]


@res_norm.register_fake
def _(a, b, act, gamma, beta, a_rows, eps):
    stat = (lambda: b.new_empty(b.shape[0])) if gamma is not None else \
        (lambda: b.new_empty(0, dtype=torch.uint8))
    return [torch.empty_like(b), stat(), stat()]


@custom_op("lgnn::res_norm_bwd", mutates_args=(), device_types="cuda")
def res_norm_bwd(dy: Tensor, a: Optional[Tensor], b: Tensor, act: int, gamma: Optional[Tensor],
                 mean: Tensor, rstd: Tensor, a_rows: int, want_da: bool,
                 want_db: bool) -> list[Tensor]:
    sv = ops.NormSaved(a.contiguous() if a is not None else None, a_rows, b.contiguous(), act,
                       gamma.contiguous() if gamma is not None else None, _opt(mean), _opt(rstd))
    return _grad_list(ops.res_norm_bwd(sv, dy, want_da, want_db), b.device)


@res_norm_bwd.register_fake
def _(dy, a, b, act, gamma, mean, rstd, a_rows, want_da, want_db):
    none = lambda: b.new_empty(0, dtype=torch.uint8)  # noqa: E731
    return [torch.empty_like(a) if (a is not None and want_da) else none(),
            torch.empty_like(b) if want_db else none(),
            torch.empty_like(gamma) if gamma is not None else none(),
            torch.empty_like(gamma) if gamma is not None else none()]


def _res_norm_setup(ctx, inputs, output):
    a, b, act, gamma, beta, a_rows, eps = inputs
    ts = [a, gamma]
    ctx.present = [t is not None for t in ts]
    ctx.save_for_backward(*[t for t in ts if t is not None], b, output[1], output[2])
    ctx.meta = (act, a_rows)


def _res_norm_backward(ctx, grads):
    st = list(ctx.saved_tensors)
    a, gamma = [st.pop(0) if p else None for p in ctx.present]
    b, mean, rstd = st
    act, a_rows = ctx.meta
    need = ctx.needs_input_grad
    da, db, dg, dbt = torch.ops.lgnn.res_norm_bwd(grads[0], a, b, act, gamma, mean, rstd, a_rows,
                                                  need[0] and a is not None, need[1])
    return _opt(da), _opt(db), None, _opt(dg), _opt(dbt), None, None


res_norm.register_autograd(_res_norm_backward, setup_context=_res_norm_setup)


@custom_op("lgnn::set_readout", mutates_args=(), device_types="cuda")
def set_readout(x: Tensor, gptr: Optional[Tensor], num_sets: int, rows: int,
                mean: bool) -> Tensor:
    return ops.set_readout_fwd(x, gptr, num_sets, rows, mean)


@set_readout.register_fake
def _(x, gptr, num_sets, rows, mean):
    return x.new_empty(num_sets, x.shape[1] if mean else rows * x.shape[1])


@custom_op("lgnn::set_readout_bwd", mutates_args=(), device_types="cuda")
def set_readout_bwd(dout: Tensor, gptr: Optional[Tensor], num_sets: int, rows: int, C: int,
                    mean: bool) -> Tensor:
    return ops.set_readout_bwd(dout, gptr, num_sets, rows, C, mean)


@set_readout_bwd.register_fake
def _(dout, gptr, num_sets, rows, C, mean):
    return dout.new_empty(num_sets * rows, C)


def _readout_setup(ctx, inputs, output):
    x, gptr, num_sets, rows, mean = inputs
    ctx.has_gptr = gptr is not None
    if ctx.has_gptr:
        ctx.save_for_backward(gptr)
    ctx.meta = (num_sets, rows, x.shape[1], mean)


def _readout_backward(ctx, dout):
    gptr = ctx.saved_tensors[0] if ctx.has_gptr else None
    return torch.ops.lgnn.set_readout_bwd(dout, gptr, *ctx.meta), None, None, None, None


set_readout.register_autograd(_readout_backward, setup_context=_readout_setup)



def _isab_params(wb: list[Tensor], ln: list[Tensor]):
    l1, l2 = (list(ln[:4]), list(ln[4:])) if len(ln) else ([None] * 4, [None] * 4)
    return list(wb[:6]) + l1, list(wb[6:]) + l2


@custom_op("lgnn::isab", mutates_args=(), device_types="cuda")
def isab(x: Tensor, ind: Tensor, wb: list[Tensor], ln: list[Tensor], ptr: Optional[Tensor],
         rows: int, num_sets: int, heads: int, mask1: Optional[Tensor],
         mask2: Optional[Tensor]) -> list[Tensor]:
    """[out, h = mab1's output, mab1's ops.MAB_SAVED, mab2's ops.MAB_SAVED]"""
    p1, p2 = _isab_params(wb, ln)
    out, (sv1, sv2) = ops.isab_fwd(x, ind, p1, p2, ptr, rows, num_sets, heads, mask1, mask2)
    return [out, sv2.y] + [_enc(getattr(sv, n), x.device) for sv in (sv1, sv2)
                           for n in ops.MAB_SAVED]


def _mab_saved_fake(x, y, C, R, heads, has_ln, mask, num_sets):
    """ops.MAB_SAVED of a block with query input x, key input y (None: x) and R output rows."""
    f = lambda *s: x.new_empty(*s, dtype=torch.float32)  # noqa: E731
    none = lambda: x.new_empty(0, dtype=torch.uint8)  # noqa: E731
    stat = (lambda: f(R)) if has_ln else none
    proj = f(x.shape[0], 3 * C if y is None else C)
    kv = none() if y is None else f(y.shape[0], 2 * C)
    moff = none() if mask is None else x.new_empty(num_sets + 1, dtype=torch.int64)
    return [proj, kv, f(R, C), f(R, heads), f(R, C), stat(), stat(), f(R, C), f(R, C), stat(),
            stat(), moff]


@isab.register_fake
def _(x, ind, wb, ln, ptr, rows, num_sets, heads, mask1, mask2):
    C = x.shape[1]
    m = ind.shape[0]
    h = x.new_empty(num_sets * m, C)
    return [torch.empty_like(x), h] \
        + _mab_saved_fake(ind, x, C, num_sets * m, heads, len(ln) > 0, mask1, num_sets) \
        + _mab_saved_fake(x, h, C, x.shape[0], heads, len(ln) > 0, mask2, num_sets)


@custom_op("lgnn::isab_bwd", mutates_args=(), device_types="cuda")
def isab_bwd(dout: Tensor, x: Tensor, ind: Tensor, h: Tensor, wb: list[Tensor],
             ln: list[Tensor], saved: list[Tensor], ptr: Optional[Tensor], rows: int,
             num_sets: int, heads: int, mask1: Optional[Tensor], mask2: Optional[Tensor],
             want_dx: bool) -> list[Tensor]:
    """[dx, dind, mab1's then mab2's six weight / bias gradients, then their four LayerNorm
    gradients each] (absent: empty)."""
    p1, p2 = _isab_params(wb, ln)
    n = len(ops.MAB_SAVED)
    f1, f2 = ops.isab_forms(ptr, rows, ind.shape[0], num_sets)
    c = lambda ps: [p.contiguous() if p is not None else None for p in ps]  # noqa: E731
    x, ind = x.contiguous(), ind.contiguous()
    sv1 = ops.MabSaved(ind, x, c(p1), f1, heads, mask1, *[_opt(t) for t in saved[:n]])
    sv2 = ops.MabSaved(x, h, c(p2), f2, heads, mask2, *[_opt(t) for t in saved[n:]])
    dx, dind, d1, d2 = ops.isab_bwd((sv1, sv2), dout, want_dx)
    return _grad_list([dx, dind] + d1[:6] + d2[:6] + d1[6:] + d2[6:], x.device)


@isab_bwd.register_fake
def _(dout, x, ind, h, wb, ln, saved, ptr, rows, num_sets, heads, mask1, mask2, want_dx):
    none = lambda: x.new_empty(0, dtype=torch.uint8)  # noqa: E731
    return [torch.empty_like(x) if want_dx else none(), torch.empty_like(ind)] + \
        [torch.empty_like(p) for p in wb] + \
        ([torch.empty_like(p) for p in ln] if len(ln) else [none() for _ in range(8)])


def _isab_setup(ctx, inputs, output):
    x, ind, wb, ln, ptr, rows, num_sets, heads, mask1, mask2 = inputs
    ts = [ptr, mask1, mask2]
    ctx.present = [t is not None for t in ts]
    ctx.counts = (len(wb), len(ln))
    ctx.save_for_backward(*[t for t in ts if t is not None], x, ind, *wb, *ln, *output[1:])
    ctx.meta = (rows, num_sets, heads)


def _isab_backward(ctx, grads):
    st = list(ctx.saved_tensors)
    ptr, mask1, mask2 = [st.pop(0) if p else None for p in ctx.present]
    x, ind = st.pop(0), st.pop(0)
    nwb, nln = ctx.counts
    wb, ln, h, saved = st[:nwb], st[nwb:nwb + nln], st[nwb + nln], st[nwb + nln + 1:]
    rows, num_sets, heads = ctx.meta
    g = torch.ops.lgnn.isab_bwd(grads[0], x, ind, h, wb, ln, saved, ptr, rows, num_sets, heads,
                                mask1, mask2, ctx.needs_input_grad[0])
    return (_opt(g[0]), g[1], list(g[2:2 + nwb]), list(g[2 + nwb:2 + nwb + nln]) if nln else [],
            None, None, None, None, None, None)


isab.register_autograd(_isab_backward, setup_context=_isab_setup)


@custom_op("lgnn::set_attn", mutates_args=(), device_types="cuda")
def set_attn(q: Tensor, k: Tensor, v: Tensor, qptr: Optional[Tensor], kptr: Optional[Tensor],
             q_rows: int, q_shared: bool, k_rows: int, num_sets: int, heads: int,
             mask: Optional[Tensor]) -> list[Tensor]:
    """[out, lse, mask_off]"""
    form = ops.AttnForm(qptr, q_rows, q_shared, kptr, k_rows, num_sets)
    out, sv = ops.set_attn_fwd(q, k, v, form, heads, mask)
    return [out, sv.lse, _enc(sv.moff, q.device)]


@set_attn.register_fake
def _(q, k, v, qptr, kptr, q_rows, q_shared, k_rows, num_sets, heads, mask):
    R = _mab_rows(q, qptr, q_rows, num_sets)
    moff = q.new_empty(0, dtype=torch.uint8) if mask is None else \
        q.new_empty(num_sets + 1, dtype=torch.int64)
    return [q.new_empty(R, q.shape[1]), q.new_empty(R, heads), moff]


@custom_op("lgnn::set_attn_bwd", mutates_args=(), device_types="cuda")
def set_attn_bwd(dout: Tensor, q: Tensor, k: Tensor, v: Tensor, out: Tensor, lse: Tensor,
                 moff: Tensor, qptr: Optional[Tensor], kptr: Optional[Tensor], q_rows: int,
                 q_shared: bool, k_rows: int, num_sets: int, heads: int,
                 mask: Optional[Tensor]) -> list[Tensor]:
    form = ops.AttnForm(qptr, q_rows, q_shared, kptr, k_rows, num_sets)
    sv = ops.AttnSaved(ops._rows_view(q), ops._rows_view(k), ops._rows_view(v), form, heads, mask,
                       _opt(moff), out, lse)
    return list(ops.set_attn_bwd(sv, dout))


@set_attn_bwd.register_fake
def _(dout, q, k, v, out, lse, moff, qptr, kptr, q_rows, q_shared, k_rows, num_sets, heads, mask):
    return [q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape)]


def _set_attn_setup(ctx, inputs, output):
    q, k, v, qptr, kptr, q_rows, q_shared, k_rows, num_sets, heads, mask = inputs
    ts = [qptr, kptr, mask]
    ctx.present = [t is not None for t in ts]
    ctx.save_for_backward(*[t for t in ts if t is not None], q, k, v, *output)
    ctx.meta = (q_rows, q_shared, k_rows, num_sets, heads)


def _set_attn_backward(ctx, grads):
    st = list(ctx.saved_tensors)
    qptr, kptr, mask = [st.pop(0) if p else None for p in ctx.present]
    q, k, v, out, lse, moff = st
    dq, dk, dv = torch.ops.lgnn.set_attn_bwd(grads[0], q, k, v, out, lse, moff, qptr, kptr,
                                             *ctx.meta, mask)
    return dq, dk, dv, None, None, None, None, None, None, None, None


set_attn.register_autograd(_set_attn_backward, setup_context=_set_attn_setup)
