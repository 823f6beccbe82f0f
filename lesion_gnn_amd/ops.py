"""Autograd ops over the HIP kernels of liblgnn.so. No CPU path: every op requires GPU tensors.

- `node_linear`     Y = act(P(X) W^T + b), P = identity or the CSR aggregation (GCN/GIN conv)
- `spmm`            Y = A X (+ self term) — torch_sparse spmm / PyG propagate(aggr='add')
- `pool_head`       logits = pool(H) Wout^T + bout (global_mean/add_pool + out_proj)
- `segment_pool`    pool(H) alone
- `gcn_stack`       the whole GCN model body as ONE autograd node: in_proj -> L x (GCNConv, ELU)
                    -> pool -> out_proj, with a fused backward chain (pool-broadcast and the
                    transposed aggregation feed the next kernel's prologue, never materialised).
- `set_attention`   segmented multi-head attention over ragged sets; `mab` / `isab`: PyG's
                    MultiheadAttentionBlock / InducedSetAttentionBlock as ONE autograd node each;
                    `res_norm` (residual + activation + LayerNorm), `set_readout`
- `edge_sub`        PointNetConv's split first Linear over the pairs of a cluster.PairGraph;
                    `bn_act_rows` (BatchNorm + ReLU / ELU [+ dropout mask] over rows),
                    `segment_max` (the max aggregation and global_max_pool)
- `collate`         a selection of graphs of a device-resident datasets.GraphStore as one batch
"""
from __future__ import annotations

import ctypes
import weakref
from collections import namedtuple
from typing import NamedTuple

import torch
from torch.utils import _pytree as pytree

from . import _lib
from .graph import NO_CSR, Csr, Graph


def _compiling() -> bool:
    """True while torch.compile / torch.export traces: the ops then dispatch to their
    torch.library custom ops (library.py) instead of the eager autograd.Functions."""
    return torch.compiler.is_compiling()


def _lgnn():
    from . import library

    return library


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    return t.contiguous()


def _s(dev) -> int:
    return _lib.stream(dev)


# ----------------------------------------------------------------------------------------------
# raw launches
# ----------------------------------------------------------------------------------------------


def fast_shape(K: int, N: int) -> bool:
    """Shapes served by the tile fast path (tile.hip): S can be saved in the forward."""
    return K <= 128 and N <= 128 and K % 4 == 0 and N % 4 == 0


# Wide linears (K or N > 128: the reference sweep's widths 256 / 512, scripts/sweep.py:126) run as
# the aggregation (lgnn_spmm) + the split-3 dense GEMMs (s3gemm.hip) instead of the fp32 generic
# node kernels, which stream the weight per 128-wide block and re-derive dZ per output block
# (GIN [512]*4: dX 1.4 ms per launch). WIDE = "f32" keeps the generic kernels (A/B).
WIDE = "s3"


def wide_shape(K: int, N: int) -> bool:
    return WIDE == "s3" and (K > 128 or N > 128) and K % 4 == 0 and N % 4 == 0


def linear_fwd(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor | None, act: int,
               csr: Csr | None = None, self_scale: float = 0.0, save_s: bool = False):
    """Y = act(P(x) W^T + b). With save_s (aggregating fast-path and wide shapes) also returns
    S = P(x)."""
    M, K = x.shape
    N = W.size(0)
    if wide_shape(K, N):
        S = spmm_raw(csr.rowptr, csr.col, csr.w, self_scale, x) if csr is not None else x
        Wp = dense_planes(W, False, False)
        y = torch.empty(M, N, dtype=torch.float32, device=x.device)
        for r0, r1 in _row_blocks(M, K, N):
            _lib.call("lgnn_s3_gemm_act", _lib.ptr(S) + r0 * K * 4, r1 - r0, K, Wp, N, b, act,
                      _lib.ptr(y) + r0 * N * 4, _s(x.device))
        return (y, S) if save_s else y
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    s_out = torch.empty(M, K, dtype=torch.float32, device=x.device) if save_s else None
    c = csr or NO_CSR
    _lib.call("lgnn_node_linear_fwd", x, M, K, c.rowptr, c.col, c.w, float(self_scale), W, b, N,
              act, y, s_out, _s(x.device))
    return (y, s_out) if save_s else y


STACK_MAX = 8  # LGNN_MAX_STACK


# fused stack backward on/off (FUSED_BWD = False selects the layer-wise backward; diagnostics)
FUSED_BWD = True
# the fused stack's graph build skips the transpose CSR when no tile is open
# (LAZY_TRANSPOSE = False: always built)
LAZY_TRANSPOSE = True


# GEMM arithmetic of the fused GCN stack: "s3" = bf16 MFMA on three-plane split operands (fp32
# accuracy, stack3.hip), "f32" = fp32 MFMA (tile.hip). MFMA_MODE = "f32" selects the latter.
MFMA_MODE = "s3"
# Backward of the fused stack (BWD_MODE): "f32" = the fp32 fused kernel (tile.hip k_stack_bwd, one
# launch); "s3" = the split-3 layer-major kernels (stack3_bwd.hip k_s3_bwd: one launch per layer,
# dZ through HBM, 512 partial slots); "s3f" = the fused split-3 kernel (stack3_bwd.hip
# k_s3_fbwd: every layer of a tile in one pass, one launch, 256 slots; the default: 121 us vs
# 154 us for f32 at C2 on MI355X). s3 / s3f need the split-3 forward (their transposed weight
# planes come out of its weight-plane launch); otherwise the f32 kernel runs.
BWD_MODE = "s3f"
BWD_S3 = BWD_MODE in ("s3", "s3f")
# open tiles (an edge leaves them) inside the fused split-3 launches, layer by layer behind grid
# barriers, instead of three layer-wise launches per direction (OPEN_IN_FUSED = "0": separate)
# The fused kernels' open phase saves the six layer-wise launches (~4.5 us each), but runs the
# open tiles ~1.5x slower than the standalone layer-wise kernels (measured C5, r02j). So it is
# taken when open tiles are expected to be rare: "auto" (default) = when every graph could sit
# whole in 64-node tiles (all graphs of one size that divides or is a multiple of 64: the
# batch's node count is B * n with 64 % n == 0 or n % 64 == 0). Either choice is exact; "1" /
# "0" force it (also "fwd" / "bwd" for one direction).
OPEN_IN_FUSED = "auto"
OPEN_IN_FUSED_BWD = OPEN_IN_FUSED
# dP = dlogits W_out formed inside the single-launch split-3 backward (HEAD_FOLD = False: by
# lgnn_pool_head_bwd before it)
HEAD_FOLD = True
# the fused split-3 backward (L <= 2) defers the in_proj fold: its closed tiles only sum
# T = G_1^T X and g = colsum G_1 (no H_0 read, no dW_1 products, no W_1^T T per workgroup) and one
# lgnn_gcn_fold_wgrad launch per step forms dW_0, db_0 and dW_1 from the reduced sums
# (DEFER_FOLD = False: the kernel's legacy mode, every gradient per workgroup)
DEFER_FOLD = True
# the fused split-3 forward (in_proj present, 1 <= L <= 2) folds in_proj into conv 1 on its closed
# tiles: P_1 = X (W_1 W_0)^T + 1 (W_1 b_0)^T from the plane job's fold slot, made from the live
# weights every step; no in_proj GEMM, and no H_0 of a closed tile when the deferred backward (which
# never reads it) follows — otherwise H_0 is stored as before (FWD_FOLD = False: the unfolded
# forward). The logits do not depend on which backward follows.
FWD_FOLD = True
_CAPACITY: dict = {}


def fused_grid_capacity(direction: str, dev) -> int:
    """Workgroups of the fused split-3 forward / backward kernel the device holds at once
    (lgnn_fused_grid_capacity: occupancy per CU x CU count), cached per device."""
    key = (direction, torch.device(dev).index)
    cap = _CAPACITY.get(key)
    if cap is None:
        with torch.cuda.device(dev):
            cap = int(_lib.load().lgnn_fused_grid_capacity(0 if direction == "fwd" else 1))
        if cap < 0:
            _lib.check(cap, "lgnn_fused_grid_capacity")
        _CAPACITY[key] = cap
    return cap


def _open_in_fused(mode, graph: Graph, direction: str) -> bool:
    """Run the open tiles inside the fused launch (behind grid barriers)? Only when every
    workgroup of that launch can be resident at once (a partitioned or smaller device, or CUs
    held by other kernels' reservations, refuse it; the C entry refuses it too)."""
    if not _mode_open_in_fused(mode, graph, direction):
        return False
    M = graph.num_nodes
    ntiles = (M + 63) // 64
    grid = min(ntiles, 512) if direction == "fwd" else \
        _lib.load().lgnn_gcn_stack_bwd_partials(M)
    return grid <= fused_grid_capacity(direction, _graph_device(graph))


def _graph_device(graph):
    """The device of a Graph, or of the graph bundle a compiled op body rebuilds (TGraph: no
    edge_index, its CSR / batch tensors instead)."""
    ei = getattr(graph, "edge_index", None)
    if ei is not None:
        return ei.device
    return (graph.gptr if graph.gptr is not None else graph.batch).device


def _mode_open_in_fused(mode, graph: Graph, direction: str) -> bool:
    if mode in ("1", True):
        return True
    if mode in ("0", False):
        return False
    if mode in ("fwd", "bwd"):
        return mode == direction
    M, B = graph.num_nodes, graph.num_graphs
    if not B or M % B:
        return False
    n = M // B
    return n > 0 and (64 % n == 0 or n % 64 == 0)


def plane_buffers(Ws: list, transposed: bool = False, extra: int = 0, fold: bool = False):
    """Uninitialised buffers for the bf16 three-plane images of the stack weights (split-3
    kernels): (planes [L+1, 3, 128, 128] int16, planes_t or None). planes_t is flat: the
    transposed planes, then `extra` int16 of room (the forward's Â^T planes, bwd_planes_numel).
    fold: `planes` is flat and also holds the fold slot (W_1 W_0's planes) and the 128 floats of
    W_1 b_0 behind the layers' slots; planes_t is the same either way."""
    nl = len(Ws)
    dev = Ws[0].device
    if fold:
        planes = torch.empty((nl + 1) * 3 * 128 * 128 + 2 * 128, dtype=torch.int16, device=dev)
    else:
        planes = torch.empty(nl, 3, 128, 128, dtype=torch.int16, device=dev)
    planes_t = torch.empty(nl * 3 * 128 * 128 + extra, dtype=torch.int16, device=dev) \
        if transposed else None
    return planes, planes_t


def plane_job(Ws: list, d_in: int, planes, planes_t, b0=None) -> _lib.PlaneJob:
    """lgnn_plane_job: the split of Ws into `planes` / `planes_t` (lgnn_weight_planes' arguments),
    run by the graph build's first launch (Graph.csr_planes) or by lgnn_weight_planes. b0
    (in_proj's bias): the job also writes the fold slot (LGNN_PLANE_JOB_FOLD; `planes` from
    plane_buffers(fold=True))."""
    nl = len(Ws)
    if nl > _lib.LGNN_PLANE_JOB_MAX - (b0 is not None):
        raise _lib.LgnnError("plane job: too many layers")
    job = _lib.PlaneJob()
    job.nl = nl | (_lib.LGNN_PLANE_JOB_FOLD if b0 is not None else 0)
    if b0 is not None:
        job.W[nl] = b0.data_ptr()
    widths = [d_in] + [W.size(0) for W in Ws]
    for i, v in enumerate(widths):
        job.widths[i] = v
    for i, W in enumerate(Ws):
        job.W[i] = W.data_ptr()
    job.planes = planes.data_ptr()
    job.planes_t = planes_t.data_ptr() if planes_t is not None else None
    job._keep = (Ws, planes, planes_t, b0)  # the pointers' owners live as long as the job
    return job


def run_plane_job(job: _lib.PlaneJob, dev) -> None:
    """The split of `job` as its own launch (lgnn_weight_planes)."""
    layers = job.nl & ~_lib.LGNN_PLANE_JOB_FOLD
    nw = layers + (1 if job.nl != layers else 0)  # folded: b_0 behind the weights
    _lib.call("lgnn_weight_planes", job.nl, job.W[:nw], job.widths[:layers + 1], job.planes,
              job.planes_t, _s(dev))


def weight_planes(Ws: list, d_in: int, transposed: bool = False, extra: int = 0):
    """bf16 three-plane images of the stack weights for the split-3 kernels (one launch):
    returns (planes [L+1, 3, 128, 128] int16, planes_t or None); see plane_buffers."""
    planes, planes_t = plane_buffers(Ws, transposed, extra)
    run_plane_job(plane_job(Ws, d_in, planes, planes_t), Ws[0].device)
    return planes, planes_t


# The split-3 weight planes are made afresh by every forward, from the live weights: when the
# forward builds its graph the split runs as extra workgroups of the build's first launch
# (lgnn_graph_build_planes), otherwise as its own launch. Nothing is cached across steps, so a
# captured step replays the split and sees any write to the weights between replays
# (load_state_dict, EMA, clipping), eager or captured alike.
def adjt_numel(M) -> int:
    """int16 elements of the Â^T planes the split-3 forward hands to the fused backward."""
    return (M + 63) // 64 * (_lib.LGNN_S3_ADJT_TILE_BYTES // 2)


def bwd_planes_numel(L: int, M) -> int:
    """Size of the buffer the fused GCN forward keeps for its backward (GcnSaved.planes_t): the
    transposed weight planes, plus the Â^T planes when the single-launch split-3 backward runs."""
    return (L + 1) * 3 * 128 * 128 + (adjt_numel(M) if _s3f(L) and ADJT else 0)


def _defers_fold(L: int, s3: bool) -> bool:
    """The fused backward of an L-conv stack runs in its deferred mode (it never reads H_0).
    stack_bwd's `defer` and the forward's choice to leave H_0's closed rows unwritten
    (gcn_stack_fwd) both come from here."""
    return DEFER_FOLD and s3 and _s3f(L) and L <= 2


def _s3f(L: int) -> bool:
    """The fused split-3 backward takes L <= 2 convs in one launch, and L = 3 with the in_proj
    weight gradient outside it (the kernel writes dZ_0; stack_bwd runs the GEMM) when its
    open-tile phase runs in the same launch (stack_bwd checks that; otherwise layer-major s3)."""
    return BWD_MODE == "s3f" and L <= 3


# the split-3 forward hands each closed tile's Â^T planes to the fused backward (ADJT = False: the
# backward rebuilds them from the CSR)
ADJT = True


def _adjt_ptr(planes_t: torch.Tensor, L: int):
    """Device address of the Â^T planes inside planes_t, or None."""
    base = (L + 1) * 3 * 128 * 128
    return planes_t.data_ptr() + 2 * base if planes_t.numel() > base else None


def stack_fwd(x: torch.Tensor, graph: Graph, Ws: list, bs: list, kind: str = "gcn"):
    """stack_fwd_planes without the backward's planes: ([H_0..H_L], [S_1..S_L])."""
    return stack_fwd_planes(x, graph, Ws, bs, kind)[:2]


def stack_fwd_planes(x: torch.Tensor, graph: Graph, Ws: list, bs: list, kind: str = "gcn",
                     keep_planes: bool = False, adjt_after_planes: bool = False,
                     fold: bool = False, keep_h0: bool = True):
    """in_proj + L x ELU(GCNConv) forward, every width <= 128: returns ([H_0..H_L],
    [S_1..S_L], planes_t, adjt_t). Tiles no edge leaves run fused through every layer
    (lgnn_gcn_stack_fwd); the rest (graphs straddling 64-node tiles) layer by layer
    (lgnn_node_linear_fwd_tiles), into the same buffers. With graphs aligned to tiles (C2: N = 64)
    the second group is empty.
    kind: the graph build ("gcn", or "gcn_lazy" when only the fused backward follows).
    keep_planes (split-3 only): planes_t = the transposed weight planes for the split-3 backward,
    adjt_t = the Â^T tiles for its single-launch form (None when ADJT is off or L > 3) — or, with
    adjt_after_planes, those tiles in room after the planes inside planes_t (one buffer: the
    compiled lgnn::gcn_stack op returns it as an output of its own) and adjt_t None.
    fold (split-3 only, L >= 1): the closed tiles take in_proj folded into conv 1
    (LGNN_S3_FWD_FOLD_H0); with keep_h0 False (LGNN_S3_FWD_FOLD) the closed tiles' rows of H_0 are
    left unwritten. H_1..H_L are the same bits either way."""
    M = x.size(0)
    L = len(Ws) - 1
    dev = x.device
    s3 = MFMA_MODE == "s3" and L >= 1
    if fold and not s3:
        raise _lib.LgnnError("stack_fwd_planes: fold needs the split-3 forward")
    mode = 1 if not fold else _lib.LGNN_S3_FWD_FOLD_H0 if keep_h0 else _lib.LGNN_S3_FWD_FOLD
    if s3:
        # the transposed planes (the split-3 backward's dH = G W_l operand) come from the same
        # split when the caller keeps them; the split rides the graph build when this forward
        # builds the graph
        want_adjt = keep_planes and _s3f(L) and ADJT
        extra = adjt_numel(M) if want_adjt and adjt_after_planes else 0
        planes, planes_t = plane_buffers(Ws, transposed=keep_planes, extra=extra, fold=fold)
        job = plane_job(Ws, x.size(1), planes, planes_t, bs[0] if fold else None)
        csr, split_done = graph.csr_planes(kind, job)
        if not split_done:
            run_plane_job(job, dev)
        if extra:  # the Â^T tiles in the room after the planes
            adjt_t, adjt = None, _adjt_ptr(planes_t, L)
        else:
            adjt_t = torch.empty(adjt_numel(M), dtype=torch.int16, device=dev) \
                if want_adjt else None
            adjt = adjt_t
    else:
        csr = graph.csr(kind)
        planes_t = adjt_t = None
    open_ = graph.tile_open(kind)
    hs = [torch.empty(M, W.size(0), dtype=torch.float32, device=dev) for W in Ws]
    ss = [torch.empty(M, Ws[l].size(1), dtype=torch.float32, device=dev) for l in range(1, L + 1)]
    widths = [W.size(0) for W in Ws]
    if s3:
        if _open_in_fused(OPEN_IN_FUSED, graph, "fwd"):  # open tiles in the same launch
            _lib.call("lgnn_gcn_stack_fwd_s3_all", x, M, x.size(1), mode, csr.rowptr, csr.col,
                      csr.w, L, planes, Ws, bs, widths, hs, ss, open_, adjt, _s(dev))
            return hs, ss, planes_t, adjt_t
        _lib.call("lgnn_gcn_stack_fwd_s3", x, M, x.size(1), mode, csr.rowptr, csr.col, csr.w, L,
                  planes, bs, widths, hs, open_, adjt, _s(dev))
    else:
        _lib.call("lgnn_gcn_stack_fwd", x, M, x.size(1), 1, csr.rowptr, csr.col, csr.w, L, Ws,
                  bs, widths, hs, open_, _s(dev))
    for l in range(L + 1):
        inp = x if l == 0 else hs[l - 1]
        c = csr if l > 0 else NO_CSR
        s_out = ss[l - 1] if l > 0 else None
        _lib.call("lgnn_node_linear_fwd_tiles", inp, M, inp.size(1), c.rowptr, c.col, c.w, 0.0,
                  Ws[l], bs[l], Ws[l].size(0),
                  _lib.LGNN_ACT_ELU if l > 0 else _lib.LGNN_ACT_NONE, hs[l], s_out, open_, 1,
                  _s(dev))
    return hs, ss, planes_t, adjt_t


def head_in_stack_bwd(graph: Graph, L: int, C: int, s3: bool) -> bool:
    """True when stack_bwd's single split-3 launch forms dP = dlogits W_out itself (out_proj
    backward folded into the kernel's pool prologue, <= 8 classes)."""
    return (HEAD_FOLD and s3 and BWD_MODE == "s3f" and L <= 3 and C <= 8 and
            _open_in_fused(OPEN_IN_FUSED_BWD, graph, "bwd"))


def stack_bwd(dp: torch.Tensor | None, x: torch.Tensor, graph: Graph, mean: bool, Ws: list,
              hs: list, ss: list, reducer: list, planes_t: torch.Tensor | None = None,
              head: tuple | None = None, kind: str = "gcn", adjt_t: torch.Tensor | None = None,
              b0: torch.Tensor | None = None):
    """Backward of stack_fwd from the pooled-output gradient dp down to in_proj, L >= 1 convs,
    no input gradient. Closed tiles run fused (one launch; L = 3 with in_proj's weight gradient
    as a split-3 GEMM after it, the layer-major split-3 kernels past that); open tiles inside the
    same launch behind grid barriers, or layer by layer (lgnn_node_linear_bwd_tiles,
    want_open = 1) into the same partial slots. Returns ([(dW_l, db_l)] for l = 0..L, after): the
    slab reductions are appended to `reducer`, and `after` (None, or the deferred fold's launch) is
    for the caller to run once they are launched. head = (dlogits, W_out) replaces dp where
    head_in_stack_bwd() allows.
    b0 (in_proj's bias; with DEFER_FOLD, s3f and L <= 2): the kernel's deferred mode — H_0 is not
    passed, the slabs gain the T / g pair, layers 0 and 1 keep open-tile-only slabs whose
    reductions carry the open-tile count as their `live` word, and the fold launch is returned
    for the caller to run behind the reductions."""
    csr = graph.csr(kind)
    open_ = graph.tile_open(kind)
    M = x.size(0)
    L = len(Ws) - 1
    dev = x.device
    lib = _lib.load()
    s3 = planes_t is not None
    s3f = s3 and _s3f(L) and (L <= 2 or _open_in_fused(OPEN_IN_FUSED_BWD, graph, "bwd"))
    # the forward's Â^T tiles: their own buffer (adjt_t), or room after the planes (weight_planes'
    # `extra`); none -> the backward rebuilds them from the CSR
    adjt = (adjt_t if adjt_t is not None else _adjt_ptr(planes_t, L)) if s3f else None
    P = lib.lgnn_gcn_stack_bwd_s3_partials(M) if s3 and not s3f else \
        lib.lgnn_gcn_stack_bwd_partials(M)
    _lib.check(0 if P > 0 else P, "lgnn_gcn_stack_bwd_partials")
    widths = [x.size(1)] + [W.size(0) for W in Ws]
    per = [widths[l + 1] * widths[l] + widths[l + 1] for l in range(L + 1)]
    defer = _defers_fold(L, s3) and b0 is not None
    if defer:  # the T [w2][d_in] / g [w2] slabs ride behind the layers'
        per.append(widths[2] * widths[0] + widths[2])
        hs = [None] + list(hs[1:])
    # (defer: one more word behind the g slab, the launch's closed-tile count)
    slab = torch.empty(P * sum(per) + int(defer), dtype=torch.float32, device=dev)
    dWp, dbp, off = [], [], 0
    for l in range(L + 2 if defer else L + 1):
        nk, n = (widths[2] * widths[0], widths[2]) if l == L + 1 else \
            (widths[l + 1] * widths[l], widths[l + 1])
        dWp.append(slab[off:off + P * nk])
        dbp.append(slab[off + P * nk:off + P * (nk + n)])
        off += P * (nk + n)
    Sx = [x] + list(ss)
    dlog, W_out = head if head is not None else (None, None)
    ce = dlog if isinstance(dlog, _lib.CeSrc) else None  # CE-formed logits gradient
    B = dp.size(0) if dp is not None else (graph.num_graphs if ce is not None else dlog.size(0))
    if s3f and _open_in_fused(OPEN_IN_FUSED_BWD, graph, "bwd"):  # one launch, open tiles last
        # L = 3: the third [M][128] block receives dZ_0, the in_proj output gradient
        dS_ws = torch.empty((3 if L == 3 else 2) * M * 128, dtype=torch.float32, device=dev)
        common = (graph.batch, graph.gptr, int(mean), B, csr.rowptr, csr.col, csr.w, csr.tptr,
                  csr.tidx, csr.tw, x, M, L, planes_t, Ws, hs, ss, widths, dWp, dbp, P, dS_ws,
                  open_)
        if ce is not None:
            _lib.call("lgnn_gcn_stack_bwd_s3f_ce", *common, ctypes.byref(ce), W_out,
                      W_out.size(0), adjt, _s(dev))
        else:
            _lib.call("lgnn_gcn_stack_bwd_s3f_all", dp, *common, dlog, W_out,
                      W_out.size(0) if head else 0, adjt, _s(dev))
        if L == 3:  # in_proj: (dW_0, db_0) = (dZ_0^T X, colsum dZ_0), one split-3 GEMM
            dz0 = dS_ws[2 * M * 128:2 * M * 128 + M * widths[1]].view(M, widths[1])
            first = dense_wgrad(dz0, x, False, want_db=True, reducer=reducer)
            return [first] + _stack_bwd_outputs(L, widths, dWp, dbp, P, dev, reducer, l0=1), None
        if defer:
            return _stack_bwd_outputs_defer(L, widths, dWp, dbp, P, dev, reducer, Ws, b0, open_,
                                            M, slab)
        return _stack_bwd_outputs(L, widths, dWp, dbp, P, dev, reducer), None
    assert head is None, "dP from the logits gradient only in the single-launch split-3 path"
    if s3f:  # one fused split-3 launch, every layer of a tile in one pass (stack3_bwd.hip)
        _lib.call("lgnn_gcn_stack_bwd_s3f", dp, graph.batch, graph.gptr, int(mean), dp.size(0),
                  csr.rowptr, csr.col, csr.w, x, M, L, planes_t, hs, widths, dWp, dbp, P, open_,
                  adjt, _s(dev))
    elif s3:  # one split-3 launch per layer (stack3_bwd.hip); dZ between them in dz_ws
        dz_ws = torch.empty(2 * M * 128, dtype=torch.float32, device=dev)
        _lib.call("lgnn_gcn_stack_bwd_s3", dp, graph.batch, graph.gptr, int(mean), dp.size(0),
                  csr.rowptr, csr.col, csr.w, x, M, L, planes_t, hs, widths, dWp, dbp, P, dz_ws,
                  open_, _s(dev))
    else:
        _lib.call("lgnn_gcn_stack_bwd", dp, graph.batch, graph.gptr, int(mean), csr.rowptr,
                  csr.col, csr.w, x, M, L, Ws, hs, widths, dWp, dbp, P, open_, _s(dev))
    dS = None
    for l in reversed(range(L + 1)):
        K, N = widths[l], widths[l + 1]
        if l == L:
            mode, dY, tc = _lib.LGNN_GRAD_POOL, dp, NO_CSR
        else:
            mode, dY, tc = _lib.LGNN_GRAD_TRANSPOSE, dS, csr
        dX = torch.empty(M, K, dtype=torch.float32, device=dev) if l > 0 else None
        _lib.call("lgnn_node_linear_bwd_tiles", mode, dY, graph.batch, graph.gptr, int(mean),
                  tc.tptr, tc.tidx, tc.tw, 0.0, hs[l] if l > 0 else None,
                  _lib.LGNN_ACT_ELU if l > 0 else _lib.LGNN_ACT_NONE, Sx[l], M, K, None, None,
                  None, 0.0, Ws[l], N, dX, dWp[l], dbp[l], P, open_, 1,
                  ((0, 4)[l] if l < 2 else 2) if defer else 2 if s3f else 1, _s(dev))
        dS = dX
    if defer:
        return _stack_bwd_outputs_defer(L, widths, dWp, dbp, P, dev, reducer, Ws, b0, open_, M,
                                        slab)
    return _stack_bwd_outputs(L, widths, dWp, dbp, P, dev, reducer), None


def _stack_bwd_outputs_defer(L, widths, dWp, dbp, P, dev, reducer, Ws, b0, open_, M, slab):
    """(_stack_bwd_outputs for the deferred fold, the fold launch as a callable). dW_0, db_0 and
    dW_1 first receive the open tiles' totals (slabs that are dead when the open-tile count word
    is 0: `live`); the fold launch, which the caller runs after the reductions, adds W_1^T T,
    W_1^T g and T W_0^T + g b_0^T. The T / g slabs are dead when the launch's closed-tile count
    (the last word of `slab`) is 0."""
    d_in, w1, w2 = widths[0], widths[1], widths[2]
    live = open_[(M + 63) // 64:]  # the open-tile count word
    closed = slab[-1:].view(torch.int32)  # the closed-tile count word
    T = torch.empty(w2, d_in, dtype=torch.float32, device=dev)
    g = torch.empty(w2, dtype=torch.float32, device=dev)
    out = []
    for l in range(L + 1):
        dW = torch.empty(widths[l + 1], widths[l], dtype=torch.float32, device=dev)
        db = torch.empty(widths[l + 1], dtype=torch.float32, device=dev)
        reducer.extend([(dWp[l], P, dW.numel(), dW, None, 0, live if l < 2 else None),
                        (dbp[l], P, db.numel(), db, None, 0, live if l < 1 else None)])
        out.append((dW, db))
    reducer.extend([(dWp[L + 1], P, T.numel(), T, None, 0, closed),
                    (dbp[L + 1], P, g.numel(), g, None, 0, closed)])
    (dW0, db0), dW1 = out[0], out[1][0]

    def fold():  # the open totals are added in place (element by element: aliasing is safe)
        _lib.call("lgnn_gcn_fold_wgrad", T, g, Ws[0], b0, Ws[1], d_in, w1, w2, dW0, db0, dW1,
                  closed, dW0, db0, dW1, _s(dev))

    return out, fold


def _stack_bwd_outputs(L, widths, dWp, dbp, P, dev, reducer, l0=0):
    out = []
    for l in range(l0, L + 1):
        dW = torch.empty(widths[l + 1], widths[l], dtype=torch.float32, device=dev)
        db = torch.empty(widths[l + 1], dtype=torch.float32, device=dev)
        reducer.extend([(dWp[l], P, dW.numel(), dW), (dbp[l], P, db.numel(), db)])
        out.append((dW, db))
    return out


def num_partials(M: int, N: int, K: int, gather: bool = False) -> int:
    p = _lib.load().lgnn_bwd_num_partials(M, N, K, int(gather))
    _lib.check(0 if p > 0 else p, "lgnn_bwd_num_partials")
    return p


def linear_bwd(grad_mode: int, dY: torch.Tensor, *, H: torch.Tensor | None, act: int,
               X: torch.Tensor, W: torch.Tensor, csr: Csr | None = None, self_scale: float = 0.0,
               graph: Graph | None = None, pool_mean: bool = True, tcsr: Csr | None = None,
               tself: float = 0.0, want_dx: bool = True, want_db: bool = True,
               reducer: list | None = None):
    """Returns (dXpre or None, dW, db or None). dXpre = dZ W (pre-aggregation input grad).
    With `reducer` (a list), the dW/db slab reductions are appended to it for one batched
    launch (reduce_multi) instead of running here."""
    M, K = X.shape
    N = W.size(0)
    dev = X.device
    if wide_shape(K, N):
        # the output gradient as given, from the pooled gradient, or gathered through the
        # transpose CSR; dZ = g * act'(H); then dXpre = dZ W and (dW, db) = (dZ^T S, sum dZ)
        if grad_mode == _lib.LGNN_GRAD_POOL:
            g = pool_bwd(_f32c(dY), graph, pool_mean, M)
        elif grad_mode == _lib.LGNN_GRAD_TRANSPOSE:
            g = spmm_raw(tcsr.tptr, tcsr.tidx, tcsr.tw, tself, dY)
        else:
            g = _f32c(dY)
        if act == _lib.LGNN_ACT_ELU:
            dZ = torch.empty_like(g)
            _lib.call("lgnn_act_bwd", g, H, dZ, g.numel(), act, _s(dev))
        else:
            dZ = g
        S = spmm_raw(csr.rowptr, csr.col, csr.w, self_scale, X) if csr is not None else X
        dX = dense_mm(dZ, dense_planes(W, True, False), K, None, False) if want_dx else None
        dW, db = dense_wgrad(dZ, S, False, want_db=want_db, reducer=reducer)
        return dX, dW, db
    P = num_partials(M, N, K, csr is not None)
    slab = torch.empty(P * N * K + (P * N if want_db else 0), dtype=torch.float32, device=dev)
    dWp = slab[: P * N * K]
    dbp = slab[P * N * K:] if want_db else None
    dX = torch.empty(M, K, dtype=torch.float32, device=dev) if want_dx else None
    batch = graph.batch if graph is not None else None
    gptr = graph.gptr if graph is not None else None
    t, c = tcsr or NO_CSR, csr or NO_CSR
    _lib.call("lgnn_node_linear_bwd", grad_mode, dY, batch, gptr, int(pool_mean), t.tptr, t.tidx,
              t.tw, float(tself), H, act, X, M, K, c.rowptr, c.col, c.w, float(self_scale), W, N,
              dX, dWp, dbp, P, _s(dev))
    dW = torch.empty(N, K, dtype=torch.float32, device=dev)
    db = torch.empty(N, dtype=torch.float32, device=dev) if want_db else None
    jobs = [(dWp, P, N * K, dW)] + ([(dbp, P, N, db)] if want_db else [])
    if reducer is not None:  # caller batches the slab reductions of several layers
        reducer.extend(jobs)
    else:
        reduce_multi(jobs, dev)
    return dX, dW, db


CE_PART = object()  # reduce_multi job part: the CE logits gradient, formed in the reduction


def reduce_multi(jobs: list, dev, ce=None, num_classes: int = 0) -> None:
    """Deterministic slab reductions [(partials, P, len, out), ...] in one launch per 16; a job
    (a, P, len, out, f, width) is the outer-product sum out[c, d] = sum_p a[p, c] f[p, d]. A job
    whose partials are CE_PART takes the [P][C] CE logits gradient formed from `ce`
    (_lib.CeSrc, lgnn_reduce_jobs_ce) instead of a materialised dlogits tensor. A seventh field is
    the job's `live` word (a device int32, lgnn_reduce_jobs_live: 0 = slab not read, out zeros)."""
    for i in range(0, len(jobs), 16):
        chunk = jobs[i:i + 16]
        n = len(chunk)
        is_ce = [j[0] is CE_PART for j in chunk]
        parts = [None if c else j[0] for j, c in zip(chunk, is_ce)]
        nps = [j[1] for j in chunk]
        lens = [j[2] for j in chunk]
        outs = [j[3] for j in chunk]
        fac = [j[4] if len(j) > 4 else None for j in chunk]
        wid = [j[5] if len(j) > 4 else 0 for j in chunk]
        live = [j[6] if len(j) > 6 else None for j in chunk]
        if any(lv is not None for lv in live):
            if any(is_ce) and ce is None:
                raise _lib.LgnnError("reduce_multi: a CE_PART job needs the CE source")
            _lib.call("lgnn_reduce_jobs_live", n, parts, fac, wid, nps, lens, outs,
                      [int(c) for c in is_ce] if any(is_ce) else None,
                      ctypes.byref(ce) if any(is_ce) else None, int(num_classes), live,
                      _s(dev))
        elif any(is_ce):
            if ce is None:
                raise _lib.LgnnError("reduce_multi: a CE_PART job needs the CE source")
            _lib.call("lgnn_reduce_jobs_ce", n, parts, fac, wid, nps, lens, outs,
                      [int(c) for c in is_ce], ctypes.byref(ce), int(num_classes), _s(dev))
        elif any(len(j) > 4 for j in chunk):
            _lib.call("lgnn_reduce_jobs", n, parts, fac, wid, nps, lens, outs, _s(dev))
        else:
            _lib.call("lgnn_reduce_partials_multi", n, parts, nps, lens, outs, _s(dev))


def spmm_raw(rowptr, col, w, self_scale: float, x: torch.Tensor) -> torch.Tensor:
    M, D = x.shape
    y = torch.empty_like(x)
    _lib.call("lgnn_spmm", rowptr, col, w, float(self_scale), x, M, D, y, _s(x.device))
    return y


def pool_head_fwd(H: torch.Tensor, graph: Graph, mean: bool, Wout=None, bout=None):
    B, D = graph.num_graphs, H.size(1)
    pooled = torch.empty(B, D, dtype=torch.float32, device=H.device)
    C = Wout.size(0) if Wout is not None else 0
    logits = torch.empty(B, C, dtype=torch.float32, device=H.device) if Wout is not None else None
    _lib.call("lgnn_pool_head_fwd", H, graph.gptr, B, D, int(mean), Wout, bout, C, pooled, logits,
              _s(H.device))
    return pooled, logits


def pool_head_bwd(dlogits: torch.Tensor, pooled: torch.Tensor, Wout: torch.Tensor):
    B, D = pooled.shape
    C = Wout.size(0)
    dev = pooled.device
    dp = torch.empty(B, D, dtype=torch.float32, device=dev)
    dWo = torch.empty(C, D, dtype=torch.float32, device=dev)
    dbo = torch.empty(C, dtype=torch.float32, device=dev)
    _lib.call("lgnn_pool_head_bwd", dlogits, pooled, B, D, Wout, C, dp, dWo, dbo, _s(dev))
    return dp, dWo, dbo


def pool_bwd(dpooled: torch.Tensor, graph: Graph, mean: bool, M: int) -> torch.Tensor:
    D = dpooled.size(1)
    dH = torch.empty(M, D, dtype=torch.float32, device=dpooled.device)
    _lib.call("lgnn_pool_bwd", dpooled, graph.batch, graph.gptr, M, D, int(mean), dH,
              _s(dpooled.device))
    return dH


# ----------------------------------------------------------------------------------------------
# autograd functions
# ----------------------------------------------------------------------------------------------


# Every op with a compiled twin (library.py) is three plain pieces, shared by its eager
# autograd.Function and its torch.library custom ops:
#   <op>_plan(shapes, flags) -> a record of the path decisions (module switches read at call time)
#   <op>_fwd(inputs...)      -> (outputs..., saved): saved is a record of what the backward needs
#   <op>_bwd(saved, grad, want_dx, ...) -> every gradient and buffer its callers use
# The autograd.Functions below only move `saved` through an autograd ctx (_save / _load).


def _save(ctx, saved) -> None:
    """A saved record onto an autograd ctx: its tensors (at any depth) through
    save_for_backward, the rest of its leaves and its structure as attributes."""
    leaves, ctx.spec = pytree.tree_flatten(saved)
    ctx.slots = [i for i, v in enumerate(leaves) if isinstance(v, torch.Tensor)]
    ctx.save_for_backward(*[leaves[i] for i in ctx.slots])
    ctx.leaves = [None if isinstance(v, torch.Tensor) else v for v in leaves]


def _load(ctx):
    leaves = list(ctx.leaves)
    for i, t in zip(ctx.slots, ctx.saved_tensors):
        leaves[i] = t
    return pytree.tree_unflatten(leaves, ctx.spec)


# graph: a Graph, or None (no aggregation)
LinearSaved = namedtuple("LinearSaved", "x W y graph kind self_scale act has_b")


def node_linear_fwd(x, W, b, graph, kind, self_scale, act):
    _lib.require_gpu(x, W)
    x, W = _f32c(x), _f32c(W)
    b = _f32c(b) if b is not None else None
    csr = graph.csr(kind) if graph is not None else None
    y = linear_fwd(x, W, b, act, csr, self_scale)
    return y, LinearSaved(x, W, y, graph, kind, self_scale, act, b is not None)


def node_linear_bwd(sv: LinearSaved, dy, want_dx: bool):
    """(dx or None, dW, db or None)"""
    csr = sv.graph.csr(sv.kind) if sv.graph is not None else None
    dxpre, dW, db = linear_bwd(_lib.LGNN_GRAD_DIRECT, _f32c(dy), H=sv.y, act=sv.act, X=sv.x,
                               W=sv.W, csr=csr, self_scale=sv.self_scale, want_dx=want_dx,
                               want_db=sv.has_b)
    dx = None
    if want_dx:
        dx = dxpre if csr is None else spmm_raw(csr.tptr, csr.tidx, csr.tw, sv.self_scale, dxpre)
    return dx, dW, db


class _NodeLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, graph, kind, self_scale, act):
        y, saved = node_linear_fwd(x, W, b, graph, kind, self_scale, act)
        _save(ctx, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        return (*node_linear_bwd(_load(ctx), dy, ctx.needs_input_grad[0]), None, None, None, None)


def node_linear(x, W, b=None, graph: Graph | None = None, kind: str = "gcn",
                self_scale: float = 0.0, act: int = _lib.LGNN_ACT_NONE):
    if _compiling():
        lib = _lgnn()
        g = lib.gparts(graph, kind) if graph is not None else lib.gparts_empty(x.device)
        return torch.ops.lgnn.node_linear(x, W, b, g, kind if graph is not None else "",
                                          float(self_scale), int(act))
    return _NodeLinear.apply(x, W, b, graph, kind, self_scale, act)


def dense_planes(W: torch.Tensor, transposed: bool, bf16: bool) -> torch.Tensor:
    """The weight operand of dense_mm for W [rows][cols] (lgnn_s3_weight_planes): B = W
    (Y = A W^T) or B = W^T (transposed: Y = A W); three bf16 planes (fp32 accuracy) or, in bf16
    mode, one RNE-rounded plane. One launch; the optimizer updates W in place each step, so the
    planes are written afresh by every forward / backward that uses them."""
    W = _f32c(W)
    rows, cols = W.shape
    out, inn = (cols, rows) if transposed else (rows, cols)
    planes = 1 if bf16 else 3
    n = _lib.load().lgnn_s3_weight_planes_numel(out, inn, planes)
    Wp = torch.empty(n, dtype=torch.int16, device=W.device)
    _lib.call("lgnn_s3_weight_planes", W, rows, cols, int(transposed), planes, Wp, _s(W.device))
    return Wp


def _s3_bundle_sizes(shapes, transposed, bf16: bool) -> list:
    """lgnn_s3_weight_planes_numel per operand, restated in Python (Dynamo traces this; a
    ctypes call would break the graph): ceil(out/128) blocks x planes x 128 x kpad(in, 64)."""
    planes = 1 if bf16 else 3
    out = []
    for (rows, cols), t in zip(shapes, transposed):
        o, i = (cols, rows) if t else (rows, cols)
        out.append((o + 127) // 128 * planes * 128 * ((i + 63) // 64 * 64))
    return out


def s3_bundle_raw(Ws: list, transposed: list, bf16: bool) -> torch.Tensor:
    """The planes of every (W, transposed) operand in one flat int16 buffer (each operand's
    numel a multiple of 8192: every view 16 KiB aligned), LGNN_MAX_WPREP jobs per launch."""
    Ws = [_f32c(W) for W in Ws]
    sizes = _s3_bundle_sizes([tuple(W.shape) for W in Ws], transposed, bf16)
    flat = torch.empty(sum(sizes), dtype=torch.int16, device=Ws[0].device)
    views = flat.split(sizes)
    for j0 in range(0, len(Ws), 16):
        js = range(j0, min(j0 + 16, len(Ws)))
        _lib.call("lgnn_s3_weight_planes_multi", len(js), [Ws[j] for j in js],
                  [Ws[j].size(0) for j in js], [Ws[j].size(1) for j in js],
                  [int(bool(transposed[j])) for j in js], 1 if bf16 else 3,
                  [views[j] for j in js], _s(flat.device))
    return flat


def s3_weight_bundle(specs: list, bf16: bool) -> list:
    """Every split-3 weight operand of a step — specs = [(W, transposed)] — in one launch
    (lgnn_s3_weight_planes_multi) instead of one dense_planes launch per GEMM: returns, per spec,
    the planes dense_planes(W, transposed, bf16) would (views of one buffer). The optimizer
    updates the weights in place, so a model asks for its bundle afresh every forward."""
    Ws = [W.detach() for W, _ in specs]
    tr = [bool(t) for _, t in specs]
    if _compiling():
        flat = torch.ops.lgnn.s3_weight_planes_multi(Ws, tr, bool(bf16))
    else:
        flat = s3_bundle_raw(Ws, tr, bf16)
    return list(flat.split(_s3_bundle_sizes([tuple(W.shape) for W in Ws], tr, bf16)))


def _row_blocks(M: int, K: int, N: int, pad_rows: int = 64) -> list:
    """Row ranges [r0, r1) of an M-row GEMM operand that the kernels' 32-bit buffer offsets
    address: (rows + pad_rows) * K * 4 < 2^31 and rows * N * 4 < 2^30 (s3gemm.hip / bflin.hip
    refuse bigger launches with LGNN_EINVAL). Blocks start on 64-row boundaries, so per-tile
    outputs (column-sum rows) of consecutive blocks are contiguous. One block below the limits:
    at the reference's d_in = 1025 a block holds ~520 k nodes."""
    if M <= 0:
        return [(0, max(M, 0))]
    rows = min(((1 << 31) - 1) // (4 * max(K, 1)) - pad_rows, ((1 << 30) - 1) // (4 * max(N, 1)))
    rows = max(64, rows // 64 * 64)
    return [(r, min(r + rows, M)) for r in range(0, M, rows)]


def dense_mm(a: torch.Tensor, Wp: torch.Tensor, N: int, bias, bf16: bool,
             want_colsum: bool = False) -> torch.Tensor:
    """Y = a B^T (+ bias) on the split-3 (fp32 accuracy) or bf16-operand MFMA kernel
    (lgnn_s3_gemm); B's planes from dense_planes. a is fp32 (a bf16 copy is widened: exact).
    Operands past the kernel's 32-bit offsets run as several row-block launches."""
    a = a.float().contiguous() if a.dtype != torch.float32 else a.contiguous()
    M, K = a.shape
    Y = torch.empty(M, N, dtype=torch.float32, device=a.device)
    cs = torch.empty((M + 63) // 64 * N, dtype=torch.float32, device=a.device) \
        if want_colsum and M > 0 else None
    bias = _f32c(bias) if bias is not None else None
    for r0, r1 in _row_blocks(M, K, N):
        _lib.call("lgnn_s3_gemm", _lib.ptr(a) + r0 * K * 4, r1 - r0, K, Wp, N,
                  1 if bf16 else 3, bias, _lib.ptr(Y) + r0 * N * 4,
                  _lib.ptr(cs) + (r0 // 64) * N * 4 if cs is not None else None, _s(a.device))
    if cs is not None:
        _COLSUMS[id(Y)] = (weakref.ref(Y), Y._version, cs)
        weakref.finalize(Y, _COLSUMS.pop, id(Y), None)
    return Y


def dense_wgrad(dy: torch.Tensor, x: torch.Tensor, bf16: bool, want_db: bool = False,
                reducer: list | None = None):
    """(dW, db) = (dy^T x, dy.sum(0)) on lgnn_s3_wgrad: partial slabs over row splits (and the
    bias gradient's partial rows from the same pass over dy), summed in fixed order by one
    reduction launch (or appended to `reducer`, the caller's batched reduction)."""
    dy = dy.float().contiguous() if dy.dtype != torch.float32 else dy.contiguous()
    x = x.float().contiguous() if x.dtype != torch.float32 else x.contiguous()
    M, K = x.shape
    N = dy.size(1)
    dev = x.device
    if N % 2:  # the kernel reads dY in column pairs: pad one zero column (exact)
        dy = torch.nn.functional.pad(dy, (0, 1))
    Ne = dy.size(1)
    lib = _lib.load()
    # row blocks past the kernel's 32-bit offsets: each block's partial slabs follow the
    # previous block's, so one fixed-order reduction sums them all
    blocks = _row_blocks(M, max(K, Ne), 0, pad_rows=64)
    Ss = [lib.lgnn_s3_wgrad_partials(r1 - r0, K, Ne) for r0, r1 in blocks]
    S = sum(Ss)
    part = torch.empty(S * Ne * K, dtype=torch.float32, device=dev)
    dbp = torch.empty(S * Ne, dtype=torch.float32, device=dev) if want_db else None
    so = 0
    for (r0, r1), Sb in zip(blocks, Ss):
        _lib.call("lgnn_s3_wgrad", _lib.ptr(dy) + r0 * Ne * 4, Ne, _lib.ptr(x) + r0 * K * 4,
                  r1 - r0, K, 1 if bf16 else 3, _lib.ptr(part) + so * Ne * K * 4, Sb,
                  _lib.ptr(dbp) + so * Ne * 4 if dbp is not None else None, _s(dev))
        so += Sb
    dW = torch.empty(Ne, K, dtype=torch.float32, device=dev)
    db = torch.empty(Ne, dtype=torch.float32, device=dev) if want_db else None
    jobs = [(part, S, Ne * K, dW)] + ([(dbp, S, Ne, db)] if want_db else [])
    if reducer is not None:
        reducer.extend(jobs)
    else:
        reduce_multi(jobs, dev)
    if Ne != N:
        dW, db = dW[:N], (db[:N] if db is not None else None)
    return dW, db


# bf16 GEMMs on the hand-written MFMA kernels (csrc/bflin.hip); BF16_MFMA = False (A/B) and widths
# N > 128 route them to the one-plane split GEMMs above (dense_mm / dense_wgrad with bf16=True)
BF16_MFMA = True


def bf16_mfma_fits(N: int) -> bool:
    return BF16_MFMA and 1 <= N <= 128 and N % 2 == 0


# operands prepared ahead for this forward (bf16_prepare_weights), each taken once
_PREPARED: dict = {}


def bf16_prepare_weights(weights: list) -> None:
    """The bf16 operands (Wb and, when K <= 128, WTb) of several weights in one launch
    (lgnn_bf16_weight_prep_multi). Each is handed out ONCE by bf16_weight_operands for the same
    tensor at the same version, so a later step (the optimizer updates weights in place, without
    a version bump) always prepares afresh."""
    ws = [_f32c(W) for W in weights if bf16_mfma_fits(W.size(0))][:8]
    if not ws:
        return
    lib = _lib.load()
    ops_ = []
    for W in ws:
        N, K = W.shape
        Wb = torch.empty(128 * lib.lgnn_bf16_kpad(K), dtype=torch.bfloat16, device=W.device)
        WTb = torch.empty(128 * lib.lgnn_bf16_kpad(N), dtype=torch.bfloat16, device=W.device) \
            if K <= 128 else None
        ops_.append((W, Wb, WTb))
    _lib.call("lgnn_bf16_weight_prep_multi", len(ops_), [o[0] for o in ops_],
              [o[0].size(0) for o in ops_], [o[0].size(1) for o in ops_],
              [o[1] for o in ops_], [o[2] for o in ops_], _s(ws[0].device))
    for W, Wb, WTb in ops_:
        _PREPARED[id(W)] = (weakref.ref(W), W._version, Wb, WTb)


def bf16_weight_operands(W: torch.Tensor, want_t: bool):
    """(Wb, WTb): bf16 W [128][kpad(K)] and, when want_t and K <= 128, bf16 W^T [128][kpad(N)]
    (zero-padded operands of lgnn_bf16_gemm), in one launch — or the pair bf16_prepare_weights
    made for W in this forward."""
    W = _f32c(W)
    rec = _PREPARED.pop(id(W), None)
    if rec is not None and rec[0]() is W and rec[1] == W._version \
            and (rec[3] is not None or not want_t or W.size(1) > 128):
        return rec[2], rec[3]
    N, K = W.shape
    lib = _lib.load()
    Wb = torch.empty(128 * lib.lgnn_bf16_kpad(K), dtype=torch.bfloat16, device=W.device)
    WTb = torch.empty(128 * lib.lgnn_bf16_kpad(N), dtype=torch.bfloat16, device=W.device) \
        if want_t and K <= 128 else None
    _lib.call("lgnn_bf16_weight_prep", W, N, K, Wb, WTb, _s(W.device))
    return Wb, WTb


def bf16_gemm(A: torch.Tensor, Wb: torch.Tensor, bias, N: int, want_yb: bool = False,
              want_colsum: bool = False):
    """Y = bf16(A) bf16(W)^T (+ bias) in fp32 (and its bf16 copy when want_yb): A fp32 (rounded
    in the kernel) or bf16. want_colsum: Y's per-tile column sums are remembered beside Y
    (colsum_of: a following Linear's bias gradient without a pass over Y)."""
    A = A.contiguous()
    M, K = A.shape
    Y = torch.empty(M, N, dtype=torch.float32, device=A.device)
    Yb = torch.empty(M, N, dtype=torch.bfloat16, device=A.device) if want_yb else None
    cs = torch.empty((M + 63) // 64 * N, dtype=torch.float32, device=A.device) \
        if want_colsum and M > 0 else None
    es = A.element_size()
    bias = _f32c(bias) if bias is not None else None
    for r0, r1 in _row_blocks(M, K, N):  # row blocks past the kernel's 32-bit offsets
        _lib.call("lgnn_bf16_gemm", _lib.ptr(A) + r0 * K * es, int(A.dtype == torch.float32),
                  r1 - r0, K, Wb, bias, N, _lib.ptr(Y) + r0 * N * 4,
                  _lib.ptr(Yb) + r0 * N * 2 if Yb is not None else None,
                  _lib.ptr(cs) + (r0 // 64) * N * 4 if cs is not None else None, _s(A.device))
    if cs is not None:
        _COLSUMS[id(Y)] = (weakref.ref(Y), Y._version, cs)
        weakref.finalize(Y, _COLSUMS.pop, id(Y), None)
    return Y, Yb


_COLSUMS: dict = {}


def colsum_of(y: torch.Tensor, reducer: list = None):
    """y.sum(0) from the per-tile column sums its producing GEMM wrote (fixed order), if y is
    that output unchanged; else None. With `reducer` the slab reduction is appended to that job
    list (the caller launches the batch, reduce_multi) instead of launched here."""
    rec = _COLSUMS.get(id(y))
    if rec is None:
        return None
    ref, version, cs = rec
    if ref() is not y or y._version != version:
        return None
    N = y.size(1)
    out = torch.empty(N, dtype=torch.float32, device=y.device)
    if reducer is not None:
        reducer.append((cs, cs.numel() // N, N, out))
    else:
        _lib.call("lgnn_reduce_partials", cs, cs.numel() // N, N, out, _s(y.device))
    return out


def bf16_wgrad(dYb: torch.Tensor, X: torch.Tensor, N: int, reducer: list = None) -> torch.Tensor:
    """dW = bf16(dY)^T bf16(X): partial slabs over row splits, summed in fixed order (with
    `reducer`: the sum is appended to the caller's job list, launched with its other slabs)."""
    X = X.contiguous()
    M, K = X.shape
    if X.dtype != torch.float32 and K % 2:  # bf16 X needs even rows; bf16 -> fp32 is exact
        X = X.float()
    dev = X.device
    lib = _lib.load()
    es = X.element_size()
    blocks = _row_blocks(M, K, 0, pad_rows=32 * 64)  # past the kernel's 32-bit offsets
    Ss = [lib.lgnn_bf16_wgrad_partials(r1 - r0, K) for r0, r1 in blocks]
    S = sum(Ss)
    part = torch.empty(S * N * K, dtype=torch.float32, device=dev)
    so = 0
    for (r0, r1), Sb in zip(blocks, Ss):
        _lib.call("lgnn_bf16_wgrad", _lib.ptr(dYb) + r0 * N * 2, N, _lib.ptr(X) + r0 * K * es,
                  int(X.dtype == torch.float32), r1 - r0, K, _lib.ptr(part) + so * N * K * 4, Sb,
                  _s(dev))
        so += Sb
    dW = torch.empty(N, K, dtype=torch.float32, device=dev)
    if reducer is not None:
        reducer.append((part, S, N * K, dW))
    else:
        _lib.call("lgnn_reduce_partials", part, S, N * K, dW, _s(dev))
    return dW


def _bf16_operand(t: torch.Tensor) -> torch.Tensor:
    """The bf16 copy a kernel wrote beside t, else t's own cast."""
    tb = _bf16_copy_of(t)
    return tb if tb is not None else t.to(torch.bfloat16)


class DensePlan(NamedTuple):
    mfma: bool    # bf16 mode on the hand-written bf16 MFMA GEMMs (bflin.hip)
    x_bf16: bool  # the compiled backward receives x rounded to bf16 (bf16 mode off those GEMMs)


def dense_plan(N: int, bf16: bool) -> DensePlan:
    mfma = bool(bf16) and bf16_mfma_fits(N)
    return DensePlan(mfma, bool(bf16) and not mfma)


# x: fp32, or the bf16 copy its producer wrote (mfma); wt: bf16 W^T from the forward's weight
# prep (mfma, K <= 128) or None
DenseSaved = namedtuple("DenseSaved", "x W wt bf16 has_b plan")


def dense_linear_fwd(x, W, b, bf16, wp=None):
    _lib.require_gpu(x, W)
    x, W = _f32c(x), _f32c(W)
    plan = dense_plan(W.size(0), bf16)
    if plan.mfma:
        # hand-written bf16 MFMA GEMM: an fp32 x is rounded as the kernel loads it (no copy);
        # the output's bf16 copy feeds the next bf16 GEMM
        xb = _bf16_copy_of(x)
        A = xb if xb is not None else x
        Wb, WTb = bf16_weight_operands(W, True)
        y, yb = bf16_gemm(A, Wb, b, W.size(0), want_yb=BF16_OUT)
        if yb is not None:
            _remember_bf16(y, yb)
        return y, DenseSaved(A, W, WTb, bf16, b is not None, plan)
    # split-3 MFMA GEMM at fp32 accuracy (bf16 mode: RNE-rounded operands, N > 128)
    y = dense_mm(x, wp if wp is not None else dense_planes(W, False, bf16), W.size(0), b, bf16)
    return y, DenseSaved(x, W, None, bf16, b is not None, plan)


def dense_linear_bwd(sv: DenseSaved, dy, want_dx: bool):
    """(dx or None, dW, db or None)"""
    x, W = sv.x, sv.W
    dy = _f32c(dy)
    N, K = W.shape
    jobs = [] if sv.plan.mfma else None  # db's and dW's slab sums in one launch
    db = None
    if sv.has_b:  # from the column sums dy's producing GEMM wrote, when it was ours
        db = colsum_of(dy, jobs)
        if db is None and sv.plan.mfma:
            db = dy.sum(0)
    if sv.plan.mfma:
        dyb = _bf16_operand(dy)
        dW = bf16_wgrad(dyb, x, N, jobs)
        reduce_multi(jobs, dW.device)
        dx = None
        if want_dx:
            if K <= 128:
                WTb = sv.wt if sv.wt is not None else bf16_weight_operands(W, True)[1]
                dx, dxb = bf16_gemm(dyb, WTb, None, K, want_yb=BF16_OUT)
                if dxb is not None:
                    _remember_bf16(dx, dxb)
            else:
                dx = dense_mm(dyb, dense_planes(W, True, True), K, None, True)
        return dx, dW, db
    dW, db2 = dense_wgrad(dy, x, sv.bf16, want_db=sv.has_b and db is None)
    if db is None and sv.has_b:
        db = db2
    dx = dense_mm(dy, dense_planes(W, True, sv.bf16), K, None, sv.bf16) if want_dx else None
    return dx, dW, db


class _DenseLinear(torch.autograd.Function):
    """y = x W^T + b for shapes outside the tile kernels (K > 128, K % 4 != 0: the reference's
    in_proj with 1025 input channels, gat.py:29 / lesions.py:142,169) or in bf16 mode, on the
    hand-written MFMA GEMMs: bf16 mode with N <= 128 on bflin.hip, everything else on the
    split-3 kernels of s3gemm.hip (fp32 accuracy; bf16 mode N > 128: one rounded plane). The
    backward is dW = dy^T x, db = colsum dy (from the same pass), dx = dy W in the same
    precision."""

    @staticmethod
    def forward(ctx, x, W, b, bf16, wp=None):
        y, saved = dense_linear_fwd(x, W, b, bf16, wp)
        _save(ctx, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        return (*dense_linear_bwd(_load(ctx), dy, ctx.needs_input_grad[0]), None, None)


def dense_linear(x, W, b=None, bf16: bool = False, wp=None):
    """wp: W's split-3 planes from s3_weight_bundle (else made here, one launch)."""
    if _compiling():
        return torch.ops.lgnn.dense_linear(x, W, b, bool(bf16), wp)
    return _DenseLinear.apply(x, W, b, bf16, wp)


def dense_path(W, bf16: bool) -> bool:
    """Whether linear_auto runs W on the split-3 GEMMs (so s3_weight_bundle can prepare it)."""
    return not bf16 and not fast_shape(W.size(1), W.size(0))


def linear_auto(x, W, b=None, bf16: bool = False, wp=None):
    """node_linear (tile kernels) where the shape allows and fp32 is asked for; else the
    hand-written dense GEMMs (dense_linear: split-3 s3gemm.hip, or one bf16 plane in bf16 mode)."""
    if not bf16 and fast_shape(W.size(1), W.size(0)):
        return node_linear(x, W, b)
    return dense_linear(x, W, b, bf16, wp)


class _Spmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, kind, self_scale):
        _lib.require_gpu(x)
        c = graph.csr(kind)
        # the Csr itself, not its key: a later weighted() call may replace the "weighted" entry
        ctx.c, ctx.self_scale = c, self_scale
        return spmm_raw(c.rowptr, c.col, c.w, self_scale, _f32c(x))

    @staticmethod
    def backward(ctx, dy):
        c = ctx.c
        return spmm_raw(c.tptr, c.tidx, c.tw, ctx.self_scale, _f32c(dy)), None, None, None


def spmm(x, graph: Graph, kind: str = "gin", self_scale: float = 0.0):
    if _compiling():
        return torch.ops.lgnn.spmm(x, _lgnn().gparts(graph, kind), float(self_scale), False)
    return _Spmm.apply(x, graph, kind, self_scale)


class _Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, mean):
        _lib.require_gpu(x)
        pooled, _ = pool_head_fwd(_f32c(x), graph, mean)
        ctx.graph, ctx.mean, ctx.M = graph, mean, x.size(0)
        return pooled

    @staticmethod
    def backward(ctx, dp):
        return pool_bwd(_f32c(dp), ctx.graph, ctx.mean, ctx.M), None, None


def segment_pool(x, graph: Graph, mean: bool = True):
    if _compiling():
        return torch.ops.lgnn.segment_pool(x, _lgnn().gparts(graph, None), bool(mean))
    return _Pool.apply(x, graph, mean)


class _PoolHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Wout, bout, graph, mean):
        _lib.require_gpu(x, Wout)
        pooled, logits = pool_head_fwd(_f32c(x), graph, mean, _f32c(Wout), _f32c(bout))
        ctx.save_for_backward(pooled, Wout)
        ctx.graph, ctx.mean, ctx.M = graph, mean, x.size(0)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        pooled, Wout = ctx.saved_tensors
        dp, dWo, dbo = pool_head_bwd(_f32c(dlogits), pooled, Wout)
        dx = pool_bwd(dp, ctx.graph, ctx.mean, ctx.M) if ctx.needs_input_grad[0] else None
        return dx, dWo, dbo, None, None


def pool_head(x, Wout, bout, graph: Graph, mean: bool = True):
    if _compiling():
        return torch.ops.lgnn.pool_head(x, Wout, bout, _lgnn().gparts(graph, None),
                                        bool(mean))[0]
    return _PoolHead.apply(x, Wout, bout, graph, mean)


class GcnPlan(NamedTuple):
    fused: bool          # the fused stack forward (stack_fwd_planes): every width on the tiles
    saved_s: tuple       # per conv: the forward saves S_l = Â H_{l-1} (else the backward gathers)
    keeps_planes: bool   # the forward keeps the transposed weight planes: split-3 backward
    fused_bwd: bool      # the fused backward (stack_bwd) when no input gradient is wanted
    kind: str            # the graph build: "gcn_lazy" when only the fused kernels read it


def gcn_plan(shapes: list, L: int, lazy_ok: bool = False) -> GcnPlan:
    """shapes: (N, K) of W_in, W_1..W_L. lazy_ok: the forward builds the graph itself (a Graph,
    not a compiled op's bundle) and no input gradient is wanted."""
    fused = L + 1 <= STACK_MAX and all(fast_shape(K, N) for N, K in shapes)
    saved_s = tuple(fused or fast_shape(K, N) or wide_shape(K, N) for N, K in shapes[1:])
    keeps_planes = fused and MFMA_MODE == "s3" and BWD_S3 and L >= 1
    fused_bwd = fused and FUSED_BWD and (1 <= L <= 2 or keeps_planes)
    # only the fused kernels read this build: its transpose CSR is built only if a tile is open
    kind = "gcn_lazy" if LAZY_TRANSPOSE and lazy_ok and fused_bwd else "gcn"
    return GcnPlan(fused, saved_s, keeps_planes, fused_bwd, kind)


# hs = [H_0..H_L]; ss = [S_1..S_L] (H_{l-1} itself where plan.saved_s[l] is False); params =
# [W_in, b_in, (W_l, b_l) * L, W_out, b_out]; planes_t (plan.keeps_planes, else None): the
# transposed weight planes (+ Â^T room); adjt: the forward's Â^T tiles when they have a buffer
# of their own, else None; h0_valid: hs[0] holds every row (False: the folded forward left its
# closed tiles' rows unwritten, for the deferred backward)
GcnSaved = namedtuple("GcnSaved", "x pooled hs ss params planes_t adjt graph mean L plan h0_valid",
                      defaults=(True,))


def _bwd_defers(plan: GcnPlan, L: int, want_dx: bool) -> bool:
    """The backward gcn_stack_bwd will run is the deferred fused one."""
    return plan.fused_bwd and not want_dx and _defers_fold(L, plan.keeps_planes)


def gcn_stack_fwd(x, graph, mean, L, params, want_dx: bool, adjt_after_planes: bool = False):
    """(logits, GcnSaved). adjt_after_planes: see stack_fwd_planes."""
    _lib.require_gpu(x, *params)
    x = _f32c(x)
    params = [_f32c(p) for p in params]
    W_in, b_in = params[0], params[1]
    Ws = [params[2 * l] for l in range(L + 1)]
    plan = gcn_plan([tuple(W.shape) for W in Ws], L,
                    lazy_ok=isinstance(graph, Graph) and not want_dx)
    planes_t = adjt = None
    h0_valid = True
    if plan.fused:  # builds the graph itself (with the weight-plane split riding along)
        fold = FWD_FOLD and MFMA_MODE == "s3" and 1 <= L <= 2
        # H_0's closed rows are dropped only when the backward that follows never reads them
        h0_valid = not (fold and _bwd_defers(plan, L, want_dx))
        hs, ss, planes_t, adjt = stack_fwd_planes(
            x, graph, Ws, [params[2 * l + 1] for l in range(L + 1)], plan.kind,
            plan.keeps_planes, adjt_after_planes, fold=fold, keep_h0=h0_valid)
    else:
        csr = graph.csr(plan.kind)
        hs = [linear_fwd(x, W_in, b_in, _lib.LGNN_ACT_NONE)]
        ss = []  # aggregated conv inputs S_l = A_hat H_{l-1} (saved on the fast path)
        for l in range(L):
            W, b = params[2 + 2 * l], params[3 + 2 * l]
            if plan.saved_s[l]:
                h, s_ = linear_fwd(hs[-1], W, b, _lib.LGNN_ACT_ELU, csr, save_s=True)
            else:
                h, s_ = linear_fwd(hs[-1], W, b, _lib.LGNN_ACT_ELU, csr), hs[-1]
            hs.append(h)
            ss.append(s_)
    W_out, b_out = params[2 + 2 * L], params[3 + 2 * L]
    pooled, logits = pool_head_fwd(hs[-1], graph, mean, W_out, b_out)
    return logits, GcnSaved(x, pooled, hs, ss, params, planes_t, adjt, graph, mean, L, plan,
                            h0_valid)


def gcn_fused_head(sv: GcnSaved, want_dx: bool) -> bool:
    """True when the backward forms dP = dlogits W_out inside the single split-3 launch."""
    return (sv.plan.fused_bwd and not want_dx and
            head_in_stack_bwd(sv.graph, sv.L, sv.params[2 + 2 * sv.L].size(0),
                              sv.planes_t is not None))


def gcn_stack_bwd(sv: GcnSaved, dlogits, want_dx: bool, ce=None):
    """(dx or None, [param gradients]). ce = (CeSrc, logits): the logits gradient is CE's,
    formed where it is consumed (the fused backward's prologue, the out_proj reduction jobs) —
    dlogits is None then."""
    L, x, pooled, hs, ss, params, graph = sv.L, sv.x, sv.pooled, sv.hs, sv.ss, sv.params, sv.graph
    kind = sv.plan.kind
    csr = graph.csr(kind)
    W_out = params[2 + 2 * L]
    dlogits = _f32c(dlogits) if dlogits is not None else None
    grads = [None] * len(params)
    red: list = []
    if not sv.h0_valid and not _bwd_defers(sv.plan, L, want_dx):
        # the switches changed since the forward: this backward reads H_0, which the folded
        # forward did not write for the closed tiles
        hs = [linear_fwd(x, params[0], params[1], _lib.LGNN_ACT_NONE)] + list(hs[1:])
    if sv.plan.fused_bwd and not want_dx:
        Ws = [params[2 * l] for l in range(L + 1)]
        if head_in_stack_bwd(graph, L, W_out.size(0), sv.planes_t is not None):
            # dP is formed inside the stack kernel; out_proj's gradients (dlogits^T pooled,
            # column sums of dlogits) join the stack's slab reductions: no head launch
            C, D = W_out.shape
            B = pooled.size(0)
            dWo = torch.empty_like(W_out)
            dbo = torch.empty(C, dtype=torch.float32, device=x.device)
            part = CE_PART if ce is not None else dlogits
            red += [(part, B, C * D, dWo, pooled, D), (part, B, C, dbo)]
            outs, after = stack_bwd(None, x, graph, sv.mean, Ws, hs, ss, red, sv.planes_t,
                                    head=(ce[0] if ce is not None else dlogits, W_out),
                                    kind=kind, adjt_t=sv.adjt, b0=params[1])
        else:
            dp, dWo, dbo = pool_head_bwd(dlogits, pooled, W_out)
            outs, after = stack_bwd(dp, x, graph, sv.mean, Ws, hs, ss, red, sv.planes_t,
                                    kind=kind, adjt_t=sv.adjt, b0=params[1])
        grads[2 + 2 * L], grads[3 + 2 * L] = dWo, dbo
        for l, (dW, db) in enumerate(outs):
            grads[2 * l], grads[2 * l + 1] = dW, db
        reduce_multi(red, x.device, ce=ce[0] if ce is not None else None,
                     num_classes=W_out.size(0))
        if after is not None:  # the deferred fold, on the reduced sums
            after()
        return None, grads
    assert ce is None, "the CE-formed logits gradient only on the fused head path"
    dp, dWo, dbo = pool_head_bwd(dlogits, pooled, W_out)
    grads[2 + 2 * L], grads[3 + 2 * L] = dWo, dbo
    if sv.plan.fused:  # the fused forward's S_l are not read here: S_l = Â H_{l-1} again
        ss = [spmm_raw(csr.rowptr, csr.col, csr.w, 0.0, hs[l]) for l in range(L)]
    dS = None
    for l in reversed(range(L)):
        W = params[2 + 2 * l]
        if l == L - 1:
            mode, dY, tc = _lib.LGNN_GRAD_POOL, dp, None
        else:
            mode, dY, tc = _lib.LGNN_GRAD_TRANSPOSE, dS, csr
        saved_s = sv.plan.saved_s[l]
        dS, dW, db = linear_bwd(mode, dY, H=hs[l + 1], act=_lib.LGNN_ACT_ELU,
                                X=ss[l] if saved_s else hs[l], W=W,
                                csr=None if saved_s else csr, graph=graph,
                                pool_mean=sv.mean, tcsr=tc, reducer=red)
        grads[2 + 2 * l], grads[3 + 2 * l] = dW, db
    # in_proj: dH0 = A^T dS_1 (transposed aggregation in the prologue); dx = dH0 W_in
    if L > 0:
        mode, dY, tc = _lib.LGNN_GRAD_TRANSPOSE, dS, csr
    else:
        mode, dY, tc = _lib.LGNN_GRAD_POOL, dp, None
    dx, dW, db = linear_bwd(mode, dY, H=None, act=_lib.LGNN_ACT_NONE, X=x, W=params[0],
                            graph=graph, pool_mean=sv.mean, tcsr=tc, want_dx=want_dx,
                            reducer=red)
    reduce_multi(red, x.device)
    grads[0], grads[1] = dW, db
    return dx, grads


class _GCNStack(torch.autograd.Function):
    """in_proj -> L x ELU(GCNConv) -> pool -> out_proj as one autograd node (dropout p = 0 or
    eval). params = [W_in, b_in, (W_l, b_l) * L, W_out, b_out]."""

    @staticmethod
    def forward(ctx, x, graph, mean, L, *params):
        logits, saved = gcn_stack_fwd(x, graph, mean, L, params, ctx.needs_input_grad[0])
        _save(ctx, saved)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        dx, grads = gcn_stack_bwd(_load(ctx), dlogits, ctx.needs_input_grad[0])
        return (dx, None, None, None, *grads)


# stack: GcnSaved; z: logits; yy: int64 targets; out: (loss, sum of weights); w: class weights or
# None; pm, wt: the logits gradient's factors (lgnn_ce_fwd_factors)
CeSaved = namedtuple("CeSaved", "stack z yy lse out w pm wt")


class _GCNStackCE(torch.autograd.Function):
    """The GCN model and its criterion nn.CrossEntropyLoss(weight) (mean reduction, reference
    models/base.py:93-94, training_step :196-201) as ONE autograd node: outputs (logits, loss).
    Forward: _GCNStack's launches + lgnn_ce_fwd. Backward with only the loss differentiated (the
    training step): the logits gradient is never materialised — the fused split-3 backward forms
    it per graph in its prologue and the out_proj reduction jobs form it per (graph, class), both
    with lgnn_ce_bwd's expression (no lgnn_ce_bwd launch, bitwise the same gradients). Anything
    else (logits also differentiated, shapes off the fused head path) forms dlogits with
    lgnn_ce_bwd and takes _GCNStack's backward."""

    @staticmethod
    def forward(ctx, x, graph, mean, L, y, weight, *params):
        ctx.set_materialize_grads(False)
        yy = y.to(torch.int64).contiguous()
        w = _f32c(weight) if weight is not None else None
        z, stack = gcn_stack_fwd(x, graph, mean, L, params, ctx.needs_input_grad[0])
        # one single-workgroup launch: loss, lse and the gradient's factors pm / wt
        B, C = z.shape
        dev = z.device
        lse = torch.empty(B, dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)  # loss, sum of weights
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        pm = torch.empty(B, C, dtype=torch.float32, device=dev)
        wt = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.call("lgnn_ce_fwd_factors", z, yy, w, B, C, lse, out, out[1:], bad, pm, wt, _s(dev))
        _save(ctx, CeSaved(stack, z, yy, lse, out, w, pm, wt))
        return z, out[0]

    @staticmethod
    def backward(ctx, dlogits, dloss):
        sv = _load(ctx)
        want_dx = ctx.needs_input_grad[0]

        def grads(r):  # gcn_stack_bwd's (dx, param grads) -> this node's inputs
            return (r[0], None, None, None, None, None, *r[1])

        if dloss is None:
            if dlogits is None:
                return (None,) * (6 + len(sv.stack.params))
            return grads(gcn_stack_bwd(sv.stack, dlogits, want_dx))
        g = _f32c(dloss.reshape(1))
        if dlogits is None and gcn_fused_head(sv.stack, want_dx):
            src = _lib.CeSrc(sv.pm.data_ptr(), sv.wt.data_ptr(), sv.out.data_ptr() + 4,
                             g.data_ptr())
            return grads(gcn_stack_bwd(sv.stack, None, want_dx, ce=(src, sv.z)))
        B, C = sv.z.shape
        dz = torch.empty_like(sv.z)
        _lib.call("lgnn_ce_bwd", sv.z, sv.yy, sv.w, B, C, sv.lse, sv.out[1:], g, dz,
                  _s(sv.z.device))
        if dlogits is not None:
            dz = dz + dlogits
        return grads(gcn_stack_bwd(sv.stack, dz, want_dx))


def gcn_stack_ce(x, graph: Graph, params: list[torch.Tensor], L: int, y: torch.Tensor,
                 weight: torch.Tensor | None = None, mean: bool = True):
    """(logits, loss): the GCN stack and its cross-entropy criterion in one node (_GCNStackCE)."""
    return _GCNStackCE.apply(x, graph, mean, L, y, weight, *params)


def gcn_stack(x, graph: Graph, params: list[torch.Tensor], L: int, mean: bool = True):
    if _compiling():
        return torch.ops.lgnn.gcn_stack(x, _lgnn().gparts(graph, "gcn"), bool(mean), int(L),
                                        list(params))[0]
    return _GCNStack.apply(x, graph, mean, L, *params)


# ----------------------------------------------------------------------------------------------
# BatchNorm1d + ELU (GIN MLP) and the fused GINConv
# ----------------------------------------------------------------------------------------------


def _bn_ws(M: int, N: int, dev) -> torch.Tensor:
    return torch.empty(_lib.load().lgnn_bn_workspace_bytes(M, N), dtype=torch.uint8, device=dev)


def bn_stats(Z: torch.Tensor) -> torch.Tensor:
    """fp64 [2N]: (sum z, sum z^2) over rows."""
    M, N = Z.shape
    sums = torch.empty(2 * N, dtype=torch.float64, device=Z.device)
    ws = _bn_ws(M, N, Z.device)
    _lib.call("lgnn_bn_stats", Z, M, N, sums, ws, ws.numel(), _s(Z.device))
    return sums


def bn_finalize(sums, count: float, bn: torch.nn.BatchNorm1d, training: bool, N: int, dev,
                part: tuple | None = None):
    """The BN constants (+ running-stat update). part = (partial rows, P): sums are first reduced
    from the BN-fused kernels' partial rows into `sums`, in the same launch (training only)."""
    f = dict(dtype=torch.float32, device=dev)
    mean, invstd, scale, shift = (torch.empty(N, **f) for _ in range(4))
    track = bn.track_running_stats and bn.running_mean is not None
    rm = bn.running_mean if track else None
    rv = bn.running_var if track else None
    nbt = bn.num_batches_tracked if (track and training) else None
    momentum = bn.momentum if bn.momentum is not None else 0.1
    if nbt is not None and bn.momentum is None:  # cumulative moving average (torch semantics)
        momentum = 1.0 / float(bn.num_batches_tracked.item() + 1)
    gamma, beta = (bn.weight, bn.bias) if bn.affine else (None, None)
    if part is not None:
        _lib.call("lgnn_bn_partials_finalize", part[0], part[1], N, sums, float(count), gamma,
                  beta, float(bn.eps), float(momentum), rm, rv, nbt, mean, invstd, scale, shift,
                  _s(dev))
        return mean, invstd, scale, shift
    _lib.call("lgnn_bn_finalize", sums, float(count), gamma, beta, float(bn.eps),
              float(momentum), int(training), N, rm, rv, nbt, mean, invstd, scale, shift, _s(dev))
    return mean, invstd, scale, shift


def bn_act(Z, scale, shift, mask=None) -> torch.Tensor:
    M, N = Z.shape
    A = torch.empty_like(Z)
    _lib.call("lgnn_bn_act", Z, M, N, scale, shift, mask, A, _s(Z.device))
    return A


def bn_bwd_stats(dA, Z, mask, scale, shift, mean, invstd) -> torch.Tensor:
    M, N = Z.shape
    sums = torch.empty(2 * N, dtype=torch.float64, device=Z.device)
    ws = _bn_ws(M, N, Z.device)
    _lib.call("lgnn_bn_bwd_stats", dA, Z, mask, M, N, scale, shift, mean, invstd, sums, ws,
              ws.numel(), _s(Z.device))
    return sums


def bn_bwd_apply(dA, Z, mask, scale, shift, mean, invstd, sums, count, training, local_sums,
                 want_param_grads: bool):
    M, N = Z.shape
    dev = Z.device
    dZ = torch.empty_like(Z)
    _lib.call("lgnn_bn_bwd_apply", dA, Z, mask, M, N, scale, shift, mean, invstd, sums,
              float(count), int(training), dZ, None, None, _s(dev))
    dg = db = None
    if want_param_grads:
        dg = torch.empty(N, dtype=torch.float32, device=dev)
        db = torch.empty(N, dtype=torch.float32, device=dev)
        _lib.call("lgnn_bn_bwd_apply", None, None, None, 0, N, scale, shift, mean, invstd,
                  local_sums, 1.0, 0, None, dg, db, _s(dev))
    return dZ, dg, db


# GIN: BatchNorm folded into the MLP's two linear launches (BN_FUSED = False: the separate
# lgnn_bn_* passes)
BN_FUSED = True



def gin_bn_fused(K: int, N1: int, N2: int) -> bool:
    """True when _GINConv runs its BatchNorm inside the linear kernels (fast-path shapes)."""
    return BN_FUSED and fast_shape(K, N1) and fast_shape(N1, N2)


def _global_count(M: int, group, dev, fixed=None) -> float:
    if group is None:
        return float(M)
    if fixed is not None:
        return float(fixed)
    import torch.distributed as dist

    t = torch.tensor([float(M)], dtype=torch.float64, device=dev)
    dist.all_reduce(t, group=group)
    return float(t.item())


class GinPlan(NamedTuple):
    bn_fused: bool  # BatchNorm inside the two linear launches (fast-path shapes)
    gathered: bool  # generic kernels: no S saved, the backward gathers x again


def gin_plan(K: int, N1: int, N2: int) -> GinPlan:
    bn_fused = gin_bn_fused(K, N1, N2)
    return GinPlan(bn_fused, not (bn_fused or fast_shape(K, N1) or wide_shape(K, N1)))


# S = (1 + eps) x + A x, or x itself when plan.gathered; mask: dropout mask or None
GinSaved = namedtuple("GinSaved", "S Z1 A1 H W1 W2 mean invstd scale shift mask graph self_scale "
                                  "training count group act affine plan")


def gin_conv_fwd(x, W1, b1, W2, b2, graph, bn, training, eps, mask, act, group=None,
                 sync_count=None):
    """One GINConv(MLP([d1,d2,d2], act=ELU, norm=batch_norm)) with the model's F.elu fused:
        S  = (1 + eps) x_i + sum_{j->i} x_j      (eps = 0 buffer; edges as given, KNN loops kept)
        Z1 = S W1^T + b1;  A1 = ELU(BN(Z1)) [* dropout mask];  H = act(A1 W2^T + b2)
    Reference: gin.py:23 (GINConv(MLP(...))), gin.py:31 (F.elu). BN per `bn` (training uses batch
    statistics; SyncBN over `group` when given). Returns (H, the batch statistics' fp64 sums or
    None in eval, GinSaved)."""
    _lib.require_gpu(x, W1, W2)
    x, W1, b1, W2, b2 = (_f32c(t) for t in (x, W1, b1, W2, b2))
    csr = graph.csr("gin")
    self_scale = 1.0 + float(eps)
    M, N1 = x.size(0), W1.size(0)
    dev = x.device
    plan = gin_plan(W1.size(1), N1, W2.size(0))
    count = float(M)
    sums = None
    if plan.bn_fused and training:
        # BatchNorm folded into the two linear launches (lgnn_node_linear_fwd_bn): the BN
        # statistics in the first one's epilogue, BN + ELU (+ mask) in the second one's prologue.
        # Same arithmetic as the unfused sequence except the fixed order of the fp64 sums.
        P = _lib.load().lgnn_bn_fused_partials(M)
        Z1 = torch.empty(M, N1, dtype=torch.float32, device=dev)
        S = torch.empty_like(x)
        part = torch.empty(P * 2 * N1, dtype=torch.float64, device=dev)
        _lib.call("lgnn_node_linear_fwd_bn", x, M, x.size(1), csr.rowptr, csr.col, csr.w,
                  float(self_scale), W1, b1, N1, _lib.LGNN_ACT_NONE, Z1, S, part, None, None,
                  None, None, _s(dev))
        sums = torch.empty(2 * N1, dtype=torch.float64, device=dev)
        count = _global_count(M, group, dev, sync_count)
        if count <= 1:
            raise ValueError("Expected more than 1 value per channel when training")
        if group is None:  # sums + the BN constants in one launch
            mean, invstd, scale, shift = bn_finalize(sums, count, bn, training, N1, dev,
                                                     part=(part, P))
        else:
            from .dist import sync_all_reduce

            _lib.call("lgnn_bn_partials_reduce", part, P, N1, sums, None, None, _s(dev))
            sync_all_reduce(sums, group)
            mean, invstd, scale, shift = bn_finalize(sums, count, bn, training, N1, dev)
    else:
        if plan.gathered:
            Z1, S = linear_fwd(x, W1, b1, _lib.LGNN_ACT_NONE, csr, self_scale), x
        else:
            Z1, S = linear_fwd(x, W1, b1, _lib.LGNN_ACT_NONE, csr, self_scale, save_s=True)
        if training:
            sums = bn_stats(Z1)
            count = _global_count(M, group, dev, sync_count)
            if count <= 1:
                raise ValueError("Expected more than 1 value per channel when training")
            if group is not None:
                from .dist import sync_all_reduce

                sync_all_reduce(sums, group)
        mean, invstd, scale, shift = bn_finalize(sums, count, bn, training, N1, dev)
    if plan.bn_fused:
        A1 = torch.empty_like(Z1)
        N2 = W2.size(0)
        H = torch.empty(M, N2, dtype=torch.float32, device=dev)
        _lib.call("lgnn_node_linear_fwd_bn", Z1, M, N1, None, None, None, 0.0, W2, b2, N2, act,
                  H, None, None, scale, shift, mask, A1, _s(dev))
    else:
        A1 = bn_act(Z1, scale, shift, mask)
        H = linear_fwd(A1, W2, b2, act)
    return H, sums, GinSaved(S, Z1, A1, H, W1, W2, mean, invstd, scale, shift, mask, graph,
                             self_scale, training, count, group, act, bn.affine, plan)


def gin_conv_bwd(sv: GinSaved, dH, want_dx: bool, pool: tuple | None = None,
                 gather: tuple | None = None, defer_dx: bool = False,
                 extra_red: list | None = None):
    """(dx, dW1, db1, dgamma, dbeta, dW2, db2). On the BN-fused path only:
    pool = (dlogits, W_out, graph, mean): the output gradient comes from the pooled readout
    (global pool + out_proj backward folded into Lin2's backward load; dH is None).
    gather = (dS, tself): the output gradient is the next conv's aggregation backward,
    tself dS + A^T dS, gathered as Lin2's backward loads it (dH is None). defer_dx: return
    this conv's pre-aggregation input gradient (for the previous layer to gather) instead
    of aggregating it here. extra_red: more slab / outer-product jobs for this conv's
    reduction launch."""
    S, Z1, A1, H, W1, W2, mask = sv.S, sv.Z1, sv.A1, sv.H, sv.W1, sv.W2, sv.mask
    mean, invstd, scale, shift = sv.mean, sv.invstd, sv.scale, sv.shift
    csr = sv.graph.csr("gin")
    if not sv.plan.bn_fused:
        assert pool is None and gather is None and not defer_dx and not extra_red
        dA1, dW2, db2 = linear_bwd(_lib.LGNN_GRAD_DIRECT, _f32c(dH), H=H, act=sv.act, X=A1, W=W2)
        local = bn_bwd_stats(dA1, Z1, mask, scale, shift, mean, invstd)
        sums = local
        if sv.training and sv.group is not None:
            from .dist import sync_all_reduce

            sums = local.clone()
            sync_all_reduce(sums, sv.group)
        dZ1, dg, dbt = bn_bwd_apply(dA1, Z1, mask, scale, shift, mean, invstd, sums, sv.count,
                                    sv.training, local, sv.affine)
        dxpre, dW1, db1 = linear_bwd(_lib.LGNN_GRAD_DIRECT, dZ1, H=None, act=_lib.LGNN_ACT_NONE,
                                     X=S, W=W1, csr=csr if sv.plan.gathered else None,
                                     self_scale=sv.self_scale if sv.plan.gathered else 0.0,
                                     want_dx=want_dx)
        dx = spmm_raw(csr.tptr, csr.tidx, csr.tw, sv.self_scale, dxpre) if want_dx else None
        return dx, dW1, db1, dg, dbt, dW2, db2
    M, N1 = Z1.shape
    N2 = W2.size(0)
    K = S.size(1)
    dev = Z1.device
    P = _lib.load().lgnn_bn_fused_partials(M)
    red: list = []
    fname = "lgnn_node_linear_bwd_bn"
    # Lin2 backward; its dX (= dA1) epilogue also sums the BN backward's (g, g xhat)
    dA1 = torch.empty_like(Z1)
    slab2 = torch.empty(P * (N2 * N1 + N2), dtype=torch.float32, device=dev)
    gpart = torch.empty(P * 2 * N1, dtype=torch.float64, device=dev)
    # from the layer's input A1 to the BN gradient partials: the same in all three entries
    lin2 = (A1, M, N1, W2, N2, dA1, slab2, slab2[P * N2 * N1:], P, Z1, mask, scale, shift, mean,
            invstd, gpart)
    if gather is not None:
        dS, tself = gather
        _lib.call("lgnn_node_linear_bwd_bn_gather", dS, csr.tptr, csr.tidx, csr.tw, float(tself),
                  H, sv.act, *lin2, _s(dev))
    elif pool is not None:
        dlog, W_out, pg, pmean = pool
        _lib.call("lgnn_node_linear_bwd_bn_pool", _lib.LGNN_BN_GSTATS, None, H, sv.act, *lin2,
                  None, 0.0, int(sv.training), pg.batch, pg.gptr, int(pmean), dlog, W_out,
                  W_out.size(0), _s(dev))
    else:
        _lib.call(fname, _lib.LGNN_BN_GSTATS, _f32c(dH), H, sv.act, *lin2, None, 0.0,
                  int(sv.training), _s(dev))
    dW2 = torch.empty(N2, N1, dtype=torch.float32, device=dev)
    db2 = torch.empty(N2, dtype=torch.float32, device=dev)
    red += [(slab2[:P * N2 * N1], P, N2 * N1, dW2), (slab2[P * N2 * N1:], P, N2, db2)]
    local = torch.empty(2 * N1, dtype=torch.float64, device=dev)
    dg = dbt = None
    if sv.affine:  # the affine gradients come out of the same launch (local sums)
        dg = torch.empty(N1, dtype=torch.float32, device=dev)
        dbt = torch.empty(N1, dtype=torch.float32, device=dev)
    _lib.call("lgnn_bn_partials_reduce", gpart, P, N1, local, dg, dbt, _s(dev))
    sums = local
    if sv.training and sv.group is not None:
        from .dist import sync_all_reduce

        sums = local.clone()
        sync_all_reduce(sums, sv.group)
    # Lin1 backward with the BN backward applied to dA1 as it is loaded
    dxpre = torch.empty(M, K, dtype=torch.float32, device=dev) if want_dx else None
    slab1 = torch.empty(P * (N1 * K + N1), dtype=torch.float32, device=dev)
    _lib.call(fname, _lib.LGNN_BN_GIN, dA1, None, _lib.LGNN_ACT_NONE, S, M, K, W1, N1, dxpre,
              slab1, slab1[P * N1 * K:], P, Z1, mask, scale, shift, mean, invstd, None, sums,
              float(sv.count), int(sv.training), _s(dev))
    dW1 = torch.empty(N1, K, dtype=torch.float32, device=dev)
    db1 = torch.empty(N1, dtype=torch.float32, device=dev)
    red += [(slab1[:P * N1 * K], P, N1 * K, dW1), (slab1[P * N1 * K:], P, N1, db1)]
    if extra_red:  # e.g. out_proj's dW / db as outer-product jobs (no k_head_bwd launch)
        red += extra_red
    reduce_multi(red, dev)
    dx = None
    if want_dx:
        dx = dxpre if defer_dx else spmm_raw(csr.tptr, csr.tidx, csr.tw, sv.self_scale,
                                             dxpre)
    return dx, dW1, db1, dg, dbt, dW2, db2


class _GINConv(torch.autograd.Function):
    """gin_conv_fwd / gin_conv_bwd as an autograd node; gamma / beta are bn's affine parameters
    (inputs so that they receive gradients)."""

    @staticmethod
    def forward(ctx, x, W1, b1, gamma, beta, W2, b2, graph, bn, training, eps, mask, act, group,
                sync_count):
        H, _, saved = gin_conv_fwd(x, W1, b1, W2, b2, graph, bn, training, eps, mask, act, group,
                                   sync_count)
        _save(ctx, saved)
        return H

    @staticmethod
    def backward(ctx, dH):
        return (*gin_conv_bwd(_load(ctx), dH, ctx.needs_input_grad[0]),) + (None,) * 8


# a model's last conv (conv: GinSaved or GatSaved) with its readout, global pool + out_proj
HeadSaved = namedtuple("HeadSaved", "conv pooled W_out mean")


def _head_grads(sv, dlogits, jobs: bool):
    """out_proj's (dW, db) buffers and either the outer-product jobs that fill them in a
    layer's slab reduction (no k_head_bwd launch) or, with jobs False, lgnn_pool_head_bwd."""
    pooled, W_out = sv.pooled, sv.W_out
    B, D = pooled.shape
    C = W_out.size(0)
    dev = pooled.device
    dWo = torch.empty(C, D, dtype=torch.float32, device=dev)
    dbo = torch.empty(C, dtype=torch.float32, device=dev)
    if jobs:
        return dWo, dbo, [(dlogits, B, C * D, dWo, pooled, D), (dlogits, B, C, dbo)]
    _lib.call("lgnn_pool_head_bwd", dlogits, pooled, B, D, W_out, C, None, dWo, dbo, _s(dev))
    return dWo, dbo, None


class _GINConvHead(torch.autograd.Function):
    """The GIN model's last conv + global pool + out_proj as one autograd node (BN-fused fp32
    path): its backward forms each row's output gradient from dlogits (out_proj backward + pool
    backward folded into Lin2's backward load, lgnn_node_linear_bwd_bn_pool) instead of
    materialising dH; out_proj's dW / db come from lgnn_pool_head_bwd (same arithmetic as the
    unfused chain)."""

    @staticmethod
    def forward(ctx, x, W1, b1, gamma, beta, W2, b2, W_out, b_out, graph, bn, training, eps,
                mask, act, group, sync_count, mean):
        _lib.require_gpu(W_out)
        W_out, b_out = _f32c(W_out), _f32c(b_out)
        H, _, conv = gin_conv_fwd(x, W1, b1, W2, b2, graph, bn, training, eps, mask, act, group,
                                  sync_count)
        pooled, logits = pool_head_fwd(H, graph, mean, W_out, b_out)
        _save(ctx, HeadSaved(conv, pooled, W_out, mean))
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        sv = _load(ctx)
        dlogits = _f32c(dlogits)
        dWo, dbo, _ = _head_grads(sv, dlogits, jobs=False)
        g = gin_conv_bwd(sv.conv, None, ctx.needs_input_grad[0],
                         pool=(dlogits, sv.W_out, sv.conv.graph, sv.mean))
        return (*g, dWo, dbo) + (None,) * 9


# out_proj's dW / db as outer-product jobs of a layer's slab reduction (GIN / GAT model nodes);
# HEAD_JOBS = False: the separate lgnn_pool_head_bwd launch
HEAD_JOBS = True


# convs: GinSaved of every conv but the last; head: HeadSaved of the last
GinStackSaved = namedtuple("GinStackSaved", "x W_in convs head")


class _GINStack(torch.autograd.Function):
    """The whole GIN model (in_proj + every GINConv + global pool + out_proj, reference
    gin.py:17-35) as one autograd node on the BN-fused fp32 kernels. Same kernels as the
    per-conv nodes, except the backward of each conv's aggregation: instead of a transpose-CSR
    pass over its input gradient (spmm), the previous layer's backward gathers that gradient as
    it loads it (lgnn_node_linear_bwd_bn_gather for a conv's Lin2, lgnn_node_linear_bwd in
    LGNN_GRAD_TRANSPOSE mode for in_proj), so no aggregated gradient goes through HBM."""

    @staticmethod
    def forward(ctx, x, graph, mean, specs, W_in, b_in, W_out, b_out, *flat):
        _lib.require_gpu(x, W_in, W_out)
        x, W_in, b_in, W_out, b_out = (_f32c(t) for t in (x, W_in, b_in, W_out, b_out))
        graph.csr("gin")  # the graph build before in_proj
        h = linear_fwd(x, W_in, b_in, _lib.LGNN_ACT_NONE)
        convs = []
        for i, sp in enumerate(specs):
            W1, b1, _gamma, _beta, W2, b2 = flat[6 * i:6 * i + 6]
            h, _, conv = gin_conv_fwd(h, W1, b1, W2, b2, graph, sp["bn"], sp["training"],
                                      sp["eps"], sp["mask"], sp["act"], sp["group"],
                                      sp["sync_count"])
            convs.append(conv)
        pooled, logits = pool_head_fwd(h, graph, mean, W_out, b_out)
        _save(ctx, GinStackSaved(x, W_in, convs[:-1], HeadSaved(convs[-1], pooled, W_out, mean)))
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        sv = _load(ctx)
        convs = [*sv.convs, sv.head.conv]
        graph = sv.head.conv.graph
        dlogits = _f32c(dlogits)
        # out_proj's dW = dlogits^T pooled and db = colsum dlogits join the last conv's slab
        # reductions (outer-product jobs): no k_head_bwd launch
        dWo, dbo, head_jobs = _head_grads(sv.head, dlogits, HEAD_JOBS)
        L = len(convs)
        grads = [None] * L
        dS = None
        # each layer's dW / db slabs are summed right after that layer, while they are still in
        # the caches (one launch at the end measured 10 us slower per C4 step)
        for i in range(L - 1, -1, -1):
            if i == L - 1:
                g = gin_conv_bwd(convs[i], None, True, defer_dx=True, extra_red=head_jobs,
                                 pool=(dlogits, sv.head.W_out, graph, sv.head.mean))
            else:
                g = gin_conv_bwd(convs[i], None, True, defer_dx=True,
                                 gather=(dS, convs[i + 1].self_scale))
            dS = g[0]
            grads[i] = g[1:]
        # in_proj: its output gradient is the first conv's aggregation backward, gathered
        dx, dW_in, db_in = linear_bwd(_lib.LGNN_GRAD_TRANSPOSE, dS, H=None, act=_lib.LGNN_ACT_NONE,
                                      X=sv.x, W=sv.W_in, tcsr=graph.csr("gin"),
                                      tself=convs[0].self_scale,
                                      want_dx=ctx.needs_input_grad[0])
        flat = [t for g in grads for t in g]
        return (dx, None, None, None, dW_in, db_in, dWo, dbo, *flat)


def gin_stack_eligible(x, W_in, convs_W) -> bool:
    """Whether the GIN model runs as one _GINStack node (eager, BN-fused fp32 kernels, every
    layer on the fast-path shapes)."""
    return (not _compiling() and fast_shape(x.size(1), W_in.size(0)) and
            all(gin_bn_fused(W1.size(1), W1.size(0), W2.size(0)) for W1, W2 in convs_W))


def gin_stack(x, W_in, b_in, convs: list, W_out, b_out, graph: Graph, mean: bool):
    """convs: per GINConv a dict (W1, b1, bn, W2, b2, eps, mask, act, group, sync_count)."""
    specs, flat = [], []
    for c in convs:
        bn = c["bn"]
        training = bn.training or not bn.track_running_stats
        specs.append(dict(bn=bn, training=training, eps=c["eps"], mask=c["mask"], act=c["act"],
                          group=c["group"], sync_count=c["sync_count"]))
        flat += [c["W1"], c["b1"], bn.weight if bn.affine else None,
                 bn.bias if bn.affine else None, c["W2"], c["b2"]]
    return _GINStack.apply(x, graph, mean, specs, W_in, b_in, W_out, b_out, *flat)


def gin_conv_head_eligible(x, W1, W2) -> bool:
    """Whether gin_conv_head runs fused (eager, BN-fused fp32 kernels, fast-path shapes)."""
    return (not _compiling() and
            gin_bn_fused(x.size(1), W1.size(0), W2.size(0)))


def gin_conv_head(x, W1, b1, bn, W2, b2, W_out, b_out, graph: Graph, eps: float = 0.0,
                  mask=None, act: int = _lib.LGNN_ACT_ELU, group=None, sync_count=None,
                  mean: bool = True):
    """gin_conv followed by pool_head (the GIN model's last conv and readout) as one node."""
    training = bn.training or not bn.track_running_stats
    gamma = bn.weight if bn.affine else None
    beta = bn.bias if bn.affine else None
    return _GINConvHead.apply(x, W1, b1, gamma, beta, W2, b2, W_out, b_out, graph, bn, training,
                              eps, mask, act, group, sync_count, mean)


def gin_conv(x, W1, b1, bn, W2, b2, graph: Graph, eps: float = 0.0, mask=None,
             act: int = _lib.LGNN_ACT_ELU, group=None, sync_count=None):
    """bn: the torch.nn.BatchNorm1d holding gamma/beta and the running statistics."""
    training = bn.training or not bn.track_running_stats
    gamma = bn.weight if bn.affine else None
    beta = bn.bias if bn.affine else None
    if _compiling():
        if group is not None:
            raise NotImplementedError("SyncBatchNorm (GIN.set_sync_bn) is not supported under "
                                      "torch.compile")
        track = bn.track_running_stats and bn.running_mean is not None
        out = torch.ops.lgnn.gin_conv(x, W1, b1, gamma, beta, W2, b2,
                                      bn.running_mean if track else None,
                                      bn.running_var if track else None,
                                      _lgnn().gparts(graph, "gin"), bool(training), float(eps),
                                      float(bn.eps), mask, int(act))
        if training and track:
            torch.ops.lgnn.bn_running_update(
                bn.running_mean, bn.running_var, bn.num_batches_tracked, out[8], x.size(0),
                float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum))
        return out[0]
    return _GINConv.apply(x, W1, b1, gamma, beta, W2, b2, graph, bn, training, eps, mask, act,
                          group, sync_count)


# ----------------------------------------------------------------------------------------------
# GATConv
# ----------------------------------------------------------------------------------------------


class GatPlan(NamedTuple):
    dense: bool   # lin on the dense MFMA GEMMs (split-3, or bf16-rounded) instead of the tiles
    mfma: bool    # bf16 mode on the hand-written bf16 MFMA GEMMs (bflin.hip)
    scored: bool  # the attention scores come out of the lin GEMM's epilogue (no lgnn_gat_att)


def gat_plan(K: int, HC: int, bf16: bool) -> GatPlan:
    # fp32: the lin on the split-3 MFMA GEMMs (s3gemm.hip) at every width — they beat the
    # fp32-MFMA tile kernels (2.7x the MFMA rate at fp32 accuracy); GAT_S3 = False: tiles
    dense = bool(bf16) or not fast_shape(K, HC) or GAT_S3
    mfma = bool(bf16) and bf16_mfma_fits(HC)
    scored = GAT_GEMM_ATT and (64 < K <= 128 if mfma else dense and not bf16 and HC <= 128)
    return GatPlan(dense, mfma, scored)


# x: fp32, or the bf16 copy its producer wrote (mfma); att_src / att_dst flat [H * C]; wt: bf16
# W^T from the forward's weight prep (mfma) or None; wpt: W^T's split-3 planes for dx
# (s3_weight_bundle) or None
GatSaved = namedtuple("GatSaved", "x W att_src att_dst XP a_s a_d alpha Y mask wt wpt graph heads "
                                  "slope act bf16 has_bias plan")


def gat_conv_fwd(x, W, att_src, att_dst, bias, graph, heads, slope, mask, act, bf16=False,
                 wp=None, wpt=None):
    """PyG 2.5.1 GATConv (reference gat.py:31) + the model's F.elu (gat.py:51):
        XP = x W^T (lin, no bias) viewed [M, H, C];  a_s = <XP, att_src>, a_d = <XP, att_dst>
        alpha = softmax_dst(leaky_relu(a_s[j] + a_d[i]));  out_i = sum_j alpha_ij mask_ij XP_j
        Y = act(out.view(M, H*C) + bias)
    over remove_self_loops + add_self_loops of edge_index (graph kind "gat").
    Returns (Y, GatSaved)."""
    _lib.require_gpu(x, W, att_src, att_dst)
    x, W = _f32c(x), _f32c(W)
    att_src, att_dst = _f32c(att_src).view(-1), _f32c(att_dst).view(-1)
    bias = _f32c(bias) if bias is not None else None
    csr = graph.csr("gat")
    M = x.size(0)
    HC = W.size(0)
    C = HC // heads
    dev = x.device
    plan = gat_plan(W.size(1), HC, bf16)
    wt = None
    if plan.mfma:  # hand-written bf16 MFMA lin; x rounded in the kernel unless a copy exists
        xb = _bf16_copy_of(x)
        xg, Wg = (xb if xb is not None else x), W
        Wb, wt = bf16_weight_operands(W, True)
    else:  # fp32, or bf16 wider than 128: the operands are split / rounded in the GEMMs
        xg, Wg = x, W
    a_s = torch.empty(M, heads, dtype=torch.float32, device=dev)
    a_d = torch.empty(M, heads, dtype=torch.float32, device=dev)
    if plan.mfma and plan.scored:
        # the attention scores come out of the lin GEMM's epilogue (no lgnn_gat_att pass)
        XP = torch.empty(M, HC, dtype=torch.float32, device=dev)
        xg = xg.contiguous()
        _lib.call("lgnn_bf16_gemm_att", xg, int(xg.dtype == torch.float32), M, xg.size(1), Wb, HC,
                  XP, None, att_src, att_dst, heads, C, a_s, a_d, _s(dev))
    elif plan.mfma:
        XP = bf16_gemm(xg, Wb, None, HC)[0]
    elif plan.scored:
        # split-3 (or one rounded plane) with the attention scores in the GEMM's epilogue
        XP = torch.empty(M, HC, dtype=torch.float32, device=dev)
        xg = xg.contiguous()
        _lib.call("lgnn_s3_gemm_att", xg, M, xg.size(1),
                  wp if wp is not None else dense_planes(Wg, False, False), HC, 3, XP, att_src,
                  att_dst, heads, C, a_s, a_d, _s(dev))
    elif plan.dense:  # split-3 MFMA GEMM (fp32 accuracy), or one rounded plane in bf16 mode
        XP = dense_mm(xg, wp if wp is not None else dense_planes(Wg, False, bf16), HC, None,
                      bf16)
    else:
        XP = linear_fwd(x, W, None, _lib.LGNN_ACT_NONE)
    if not plan.scored:
        _lib.call("lgnn_gat_att", XP, M, heads, C, att_src, att_dst, a_s, a_d, _s(dev))
    cap = csr.col.numel()
    alpha = torch.empty(cap, heads, dtype=torch.float32, device=dev)
    Y = torch.empty(M, HC, dtype=torch.float32, device=dev)
    # bf16 mode: the kernel also writes Y in bf16 for the next layer's GEMM (no cast pass)
    Yb = torch.empty(M, HC, dtype=torch.bfloat16, device=dev) if bf16 and BF16_OUT else None
    _lib.call("lgnn_gat_fwd", csr.rowptr, csr.col, XP, a_s, a_d, M, heads, C, float(slope), mask,
              bias, act, alpha, Y, Yb, _s(dev))
    if Yb is not None:
        _remember_bf16(Y, Yb)
    return Y, GatSaved(xg, Wg, att_src, att_dst, XP, a_s, a_d, alpha, Y, mask, wt, wpt, graph,
                       heads, slope, act, bf16, bias is not None, plan)


def gat_conv_bwd(sv: GatSaved, dY, want_dx: bool, pool: tuple | None = None,
                 extra_red: list | None = None):
    """(dx or None, dW, red): red is the one reduction buffer [datt_src | datt_dst | dbias]
    (att_grads splits it). pool = (dlogits, W_out, graph, mean): the output gradient is formed
    from the readout's gradient inside the edge kernel (lgnn_gat_bwd_edge_pool; dY is None).
    extra_red: more slab / outer-product jobs for this layer's reduction launch."""
    x, W, att_src, att_dst, XP = sv.x, sv.W, sv.att_src, sv.att_dst, sv.XP
    a_s, a_d, alpha, Y, mask = sv.a_s, sv.a_d, sv.alpha, sv.Y, sv.mask
    csr = sv.graph.csr("gat")
    M, HC = Y.shape
    H = sv.heads
    C = HC // H
    dev = Y.device
    dZ = torch.empty_like(Y)
    da_e = torch.empty_like(alpha)
    da_d = torch.empty(M, H, dtype=torch.float32, device=dev)
    if pool is not None:
        dlog, W_out, pg, pmean = pool
        _lib.call("lgnn_gat_bwd_edge_pool", csr.rowptr, csr.col, XP, a_s, a_d, alpha, mask, Y,
                  sv.act, M, H, C, float(sv.slope), pg.batch, pg.gptr, int(pmean), dlog, W_out,
                  W_out.size(0), dZ, da_e, da_d, _s(dev))
    else:
        _lib.call("lgnn_gat_bwd_edge", csr.rowptr, csr.col, XP, a_s, a_d, alpha, mask, _f32c(dY),
                  Y, sv.act, M, H, C, float(sv.slope), dZ, da_e, da_d, _s(dev))
    P = _lib.load().lgnn_gat_bwd_num_partials(M)
    part = torch.empty(P * 3 * HC, dtype=torch.float32, device=dev)
    dXP = torch.empty_like(XP)
    # bf16 MFMA lin: the kernel also writes dXP in bf16 (the GEMMs' operand, no cast pass)
    dXPb = torch.empty(M, HC, dtype=torch.bfloat16, device=dev) \
        if sv.plan.mfma and BF16_OUT else None
    _lib.call("lgnn_gat_bwd_node", csr.tptr, csr.tidx, csr.tmap, alpha, mask, da_e, da_d, dZ, XP,
              att_src, att_dst, M, H, C, dXP, part, P, dXPb, _s(dev))
    red = torch.empty(3 * HC, dtype=torch.float32, device=dev)
    if sv.plan.mfma:
        dg = dXPb if dXPb is not None else dXP.to(torch.bfloat16)
        # the attention partials and lin's dW slabs summed in one launch
        jobs = [(part, P, 3 * HC, red)] + (extra_red or [])
        dW = bf16_wgrad(dg, x, HC, jobs)
        reduce_multi(jobs, dev)
        dx = None
        if want_dx:
            K = W.size(1)
            if K <= 128:
                WTb = sv.wt if sv.wt is not None else bf16_weight_operands(W, True)[1]
                # dx's column sums ride along: the in_proj backward's bias gradient
                dx, dxb = bf16_gemm(dg, WTb, None, K, want_yb=BF16_OUT, want_colsum=True)
                if dxb is not None:
                    _remember_bf16(dx, dxb)
            else:
                dx = dense_mm(dg, dense_planes(W, True, True), K, None, True)
    else:
        jobs = [(part, P, 3 * HC, red)] + (extra_red or [])
        if sv.plan.dense:  # split-3 (or bf16-rounded) MFMA GEMMs on the fp32 dXP
            # lin's dW slabs join the attention partials' reduction: one launch per conv
            dW = dense_wgrad(dXP, x, sv.bf16, reducer=jobs)[0]
            reduce_multi(jobs, dev)
            dx = None
            if want_dx:
                wpt = sv.wpt if sv.wpt is not None else dense_planes(W, True, sv.bf16)
                dx = dense_mm(dXP, wpt, W.size(1), None, sv.bf16)
        else:
            if extra_red:
                reduce_multi(jobs, dev)
            else:
                _lib.call("lgnn_reduce_partials", part, P, 3 * HC, red, _s(dev))
            dx, dW, _ = linear_bwd(_lib.LGNN_GRAD_DIRECT, dXP, H=None,
                                   act=_lib.LGNN_ACT_NONE, X=x, W=W, want_dx=want_dx,
                                   want_db=False)
    return dx, dW, red


def att_grads(red: torch.Tensor, heads: int, has_bias: bool):
    """(datt_src, datt_dst, dbias or None) [1, H, C] / [H * C]: views of gat_conv_bwd's one
    reduction buffer (no copies)."""
    HC = red.numel() // 3
    shape = (1, heads, HC // heads)
    return (red[:HC].view(shape), red[HC:2 * HC].view(shape), red[2 * HC:] if has_bias else None)


def gat_head_fwd(x, W, att_src, att_dst, bias, W_out, b_out, graph, heads, slope, mask, act,
                 bf16, mean, wp=None, wpt=None):
    """The last GATConv + global pool + out_proj: (logits, HeadSaved)."""
    Y, conv = gat_conv_fwd(x, W, att_src, att_dst, bias, graph, heads, slope, mask, act, bf16, wp,
                           wpt)
    W_out, b_out = _f32c(W_out), _f32c(b_out)
    pooled, logits = pool_head_fwd(Y, graph, mean, W_out, b_out)
    return logits, HeadSaved(conv, pooled, W_out, mean)


def gat_head_bwd(sv: HeadSaved, dlogits, want_dx: bool):
    """(dx or None, dW, red, dW_out, db_out): the readout's backward formed inside the edge
    kernel's load (lgnn_gat_bwd_edge_pool), no dH tensor; out_proj's dW / db as outer-product
    jobs of the layer's reduction (HEAD_JOBS)."""
    dlogits = _f32c(dlogits)
    dWo, dbo, head_jobs = _head_grads(sv, dlogits, HEAD_JOBS)
    dx, dW, red = gat_conv_bwd(sv.conv, None, want_dx, extra_red=head_jobs,
                               pool=(dlogits, sv.W_out, sv.conv.graph, sv.mean))
    return dx, dW, red, dWo, dbo


class _GATConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, att_src, att_dst, bias, graph, heads, slope, mask, act, bf16=False,
                wp=None, wpt=None):
        Y, saved = gat_conv_fwd(x, W, att_src, att_dst, bias, graph, heads, slope, mask, act,
                                bf16, wp, wpt)
        _save(ctx, saved)
        return Y

    @staticmethod
    def backward(ctx, dY):
        sv = _load(ctx)
        dx, dW, red = gat_conv_bwd(sv, dY, ctx.needs_input_grad[0])
        return (dx, dW, *att_grads(red, sv.heads, sv.has_bias)) + (None,) * 8


GAT_S3 = True
# bf16 GAT: the attention kernels write their fp32 outputs' bf16 copies for the following bf16
# GEMMs (BF16_OUT = False: torch casts instead; the values are identical, RNE both ways)
BF16_OUT = True
# bf16 GATConv.lin forward with the attention scores in its epilogue (lgnn_bf16_gemm_att)
GAT_GEMM_ATT = True
_BF16_COPIES: dict = {}


def _remember_bf16(y: torch.Tensor, yb: torch.Tensor) -> None:
    key = id(y)
    _BF16_COPIES[key] = (weakref.ref(y), y._version, yb)
    weakref.finalize(y, _BF16_COPIES.pop, key, None)


def _bf16_copy_of(x: torch.Tensor):
    """The bf16 copy a GAT layer wrote beside its output x, if x is that output unchanged."""
    rec = _BF16_COPIES.get(id(x))
    if rec is None:
        return None
    ref, version, xb = rec
    if ref() is not x or x._version != version:
        return None
    return xb


class _GATConvHead(torch.autograd.Function):
    """The GAT model's last GATConv + global pool + out_proj as one autograd node: its backward
    forms the conv's output gradient from dlogits inside the edge kernel (out_proj backward +
    pool backward folded into the load, lgnn_gat_bwd_edge_pool) instead of writing dH
    (k_pool_bwd); out_proj's dW / db are outer-product jobs of the layer's slab reduction.
    Bitwise the separate nodes except out_proj's dW / db (another fixed summation order)."""

    @staticmethod
    def forward(ctx, x, W, att_src, att_dst, bias, W_out, b_out, graph, heads, slope, mask, act,
                bf16, mean, wp=None, wpt=None):
        logits, saved = gat_head_fwd(x, W, att_src, att_dst, bias, W_out, b_out, graph, heads,
                                     slope, mask, act, bf16, mean, wp, wpt)
        _save(ctx, saved)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        sv = _load(ctx)
        dx, dW, red, dWo, dbo = gat_head_bwd(sv, dlogits, ctx.needs_input_grad[0])
        return (dx, dW, *att_grads(red, sv.conv.heads, sv.conv.has_bias), dWo, dbo) + (None,) * 9


def gat_conv_head(x, W, att_src, att_dst, bias, W_out, b_out, graph: Graph, heads: int,
                  slope: float = 0.2, mask=None, act: int = _lib.LGNN_ACT_NONE,
                  bf16: bool = False, mean: bool = True, planes=None):
    """gat_conv followed by pool_head (the GAT model's last conv and readout) as one node."""
    wp, wpt = planes if planes is not None else (None, None)
    if _compiling():
        return torch.ops.lgnn.gat_conv_head(
            x, W, att_src, att_dst, bias, W_out, b_out, _lgnn().gparts(graph, "gat"), int(heads),
            float(slope), mask, int(act), bool(bf16), bool(mean), wp, wpt)[0]
    return _GATConvHead.apply(x, W, att_src, att_dst, bias, W_out, b_out, graph, heads, slope,
                              mask, act, bf16, mean, wp, wpt)


def gat_conv(x, W, att_src, att_dst, bias, graph: Graph, heads: int, slope: float = 0.2,
             mask=None, act: int = _lib.LGNN_ACT_NONE, bf16: bool = False, planes=None):
    """bf16: the lin GEMM (and its backward) on bf16-rounded operands, fp32 accumulate/out;
    attention, softmax and aggregation stay fp32. planes = (W's, W^T's) split-3 planes from
    s3_weight_bundle (fp32 / dense path), else each GEMM prepares its own."""
    wp, wpt = planes if planes is not None else (None, None)
    if _compiling():
        return torch.ops.lgnn.gat_conv(x, W, att_src, att_dst, bias, _lgnn().gparts(graph, "gat"),
                                       int(heads), float(slope), mask, int(act), bool(bf16), wp,
                                       wpt)[0]
    return _GATConv.apply(x, W, att_src, att_dst, bias, graph, heads, slope, mask, act, bf16, wp,
                          wpt)


# ----------------------------------------------------------------------------------------------
# criterion
# ----------------------------------------------------------------------------------------------


class _Regression(torch.autograd.Function):
    """The regression head and criterion: pred = clamp(z.squeeze(1), lo, hi) (reference
    gat.py:94-95 / gin.py:66-67) and loss = nn.MSELoss / nn.SmoothL1Loss (models/base.py:95-96)
    of (pred, y.float()), in one HIP launch forward (lgnn_regression_fwd) and one backward,
    instead of torch's clamp / compare / mse / mean / where kernels. Returns (pred, loss)."""

    @staticmethod
    def forward(ctx, z, y, lo, hi, smooth):
        _lib.require_gpu(z, y)
        ctx.needs_reshape = z.dim() == 2
        z = _f32c(z).reshape(-1)
        B = z.numel()
        if y.numel() != B:
            raise ValueError("regression target must have one value per graph")
        yi64 = y.dtype == torch.int64
        yc = y.contiguous() if yi64 else y.to(torch.float32).contiguous()
        pred = torch.empty(B, dtype=torch.float32, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        _lib.call("lgnn_regression_fwd", z, yc, int(yi64), B, float(lo), float(hi), int(smooth),
                  pred, loss, _s(z.device))
        ctx.save_for_backward(z, yc)
        ctx.cfg = (int(yi64), B, float(lo), float(hi), int(smooth))
        ctx.set_materialize_grads(False)
        return pred, loss

    @staticmethod
    def backward(ctx, gpred, gloss):
        z, yc = ctx.saved_tensors
        yi64, B, lo, hi, smooth = ctx.cfg
        dz = torch.empty_like(z)
        if gpred is None and gloss is None:
            return None, None, None, None, None
        _lib.call("lgnn_regression_bwd", z, yc, yi64, B, lo, hi, smooth,
                  _f32c(gloss) if gloss is not None else None,
                  _f32c(gpred).reshape(-1) if gpred is not None else None, dz, _s(z.device))
        return dz.view(-1, 1) if ctx.needs_reshape else dz, None, None, None, None


def regression_loss(logits: torch.Tensor, y: torch.Tensor, lo: float, hi: float,
                    kind: str = "MSE"):
    """(pred, loss): pred = clamp(logits.squeeze(1), lo, hi); loss = MSE or SmoothL1 (beta 1,
    mean) of (pred, y.float()). lo = -inf, hi = inf: the bare criterion."""
    if kind not in ("MSE", "SmoothL1"):
        raise ValueError(kind)
    if logits.dim() == 2 and logits.size(1) != 1:
        raise ValueError("regression logits must be [B] or [B, 1]")
    return _Regression.apply(logits, y, lo, hi, kind == "SmoothL1")


class _CrossEntropy(torch.autograd.Function):
    """nn.CrossEntropyLoss(weight) with mean reduction (reference models/base.py:93-94) in two
    HIP kernels (lgnn_ce_fwd / lgnn_ce_bwd) instead of log_softmax + nll_loss + their backward."""

    @staticmethod
    def forward(ctx, logits, target, weight, validate):
        _lib.require_gpu(logits, target)
        z = _f32c(logits)
        y = target.to(torch.int64).contiguous()
        B, C = z.shape
        dev = z.device
        lse = torch.empty(B, dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)  # loss, sum of weights
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        w = _f32c(weight) if weight is not None else None
        _lib.call("lgnn_ce_fwd", z, y, w, B, C, lse, out, out[1:], bad, _s(dev))
        if validate and int(bad.item()):
            raise ValueError("cross_entropy: a target is outside [0, num_classes)")
        ctx.save_for_backward(z, y, w, lse, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        z, y, w, lse, out = ctx.saved_tensors
        B, C = z.shape
        dz = torch.empty_like(z)
        g = _f32c(g.reshape(1))
        _lib.call("lgnn_ce_bwd", z, y, w, B, C, lse, out[1:], g, dz, _s(z.device))
        return dz, None, None, None


def cross_entropy(logits, target, weight=None, validate: bool = False):
    """Weighted-mean cross-entropy of [B, C] logits vs int64 targets. validate=True checks the
    targets (one host read); otherwise out-of-range targets are skipped silently."""
    return _CrossEntropy.apply(logits, target, weight, validate)


# ----------------------------------------------------------------------------------------------
# SortAggregation (DRGNet) and per-component feature pooling
# ----------------------------------------------------------------------------------------------


SortSaved = namedtuple("SortSaved", "x rank fill graph k")


def sort_pool_fwd(x, graph, k):
    """PyG 2.5.1 SortAggregation(k) (reference drgnet.py:37,59) on lgnn_sort_pool_fwd/_bwd:
    (out, SortSaved)."""
    _lib.require_gpu(x)
    x = _f32c(x)
    M, D = x.shape
    B = graph.num_graphs
    dev = x.device
    out = torch.empty(B, k * D, dtype=torch.float32, device=dev)
    rank = torch.empty(M, dtype=torch.int32, device=dev)
    fill = torch.empty(1, dtype=torch.float32, device=dev)
    nws = _lib.load().lgnn_sort_pool_workspace_bytes()
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _lib.call("lgnn_sort_pool_fwd", x, M, D, graph.gptr, B, int(k), out, rank, fill, ws, nws,
              _s(dev))
    return out, SortSaved(x, rank, fill, graph, int(k))


def sort_pool_bwd(sv: SortSaved, dout):
    M, D = sv.x.shape
    dx = torch.empty_like(sv.x)
    _lib.call("lgnn_sort_pool_bwd", _f32c(dout), sv.x, sv.rank, sv.graph.batch, sv.fill, M, D,
              sv.k, dx, _s(sv.x.device))
    return dx


class _SortPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, k):
        out, saved = sort_pool_fwd(x, graph, k)
        _save(ctx, saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        return sort_pool_bwd(_load(ctx), dout), None, None


def sort_pool(x, graph: Graph, k: int):
    """x [ΣN, D] -> [B, k * D]; graph carries batch / Batch.ptr."""
    if graph.batch is None:
        raise ValueError("sort_pool needs the graph's batch vector")
    if _compiling():
        return torch.ops.lgnn.sort_pool(x, _lgnn().gparts(graph, None), int(k))[0]
    return _SortPool.apply(x, graph, k)


def add_act_fwd(a, b):
    """ELU(a + b) on lgnn_add_act."""
    _lib.require_gpu(a, b)
    a, b = _f32c(a), _f32c(b)
    if a.shape != b.shape:
        raise ValueError(f"add_elu: shapes differ, {tuple(a.shape)} and {tuple(b.shape)}")
    y = torch.empty_like(a)
    _lib.call("lgnn_add_act", a, b, y, a.numel(), _lib.LGNN_ACT_ELU, _s(a.device))
    return y


def add_act_bwd(dy, y):
    """dZ = dy * ELU'(y) from the saved output (lgnn_act_bwd): the gradient of both summands."""
    dy = _f32c(dy)
    dz = torch.empty_like(dy)
    _lib.call("lgnn_act_bwd", dy, y, dz, dy.numel(), _lib.LGNN_ACT_ELU, _s(dy.device))
    return dz


class _AddElu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        y = add_act_fwd(a, b)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        dz = add_act_bwd(dy, ctx.saved_tensors[0])
        return dz, dz


def add_elu(a, b):
    """ELU(a + b) as one HIP launch, forward and backward (GraphConv's two branches and the
    activation after it): the same kernel eager and compiled."""
    if _compiling():
        _lgnn()
        return torch.ops.lgnn.add_elu(a, b)
    return _AddElu.apply(a, b)


# ----------------------------------------------------------------------------------------------
# DRGNet head: Conv1d / ELU / MaxPool1d / Conv1d / ELU / Lin / ELU / dropout / Lin
# ----------------------------------------------------------------------------------------------


DrgHeadSaved = namedtuple("DrgHeadSaved", "x k params mask a1 sel a2 h")

# the envelope of lgnn_drgnet_head_fwd / _bwd (include/lgnn.h)
_HEAD_LIMITS = {"D": (1, 4097), "k": (10, 512), "c0": (1, 64), "c1": (1, 64), "H": (1, 256),
                "C": (1, 16)}


def drgnet_head_dims(x, k, params, mask=None) -> tuple:
    """(B, D, c0, c1, H, dense, C) of a head call, every shape checked against k and
    D = x.size(1) // k and against the kernels' limits (ValueError naming what is off)."""
    w1, b1, w2, b2, l0w, l0b, l1w, l1b = params
    k = int(k)
    if x.dim() != 2 or k < 1 or x.size(1) % k != 0 or x.size(1) == 0:
        raise ValueError(f"drgnet_head: x must be [B, k * D] with k = {k}, got "
                         f"{tuple(x.shape)}")
    B, D = x.size(0), x.size(1) // k
    if w1.dim() != 3 or w1.size(1) != 1 or w1.size(2) != D:
        raise ValueError(f"drgnet_head: conv1.weight must be [c0, 1, D = {D}], got "
                         f"{tuple(w1.shape)}")
    c0 = w1.size(0)
    if w2.dim() != 3 or w2.size(1) != c0 or w2.size(2) != 5:
        raise ValueError(f"drgnet_head: conv2.weight must be [c1, c0 = {c0}, 5], got "
                         f"{tuple(w2.shape)}")
    c1 = w2.size(0)
    dense = c1 * (k // 2 - 4)
    if l0w.dim() != 2 or l0w.size(1) != dense:
        raise ValueError(f"drgnet_head: lins.0.weight must be [H, c1 * (k // 2 - 4) = {dense}], "
                         f"got {tuple(l0w.shape)}")
    H = l0w.size(0)
    if l1w.dim() != 2 or l1w.size(1) != H:
        raise ValueError(f"drgnet_head: lins.1.weight must be [C, H = {H}], got "
                         f"{tuple(l1w.shape)}")
    C = l1w.size(0)
    for name, b, n in (("conv1", b1, c0), ("conv2", b2, c1), ("lins.0", l0b, H),
                       ("lins.1", l1b, C)):
        if tuple(b.shape) != (n,):
            raise ValueError(f"drgnet_head: {name}.bias must be [{n}], got {tuple(b.shape)}")
    if mask is not None and tuple(mask.shape) != (B, H):
        raise ValueError(f"drgnet_head: mask must be [B, H] = [{B}, {H}], got "
                         f"{tuple(mask.shape)}")
    if not torch.compiler.is_compiling():  # under a trace B and the widths may be symbolic
        for name, v in (("D", D), ("k", k), ("c0", c0), ("c1", c1), ("H", H), ("C", C)):
            lo, hi = _HEAD_LIMITS[name]
            if not lo <= v <= hi:
                raise ValueError(f"drgnet_head: {name} = {v} is outside the kernels' limit "
                                 f"{lo} <= {name} <= {hi}")
        if B < 1:
            raise ValueError("drgnet_head: B = 0 graphs (the kernels take B >= 1)")
        if (B + 64) * max(dense, H + H % 2) >= 2 ** 29:
            raise ValueError(f"drgnet_head: B = {B} is outside the kernels' limit "
                             "(B + 64) * max(dense, H) < 2^29")
    return B, D, c0, c1, H, dense, C


def drgnet_head_fwd(x, k, params, mask=None):
    """The DRGNet head after SortAggregation (reference drgnet.py:60-64) on lgnn_drgnet_head_fwd:
    (logits [B, C], DrgHeadSaved). params: conv1.weight / bias, conv2.weight / bias,
    lins.0.weight / bias, lins.1.weight / bias; mask: the dropout mask [B, H] or None."""
    B, D, c0, c1, H, dense, C = drgnet_head_dims(x, k, params, mask)
    _lib.require_gpu(x, *params, mask)
    x = _f32c(x)
    params = tuple(_f32c(p) for p in params)
    mask = _f32c(mask) if mask is not None else None
    dev, K2 = x.device, int(k) // 2
    f32 = dict(dtype=torch.float32, device=dev)
    logits = torch.empty(B, C, **f32)
    a1 = torch.empty(B, K2, c0, **f32)
    sel = torch.empty(B, K2, (c0 + 15) // 16, dtype=torch.int16, device=dev)
    a2 = torch.empty(B, dense, **f32)
    h = torch.empty(B, H, **f32)
    w1, b1, w2, b2, l0w, l0b, l1w, l1b = params
    _lib.call("lgnn_drgnet_head_fwd", x, B, int(k), D, w1, b1, c0, w2, b2, c1, l0w, l0b, H, dense,
              l1w, l1b, C, mask, logits, a1, sel, a2, h, _s(dev))
    return logits, DrgHeadSaved(x, int(k), params, mask, a1, sel, a2, h)


def drgnet_head_bwd(sv: DrgHeadSaved, dlogits):
    """(dx, [the eight parameter gradients in DrgHeadSaved.params order]) on lgnn_drgnet_head_bwd:
    three launches, no atomics, bitwise reproducible."""
    w1, _, w2, _, l0w, _, l1w, _ = sv.params
    B, D = sv.x.size(0), sv.x.size(1) // sv.k
    c0, c1, (H, dense), C = w1.size(0), w2.size(0), l0w.shape, l1w.size(0)
    He = H + H % 2
    dev = sv.x.device
    f32 = dict(dtype=torch.float32, device=dev)
    nws = _lib.query("lgnn_drgnet_head_workspace_bytes", B, sv.k, D, c0, c1, H, C)
    if nws == 0:
        raise ValueError("drgnet_head: shape outside the kernels' limits")
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    dx = torch.empty_like(sv.x)
    dh = torch.empty(B, He, **f32)
    dw1, db1 = torch.empty_like(w1), torch.empty(c0, **f32)
    dw2, db2 = torch.empty_like(w2), torch.empty(c1, **f32)
    dl0w, dl0b = torch.empty(He, dense, **f32), torch.empty(He, **f32)
    dl1w, dl1b = torch.empty_like(l1w), torch.empty(C, **f32)
    _lib.call("lgnn_drgnet_head_bwd", _f32c(dlogits), sv.x, B, sv.k, D, w1, c0, w2, c1, l0w, H,
              dense, l1w, C, sv.mask, sv.a1, sv.sel, sv.a2, sv.h, dx, dh, dw1, db1, dw2, db2,
              dl0w, dl0b, dl1w, dl1b, ws, nws, _s(dev))
    return dx, [dw1, db1, dw2, db2, dl0w[:H], dl0b[:H], dl1w, dl1b]


class _DrgnetHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, mask, *params):
        logits, saved = drgnet_head_fwd(x, k, params, mask)
        _save(ctx, saved)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        dx, dparams = drgnet_head_bwd(_load(ctx), dlogits)
        return (dx, None, None, *dparams)


def drgnet_head(x, k, conv1_w, conv1_b, conv2_w, conv2_b, lin0_w, lin0_b, lin1_w, lin1_b,
                mask=None):
    """DRGNet's head on the sort-pooled x [B, k * D]: logits [B, C], with gradients for x and the
    eight parameters (none for the mask). HIP only: no torch route."""
    params = (conv1_w, conv1_b, conv2_w, conv2_b, lin0_w, lin0_b, lin1_w, lin1_b)
    if _compiling():
        _lgnn()
        return torch.ops.lgnn.drgnet_head(x, int(k), list(params), mask)[0]
    return _DrgnetHead.apply(x, k, mask, *params)


def cc_pool(features: torch.Tensor, cc: torch.Tensor, num_segments: int, reduce_max: bool,
            validate: bool = True) -> torch.Tensor:
    """features (C, P) fp32 channel-major, cc (P,) int64 -> (num_segments, C): per-label mean or
    max (lgnn_cc_pool). validate: raise if a label falls outside [0, num_segments) (one host
    read)."""
    _lib.require_gpu(features, cc)
    f = _f32c(features)
    C, P = f.shape
    lab = cc.reshape(-1).to(torch.int64).contiguous()
    if lab.numel() != P:
        raise ValueError("cc must hold one label per pixel")
    dev = f.device
    out = torch.empty(num_segments, C, dtype=torch.float32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    nws = _lib.load().lgnn_cc_pool_workspace_bytes(P, C, num_segments)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _lib.call("lgnn_cc_pool", f, C, P, lab, int(num_segments), int(reduce_max), out, None, err,
              ws, nws, _s(dev))
    if validate and int(err.item()):
        raise IndexError(f"cc_pool: {int(err.item())} labels outside [0, {num_segments})")
    return out


def label_pool(logits: torch.Tensor, size: tuple[int, int]) -> torch.Tensor:
    """logits (K, Hin, Win) fp32, K <= 255 -> (H, W) uint8 class map equal to
    F.adaptive_max_pool2d(argmax(logits, 0).float(), size), in one launch (lgnn_label_pool)."""
    _lib.require_gpu(logits)
    if logits.dim() != 3:
        raise ValueError("logits must be (K, H, W)")
    f = _f32c(logits)
    K, Hin, Win = f.shape
    if not 1 <= K <= 255:
        raise ValueError("label_pool takes 1 to 255 classes")
    H, W = int(size[0]), int(size[1])
    out = torch.empty(H, W, dtype=torch.uint8, device=f.device)
    _lib.call("lgnn_label_pool", f, K, Hin, Win, out, H, W, _s(f.device))
    return out


def ccl(image: torch.Tensor, connectivity: int = 8) -> tuple[torch.Tensor, torch.Tensor]:
    """image (H, W) uint8, nonzero = foreground -> (labels (H, W) int64, num_labels int32 [1] on
    the device, background included): 0 the background, components 1, 2, ... in raster order of
    their first pixel (lgnn_ccl). No host synchronisation."""
    _lib.require_gpu(image)
    if image.dim() != 2 or image.dtype != torch.uint8:
        raise ValueError("image must be a (H, W) uint8 tensor")
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    img = image.contiguous()
    H, W = img.shape
    dev = img.device
    labels = torch.empty(H, W, dtype=torch.int64, device=dev)
    num = torch.empty(1, dtype=torch.int32, device=dev)
    nws = _lib.load().lgnn_ccl_workspace_bytes(H, W)
    ws = torch.empty(max(1, nws), dtype=torch.uint8, device=dev)
    _lib.call("lgnn_ccl", img, H, W, int(connectivity), labels, num, ws, nws, _s(dev))
    return labels, num


def ccl_stats(labels: torch.Tensor, num_labels: int,
              validate: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """labels (H, W) int64 in [0, num_labels) -> (stats (num_labels, 5) int32: left, top, width,
    height, area; centroids (num_labels, 2) fp64: mean x, mean y) (lgnn_ccl_stats). validate:
    raise if a label falls outside the range (one host read)."""
    _lib.require_gpu(labels)
    if labels.dim() != 2 or labels.dtype != torch.int64:
        raise ValueError("labels must be a (H, W) int64 tensor")
    lab = labels.contiguous()
    H, W = lab.shape
    dev = lab.device
    n = int(num_labels)
    stats = torch.empty(n, 5, dtype=torch.int32, device=dev)
    centroids = torch.empty(n, 2, dtype=torch.float64, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("lgnn_ccl_stats", lab, H, W, n, stats, centroids, err, _s(dev))
    if validate and int(err.item()):
        raise IndexError(f"ccl_stats: {int(err.item())} labels outside [0, {n})")
    return stats, centroids


def label_pool_batch(logits: torch.Tensor, size: tuple[int, int]) -> torch.Tensor:
    """logits (B, K, Hin, Win) fp32, K <= 255 -> (B, H, W) uint8: `label_pool` of every image, in
    one launch (lgnn_label_pool_batch)."""
    _lib.require_gpu(logits)
    if logits.dim() != 4:
        raise ValueError("logits must be (B, K, H, W)")
    f = _f32c(logits)
    B, K, Hin, Win = f.shape
    if not 1 <= K <= 255:
        raise ValueError("label_pool_batch takes 1 to 255 classes")
    H, W = int(size[0]), int(size[1])
    out = torch.empty(B, H, W, dtype=torch.uint8, device=f.device)
    _lib.call("lgnn_label_pool_batch", f, B, K, Hin, Win, out, H, W, _s(f.device))
    return out


def ccl_batch(image: torch.Tensor, connectivity: int = 8
              ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """image (B, H, W) uint8, nonzero = foreground -> (labels (B, H, W) int64, num_labels int32
    [B], node_ptr int64 [B + 1], all on the device): per image what `ccl` gives for it alone,
    the numbering restarting in every image; node_ptr is the exclusive scan of num_labels
    (lgnn_ccl_batch). Six launches whatever B is, no host synchronisation."""
    _lib.require_gpu(image)
    if image.dim() != 3 or image.dtype != torch.uint8:
        raise ValueError("image must be a (B, H, W) uint8 tensor")
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    img = image.contiguous()
    B, H, W = img.shape
    dev = img.device
    labels = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    num = torch.empty(B, dtype=torch.int32, device=dev)
    node_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    nws = _lib.load().lgnn_ccl_batch_workspace_bytes(B, H, W)
    ws = torch.empty(max(1, nws), dtype=torch.uint8, device=dev)
    _lib.call("lgnn_ccl_batch", img, B, H, W, int(connectivity), labels, num, node_ptr, ws, nws,
              _s(dev))
    return labels, num, node_ptr


def ccl_stats_batch(labels: torch.Tensor, node_ptr: torch.Tensor, total_nodes: int,
                    validate: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """labels (B, H, W) int64 and node_ptr int64 [B + 1] as `ccl_batch` gives them, total_nodes =
    node_ptr[B] -> (stats (total_nodes, 5) int32, centroids (total_nodes, 2) fp64): row
    node_ptr[b] + l is `ccl_stats`' row l for image b (lgnn_ccl_stats_batch). validate: raise if
    a label falls outside its image's range (one host read)."""
    _lib.require_gpu(labels, node_ptr)
    if labels.dim() != 3 or labels.dtype != torch.int64:
        raise ValueError("labels must be a (B, H, W) int64 tensor")
    lab = labels.contiguous()
    B, H, W = lab.shape
    if node_ptr.dtype != torch.int64 or node_ptr.numel() != B + 1:
        raise ValueError("node_ptr must be an int64 tensor of B + 1 offsets")
    dev = lab.device
    n = int(total_nodes)
    stats = torch.empty(n, 5, dtype=torch.int32, device=dev)
    centroids = torch.empty(n, 2, dtype=torch.float64, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("lgnn_ccl_stats_batch", lab, B, H, W, node_ptr.contiguous(), n, stats, centroids,
              err, _s(dev))
    if validate and int(err.item()):
        raise IndexError(f"ccl_stats_batch: {int(err.item())} labels outside their image's range")
    return stats, centroids


def cc_pool_resample(features: torch.Tensor, labels: torch.Tensor, node_ptr: torch.Tensor,
                     total_nodes: int, reduce_max: bool, max_nodes: int | None = None,
                     validate: bool = True, return_counts: bool = False):
    """features (B, C, h, w) fp32, labels (B, H, W) int64 and node_ptr int64 [B + 1] as
    `ccl_batch` gives them, total_nodes = node_ptr[B] -> (total_nodes, C): row node_ptr[b] + l
    is the mean or max, over the pixels of label l of image b, of the feature map sampled
    bilinearly at (H, W) (F.interpolate's align_corners=False), which is never stored
    (lgnn_cc_pool_resample); (H, W) == (h, w) pools the map itself. h * w * 4 <=
    LGNN_CC_POOL_RESAMPLE_MAX_SOURCE_BYTES unless the sizes are equal. max_nodes: an upper bound
    of the labels per image the caller knows (default: the limit, 4032); a tight one runs
    faster. validate: raise if a label falls outside its image's range (one host read).
    return_counts: also the pixels per label, (total_nodes,) int32."""
    _lib.require_gpu(features, labels, node_ptr)
    if features.dim() != 4:
        raise ValueError("features must be (B, C, h, w)")
    if labels.dim() != 3 or labels.dtype != torch.int64:
        raise ValueError("labels must be a (B, H, W) int64 tensor")
    f = _f32c(features)
    lab = labels.contiguous()
    B, C, h, w = f.shape
    H, W = lab.shape[1:]
    if lab.size(0) != B:
        raise ValueError("features and labels must hold the same number of images")
    if node_ptr.dtype != torch.int64 or node_ptr.numel() != B + 1:
        raise ValueError("node_ptr must be an int64 tensor of B + 1 offsets")
    limit = _lib.LGNN_CC_POOL_MAX_SEGMENTS
    nmax = limit if max_nodes is None else int(max_nodes)
    if not 1 <= nmax <= limit:
        raise ValueError(f"max_nodes must be in [1, {limit}]")
    if (h, w) != (H, W) and h * w * 4 > _lib.LGNN_CC_POOL_RESAMPLE_MAX_SOURCE_BYTES:
        raise ValueError(f"cc_pool_resample stages a source map of at most "
                         f"{_lib.LGNN_CC_POOL_RESAMPLE_MAX_SOURCE_BYTES} bytes, got {h} x {w}")
    dev = f.device
    n = int(total_nodes)
    out = torch.empty(n, C, dtype=torch.float32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev) if return_counts else None
    err = torch.empty(1, dtype=torch.int32, device=dev)
    nws = _lib.load().lgnn_cc_pool_resample_workspace_bytes(B, H, W, n)
    ws = torch.empty(max(1, nws), dtype=torch.uint8, device=dev)
    _lib.call("lgnn_cc_pool_resample", f, B, C, h, w, lab, H, W, node_ptr.contiguous(), n, nmax,
              int(reduce_max), out, counts, err, ws, nws, _s(dev))
    if validate and int(err.item()):
        raise IndexError(f"cc_pool_resample: {int(err.item())} labels outside their image's "
                         f"range or at or above max_nodes = {nmax}")
    return (out, counts) if return_counts else out


def collate(store, ids, validate: bool = False, ids_dev: torch.Tensor | None = None):
    """The graphs `ids` (host int64 tensor or list; repeats allowed) of a datasets.GraphStore as
    one synth.Batch on the store's device (lgnn_collate): x, pos, y, batch, ptr as PyG's Collater
    gives them and num_graphs set. A store with edges (GraphStore.with_edges) gives edge_index
    [2, sum m_b] too, the graphs' edges offset to the batch's rows (lgnn_collate_edges, on the same
    stream), `batch.edge_ptr` and, when the store has weights, `batch.edge_weight`; a store without
    gives an empty [2, 0] edge_index and no further launch. An id outside [0, len(store)) raises
    IndexError before any launch. The outputs are sized from the store's host copies of ptr and
    edge_ptr: nothing is read back from the device, unless validate, which reads both err words
    and raises if a kernel skipped an id or ran out of room. ids_dev: the same ids already on the
    device (GraphLoader uploads an epoch's order once, without a synchronising copy); by default
    they are copied there."""
    from .synth import Batch

    ids = torch.as_tensor(ids, dtype=torch.int64, device="cpu").reshape(-1)
    G, B = len(store), ids.numel()
    if B and (int(ids.min()) < 0 or int(ids.max()) >= G):
        raise IndexError(f"collate: graph ids must be in [0, {G})")
    _lib.require_gpu(store.x, store.pos, store.y, store.ptr)
    dev = store.x.device
    sizes = store.ptr_host[ids + 1] - store.ptr_host[ids]
    total = int(sizes.sum())
    C = store.x.size(1)
    # a tensor without elements has no address: the buffers hold one row at least
    x = store.x if store.x.size(0) else torch.zeros(1, C, dtype=torch.float32, device=dev)
    out_x = torch.empty(max(total, 1), C, dtype=torch.float32, device=dev)
    out_batch = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    pos, out_pos, dims = store.pos, None, 0
    if pos is not None:
        dims = pos.size(1)
        out_pos = torch.empty(max(total, 1), dims, dtype=torch.float64, device=dev)
        if not pos.size(0):
            pos = torch.zeros(1, dims, dtype=torch.float64, device=dev)
    out_y = torch.empty(max(B, 1), dtype=torch.int64, device=dev)
    out_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    err = torch.empty(2, dtype=torch.int32, device=dev)  # [rows, edges]
    nws = _lib.load().lgnn_collate_workspace_bytes(B)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
    if ids_dev is None:
        ids_dev = ids.to(dev)
    elif ids_dev.dtype != torch.int64 or ids_dev.device != dev or ids_dev.shape != ids.shape \
            or not ids_dev.is_contiguous():
        raise ValueError("collate: ids_dev must be the ids as a contiguous int64 tensor on the "
                         "store's device")
    _lib.call("lgnn_collate", ids_dev if B else None, B, store.ptr, G, x, C, pos, dims,
              store.y if G else out_y, out_x, out_pos, out_y, out_batch, out_ptr, total, err, ws,
              nws, _s(dev))
    edge_index = edge_ptr = edge_weight = None
    if getattr(store, "edge_index", None) is not None:
        m = store.edge_ptr_host[ids + 1] - store.edge_ptr_host[ids]
        E, w = int(m.sum()), store.edge_weight
        edge_index = torch.empty(2, max(E, 1), dtype=torch.int64, device=dev)
        edge_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
        if w is not None:
            edge_weight = torch.empty(max(E, 1), dtype=w.dtype, device=dev)
        ews = torch.empty(_lib.load().lgnn_collate_edges_workspace_bytes(B), dtype=torch.uint8,
                          device=dev)
        has_w = w is not None and w.numel() > 0
        # the row stride of the output is the capacity: E edges exactly, unless E is 0, when
        # nothing is written
        _lib.call("lgnn_collate_edges", ids_dev if B else None, B, store.ptr, store.edge_ptr, G,
                  store.edge_index if store.edge_index.numel() else None,
                  store.edge_index.size(1), w if has_w else None, w.element_size() if has_w else 0,
                  out_ptr, edge_index, edge_weight if has_w else None, edge_ptr, E, err[1:], ews,
                  ews.numel(), _s(dev))
        edge_index = edge_index[:, :E]
        edge_weight = None if edge_weight is None else edge_weight[:E]
    if validate:
        e = err.tolist()
        e[1] = e[1] if edge_ptr is not None else 0  # written only for a store with edges
        if e[0] or e[1]:
            raise IndexError(f"collate: err = {e[0]} for the rows, {e[1]} for the edges (ids the "
                             f"kernel skipped, plus {_lib.LGNN_COLLATE_OVERFLOW} on overflow)")
    if edge_index is None:
        edge_index = torch.empty(2, 0, dtype=torch.int64, device=dev)
    out = Batch(out_x[:total], edge_index, out_batch[:total], out_ptr, out_y[:B],
                None if out_pos is None else out_pos[:total], B)
    if edge_ptr is not None:
        out.edge_ptr = edge_ptr
    if edge_weight is not None:
        out.edge_weight = edge_weight
    return out


# ----------------------------------------------------------------------------------------------
# SIFT nodes (sift.hip): scale space, candidates, keypoints, descriptors for a batch of images
# ----------------------------------------------------------------------------------------------


def sift_octave_dims(height: int, width: int) -> list[tuple[int, int]]:
    """The (h, w) of every octave lgnn_sift_pyramid builds for (height, width) images: the
    doubled image, halved per octave, while the smaller side exceeds 10."""
    n = _lib.load().lgnn_sift_num_octaves(int(height), int(width))
    return [((2 * height) >> o, (2 * width) >> o) for o in range(n)]


class SiftPyramid(NamedTuple):
    """The scale space of B images of one size as the kernels hold it: gray (B, H, W) uint8 (or
    None), the Gaussian levels octave after octave as one flat fp32 buffer of (B, 6, h, w) blocks,
    the DoG levels likewise as (B, 5, h, w). `gauss` / `dog` are the per-octave views."""

    gray: torch.Tensor | None
    gauss_flat: torch.Tensor
    dog_flat: torch.Tensor
    shape: tuple  # (B, H, W)

    def _views(self, flat: torch.Tensor, levels: int) -> list[torch.Tensor]:
        B, H, W = self.shape
        out, at = [], 0
        for h, w in sift_octave_dims(H, W):
            n = B * levels * h * w
            out.append(flat[at:at + n].view(B, levels, h, w))
            at += n
        return out

    @property
    def gauss(self) -> list[torch.Tensor]:
        return self._views(self.gauss_flat, 6)

    @property
    def dog(self) -> list[torch.Tensor]:
        return self._views(self.dog_flat, 5)

    @classmethod
    def from_levels(cls, gauss, dog, gray: torch.Tensor | None = None) -> "SiftPyramid":
        """From per-octave tensors (B, 6, h, w) and (B, 5, h, w) (either list may be None: the
        stage that is run does not read it), e.g. an oracle's levels."""
        some = gauss if gauss is not None else dog
        _lib.require_gpu(*some)
        B, _, h, w = some[0].shape
        if h % 2 or w % 2:
            raise ValueError("octave 0 is the doubled image: its sides are even")
        shape = (B, h // 2, w // 2)
        dims = sift_octave_dims(*shape[1:])

        def pack(levels, count):
            if levels is None:
                return torch.empty(0, dtype=torch.float32, device=some[0].device)
            if [tuple(t.shape) for t in levels] != [(B, count, a, b) for a, b in dims]:
                raise ValueError(f"expected the octaves {[(B, count, a, b) for a, b in dims]}")
            return torch.cat([_f32c(t).reshape(-1) for t in levels])

        return cls(gray, pack(gauss, 6), pack(dog, 5), shape)


def sift_pyramid(images: torch.Tensor, sigma: float) -> SiftPyramid:
    """images (B, H, W, 3) or (B, H, W) uint8 -> the gray images (the reference's RGB array read
    as BGR: red gets the 0.114 weight) and the Gaussian and DoG levels of every octave, fp32
    (lgnn_sift_pyramid). 1 + 6 launches per octave whatever B is, no host synchronisation."""
    if images.dtype != torch.uint8 or images.dim() not in (3, 4) or \
            (images.dim() == 4 and images.size(3) != 3):
        raise ValueError("images must be a (B, H, W, 3) or (B, H, W) uint8 tensor")
    _lib.require_gpu(images)
    img = images.contiguous()
    B, H, W = img.shape[:3]
    dev = img.device
    if B < 1 or H < 2 or W < 2:
        raise ValueError("sift_pyramid takes at least one image of at least 2 x 2 pixels")
    n = _lib.load().lgnn_sift_pyramid_floats(B, H, W)
    gray = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    gauss = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    dog = torch.empty(max(n // 6 * 5, 1), dtype=torch.float32, device=dev)
    _lib.call("lgnn_sift_pyramid", img, B, H, W, 3 if img.dim() == 4 else 1, float(sigma), gray,
              gauss, n, dog, n // 6 * 5, _s(dev))
    return SiftPyramid(gray, gauss[:n], dog[:n // 6 * 5], (B, H, W))


def sift_candidates(pyramid: SiftPyramid) -> torch.Tensor:
    """The 26-neighbour extrema of DoG layers 1..3 at least 5 pixels from every edge -> cand
    (n, 5) int32 (image, octave, layer, row, column), in that order (lgnn_sift_count,
    lgnn_sift_candidates). Three launches and one host read: the total, which sizes cand."""
    B, H, W = pyramid.shape
    dog = pyramid.dog_flat
    _lib.require_gpu(dog)
    dev = dog.device
    rows = _lib.load().lgnn_sift_rows(B, H, W)
    counts = torch.empty(max(rows, 1), dtype=torch.int32, device=dev)
    row_ptr = torch.empty(rows + 1, dtype=torch.int32, device=dev)
    _lib.call("lgnn_sift_count", dog if rows else None, B, H, W, counts, row_ptr, _s(dev))
    n = int(row_ptr[rows].item())
    cand = torch.empty(max(n, 1), 5, dtype=torch.int32, device=dev)
    _lib.call("lgnn_sift_candidates", dog if rows else None, B, H, W, row_ptr, cand, n, _s(dev))
    return cand[:n]


def sift_keypoints(pyramid: SiftPyramid, cand: torch.Tensor, sigma: float, num_keypoints: int
                   ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """cand (n, 5) int32 as `sift_candidates` gives them -> (kf (m, 5) fp32: x, y, size, angle,
    response, pt and size halved for the doubled image; ki (m, 3) int32: image, octave, layer;
    node_ptr (B + 1) int64 on the device; its host copy): refinement, orientation peaks,
    duplicate removal and the cut at the num_keypoints-th largest response (ties kept), per image
    by response descending, then candidate order (lgnn_sift_keypoints, lgnn_sift_gather). Ten
    launches and one host read: node_ptr, which sizes the outputs."""
    B, H, W = pyramid.shape
    _lib.require_gpu(pyramid.gauss_flat, pyramid.dog_flat, cand)
    if cand.dim() != 2 or cand.size(1) != 5 or cand.dtype != torch.int32:
        raise ValueError("cand must be a (n, 5) int32 tensor")
    if int(num_keypoints) < 1:
        raise ValueError("num_keypoints must be at least 1")
    c = cand.contiguous()
    n = c.size(0)
    dev = c.device
    nws = _lib.load().lgnn_sift_keypoints_workspace_bytes(B, n)
    if nws == 0:
        raise ValueError(f"sift_keypoints: {n} candidates are more than the entry takes")
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    node_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    on = bool(n)
    _lib.call("lgnn_sift_keypoints", pyramid.gauss_flat if on else None,
              pyramid.dog_flat if on else None, B, H, W, float(sigma), c if on else None, n,
              int(num_keypoints), node_ptr, ws, nws, _s(dev))
    ptr_host = node_ptr.cpu()
    m = int(ptr_host[-1])
    kf = torch.empty(max(m, 1), 5, dtype=torch.float32, device=dev)
    ki = torch.empty(max(m, 1), 3, dtype=torch.int32, device=dev)
    _lib.call("lgnn_sift_gather", B, n, node_ptr, m, kf, ki, ws, nws, _s(dev))
    return kf[:m], ki[:m], node_ptr, ptr_host


def sift_descriptors(pyramid: SiftPyramid, kf: torch.Tensor, ki: torch.Tensor) -> torch.Tensor:
    """kf (m, 5) fp32 and ki (m, 3) int32 as `sift_keypoints` gives them -> (m, 128) fp32, the
    4 x 4 x 8 descriptors as integers in 0..255, read from each keypoint's Gaussian level
    (lgnn_sift_descriptors). One launch, no host synchronisation."""
    B, H, W = pyramid.shape
    _lib.require_gpu(pyramid.gauss_flat, kf, ki)
    if kf.dim() != 2 or kf.size(1) != 5 or ki.dim() != 2 or ki.size(1) != 3 or \
            ki.dtype != torch.int32 or kf.size(0) != ki.size(0):
        raise ValueError("kf must be (m, 5) fp32 and ki (m, 3) int32")
    f, k = _f32c(kf), ki.contiguous()
    m = f.size(0)
    dev = f.device
    x = torch.empty(max(m, 1), 128, dtype=torch.float32, device=dev)
    if m:
        _lib.call("lgnn_sift_descriptors", pyramid.gauss_flat, B, H, W, f, k, m, x, _s(dev))
    return x[:m]


# ----------------------------------------------------------------------------------------------
# Fundus image preprocessing (fundus.hip): autocrop box, resize, pad, normalise for a batch of
# images of different sizes
# ----------------------------------------------------------------------------------------------


def _fundus_images(images, what: str = "images", channels: int | None = 3) -> list[torch.Tensor]:
    """A (B, H, W, 3) uint8 tensor or a list of (H_b, W_b, 3) uint8 tensors -> the contiguous
    per-image tensors (views where the input already is contiguous). channels None: (H, W)
    label masks."""
    shape = "(H, W, 3)" if channels else "(H, W)"
    imgs = list(images.unbind(0)) if isinstance(images, torch.Tensor) and \
        images.dim() == (4 if channels else 3) else images
    if isinstance(imgs, torch.Tensor) or len(imgs) == 0:
        raise ValueError(f"{what} must be a batch or a non-empty list of {shape} uint8 tensors")
    for t in imgs:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"{what} must be uint8 tensors, got "
                             f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.dim() != (3 if channels else 2) or (channels and t.size(2) != channels):
            raise ValueError(f"each of {what} must be {shape}, got {tuple(t.shape)}")
    _lib.require_gpu(*imgs)
    side = _lib.LGNN_FUNDUS_MAX_SIDE
    for t in imgs:
        if not (2 <= t.size(0) <= side and 2 <= t.size(1) <= side):
            raise ValueError(f"each of {what} must have sides in [2, {side}], got "
                             f"{tuple(t.shape)}")
    return [t.contiguous() for t in imgs]


def fundus_bbox(images, threshold: float = 25.0) -> torch.Tensor:
    """images: a (B, H, W, 3) uint8 tensor or a list of (H_b, W_b, 3) uint8 tensors of any sizes
    -> boxes (B, 4) int32 (x_min, x_max, y_min, y_max): the extreme coordinates of the pixels with
    red > threshold, or (0, W, 0, H) for an image with none or with x_min == x_max or y_min ==
    y_max (lgnn_fundus_bbox). No host read; two launches per 16 images."""
    imgs = _fundus_images(images)
    dev = imgs[0].device
    boxes = torch.empty(len(imgs), 4, dtype=torch.int32, device=dev)
    _lib.call("lgnn_fundus_bbox", len(imgs), imgs, [t.size(0) for t in imgs],
              [t.size(1) for t in imgs], float(threshold), boxes, _s(dev))
    return boxes


def fundus_preprocess(images, boxes: torch.Tensor, size: int, mean, std, masks=None,
                      want_float: bool = True, want_uint8: bool = False):
    """The crop boxes[b] of image b resized so that its longer side is `size` (8-bit INTER_LINEAR
    restated in integers; the label mask INTER_NEAREST), centred in size x size on zeros and
    normalised -> (image (B, 3, size, size) fp32 or None, uint8 (B, size, size, 3) or None, mask
    (B, size, size) uint8 or None, geom (B, 8) int32: x_min, y_min, w, h, new_w, new_h, pad_left,
    pad_top) (lgnn_fundus_preprocess). images / masks as `fundus_bbox` takes them, masks (H_b,
    W_b) uint8. No host read; one launch per 16 images."""
    imgs = _fundus_images(images)
    B = len(imgs)
    dev = imgs[0].device
    S = int(size)
    if not 2 <= S <= _lib.LGNN_FUNDUS_MAX_SIDE:
        raise ValueError(f"size must be in [2, {_lib.LGNN_FUNDUS_MAX_SIDE}], got {size}")
    if not (want_float or want_uint8):
        raise ValueError("fundus_preprocess: at least one of want_float and want_uint8")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3 or not all(s > 0 for s in std):
        raise ValueError("mean and std are three numbers each, every std positive")
    _lib.require_gpu(boxes)
    if boxes.dtype != torch.int32 or tuple(boxes.shape) != (B, 4):
        raise ValueError(f"boxes must be ({B}, 4) int32")
    mks = None
    if masks is not None:
        mks = _fundus_images(masks, "masks", None)
        if [tuple(m.shape) for m in mks] != [tuple(t.shape[:2]) for t in imgs]:
            raise ValueError("masks must match the images' heights and widths")
    out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev) if want_float else None
    u8 = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev) if want_uint8 else None
    om = torch.empty(B, S, S, dtype=torch.uint8, device=dev) if mks is not None else None
    geom = torch.empty(B, 8, dtype=torch.int32, device=dev)
    _lib.call("lgnn_fundus_preprocess", B, imgs, mks, [t.size(0) for t in imgs],
              [t.size(1) for t in imgs], boxes.contiguous(), S, *mean, *std, out, u8, om, geom,
              _s(dev))
    return out, u8, om, geom


# ----------------------------------------------------------------------------------------------
# Set attention (setattn.hip): segmented multi-head attention over ragged sets, the residual +
# activation + LayerNorm of PyG's MultiheadAttentionBlock, the set readout
# ----------------------------------------------------------------------------------------------


# Which rows of q and k / v belong to set g (lgnn_set_attn_fwd): qptr / kptr int32 [B + 1]
# offsets (ragged rows, Batch.ptr) or None with q_rows / k_rows rows per set; q_shared: the same
# q_rows query rows for every set (PMA's seeds, ISAB's inducing points).
AttnForm = namedtuple("AttnForm", "qptr q_rows q_shared kptr k_rows num_sets")


def set_attn_plan(heads: int, head_dim: int) -> None:
    """The shapes the attention kernels take; anything else raises (no other path exists)."""
    if heads < 1 or not 1 <= head_dim <= _lib.LGNN_SET_ATTN_MAX_D \
            or heads * head_dim > _lib.LGNN_SET_ATTN_MAX_HD:
        raise NotImplementedError(
            f"set attention takes head_dim in 1..{_lib.LGNN_SET_ATTN_MAX_D} and heads * head_dim "
            f"<= {_lib.LGNN_SET_ATTN_MAX_HD}; got heads = {heads}, head_dim = {head_dim}")


def _rows_view(t: torch.Tensor) -> torch.Tensor:
    """t as the kernels read a row operand: fp32 [rows, cols] with unit column stride (a column
    block of a packed projection output stays a view)."""
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    if t.dim() != 2:
        raise ValueError("expected [rows, channels]")
    return t if t.size(1) == 1 or t.stride(1) == 1 else t.contiguous()


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else t.size(1)


def attn_out_rows(form: AttnForm, q_rows_given: int) -> int:
    return q_rows_given if form.qptr is not None else form.num_sets * form.q_rows


def set_attn_mask_numel(form: AttnForm, heads: int, Mq: int, Mk: int):
    """Elements of the [set][head][query][key] dropout mask, or None when both sides are ragged
    (the size then depends on the set sizes: sum_g heads * n_g^2)."""
    if form.qptr is None and form.kptr is None:
        return form.num_sets * heads * form.q_rows * form.k_rows
    if form.qptr is None:
        return heads * form.q_rows * Mk
    if form.kptr is None:
        return heads * Mq * form.k_rows
    return None


def set_attn_mask_offsets(form: AttnForm, heads: int, dev) -> torch.Tensor:
    """int64 [B + 1]: where each set's [head][query][key] block of the mask starts."""
    moff = torch.empty(form.num_sets + 1, dtype=torch.int64, device=dev)
    _lib.call("lgnn_set_attn_mask_offsets", form.qptr, form.q_rows, form.kptr, form.k_rows,
              form.num_sets, heads, moff, _s(dev))
    return moff


AttnSaved = namedtuple("AttnSaved", "q k v form heads mask moff out lse")


def _attn_args(q, k, v, form: AttnForm, heads: int, mask, moff):
    return (q, _ld(q), k, _ld(k), v, _ld(v), form.qptr, form.q_rows, int(form.q_shared),
            form.kptr, form.k_rows, form.num_sets, heads, q.size(1) // heads, mask, moff)


def set_attn_fwd(q, k, v, form: AttnForm, heads: int, mask=None, moff=None):
    """softmax(q_h k_h^T / sqrt(D)) [* mask] v_h per set and head: (out [rows, C], AttnSaved).
    q, k, v [rows, C] fp32, column blocks of a packed projection allowed."""
    _lib.require_gpu(q, k, v)
    q, k, v = _rows_view(q), _rows_view(k), _rows_view(v)
    C = q.size(1)
    if C % heads or k.size(1) != C or v.size(1) != C:
        raise ValueError("set attention: q, k, v must be [rows, heads * head_dim]")
    set_attn_plan(heads, C // heads)
    dev = q.device
    if mask is not None and moff is None:
        moff = set_attn_mask_offsets(form, heads, dev)
    R = attn_out_rows(form, q.size(0))
    out = torch.empty(R, C, dtype=torch.float32, device=dev)
    lse = torch.empty(R, heads, dtype=torch.float32, device=dev)
    _lib.call("lgnn_set_attn_fwd", *_attn_args(q, k, v, form, heads, mask, moff), out, lse,
              _s(dev))
    return out, AttnSaved(q, k, v, form, heads, mask, moff, out, lse)


def set_attn_bwd(sv: AttnSaved, dout, dq=None, dk=None, dv=None, jobs: list | None = None):
    """(dq, dk, dv); given dq / dk / dv (views with unit column stride, e.g. column blocks of one
    packed gradient) are written in place. Shared queries: the per-set dq rows are summed over the
    sets in fixed order (a reduce_multi job: appended to `jobs`, else run here)."""
    q, k, v, form = sv.q, sv.k, sv.v, sv.form
    dev = q.device
    dout = _f32c(dout)
    C = q.size(1)
    S, B = form.q_rows, form.num_sets
    dq_out = dq if dq is not None else torch.empty(q.size(0), C, dtype=torch.float32, device=dev)
    dk = dk if dk is not None else torch.empty(k.size(0), C, dtype=torch.float32, device=dev)
    dv = dv if dv is not None else torch.empty(v.size(0), C, dtype=torch.float32, device=dev)
    dq_k = torch.empty(B * S, C, dtype=torch.float32, device=dev) if form.q_shared else dq_out
    _lib.call("lgnn_set_attn_bwd", *_attn_args(q, k, v, form, sv.heads, sv.mask, sv.moff),
              sv.out, dout, sv.lse, dq_k, _ld(dq_k), dk, _ld(dk), dv, _ld(dv), _s(dev))
    if form.q_shared:
        if not dq_out.is_contiguous():
            raise ValueError("shared-query dq must be contiguous")
        if B == 0:
            dq_out.zero_()
        else:
            job = [(dq_k, B, S * C, dq_out)]
            if jobs is not None:
                jobs.extend(job)
            else:
                reduce_multi(job, dev)
    return dq_out, dk, dv


class _SetAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, form, heads, mask):
        out, saved = set_attn_fwd(q, k, v, form, heads, mask)
        _save(ctx, saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        return (*set_attn_bwd(_load(ctx), dout), None, None, None)


def set_attention(q, k, v, form: AttnForm, heads: int, mask=None):
    """Segmented multi-head attention as one autograd node (the blocks of conv.py run it inside
    ops.mab, with their projections)."""
    if _compiling():
        return torch.ops.lgnn.set_attn(q, k, v, form.qptr, form.kptr, int(form.q_rows),
                                       bool(form.q_shared), int(form.k_rows), form.num_sets,
                                       int(heads), mask)[0]
    return _SetAttn.apply(q, k, v, form, heads, mask)


NormSaved = namedtuple("NormSaved", "a a_rows b act gamma mean rstd")


def res_norm_fwd(a, a_rows: int, b, act: int, gamma=None, beta=None, eps: float = 1e-5):
    """y = LN(a + act(b)) (a None: LN(act(b)); gamma None: no LayerNorm): (y, NormSaved).
    a_rows > 0: a is [a_rows, C], broadcast over the sets (row r reads a[r % a_rows])."""
    _lib.require_gpu(a, b, gamma)
    b = _f32c(b)
    a = _f32c(a) if a is not None else None
    M, C = b.shape
    dev = b.device
    y = torch.empty_like(b)
    mean = rstd = None
    if gamma is not None:
        gamma, beta = _f32c(gamma), _f32c(beta)
        mean = torch.empty(M, dtype=torch.float32, device=dev)
        rstd = torch.empty(M, dtype=torch.float32, device=dev)
    _lib.call("lgnn_res_norm_fwd", a, int(a_rows), b, int(act), gamma, beta, float(eps), M, C, y,
              mean, rstd, _s(dev))
    return y, NormSaved(a, int(a_rows), b, int(act), gamma, mean, rstd)


def res_norm_bwd(sv: NormSaved, dy, want_da: bool = True, want_db: bool = True,
                 jobs: list | None = None):
    """(da, db, dgamma, dbeta), None where not asked for / absent. da of a broadcast a and the
    affine gradients are fixed-order sums (reduce_multi jobs: appended to `jobs`, else run)."""
    dy = _f32c(dy)
    M, C = sv.b.shape
    dev = sv.b.device
    want_da = want_da and sv.a is not None
    da_rows = torch.empty(M, C, dtype=torch.float32, device=dev) if want_da else None
    db = torch.empty(M, C, dtype=torch.float32, device=dev) if want_db else None
    P = _lib.load().lgnn_res_norm_bwd_partials(M)
    part = torch.empty(P * 2 * C, dtype=torch.float32, device=dev) \
        if sv.gamma is not None else None
    _lib.call("lgnn_res_norm_bwd", sv.a, sv.a_rows, sv.b, sv.act, sv.gamma, M, C, sv.mean,
              sv.rstd, dy, da_rows, db, part, P, _s(dev))
    local = []
    da = da_rows
    if want_da and sv.a_rows > 0:
        da = torch.empty(sv.a_rows, C, dtype=torch.float32, device=dev)
        if M == 0:
            da.zero_()
        else:
            local.append((da_rows, M // sv.a_rows, sv.a_rows * C, da))
    dgamma = dbeta = None
    if part is not None:
        dgamma = torch.empty(C, dtype=torch.float32, device=dev)
        dbeta = torch.empty(C, dtype=torch.float32, device=dev)
        local += [(part[:P * C], P, C, dgamma), (part[P * C:], P, C, dbeta)]
    if jobs is not None:
        jobs.extend(local)
    else:
        reduce_multi(local, dev)
    return da, db, dgamma, dbeta


class _ResNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, act, gamma, beta, a_rows, eps):
        y, saved = res_norm_fwd(a, a_rows, b, act, gamma, beta, eps)
        _save(ctx, saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        need = ctx.needs_input_grad
        da, db, dg, dbt = res_norm_bwd(_load(ctx), dy, need[0], need[1])
        return da, db, None, dg, dbt, None, None


def res_norm(a, b, act: int = _lib.LGNN_ACT_NONE, gamma=None, beta=None, a_rows: int = 0,
             eps: float = 1e-5):
    """y = LN(a + act(b)); a None: LN(act(b)); gamma None: no LayerNorm."""
    if _compiling():
        return torch.ops.lgnn.res_norm(a, b, int(act), gamma, beta, int(a_rows), float(eps))[0]
    return _ResNorm.apply(a, b, act, gamma, beta, a_rows, eps)


def set_readout_fwd(x, gptr, num_sets: int, rows: int, mean: bool):
    _lib.require_gpu(x)
    x = _f32c(x)
    C = x.size(1)
    out = torch.empty(num_sets, C if mean else rows * C, dtype=torch.float32, device=x.device)
    _lib.call("lgnn_set_readout_fwd", x, gptr, num_sets, int(rows), C, int(mean), out,
              _s(x.device))
    return out


def set_readout_bwd(dout, gptr, num_sets: int, rows: int, C: int, mean: bool):
    dout = _f32c(dout)
    dx = torch.empty(num_sets * rows, C, dtype=torch.float32, device=dout.device)
    _lib.call("lgnn_set_readout_bwd", dout, gptr, num_sets, int(rows), C, int(mean), dx,
              _s(dout.device))
    return dx


class _SetReadout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gptr, num_sets, rows, mean):
        ctx.gptr, ctx.meta = gptr, (num_sets, rows, x.size(1), mean)
        return set_readout_fwd(x, gptr, num_sets, rows, mean)

    @staticmethod
    def backward(ctx, dout):
        return set_readout_bwd(dout, ctx.gptr, *ctx.meta), None, None, None, None


def set_readout(x, gptr, num_sets: int, rows: int, mean: bool):
    """[num_sets * rows, C] -> [num_sets, C] (mean over a set's rows) or [num_sets, rows * C];
    with gptr (the input sets' offsets) the rows of an empty set are zero."""
    if _compiling():
        return torch.ops.lgnn.set_readout(x, gptr, num_sets, int(rows), bool(mean))
    return _SetReadout.apply(x, gptr, num_sets, rows, mean)


def _add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a + b on lgnn_add (two gradient paths meeting at a block's input)."""
    y = torch.empty_like(a)
    _lib.call("lgnn_add", a, b, y, a.numel(), _s(a.device))
    return y


def _mab_lin_fwd(x, W, b):
    """x W^T + b on the existing linears, chosen as linear_auto chooses: the tile kernels where
    the shape is theirs, else the split-3 dense GEMM (any M >= 0, any width)."""
    if fast_shape(W.size(1), W.size(0)):
        return linear_fwd(x, W, b, _lib.LGNN_ACT_NONE)
    return dense_mm(x, dense_planes(W, False, False), W.size(0), b, False)


def _mab_lin_bwd(x, W, dy, want_dx: bool, jobs: list, copies: list, dW_out=None, db_out=None):
    """(dx or None, dW, db) of _mab_lin_fwd; the slab reductions go to `jobs`, retargeted at
    dW_out / db_out (row blocks of in_proj_weight.grad / in_proj_bias.grad) when given."""
    N, K = W.shape
    local: list = []
    if fast_shape(K, N):
        dx, dW, db = linear_bwd(_lib.LGNN_GRAD_DIRECT, dy, H=None, act=_lib.LGNN_ACT_NONE, X=x,
                                W=W, want_dx=want_dx, want_db=True, reducer=local)
    else:
        dW, db = dense_wgrad(dy, x, False, want_db=True, reducer=local)
        dx = dense_mm(dy, dense_planes(W, True, False), K, None, False) if want_dx else None
    if dW_out is not None:
        if local[0][3].shape == dW_out.shape:  # the reduction writes the row block itself
            local = [(*local[0][:3], dW_out), (*local[1][:3], db_out)]
        else:  # an odd width the GEMM padded: copied after the reduction
            copies += [(dW_out, dW), (db_out, db)]
        dW, db = dW_out, db_out
    jobs.extend(local)
    return dx, dW, db


# params: [in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, lin.weight, lin.bias,
# layer_norm1.weight, layer_norm1.bias, layer_norm2.weight, layer_norm2.bias] (the last four None
# without LayerNorm). y None: self attention (mab(x, x): one packed q/k/v projection).
MAB_SAVED = ("proj", "kv", "o", "lse", "a", "mean1", "rstd1", "u1", "t", "mean2", "rstd2", "moff")
MabSaved = namedtuple("MabSaved", ("x", "y", "params", "form", "heads", "mask") + MAB_SAVED)


def mab_fwd(x, y, params: list, form: AttnForm, heads: int, mask=None):
    """PyG 2.5.1 MultiheadAttentionBlock.forward(x, y) on ragged sets: (out, MabSaved)."""
    _lib.require_gpu(x, y, params[0])
    x = _f32c(x)
    y = _f32c(y) if y is not None else None
    params = [_f32c(p) if p is not None else None for p in params]
    Win, bin_, Wo, bo, Wl, bl, g1, b1, g2, b2 = params
    C = Win.size(1)
    set_attn_plan(heads, C // heads)
    if y is None:
        proj, kv = _mab_lin_fwd(x, Win, bin_), None
        q, k, v = proj[:, :C], proj[:, C:2 * C], proj[:, 2 * C:]
    else:
        proj = _mab_lin_fwd(x, Win[:C], bin_[:C])
        kv = _mab_lin_fwd(y, Win[C:], bin_[C:])
        q, k, v = proj, kv[:, :C], kv[:, C:]
    o, asv = set_attn_fwd(q, k, v, form, heads, mask)
    a = _mab_lin_fwd(o, Wo, bo)
    u1, n1 = res_norm_fwd(x, form.q_rows if form.q_shared else 0, a, _lib.LGNN_ACT_NONE, g1, b1)
    t = _mab_lin_fwd(u1, Wl, bl)
    u2, n2 = res_norm_fwd(u1, 0, t, _lib.LGNN_ACT_RELU, g2, b2)
    return u2, MabSaved(x, y, params, form, heads, mask, proj, kv, o, asv.lse, a, n1.mean,
                        n1.rstd, u1, t, n2.mean, n2.rstd, asv.moff)


def mab_bwd(sv: MabSaved, dout, want_dx: bool = True, want_dy: bool = True):
    """(dx or None, dy or None, [the gradients of params, None where the parameter is None])."""
    x, y, form, heads = sv.x, sv.y, sv.form, sv.heads
    Win, bin_, Wo, bo, Wl, bl, g1, b1, g2, b2 = sv.params
    C = Win.size(1)
    dev = x.device
    jobs: list = []
    copies: list = []
    n2 = NormSaved(sv.u1, 0, sv.t, _lib.LGNN_ACT_RELU, g2, sv.mean2, sv.rstd2)
    du1_res, dt, dg2, db2 = res_norm_bwd(n2, dout, True, True, jobs)
    du1_lin, dWl, dbl = _mab_lin_bwd(sv.u1, Wl, dt, True, jobs, copies)
    du1 = _add(du1_res, du1_lin)
    n1 = NormSaved(x, form.q_rows if form.q_shared else 0, sv.a, _lib.LGNN_ACT_NONE, g1, sv.mean1,
                   sv.rstd1)
    dx_res, da, dg1, db1 = res_norm_bwd(n1, du1, want_dx, True, jobs)
    do, dWo, dbo = _mab_lin_bwd(sv.o, Wo, da, True, jobs, copies)
    dWin = torch.empty_like(Win)
    dbin = torch.empty_like(bin_)
    if y is None:
        q, k, v = sv.proj[:, :C], sv.proj[:, C:2 * C], sv.proj[:, 2 * C:]
        dproj = torch.empty_like(sv.proj)
        dq, dk, dv = dproj[:, :C], dproj[:, C:2 * C], dproj[:, 2 * C:]
    else:
        q, k, v = sv.proj, sv.kv[:, :C], sv.kv[:, C:]
        dproj, dkv = torch.empty_like(sv.proj), torch.empty_like(sv.kv)
        dq, dk, dv = dproj, dkv[:, :C], dkv[:, C:]
    asv = AttnSaved(q, k, v, form, heads, sv.mask, sv.moff, sv.o, sv.lse)
    set_attn_bwd(asv, do, dq, dk, dv, jobs)
    if form.q_shared and jobs and jobs[-1][3] is dq:
        # the q projection's backward reads the summed dq: run what is queued so far
        reduce_multi(jobs, dev)
        jobs = []
    dy = None
    if y is None:
        dx_lin, _, _ = _mab_lin_bwd(x, Win, dproj, want_dx, jobs, copies, dWin, dbin)
    else:
        dx_lin, _, _ = _mab_lin_bwd(x, Win[:C], dproj, want_dx, jobs, copies, dWin[:C], dbin[:C])
        dy, _, _ = _mab_lin_bwd(y, Win[C:], dkv, want_dy, jobs, copies, dWin[C:], dbin[C:])
    reduce_multi(jobs, dev)
    for dst, src in copies:
        dst.copy_(src)
    dx = _add(dx_res, dx_lin) if want_dx else None
    return dx, dy, [dWin, dbin, dWo, dbo, dWl, dbl, dg1, db1, dg2, db2]


class _Mab(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, form, heads, mask, *params):
        out, saved = mab_fwd(x, y, list(params), form, heads, mask)
        _save(ctx, saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        need = ctx.needs_input_grad
        dx, dy, dps = mab_bwd(_load(ctx), dout, need[0], need[1])
        return (dx, dy, None, None, None, *dps)


def mab(x, y, params: list, form: AttnForm, heads: int, mask=None):
    """MultiheadAttentionBlock(x, y) as ONE autograd node: the q / k / v projections (one packed
    GEMM when y is None, i.e. y is x), the segmented attention, out_proj, the residuals, the ReLU
    Linear and both LayerNorms. in_proj_weight's gradient comes out as one [3C, C] tensor."""
    if _compiling():
        return torch.ops.lgnn.mab(x, y, list(params[:6]), list(params[6:]) if params[6] is not None
                                  else [], form.qptr, form.kptr, int(form.q_rows),
                                  bool(form.q_shared), int(form.k_rows), form.num_sets,
                                  int(heads), mask)[0]
    return _Mab.apply(x, y, form, heads, mask, *params)


def isab_forms(ptr, rows: int, m: int, num_sets: int):
    """The two attention forms of an InducedSetAttentionBlock over sets laid out by (ptr | rows):
    the m inducing rows query each set; each set's rows query its m induced rows."""
    return (AttnForm(None, m, True, ptr, rows, num_sets),
            AttnForm(ptr, rows, False, None, m, num_sets))


def isab_fwd(x, ind, params1: list, params2: list, ptr, rows: int, num_sets: int, heads: int,
             mask1=None, mask2=None):
    """PyG InducedSetAttentionBlock: mab2(x, mab1(ind, x)): (out, (MabSaved, MabSaved))."""
    f1, f2 = isab_forms(ptr, rows, ind.size(0), num_sets)
    h, sv1 = mab_fwd(ind, x, params1, f1, heads, mask1)
    out, sv2 = mab_fwd(x, h, params2, f2, heads, mask2)
    return out, (sv1, sv2)


def isab_bwd(svs, dout, want_dx: bool = True):
    """(dx or None, dind, grads of params1, grads of params2). x feeds both blocks (mab1's keys,
    mab2's queries): its two gradients meet in lgnn_add."""
    sv1, sv2 = svs
    dx2, dh, dps2 = mab_bwd(sv2, dout, want_dx, True)
    dind, dx1, dps1 = mab_bwd(sv1, dh, True, want_dx)
    return (_add(dx2, dx1) if want_dx else None), dind, dps1, dps2


class _Isab(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ind, ptr, rows, num_sets, heads, mask1, mask2, *params):
        out, saved = isab_fwd(x, ind, list(params[:10]), list(params[10:]), ptr, rows, num_sets,
                              heads, mask1, mask2)
        _save(ctx, saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        dx, dind, dps1, dps2 = isab_bwd(_load(ctx), dout, ctx.needs_input_grad[0])
        return (dx, dind, None, None, None, None, None, None, *dps1, *dps2)


def isab(x, ind, params1: list, params2: list, ptr, rows: int, num_sets: int, heads: int,
         mask1=None, mask2=None):
    """InducedSetAttentionBlock as ONE autograd node (x is read by both of its attention blocks;
    inside one node the two input gradients are summed by a HIP kernel)."""
    if _compiling():
        ln = params1[6] is not None
        return torch.ops.lgnn.isab(x, ind, list(params1[:6]) + list(params2[:6]),
                                   (list(params1[6:]) + list(params2[6:])) if ln else [], ptr,
                                   int(rows), num_sets, int(heads), mask1, mask2)[0]
    return _Isab.apply(x, ind, ptr, rows, num_sets, heads, mask1, mask2, *params1, *params2)


# ----------------------------------------------------------------------------------------------
# PointNet++ (cluster.py builds the PairGraph): the split first Linear of PointNetConv's per-edge
# MLP, BatchNorm + activation over rows, the max aggregation. Eager only (data-dependent shapes).
# ----------------------------------------------------------------------------------------------


def segment_sum(X, ptr, perm, S: int, sign: float) -> torch.Tensor:
    """out [S, C] = sign * the sum of X's rows perm[ptr[s] .. ptr[s+1]) (perm None: the rows
    themselves), ascending."""
    out = torch.empty(S, X.size(1), dtype=torch.float32, device=X.device)
    _lib.call("lgnn_segment_sum", X, ptr, perm, S, X.size(1), float(sign), out, _s(X.device))
    return out


class _EdgeSub(torch.autograd.Function):
    """(Z, sums) = (U[col] - V[row], Z's fp64 column sums (sum z, sum z^2)); backward: dU and dV
    as segment sums of dZ (no atomics)."""

    @staticmethod
    def forward(ctx, U, V, pg):
        _lib.require_gpu(U, V)
        U, V = _f32c(U), _f32c(V)
        E, C = pg.num_pairs, U.size(1)
        if U.size(0) != pg.num_candidates or V.size(0) != pg.num_queries or V.size(1) != C:
            raise ValueError("edge_sub: U [candidates, C] and V [queries, C] expected")
        Z = torch.empty(E, C, dtype=torch.float32, device=U.device)
        sums = torch.empty(2 * C, dtype=torch.float64, device=U.device)
        ws = _bn_ws(E, C, U.device)
        _lib.call("lgnn_edge_sub_fwd", U, V, pg.row, pg.col, E, C, Z, sums, ws, ws.numel(),
                  _s(U.device))
        ctx.pg = pg
        ctx.mark_non_differentiable(sums)
        return Z, sums

    @staticmethod
    def backward(ctx, dZ, _):
        pg = ctx.pg
        dZ = _f32c(dZ)
        dU = dV = None
        if ctx.needs_input_grad[0]:
            tptr, perm = pg.transpose()
            dU = segment_sum(dZ, tptr, perm, pg.num_candidates, 1.0)
        if ctx.needs_input_grad[1]:
            dV = segment_sum(dZ, pg.rowoff, None, pg.num_queries, -1.0)
        return dU, dV, None


def edge_sub(U, V, pg):
    return _EdgeSub.apply(U, V, pg)


class _BnAct(torch.autograd.Function):
    """A = act(BatchNorm(Z)) [* mask] over rows (torch.nn.BatchNorm1d semantics; bn None: no
    norm, A = act(Z) [* mask]). sums: Z's column sums when its producer formed them."""

    @staticmethod
    def forward(ctx, Z, gamma, beta, bn, training, act, mask, sums):
        _lib.require_gpu(Z)
        Z = _f32c(Z)
        M, N = Z.shape
        dev = Z.device
        if bn is None:
            scale = torch.ones(N, dtype=torch.float32, device=dev)
            shift = torch.zeros(N, dtype=torch.float32, device=dev)
            mean = invstd = scale
            training = False
        else:
            if training and M == 0:
                raise ValueError("BatchNorm in training mode needs at least one row")
            if training and sums is None:
                sums = bn_stats(Z)
            mean, invstd, scale, shift = bn_finalize(sums, float(M), bn, training, N, dev)
        A = torch.empty_like(Z)
        _lib.call("lgnn_bn_act_a", Z, M, N, scale, shift, mask, int(act), A, _s(dev))
        ctx.save_for_backward(Z, scale, shift, mean, invstd, mask)
        ctx.meta = (bn is not None, bool(training), int(act))
        return A

    @staticmethod
    def backward(ctx, dA):
        Z, scale, shift, mean, invstd, mask = ctx.saved_tensors
        has_bn, training, act = ctx.meta
        dA = _f32c(dA)
        M, N = Z.shape
        dev = Z.device
        dg = db = None
        if has_bn:
            sums = torch.empty(2 * N, dtype=torch.float64, device=dev)
            ws = _bn_ws(M, N, dev)
            _lib.call("lgnn_bn_bwd_stats_a", dA, Z, mask, M, N, scale, shift, mean, invstd, act,
                      sums, ws, ws.numel(), _s(dev))
            if ctx.needs_input_grad[1]:
                dg = torch.empty(N, dtype=torch.float32, device=dev)
                db = torch.empty(N, dtype=torch.float32, device=dev)
        else:
            sums = torch.zeros(2 * N, dtype=torch.float64, device=dev)  # not read (eval form)
        dZ = torch.empty_like(Z)
        _lib.call("lgnn_bn_bwd_apply_a", dA, Z, mask, M, N, scale, shift, mean, invstd, act, sums,
                  float(max(M, 1)), int(training), dZ, dg, db, _s(dev))
        return dZ, dg, db, None, None, None, None, None


def bn_act_rows(Z, bn, training: bool, act: int, mask=None, sums=None):
    """act(bn(Z)) [* mask]; bn a torch.nn.BatchNorm1d (affine) or None."""
    gamma, beta = (bn.weight, bn.bias) if bn is not None else (None, None)
    return _BnAct.apply(Z, gamma, beta, bn, training, act, mask, sums)


class _SegmentMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, ptr, S):
        _lib.require_gpu(X, ptr)
        X = _f32c(X)
        C = X.size(1)
        out = torch.empty(S, C, dtype=torch.float32, device=X.device)
        arg = torch.empty(S, C, dtype=torch.int32, device=X.device)
        _lib.call("lgnn_segment_max_fwd", X, ptr, S, C, out, arg, _s(X.device))
        ctx.save_for_backward(arg, ptr)
        ctx.rows = X.size(0)
        return out

    @staticmethod
    def backward(ctx, dout):
        arg, ptr = ctx.saved_tensors
        S, C = arg.shape
        dX = torch.empty(ctx.rows, C, dtype=torch.float32, device=dout.device)
        _lib.call("lgnn_segment_max_bwd", _f32c(dout), arg, ptr, S, C, dX, _s(dout.device))
        return dX, None, None


def segment_max(X, ptr, num_segments: int):
    """out [S, C] = the max over each segment's rows (ptr int64 [S + 1], the segments tiling X's
    rows in order); 0 for an empty segment. The gradient goes to the lowest row that gave it."""
    if ptr.dtype != torch.int64 or ptr.numel() != num_segments + 1:
        raise ValueError("segment_max: ptr must be int64 [num_segments + 1]")
    return _SegmentMax.apply(X, ptr, int(num_segments))
