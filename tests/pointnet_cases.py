"""Shared inputs and bars of the PointNet++ tests (CPU reference test and GPU tests).

Bars: those of tests/set_transformer_cases.py (outputs within 1e-4 absolute at unit-scale inputs;
each gradient within 1e-4 x max|grad| of its tensor, with the 5e-6 floor — every bias feeding a
BatchNorm has an analytically zero gradient, so the floor is what bounds it).

A max over neighbours is discontinuous in its argmax, so the inputs must stay clear of ties: for
every (centroid, channel) and (graph, channel) the float64 restatement's top-two gap is at least
GAP = 1e-5, ten times the fp32 path's output error (~1e-6). tests/test_pointnet_ref.py asserts it
on the CPU for every case below; the seeds here were chosen to pass it.
"""
from __future__ import annotations

import torch

from lesion_gnn_amd import _lib, synth
from tests import pointnet_ref as ref
from tests.set_transformer_cases import (GRAD_FLOOR, GRAD_RTOL, OUT_ATOL,  # noqa: F401
                                         assert_grad, assert_output)

GAP = 1e-5

# PointNetConv: one set-abstraction level (ratio 0.5, r 0.2) over graphs of these sizes
CONV_SIZES = [1, 2, 5, 64, 65, 130, 3, 40]
CONV_RATIO, CONV_R = 0.5, 0.2
CONV_WIDTHS = [64, 64, 128]
CONV_SEEDS = {37: 15, 128: 12}  # c_in -> seed of the inputs and the weights

# geometry: graph sizes of the FPS test (the on-chip capacity and one above it last) and of the
# radius test (a 200-node graph, where the cap of 64 binds at r = 0.4; an empty graph)
FPS_SIZES = [1, 0, 2, 3, 63, 64, 65, 255, 257, _lib.LGNN_FPS_CAPACITY + 1]
GEOMETRY_SIZES = [200, 0, 3, 65, 1, 130]
GEOMETRY_SEED = 7

MODEL_KW = dict(input_features=37, pos_dim=2, num_classes=5)
MODEL_SEED = 23
MODEL_LR, MODEL_WD = 1e-3, 0.01  # OptimizerConfig's defaults with Adam


def points(sizes: list[int], dims: int, seed: int) -> torch.Tensor:
    """fp64 positions in the unit square / cube, fp32-representable (what pos.to(x.dtype)
    leaves)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(sum(sizes), dims, generator=g, dtype=torch.float64).float().double()


def batch_of(sizes: list[int]) -> torch.Tensor:
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def device_sets(sizes: list[int], dev):
    """The cluster.Sets of graphs of these sizes (offsets on `dev`, sizes on the host)."""
    from lesion_gnn_amd import cluster

    ptr = torch.tensor(ref.offsets(sizes), dtype=torch.int32, device=dev)
    return cluster.Sets(ptr, torch.tensor(sizes, dtype=torch.int64), len(sizes))


def poison(dev) -> None:
    """Fill what the caching allocator hands out next with NaN: a large and many small blocks,
    written and freed. A kernel that reads a row nobody wrote then computes NaN."""
    torch.cuda.synchronize()
    blocks = [torch.full((32 << 20,), float("nan"), device=dev)]
    blocks += [torch.full((n,), float("nan"), device=dev) for n in (1 << 8, 1 << 12, 1 << 16)
               for _ in range(32)]
    torch.cuda.synchronize()
    del blocks


def conv_case(c_in: int):
    """(reference SAModule in float64, x [N, c_in] float64, pos [N, 2] float64, sizes)."""
    seed = CONV_SEEDS[c_in]
    g = torch.Generator().manual_seed(seed)
    N = sum(CONV_SIZES)
    x = torch.randn(N, c_in, generator=g, dtype=torch.float64).float().double()
    pos = points(CONV_SIZES, 2, seed + 100)
    theirs = ref.SAModule(CONV_RATIO, CONV_R, ref.MLP([c_in + 2] + CONV_WIDTHS)).double()
    ref.randomize_(theirs, seed)
    return theirs, x, pos, list(CONV_SIZES)


def conv_gap(theirs: ref.SAModule, x, pos, sizes) -> float:
    """The top-two gap of the level's messages, in the module's current train / eval mode (its
    running statistics are left as they were)."""
    state = {k: v.clone() for k, v in theirs.state_dict().items()}
    pos = pos.float().double()
    idx, pairs, _ = theirs.sample(pos, sizes)
    with torch.no_grad():
        msg = theirs.conv.messages(x, pos, pos[idx], pairs)
    theirs.load_state_dict(state)
    return ref.top2_gap(msg, ref.row_offsets(pairs[0], idx.numel()))


def model_batch():
    """(synth batch, sizes): 12 log-normal graphs, one above 32 nodes and one without nodes."""
    sizes = synth.graph_sizes(12, "lognormal", torch.Generator().manual_seed(5))
    sizes = [min(s, 30) for s in sizes]
    sizes[7] = 41
    sizes[3] = 0
    b = synth.make_batch(12, k=2, d_in=MODEL_KW["input_features"], seed=3, sizes=sizes)
    return b, sizes


def reference_model(num_classes: int | None = None) -> ref.PointNet:
    kw = dict(MODEL_KW, num_classes=num_classes or MODEL_KW["num_classes"])
    theirs = ref.PointNet(**kw).double()
    ref.randomize_(theirs, MODEL_SEED)
    return theirs


def model_gaps(theirs: ref.PointNet, x, pos, sizes) -> dict:
    """The top-two gaps at the model's three max aggregations, in its current mode (running
    statistics left as they were)."""
    state = {k: v.clone() for k, v in theirs.state_dict().items()}
    gaps = {}
    with torch.no_grad():
        for name in ("sa1_module", "sa2_module"):
            sa = getattr(theirs, name)
            pos = pos.float().double()
            idx, pairs, counts = sa.sample(pos, sizes)
            msg = sa.conv.messages(x, pos, pos[idx], pairs)
            ptr = ref.row_offsets(pairs[0], idx.numel())
            gaps[name] = ref.top2_gap(msg, ptr)
            x, pos, sizes = ref.segment_max(msg, ptr), pos[idx], counts
        h = theirs.sa3_module.nn(torch.cat([x, pos], dim=1))
        gaps["sa3_module"] = ref.top2_gap(h, ref.offsets(sizes))
    theirs.load_state_dict(state)
    return gaps
