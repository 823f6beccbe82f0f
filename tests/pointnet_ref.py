"""Float64 restatement of PointNet++ as the reference model composes it (PyG 2.5.1 MLP,
PointNetConv(aggr='max'), global_max_pool; torch_cluster 1.6.3 fps and radius), written from the
operator definitions: plain concatenation, the first Linear applied per edge, loops over graphs
and centroids. Test infrastructure for the HIP path; its modules' state_dict() carries the
reference's keys.

    fps:     first pick ptr[g] + start[g]; d[i] = min(d[i], |p_i - p_pick|^2); next = argmax d,
             lowest index on ties; m_g = ceil(fp32(n_g) * fp32(ratio)).
    radius:  per query, the candidates of its graph in index order with |y - x|^2 < r^2, the first
             max_num_neighbors of them.
    conv:    out_i = max_j nn(cat[x_j, pos_j - pos_i]); 0 for a centroid without neighbours.
"""
from __future__ import annotations

import torch
import torch.nn as nn


def sqdist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """|a_i - b_j|^2 [len(a), len(b)] in float64: dx*dx + dy*dy (+ dz*dz), left to right."""
    d = a.double()[:, None, :] - b.double()[None, :, :]
    s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    if a.size(1) == 3:
        s = s + d[..., 2] * d[..., 2]
    return s


def fps_counts(sizes: list[int], ratio: float) -> list[int]:
    n = torch.tensor(sizes, dtype=torch.float32)
    return torch.ceil(n * torch.tensor(ratio, dtype=torch.float32)).long().tolist()


def offsets(sizes: list[int]) -> list[int]:
    out = [0]
    for s in sizes:
        out.append(out[-1] + s)
    return out


def fps(pos: torch.Tensor, sizes: list[int], counts: list[int], start: list[int]) -> torch.Tensor:
    """Global indices of counts[g] picks per graph, in selection order."""
    out, off = [], offsets(sizes)
    for g, (n, m) in enumerate(zip(sizes, counts)):
        if n == 0 or m == 0:
            continue
        p = pos[off[g]:off[g] + n].double()
        d = torch.full((n,), float("inf"), dtype=torch.float64)
        pick = int(start[g])
        for j in range(m):
            out.append(off[g] + pick)
            if j + 1 == m:
                break
            d = torch.minimum(d, sqdist(p, p[pick:pick + 1])[:, 0])
            pick = int(torch.nonzero(d == d.max())[0, 0])  # lowest index among the farthest
    return torch.tensor(out, dtype=torch.int64)


def radius(x: torch.Tensor, y: torch.Tensor, r: float, sizes_x: list[int], sizes_y: list[int],
           max_num_neighbors: int = 32) -> torch.Tensor:
    """[2, E] = (query index into y, candidate index into x), grouped by query, candidates
    ascending."""
    ox, oy = offsets(sizes_x), offsets(sizes_y)
    rows, cols = [], []
    for g, (nx, ny) in enumerate(zip(sizes_x, sizes_y)):
        if nx == 0 or ny == 0:
            continue
        near = sqdist(y[oy[g]:oy[g] + ny], x[ox[g]:ox[g] + nx]) < float(r) * float(r)
        near &= near.cumsum(1) <= max_num_neighbors
        i, j = torch.nonzero(near, as_tuple=True)  # row-major: by query, candidates ascending
        rows.append(i + oy[g])
        cols.append(j + ox[g])
    if not rows:
        return torch.empty(2, 0, dtype=torch.int64)
    return torch.stack([torch.cat(rows), torch.cat(cols)])


def row_offsets(row: torch.Tensor, num_rows: int) -> torch.Tensor:
    return torch.searchsorted(row.contiguous(), torch.arange(num_rows + 1))


def segment_max(x: torch.Tensor, ptr: list[int] | torch.Tensor) -> torch.Tensor:
    """Max over each segment's rows; zeros for an empty segment."""
    ptr = [int(v) for v in ptr]
    out = []
    for a, b in zip(ptr[:-1], ptr[1:]):
        out.append(x[a:b].max(0).values if b > a else x.new_zeros(x.size(1)))
    return torch.stack(out) if out else x.new_zeros(0, x.size(1))


def top2_gap(x: torch.Tensor, ptr: list[int] | torch.Tensor) -> float:
    """The smallest gap between the largest and second largest entry of a (segment, column),
    over the segments of at least two rows: how far the inputs are from an argmax tie."""
    ptr = [int(v) for v in ptr]
    gap = float("inf")
    for a, b in zip(ptr[:-1], ptr[1:]):
        if b - a >= 2:
            top = x[a:b].detach().topk(2, dim=0).values
            gap = min(gap, (top[0] - top[1]).min().item())
    return gap


class Norm(nn.Module):
    """torch_geometric.nn.norm.BatchNorm: keys `module.*`."""

    def __init__(self, channels: int):
        super().__init__()
        self.module = nn.BatchNorm1d(channels)

    def forward(self, x):
        return self.module(x)


class MLP(nn.Module):
    """PyG MLP(channel_list, dropout, act='relu', norm='batch_norm' | None, plain_last=True)."""

    def __init__(self, channel_list: list[int], dropout: float = 0.0,
                 norm: str | None = "batch_norm"):
        super().__init__()
        self.p = dropout
        self.lins = nn.ModuleList([nn.Linear(a, b) for a, b in
                                   zip(channel_list[:-1], channel_list[1:])])
        self.norms = nn.ModuleList([Norm(c) if norm else nn.Identity()
                                    for c in channel_list[1:-1]])

    def forward(self, x, masks=None):
        """masks: the step's dropout keep-masks per hidden layer (training with p > 0)."""
        for i, (lin, norm) in enumerate(zip(self.lins[:-1], self.norms)):
            x = torch.relu(norm(lin(x)))
            if masks is not None and self.training and self.p > 0.0:
                x = x * masks[i].view_as(x).to(x.dtype)
        return self.lins[-1](x)


class PointNetConv(nn.Module):
    def __init__(self, local_nn: MLP):
        super().__init__()
        self.local_nn = local_nn

    def messages(self, x, pos, pos_dst, pairs):
        row, col = pairs
        return self.local_nn(torch.cat([x[col], pos[col] - pos_dst[row]], dim=1))

    def forward(self, x, pos, pos_dst, pairs):
        msg = self.messages(x, pos, pos_dst, pairs)
        return segment_max(msg, row_offsets(pairs[0], pos_dst.size(0)))


class SAModule(nn.Module):
    def __init__(self, ratio: float, radius: float, nn_: MLP):
        super().__init__()
        self.ratio, self.r = ratio, radius
        self.conv = PointNetConv(nn_)

    def sample(self, pos, sizes, start=None):
        """(idx, pairs, centroid counts) of this level for fp32-rounded positions."""
        counts = fps_counts(sizes, self.ratio)
        p = pos.float().double()
        idx = fps(p, sizes, counts, start if start is not None else [0] * len(sizes))
        return idx, radius(p, p[idx], self.r, sizes, counts, 64), counts

    def forward(self, x, pos, sizes, start=None):
        pos = pos.float().to(x.dtype)  # the reference's pos.to(x.dtype) on fp32 features
        idx, pairs, counts = self.sample(pos, sizes, start)
        return self.conv(x, pos, pos[idx], pairs), pos[idx], counts


class GlobalSAModule(nn.Module):
    def __init__(self, nn_: MLP):
        super().__init__()
        self.nn = nn_

    def forward(self, x, pos, sizes):
        return segment_max(self.nn(torch.cat([x, pos], dim=1)), offsets(sizes))


class PointNet(nn.Module):
    def __init__(self, input_features: int, pos_dim: int, num_classes: int):
        super().__init__()
        self.sa1_module = SAModule(0.5, 0.2, MLP([input_features + pos_dim, 64, 64, 128]))
        self.sa2_module = SAModule(0.25, 0.4, MLP([128 + pos_dim, 128, 128, 256]))
        self.sa3_module = GlobalSAModule(MLP([256 + pos_dim, 256, 512, 1024]))
        self.mlp = MLP([1024, 512, 256, num_classes], dropout=0.5, norm=None)

    def forward(self, x, pos, sizes, masks=None):
        """FPS starts at each graph's first point (SAModule.random_start = False)."""
        x, pos, sizes = self.sa1_module(x, pos, sizes)
        x, pos, sizes = self.sa2_module(x, pos, sizes)
        x = self.sa3_module(x, pos, sizes)
        return self.mlp(x, masks).log_softmax(dim=-1)


def randomize_(module: nn.Module, seed: int = 0, scale: float = 0.3) -> None:
    """Non-trivial values for every parameter and BatchNorm statistic (the defaults — zero
    biases, unit affine, zero / unit running statistics — would hide a swapped or dropped
    term)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            fan_in = p.size(1) if p.dim() == 2 else 1
            s = scale if p.dim() == 1 else 1.0 / fan_in ** 0.5
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64).to(p.dtype) * s)
            if name.endswith("module.weight"):
                p.add_(1.0)
        for name, b in module.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g, dtype=torch.float64).to(b.dtype) * scale)
            if name.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g, dtype=torch.float64).to(b.dtype) + 0.5)
