"""Point-set geometry of PointNet++ on the GPU: farthest point sampling and the bipartite radius
search (liblgnn `lgnn_fps`, `lgnn_radius_pairs_count` / `lgnn_radius_pairs`,
`lgnn_pairs_transpose`).

`fps` / `radius` mirror `torch_cluster.fps(src, batch, ratio, random_start)` and
`torch_cluster.radius(x, y, r, batch_x, batch_y, max_num_neighbors)` (1.6.3) as the reference's
SAModule calls them (src/lesion_gnn/models/pointnet.py): whole batches in one launch each,
selections bit-exact against a float64 restatement (squared distances in fp64; fp32 positions
widen exactly). The neighbour choice when more than max_num_neighbors candidates are in range is
torch_cluster's CUDA one (the first in index order), as `knn.radius_graph`.

`Sets` is the host + device description of how a batch's rows split into graphs; a model reads the
graph sizes once and derives every sampling level's counts and offsets from them on the host
(`sampled`), so FPS needs no host read of its own. `PairGraph` is what the radius search returns
to PointNetConv: the pairs, their row offsets and (built on first use, for the backward) the
candidate-grouped permutation.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from .knn import _batch_ptr


class Sets(NamedTuple):
    ptr: torch.Tensor    # int32 [B + 1], device: row offsets of the graphs
    sizes: torch.Tensor  # int64 [B], host
    num_graphs: int

    @property
    def total(self) -> int:
        return int(self.sizes.sum())


def sets_of(rows: torch.Tensor, batch: torch.Tensor | None, num_graphs: int | None) -> Sets:
    """The graphs of `rows` by the sorted `batch` vector. One host read (the graph sizes); a
    second (batch's last entry) when num_graphs is not given."""
    _, ptr, B = _batch_ptr(rows, batch, num_graphs)
    return Sets(ptr, (ptr[1:] - ptr[:-1]).to(torch.int64).cpu(), B)


def fps_counts(sizes: torch.Tensor, ratio: float) -> torch.Tensor:
    """torch_cluster's sample counts for fp32 points: ceil(fp32(n_g) * fp32(ratio))."""
    return torch.ceil(sizes.to(torch.float32) * torch.tensor(ratio, dtype=torch.float32)).long()


def sampled(sets: Sets, ratio: float) -> Sets:
    """The graphs of the rows FPS keeps at `ratio` (host arithmetic and one upload)."""
    m = fps_counts(sets.sizes, ratio)
    ptr = torch.zeros(sets.num_graphs + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(m, 0)
    return Sets(ptr.to(sets.ptr.device, non_blocking=True), m, sets.num_graphs)


def _pos64(pos: torch.Tensor, what: str) -> torch.Tensor:
    _lib.require_gpu(pos)
    if pos.dim() != 2 or pos.size(1) not in (2, 3):
        raise ValueError(f"{what} must be [N, 2] or [N, 3]")
    return pos.to(torch.float64).contiguous()


def fps_sets(pos: torch.Tensor, sets: Sets, out: Sets, start: torch.Tensor | None = None,
             random_start: bool = True) -> torch.Tensor:
    """idx [out.total] int64: per graph of `sets`, out.sizes[g] farthest-point picks in selection
    order (global row indices). No host read."""
    pos = _pos64(pos, "pos")
    dev, B, N = pos.device, sets.num_graphs, pos.size(0)
    if start is None:
        if random_start:  # torch_cluster's CUDA rule: (rand(B) * n_g).long()
            n = (sets.ptr[1:] - sets.ptr[:-1]).to(torch.float32)
            start = (torch.rand(B, device=dev) * n).long()
        else:
            start = torch.zeros(B, dtype=torch.int64, device=dev)
    start = start.to(device=dev, dtype=torch.int64).contiguous()
    if start.numel() != B:
        raise ValueError("start must hold one index per graph")
    total = out.total
    idx = torch.empty(total, dtype=torch.int64, device=dev)
    ws = torch.empty(max(1, _lib.load().lgnn_fps_workspace_bytes(N)), dtype=torch.uint8,
                     device=dev)
    _lib.call("lgnn_fps", pos, N, pos.size(1), sets.ptr, out.ptr, start, B, idx, total, ws,
              ws.numel(), _lib.stream(dev))
    return idx


def fps(pos: torch.Tensor, batch: torch.Tensor | None = None, ratio: float = 0.5,
        random_start: bool = True, num_graphs: int | None = None,
        start: torch.Tensor | None = None) -> torch.Tensor:
    """torch_cluster.fps: indices of ceil(n_g * ratio) farthest-point samples per graph, in
    selection order. `start` [B] (local first picks) overrides the random / zero start. One host
    read (the graph sizes) sizes the output; pass num_graphs to avoid a second."""
    if not 0.0 < float(ratio) <= 1.0:
        raise ValueError("ratio must be in (0, 1]")
    pos = _pos64(pos, "pos")
    sets = sets_of(pos, batch, num_graphs)
    return fps_sets(pos, sets, sampled(sets, float(ratio)), start, random_start)


class PairGraph:
    """(query i, candidate j) pairs grouped by i with j ascending: `row`, `col` int64 [E],
    `rowoff` int64 [num_queries + 1]; transpose() -> (tptr int64 [num_candidates + 1], perm int64
    [E]): the pairs of each candidate in ascending pair order, built once."""

    def __init__(self, pairs: torch.Tensor, rowoff: torch.Tensor, num_candidates: int,
                 ptr_x: torch.Tensor, ptr_y: torch.Tensor, num_graphs: int):
        self.pairs, self.rowoff = pairs, rowoff
        self.row, self.col = pairs[0], pairs[1]
        self.num_queries, self.num_candidates = rowoff.numel() - 1, int(num_candidates)
        self.ptr_x, self.ptr_y, self.num_graphs = ptr_x, ptr_y, int(num_graphs)
        self._t = None

    @property
    def num_pairs(self) -> int:
        return self.pairs.size(1)

    @classmethod
    def from_edge_index(cls, edge_index: torch.Tensor, num_candidates: int,
                        num_queries: int) -> "PairGraph":
        """From PyG's edge_index = [candidate j; query i], sorted by i then j (what
        torch.stack([col, row]) of a radius search is). The transpose then treats the whole
        batch as one graph — every candidate looks itself up in every query row — which is
        correct, and far slower on a large batch than the per-graph one of `radius_sets`."""
        _lib.require_gpu(edge_index)
        dev = edge_index.device
        pairs = edge_index.to(torch.int64).flip(0).contiguous()
        rowoff = torch.searchsorted(pairs[0], torch.arange(num_queries + 1, device=dev))
        px = torch.tensor([0, num_candidates], dtype=torch.int32, device=dev)
        py = torch.tensor([0, num_queries], dtype=torch.int32, device=dev)
        return cls(pairs, rowoff.contiguous(), num_candidates, px, py, 1)

    def transpose(self):
        if self._t is None:
            dev, Nx, E = self.pairs.device, self.num_candidates, self.num_pairs
            tptr = torch.empty(Nx + 1, dtype=torch.int64, device=dev)
            perm = torch.empty(E, dtype=torch.int64, device=dev)
            ws = torch.empty(max(1, _lib.load().lgnn_pairs_transpose_workspace_bytes(Nx)),
                             dtype=torch.uint8, device=dev)
            _lib.call("lgnn_pairs_transpose", self.col, self.rowoff, self.num_queries, E,
                      self.ptr_x, self.ptr_y, self.num_graphs, Nx, tptr, perm, ws, ws.numel(),
                      _lib.stream(dev))
            self._t = (tptr, perm)
        return self._t


def radius_sets(x: torch.Tensor, y: torch.Tensor, sets_x: Sets, sets_y: Sets, r: float,
                max_num_neighbors: int = 32) -> PairGraph:
    """The radius search of queries y against candidates x, graph by graph. Two launches, one
    host read of the pair count, one launch."""
    if int(max_num_neighbors) < 1:
        raise ValueError("max_num_neighbors must be >= 1")
    if not float(r) >= 0.0:
        raise ValueError("r must be >= 0")
    x, y = _pos64(x, "x"), _pos64(y, "y")
    if x.size(1) != y.size(1) or sets_x.num_graphs != sets_y.num_graphs:
        raise ValueError("x and y must share their dimension and their graphs")
    dev, Nx, Ny, B = x.device, x.size(0), y.size(0), sets_x.num_graphs
    ws = torch.empty(max(8, _lib.load().lgnn_radius_pairs_workspace_bytes(Ny)),
                     dtype=torch.uint8, device=dev)
    args = (x, Nx, y, Ny, x.size(1), sets_x.ptr, sets_y.ptr, B, float(r), int(max_num_neighbors))
    _lib.call("lgnn_radius_pairs_count", *args, ws, ws.numel(), _lib.stream(dev))
    rowoff = ws[:8 * (Ny + 1)].view(torch.int64)
    E = int(rowoff[Ny].item())  # one host sync: sizes the output
    pairs = torch.empty(2, E, dtype=torch.int64, device=dev)
    _lib.call("lgnn_radius_pairs", *args, pairs, E, ws, ws.numel(), _lib.stream(dev))
    return PairGraph(pairs, rowoff, Nx, sets_x.ptr, sets_y.ptr, B)


def radius(x: torch.Tensor, y: torch.Tensor, r: float, batch_x: torch.Tensor | None = None,
           batch_y: torch.Tensor | None = None, max_num_neighbors: int = 32,
           num_workers: int = 1, num_graphs: int | None = None) -> torch.Tensor:
    """torch_cluster.radius: [2, E] int64 = (index into y, index into x) of every x within r of
    each y (same graph), grouped by y, at most max_num_neighbors each (the first in index order).
    num_workers is a CPU knob there; ignored. Pass num_graphs to keep to the one host read."""
    _lib.require_gpu(x, y)
    if (batch_x is None) != (batch_y is None):
        raise ValueError("give both batch_x and batch_y, or neither")
    if batch_x is None:  # one graph
        B = 1
        px = torch.tensor([0, x.size(0)], dtype=torch.int32, device=x.device)
        py = torch.tensor([0, y.size(0)], dtype=torch.int32, device=x.device)
    else:
        if num_graphs is None:
            last = [int(b[-1].item()) for b in (batch_x, batch_y) if b.numel()]
            num_graphs = max(last) + 1 if last else 0
        _, px, B = _batch_ptr(x, batch_x, num_graphs)
        _, py, _ = _batch_ptr(y, batch_y, B)
    empty = torch.empty(0, dtype=torch.int64)
    return radius_sets(x, y, Sets(px, empty, B), Sets(py, empty, B), r, max_num_neighbors).pairs
