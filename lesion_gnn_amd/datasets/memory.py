"""A graph dataset resident on the GPU and a loader over it: what the reference does per step with
`DataLoader(shuffle=True)` over its InMemoryDataset (src/lesion_gnn/datasets/datamodule.py:63-81,
datasets/base.py:27-115) — draw an order, pick the graphs of one batch, collate them — with the
collation as one HIP call (`ops.collate`, lgnn_collate) on data that never leaves the device.

`GraphStore` holds every graph's rows flat (x, pos) with the graphs' row offsets `ptr` and labels
`y`; `ConcatGraphs` is the reference's ConcatDataset; `GraphLoader` yields one `synth.Batch` per
step, run through the transform chain (KNNGraph, GaussianDistance, ...). The order of an epoch
and its cut into batches are the pure host functions `epoch_order` and `batch_bounds`.

A store may keep each graph's edges too (`GraphStore.with_edges`: the reference applies its
transforms per graph, before the Collater, datamodule.py:43-45); `ops.collate` then gathers them
into the batch's edge_index (lgnn_collate_edges) and the chain has no graph to build per step.
"""
from __future__ import annotations

import torch

from ..utils import ClassWeights


def epoch_order(num_graphs: int, shuffle: bool, generator: torch.Generator | None = None
                ) -> torch.Tensor:
    """The graph order of one epoch, int64 [num_graphs] on the host: arange unshuffled, else
    torch.randperm on `generator` (a CPU generator; it advances, so the next epoch differs).
    Without one, a fresh generator seeded from the default generator, as
    torch.utils.data.RandomSampler does it."""
    if not shuffle:
        return torch.arange(num_graphs, dtype=torch.int64)
    if generator is None:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        generator = torch.Generator().manual_seed(seed)
    return torch.randperm(num_graphs, generator=generator)


def batch_bounds(num_graphs: int, batch_size: int, drop_last: bool = False
                 ) -> list[tuple[int, int]]:
    """[start, stop) of every batch of an epoch's order."""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    stop = num_graphs - num_graphs % batch_size if drop_last else num_graphs
    return [(s, min(s + batch_size, stop)) for s in range(0, stop, batch_size)]


def class_weights(counts: torch.Tensor, mode: ClassWeights = ClassWeights.INVERSE_FREQUENCY
                  ) -> torch.Tensor:
    """Reference BaseDataset.get_class_weights (base.py:81-95) from the per-class counts."""
    mode = ClassWeights(mode)
    if mode == ClassWeights.UNIFORM:
        return torch.ones_like(counts).float()
    if mode == ClassWeights.INVERSE:
        return 1 / counts
    if mode == ClassWeights.QUADRATIC_INVERSE:
        return 1 / counts ** 2
    return counts.sum() / (len(counts) * counts)


class GraphStore:
    """The in-memory dataset: x [sum n, d] fp32, pos [sum n, 2 or 3] fp64 (or None), y [G] int64
    and ptr [G + 1] int64 on one GPU, graph g owning rows [ptr[g], ptr[g + 1]); `ptr_host` and
    `y_host` are host copies (batch sizing and the label statistics read no device memory). GPU
    tensors only, like the rest of the package.

    A store may keep each graph's edges as well (`with_edges`): `edge_index` [2, E] int64 over the
    store's rows, grouped by graph in graph order, `edge_weight` [E] or None, and `edge_ptr`
    [G + 1] int64 (graph g owns the edges [edge_ptr[g], edge_ptr[g + 1])) with its host copy
    `edge_ptr_host`; all None on a store without edges. ops.collate then collates the edges too."""

    edge_index = edge_weight = edge_ptr = edge_ptr_host = None

    def __init__(self, x: torch.Tensor, pos: torch.Tensor | None, y: torch.Tensor,
                 ptr: torch.Tensor):
        from .. import _lib

        _lib.require_gpu(x)
        dev = x.device
        if x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("x must be a [rows, d] float32 tensor")
        if pos is not None:
            _lib.require_gpu(pos)
            if pos.dim() != 2 or pos.size(1) not in (2, 3) or pos.size(0) != x.size(0):
                raise ValueError("pos must be [rows, 2] or [rows, 3]")
            pos = pos.to(device=dev, dtype=torch.float64).contiguous()
        self.ptr_host = ptr.detach().to("cpu", torch.int64).reshape(-1).contiguous()
        self.y_host = y.detach().to("cpu", torch.int64).reshape(-1).contiguous()
        p = self.ptr_host
        if p.numel() != self.y_host.numel() + 1 or int(p[0]) != 0 or \
                int(p[-1]) != x.size(0) or bool((p[1:] < p[:-1]).any()):
            raise ValueError("ptr must be [G + 1] non-decreasing offsets from 0 to the row count")
        self.x = x.contiguous()
        self.pos = pos
        self.y = self.y_host.to(dev)
        self.ptr = self.ptr_host.to(dev)

    # -- constructors --------------------------------------------------------------------------

    @classmethod
    def from_tensors(cls, x, pos, y, ptr) -> "GraphStore":
        return cls(x, pos, y, ptr)

    @classmethod
    def from_list(cls, items) -> "GraphStore":
        """Objects with x [n, d], pos [n, 2 or 3] and y (one label), such as the LesionNodes of
        LesionsExtractor.nodes_from_maps."""
        items = list(items)
        if not items:
            raise ValueError("from_list needs one graph at least")
        dev = items[0].x.device
        sizes = torch.tensor([0] + [it.x.size(0) for it in items], dtype=torch.int64)
        y = torch.cat([torch.as_tensor(it.y).reshape(-1)[:1].cpu() for it in items])
        has_pos = getattr(items[0], "pos", None) is not None
        pos = torch.cat([it.pos.to(dev) for it in items]) if has_pos else None
        return cls(torch.cat([it.x for it in items]), pos, y, sizes.cumsum(0))

    @classmethod
    def from_slices(cls, x, pos, y, slices: dict) -> "GraphStore":
        """The (data, slices) layout of the reference's processed data.pt (base.py:49,111-112),
        tensors only: slices["x"] is ptr; the other attributes must be sliced alike."""
        ptr = torch.as_tensor(slices["x"]).cpu()
        G = ptr.numel() - 1
        if pos is not None and "pos" in slices and \
                not torch.equal(torch.as_tensor(slices["pos"]).cpu(), ptr):
            raise ValueError("slices of pos and x differ")
        if "y" in slices and not torch.equal(torch.as_tensor(slices["y"]).cpu(),
                                             torch.arange(G + 1)):
            raise ValueError("y must hold one label per graph")
        return cls(x, pos, y, ptr)

    def with_edges(self, edge_index: torch.Tensor, edge_weight: torch.Tensor | None = None
                   ) -> "GraphStore":
        """A store sharing this one's x, pos, y and ptr that keeps the edges `edge_index` [2, E]
        int64 (source, target; ids are this store's rows) and `edge_weight` [E] float32 / float64
        or None. Both endpoints of an edge must lie in one graph; edges not grouped by graph in
        graph order are sorted by graph once (stable: the order inside a graph is kept). Checked
        here, once, with one host read: ValueError gives the number of endpoints outside
        [0, rows) or of edges that cross graphs."""
        from .. import _lib

        _lib.require_gpu(edge_index, edge_weight)
        dev = self.x.device
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be a [2, E] int64 tensor")
        E, G, rows = edge_index.size(1), len(self), self.x.size(0)
        if edge_weight is not None and (edge_weight.dim() != 1 or edge_weight.numel() != E or
                                        edge_weight.dtype not in (torch.float32, torch.float64)):
            raise ValueError("edge_weight must be [E] float32 or float64")
        ei = edge_index.to(dev).contiguous()
        outside = (ei < 0) | (ei >= rows)
        # the graph of every endpoint: the number of graph ends at or below it
        graph = torch.bucketize(ei.clamp(0, max(rows - 1, 0)), self.ptr[1:], right=True)
        graph = graph.clamp_(max=max(G - 1, 0))
        crossing = (graph[0] != graph[1]) & ~outside.any(0)
        ungrouped = (graph[1, 1:] < graph[1, :-1]).any() if E > 1 else torch.zeros((), device=dev)
        counts = torch.bincount(graph[1], minlength=G)[:G] if E else \
            torch.zeros(G, dtype=torch.int64, device=dev)
        head = torch.stack([outside.sum(), crossing.sum(), ungrouped.to(torch.int64)])
        host = torch.cat([head, counts]).cpu()  # the one host read
        if int(host[0]) or int(host[1]):
            raise ValueError(f"with_edges: {int(host[0])} endpoint(s) outside [0, {rows}), "
                             f"{int(host[1])} edge(s) with endpoints in two graphs")
        if int(host[2]):
            order = torch.sort(graph[1], stable=True).indices
            ei = ei[:, order].contiguous()
            edge_weight = None if edge_weight is None else edge_weight[order]
        out = object.__new__(type(self))
        out.__dict__.update(self.__dict__)
        out.edge_index = ei
        out.edge_weight = None if edge_weight is None else edge_weight.to(dev).contiguous()
        out.edge_ptr_host = torch.cat([torch.zeros(1, dtype=torch.int64), host[3:].cumsum(0)])
        out.edge_ptr = out.edge_ptr_host.to(dev)
        return out

    def save(self, path) -> None:
        """A plain dict of host tensors (torch.load(weights_only=True) reads it)."""
        d = {"x": self.x.cpu(), "y": self.y_host, "ptr": self.ptr_host}
        if self.pos is not None:
            d["pos"] = self.pos.cpu()
        if self.edge_index is not None:
            d["edge_index"] = self.edge_index.cpu()
            if self.edge_weight is not None:
                d["edge_weight"] = self.edge_weight.cpu()
        torch.save(d, path)

    @classmethod
    def load(cls, path, device) -> "GraphStore":
        d = torch.load(path, map_location="cpu", weights_only=True)
        pos = d.get("pos")
        store = cls(d["x"].to(device), None if pos is None else pos.to(device), d["y"], d["ptr"])
        if "edge_index" in d:
            w = d.get("edge_weight")
            store = store.with_edges(d["edge_index"].to(device),
                                     None if w is None else w.to(device))
        return store

    # -- the dataset's properties (PyG InMemoryDataset's, reference base.py:75-95) --------------

    def __len__(self) -> int:
        return self.y_host.numel()

    @property
    def num_features(self) -> int:
        return self.x.size(1)

    @property
    def num_classes(self) -> int:
        return int(self.y_host.max()) + 1 if len(self) else 0

    @property
    def classes_counts(self) -> torch.Tensor:
        return torch.unique(self.y_host, return_counts=True)[1]

    def get_class_weights(self, mode: ClassWeights = ClassWeights.INVERSE_FREQUENCY
                          ) -> torch.Tensor:
        return class_weights(self.classes_counts, mode)


class ConcatGraphs(GraphStore):
    """Reference ConcatDataset (datamodule.py:84-117): the stores' graphs in order as one flat
    store, concatenated once here; class weights from the summed per-store counts."""

    def __init__(self, stores):
        stores = list(stores)
        if len(set(s.num_features for s in stores)) != 1:
            raise ValueError("All datasets should have the same number of features.")
        if len(set(s.num_classes for s in stores)) != 1:
            raise ValueError("All datasets should have the same number of classes.")
        if len(set(s.pos is None for s in stores)) != 1:
            raise ValueError("All datasets should have positions, or none.")
        self.stores = stores
        ptrs, base = [torch.zeros(1, dtype=torch.int64)], 0
        for s in stores:
            ptrs.append(s.ptr_host[1:] + base)
            base += int(s.ptr_host[-1])
        pos = None if stores[0].pos is None else torch.cat([s.pos for s in stores])
        with_edges = [s.edge_index is not None for s in stores]
        if any(with_edges) and not all(with_edges):
            raise ValueError("All datasets should have edges, or none.")
        if len(set(None if s.edge_weight is None else s.edge_weight.dtype for s in stores)) != 1:
            raise ValueError("All datasets should have edge weights of one dtype, or none.")
        super().__init__(torch.cat([s.x for s in stores]), pos,
                         torch.cat([s.y_host for s in stores]), torch.cat(ptrs))
        if all(with_edges) and stores:
            # every store's edges are valid and grouped: concatenated with the row offset added,
            # they are too (no second check, no host read)
            row0 = [0]
            for s in stores:
                row0.append(row0[-1] + int(s.ptr_host[-1]))
            eptrs, ebase = [torch.zeros(1, dtype=torch.int64)], 0
            for s in stores:
                eptrs.append(s.edge_ptr_host[1:] + ebase)
                ebase += int(s.edge_ptr_host[-1])
            self.edge_index = torch.cat([s.edge_index + r for s, r in zip(stores, row0)], dim=1)
            self.edge_weight = None if stores[0].edge_weight is None else \
                torch.cat([s.edge_weight for s in stores])
            self.edge_ptr_host = torch.cat(eptrs)
            self.edge_ptr = self.edge_ptr_host.to(self.x.device)

    @property
    def classes_counts(self) -> torch.Tensor:
        return sum(s.classes_counts for s in self.stores)


class GraphLoader:
    """One pass over `store` per iter(): the order `epoch_order(len(store), shuffle, generator)`
    cut by `batch_bounds`, each batch `transform(ops.collate(store, ids))` with its ids kept as
    `batch.ids` (host int64)."""

    def __init__(self, store: GraphStore, batch_size: int, shuffle: bool = False,
                 drop_last: bool = False, transform=None,
                 generator: torch.Generator | None = None):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.store, self.batch_size = store, int(batch_size)
        self.shuffle, self.drop_last = shuffle, drop_last
        self.transform, self.generator = transform, generator

    def __len__(self) -> int:
        return len(batch_bounds(len(self.store), self.batch_size, self.drop_last))

    def __iter__(self):
        from .. import ops

        order = epoch_order(len(self.store), self.shuffle, self.generator)
        # the epoch's order goes to the device once, from pinned memory: no synchronising copy
        order_dev = order.pin_memory().to(self.store.x.device, non_blocking=True) \
            if order.numel() else order
        for start, stop in batch_bounds(len(self.store), self.batch_size, self.drop_last):
            ids = order[start:stop]
            batch = ops.collate(self.store, ids, ids_dev=order_dev[start:stop])
            batch.ids = ids
            yield batch if self.transform is None else self.transform(batch)
