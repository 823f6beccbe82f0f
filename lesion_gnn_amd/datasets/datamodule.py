"""Reference src/lesion_gnn/datasets/datamodule.py:27-34 (`DataConfig`) and the transform
composition of `DataModule.__init__` (:42-48): the configured transforms in order, plus
`ToSparseTensor` when the model is not compiled (:44-45). `compose_transforms` returns the
per-batch transform chain this package runs on the GPU (KNNGraph, GaussianDistance) so a
synthetic or pre-collated batch goes through the same graph construction the reference applies
per sample. `DataModule` is the reference class (:37-81) without Lightning, over GPU-resident
`GraphStore`s (memory.py) in place of the image datasets, which stay out of scope (DESIGN.md
§7): the caller builds the stores and hands them over by dataset name."""
from __future__ import annotations

import dataclasses

from ..transforms import TransformConfig, get_transform
from ..utils import ClassWeights
from .aptos import AptosConfig
from .ddr import DDRConfig
from .memory import ConcatGraphs, GraphLoader, GraphStore


@dataclasses.dataclass(kw_only=True)
class DataConfig:
    train_datasets: list[AptosConfig | DDRConfig]
    val_datasets: list[AptosConfig | DDRConfig]
    test_datasets: list[AptosConfig | DDRConfig]
    transforms: list[TransformConfig]
    batch_size: int
    num_workers: int


class Compose:
    """torch_geometric.transforms.Compose: apply the transforms in order."""

    def __init__(self, transforms: list):
        self.transforms = list(transforms)

    def __call__(self, data):
        for t in self.transforms:
            data = t(data)
        return data

    def __repr__(self) -> str:
        return f"Compose({self.transforms!r})"


class ToSparseTensor:
    """The reference appends torch_geometric's ToSparseTensor when `compile=False`
    (datamodule.py:44-45) so the model receives `adj_t` (target-major CSR). This package's
    models build that CSR on the GPU from either input (graph.py), so the transform records
    the choice and leaves `edge_index` in place; `as_graph` accepts both forms."""

    def __call__(self, data):
        return data

    def __repr__(self) -> str:
        return "ToSparseTensor()"


def compose_transforms(config: DataConfig, compile: bool = False) -> Compose:
    """The transform chain of DataModule.__init__ (datamodule.py:43-45)."""
    t = Compose([get_transform(c) for c in config.transforms])
    if not compile:
        t.transforms.append(ToSparseTensor())
    return t


def hoisted_transforms(config: DataConfig) -> tuple[list, list]:
    """(hoisted, rest) of config.transforms, as transform objects: `hoisted` is the leading run of
    KNNGraph, RadiusGraph and GaussianDistance(save_as=EDGE_WEIGHT_REPLACE) — the transforms whose
    result for a graph depends on that graph alone and fits a GraphStore's edge_index and
    edge_weight, so they can run once per store instead of once per batch — and `rest` what
    follows. The run must start with a graph builder (GaussianDistance needs edges): otherwise
    nothing is hoisted."""
    from ..knn import KNNGraph, RadiusGraph
    from ..transforms import GaussianDistance, SaveAs

    ts = [get_transform(c) for c in config.transforms]
    n = 0
    while n < len(ts):
        t = ts[n]
        builder = isinstance(t, (KNNGraph, RadiusGraph))
        weights = n > 0 and isinstance(t, GaussianDistance) and \
            t.save_as in (SaveAs.EDGE_WEIGHT_REPLACE, SaveAs.EDGE_WEIGHT_REPLACE.value)
        if not (builder or weights):
            break
        n += 1
    return ts[:n], ts[n:]


class DataModule:
    """Reference DataModule (datamodule.py:37-81), minus Lightning. `stores` maps a dataset
    config's `name` to its GraphStore (the key of the reference's val / test loader dicts too);
    a config without a store raises KeyError naming it.

    hoist=True applies the reference's order of operations (transforms per graph, then collate,
    datamodule.py:43-45,63-69): in `setup`, a store without edges gets them once, from
    `hoisted_transforms` run over the whole store as one batch, and the loaders run only the
    remaining transforms on edges that ops.collate gathers. A store that already has edges, or a
    chain that does not start with a hoistable transform, keeps the whole chain per batch, as
    hoist=False does for every store. The train datasets are concatenated, so they must all come
    with edges or all without: a mixture raises ValueError naming both groups."""

    def __init__(self, config: DataConfig, compile: bool = False, *,
                 stores: dict[str, GraphStore], hoist: bool = False):
        self.batch_size = config.batch_size
        self.config = config
        self.transform = compose_transforms(config, compile)
        self.stores = dict(stores)
        self.hoist = bool(hoist)
        self._hoisted, rest = hoisted_transforms(config) if hoist else ([], [])
        self._rest = Compose(rest + ([] if compile else [ToSparseTensor()]))
        self._edged: dict[str, GraphStore] = {}
        self.generator = None  # the train loader's (a CPU torch.Generator), set by the caller

    def _given(self, cfg) -> GraphStore:
        if cfg.name not in self.stores:
            raise KeyError(f"no GraphStore for dataset {cfg.name!r} (given: {sorted(self.stores)})")
        return self.stores[cfg.name]

    def _store(self, cfg) -> GraphStore:
        store = self._given(cfg)
        if not self._hoisted or store.edge_index is not None:
            return store
        if cfg.name not in self._edged:
            self._edged[cfg.name] = self._with_hoisted_edges(store)
        return self._edged[cfg.name]

    def _with_hoisted_edges(self, store: GraphStore) -> GraphStore:
        """The hoisted transforms over the whole store viewed as one batch of len(store) graphs."""
        import torch

        from ..synth import Batch

        rows, dev = store.x.size(0), store.x.device
        sizes = store.ptr[1:] - store.ptr[:-1]
        batch = torch.repeat_interleave(torch.arange(len(store), device=dev), sizes,
                                        output_size=rows)
        data = Batch(store.x, torch.empty(2, 0, dtype=torch.int64, device=dev), batch, store.ptr,
                     store.y, store.pos, len(store))
        for t in self._hoisted:
            data = t(data)
        return store.with_edges(data.edge_index, getattr(data, "edge_weight", None))

    def _transform_for(self, store: GraphStore):
        """The per-batch chain of a loader over `store`: the remaining transforms when its edges
        come from the hoisted ones, else the whole chain."""
        hoisted = any(store is s for s in self._edged.values()) or \
            getattr(store, "_hoisted_edges", False)
        return self._rest if hoisted else self.transform

    def setup(self, stage: str) -> None:
        if stage == "fit":
            given = {c.name: self._given(c).edge_index is not None
                     for c in self.config.train_datasets}
            if self._hoisted and len(set(given.values())) > 1:
                # hoisting the rest would concatenate edges of two origins, which the per-batch
                # chain would then have to rebuild (and their weights need not match)
                raise ValueError(
                    "hoist=True: the train datasets "
                    f"{sorted(n for n, e in given.items() if e)} already have edges and "
                    f"{sorted(n for n, e in given.items() if not e)} have none; give every train "
                    "store its edges (GraphStore.with_edges), or none of them")
            parts = [self._store(c) for c in self.config.train_datasets]
            self.train_datasets = ConcatGraphs(parts)
            # the concatenation's edges are the hoisted ones when every part's are
            self.train_datasets._hoisted_edges = bool(parts) and all(
                any(p is s for s in self._edged.values()) for p in parts)
        if stage in ("fit", "validate"):
            self.val_datasets = {c.name: self._store(c) for c in self.config.val_datasets}
        if stage == "test":
            self.test_datasets = {c.name: self._store(c) for c in self.config.test_datasets}
        if stage == "predict":
            raise NotImplementedError("Predict stage not implemented.")

    def _loader(self, store: GraphStore, shuffle: bool = False) -> GraphLoader:
        return GraphLoader(store, self.batch_size, shuffle=shuffle,
                           transform=self._transform_for(store),
                           generator=self.generator if shuffle else None)

    def train_dataloader(self) -> GraphLoader:
        return self._loader(self.train_datasets, shuffle=True)

    def val_dataloader(self) -> dict[str, GraphLoader]:
        return {name: self._loader(s) for name, s in self.val_datasets.items()}

    def test_dataloader(self) -> dict[str, GraphLoader]:
        return {name: self._loader(s) for name, s in self.test_datasets.items()}

    # the inputs of the reference's placeholder filling (training.py:23-27), from the train set
    @property
    def num_features(self) -> int:
        return self.train_datasets.num_features

    @property
    def num_classes(self) -> int:
        return self.train_datasets.num_classes

    def get_class_weights(self, mode: ClassWeights = ClassWeights.INVERSE_FREQUENCY):
        return self.train_datasets.get_class_weights(mode)
