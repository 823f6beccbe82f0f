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


class DataModule:
    """Reference DataModule (datamodule.py:37-81), minus Lightning. `stores` maps a dataset
    config's `name` to its GraphStore (the key of the reference's val / test loader dicts too);
    a config without a store raises KeyError naming it."""

    def __init__(self, config: DataConfig, compile: bool = False, *,
                 stores: dict[str, GraphStore]):
        self.batch_size = config.batch_size
        self.config = config
        self.transform = compose_transforms(config, compile)
        self.stores = dict(stores)

    def _store(self, cfg) -> GraphStore:
        if cfg.name not in self.stores:
            raise KeyError(f"no GraphStore for dataset {cfg.name!r} (given: {sorted(self.stores)})")
        return self.stores[cfg.name]

    def setup(self, stage: str) -> None:
        if stage == "fit":
            self.train_datasets = ConcatGraphs([self._store(c)
                                                for c in self.config.train_datasets])
        if stage in ("fit", "validate"):
            self.val_datasets = {c.name: self._store(c) for c in self.config.val_datasets}
        if stage == "test":
            self.test_datasets = {c.name: self._store(c) for c in self.config.test_datasets}
        if stage == "predict":
            raise NotImplementedError("Predict stage not implemented.")

    def _loader(self, store: GraphStore, shuffle: bool = False) -> GraphLoader:
        return GraphLoader(store, self.batch_size, shuffle=shuffle, transform=self.transform)

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
