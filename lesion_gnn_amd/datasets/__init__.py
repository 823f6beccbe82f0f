"""Data-side configuration surface of the reference (src/lesion_gnn/datasets): the config
dataclasses that an experiment file such as configs/config.py builds (DataConfig, DDRConfig,
AptosConfig, LesionsNodesConfig, ...), with the reference's names and fields, so the file loads
unchanged against this package (utils.config.get_config). The datasets themselves (DDR / APTOS
image folders, the segmentation / timm feature extraction) are out of scope. The
preprocessing every image of theirs goes through first is here (fundus.py: `FundusPreprocess`,
autocrop, resize, pad and normalise in HIP), and so is what holds and serves their graphs:
`GraphStore` / `ConcatGraphs` (memory.py), the dataset resident on the GPU, `GraphLoader`, which
shuffles it and collates each batch in one HIP call (ops.collate), and `DataModule`
(datamodule.py). The node extractor's kernels are under nodes.lesions.
"""
from .datamodule import DataConfig, DataModule, compose_transforms, hoisted_transforms
from .fundus import FundusAutocrop, FundusBatch, FundusPreprocess
from .memory import (ConcatGraphs, GraphLoader, GraphStore, batch_bounds, class_weights,
                     epoch_order)

__all__ = ["ConcatGraphs", "DataConfig", "DataModule", "FundusAutocrop", "FundusBatch",
           "FundusPreprocess", "GraphLoader", "GraphStore", "batch_bounds", "class_weights",
           "compose_transforms", "epoch_order", "hoisted_transforms"]
