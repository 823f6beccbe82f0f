"""Model registry (reference src/lesion_gnn/models/__init__.py:10,22-35: isinstance dispatch on
the config type): the message-passing families of the hot path, the SetTransformer and
PointNet++."""
from .base import (BaseModelConfig, BaseModule, LossType, LRSchedulerConfig, OptimizerAlgo,
                   OptimizerConfig)
from .gcn import GCN, GCNConfig, GCNModule
from .gat import GAT, GATConfig, GATModule
from .gin import GIN, GINConfig, GINModule
from .drgnet import DRGNet, DRGNetModelConfig, DRGNetModule
from .set_transformer import SetTransformer, SetTransformerModelConfig, SetTransformerModule
from .pointnet import PointNet, PointNetModelConfig, PointNetModule

ModelConfig = (DRGNetModelConfig | GCNConfig | GINConfig | GATConfig | SetTransformerModelConfig
               | PointNetModelConfig)

__all__ = ["GCN", "GCNConfig", "GCNModule", "GIN", "GINConfig", "GINModule", "GAT", "GATConfig",
           "GATModule", "DRGNet", "DRGNetModelConfig", "DRGNetModule", "SetTransformer",
           "SetTransformerModelConfig", "SetTransformerModule", "PointNet",
           "PointNetModelConfig", "PointNetModule", "BaseModule",
           "BaseModelConfig", "OptimizerConfig", "OptimizerAlgo", "LossType", "LRSchedulerConfig",
           "ModelConfig", "get_model"]


def get_model(config) -> BaseModule:
    if isinstance(config, DRGNetModelConfig):
        return DRGNetModule(config)
    if isinstance(config, GCNConfig):
        return GCNModule(config)
    if isinstance(config, GINConfig):
        return GINModule(config)
    if isinstance(config, GATConfig):
        return GATModule(config)
    if isinstance(config, SetTransformerModelConfig):
        return SetTransformerModule(config)
    if isinstance(config, PointNetModelConfig):
        return PointNetModule(config)
    raise ValueError(f"Unknown model config type {type(config)}")
