"""Host-side surface of the PointNet++ addition (no GPU): the registry, the state_dict keys (the
reference file's with PyG 2.5.1's MLP / PointNetConv), the header entries, and what raises."""
import pytest
import torch

import lesion_gnn_amd
from lesion_gnn_amd import _lib, cluster, conv
from lesion_gnn_amd.models import (ModelConfig, OptimizerConfig, PointNet, PointNetModelConfig,
                                   PointNetModule, get_model)
from lesion_gnn_amd.models.pointnet import GlobalSAModule, SAModule
from tests import pointnet_cases as cases
from tests import pointnet_ref as ref

BN_KEYS = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]


def _config(loss_type="CE", **kw):
    cfg = PointNetModelConfig(optimizer=OptimizerConfig(loss_type=loss_type), pos_dim=2, **kw)
    cfg.input_features.value = 37
    cfg.num_classes.value = 5
    cfg.optimizer.class_weights.value = torch.ones(5)
    return cfg


def test_get_model_returns_the_module():
    cfg = _config()
    assert cfg.name == "PointNet" and cfg.compile is False
    assert isinstance(cfg, ModelConfig)
    m = get_model(cfg)
    assert isinstance(m, PointNetModule) and isinstance(m.model, PointNet)
    assert isinstance(m.model.sa1_module, SAModule)
    assert isinstance(m.model.sa3_module, GlobalSAModule)
    assert (m.model.sa1_module.ratio, m.model.sa1_module.r) == (0.5, 0.2)
    assert (m.model.sa2_module.ratio, m.model.sa2_module.r) == (0.25, 0.4)
    assert m.model.sa1_module.random_start is True  # torch_cluster's default; a plain attribute
    assert m.model.mlp.lins[-1].out_features == 5
    assert "_dropout_rng" not in m.model.state_dict() and m.model._dropout_rng.shape == (8,)
    reg = get_model(_config("MSE"))
    assert reg.is_regression and reg.model.mlp.lins[-1].out_features == 1


def test_package_exports():
    for name in ("fps", "radius", "global_max_pool", "PointNetConv", "PointNet",
                 "PointNetModelConfig"):
        assert name in lesion_gnn_amd.__all__ and hasattr(lesion_gnn_amd, name), name


def test_model_state_dict_keys():
    want = []
    for sa in ("sa1_module.conv.local_nn", "sa2_module.conv.local_nn", "sa3_module.nn"):
        want += [f"{sa}.lins.{i}.{p}" for i in range(3) for p in ("weight", "bias")]
        want += [f"{sa}.norms.{i}.module.{k}" for i in range(2) for k in BN_KEYS]
    want += [f"mlp.lins.{i}.{p}" for i in range(3) for p in ("weight", "bias")]
    m = PointNet(**cases.MODEL_KW)
    assert sorted(m.state_dict()) == sorted(want)
    assert m.state_dict()["sa1_module.conv.local_nn.lins.0.weight"].shape == (64, 39)
    assert m.state_dict()["sa3_module.nn.lins.0.weight"].shape == (256, 258)


def test_reference_state_dicts_load_strict():
    theirs, ours = ref.PointNet(**cases.MODEL_KW), PointNet(**cases.MODEL_KW)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    c = conv.PointNetConv(conv.DenseMLP([39, 64, 64, 128]))
    c.load_state_dict(ref.PointNetConv(ref.MLP([39, 64, 64, 128])).state_dict(), strict=True)


def test_dense_mlp_layouts():
    m = conv.DenseMLP([8, 16, 4], dropout=0.25, norm=None)
    assert sorted(m.state_dict()) == ["lins.0.bias", "lins.0.weight", "lins.1.bias",
                                      "lins.1.weight"]
    assert m.dropout == [0.25] and m.mask_shapes(3) == [(3, 16)]
    assert list(conv.DenseMLP([8, 4]).state_dict()) == ["lins.0.weight", "lins.0.bias"]
    assert conv.DenseMLP([8, 16, 16, 4], dropout=[0.1, 0.0]).dropout == [0.1, 0.0]
    with pytest.raises(NotImplementedError, match="batch_norm"):
        conv.DenseMLP([8, 16, 4], norm="layer_norm")
    # the GIN container is what it was
    gin = conv.MLP([8, 16, 16], dropout=0.5)
    assert len(gin.norms) == 1 and gin.dropout == 0.5
    with pytest.raises(ValueError):
        conv.MLP([8, 16, 16, 4])


def test_header_entries_are_exported_and_bound():
    lib = _lib.load()
    for name in ("lgnn_fps", "lgnn_fps_workspace_bytes", "lgnn_radius_pairs_count",
                 "lgnn_radius_pairs", "lgnn_radius_pairs_workspace_bytes",
                 "lgnn_pairs_transpose", "lgnn_pairs_transpose_workspace_bytes",
                 "lgnn_edge_sub_fwd", "lgnn_segment_sum", "lgnn_segment_max_fwd",
                 "lgnn_segment_max_bwd", "lgnn_bn_act_a", "lgnn_bn_bwd_stats_a",
                 "lgnn_bn_bwd_apply_a"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.LGNN_FPS_CAPACITY >= 256 and _lib.LGNN_FPS_CAPACITY % 256 == 0
    assert lib.lgnn_fps_workspace_bytes(10) == 80
    assert lib.lgnn_radius_pairs_workspace_bytes(10) == 11 * 8 + 10 * 4
    # argument validation runs before any launch: no GPU needed
    E = _lib.LGNN_EINVAL
    assert lib.lgnn_fps(None, 4, 4, None, None, None, 1, None, 2, None, 0, None) == E  # dims
    assert lib.lgnn_fps(None, 4, 2, None, None, None, 1, None, 2, None, 0, None) == E  # no ptr
    assert lib.lgnn_radius_pairs_count(None, 0, None, 0, 2, None, None, 0, -1.0, 64, None, 0,
                                       None) == E  # r < 0
    assert lib.lgnn_radius_pairs_count(None, 0, None, 0, 2, None, None, 0, 0.2, 0, None, 0,
                                       None) == E  # max_num_neighbors < 1
    assert lib.lgnn_edge_sub_fwd(None, None, None, None, 0, 6, None, None, None, 0, None) == E
    assert lib.lgnn_segment_max_fwd(None, None, 1, 0, None, None, None) == E
    assert lib.lgnn_bn_act_a(None, 0, 8, None, None, None, _lib.LGNN_ACT_RELU, None, None) == E
    x = torch.zeros(8)
    assert lib.lgnn_bn_act_a(None, 0, 8, x.data_ptr(), x.data_ptr(), None, _lib.LGNN_ACT_NONE,
                             None, None) == E  # the activation must be ELU or ReLU
    assert lib.lgnn_bn_act_a(None, 0, 8, x.data_ptr(), x.data_ptr(), None, _lib.LGNN_ACT_RELU,
                             None, None) == _lib.LGNN_OK  # no rows: nothing launched


def test_cpu_tensors_raise():
    pos = torch.rand(6, 2)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        lesion_gnn_amd.fps(pos)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        lesion_gnn_amd.radius(pos, pos[:2], 0.5)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        lesion_gnn_amd.global_max_pool(torch.rand(6, 4), torch.zeros(6, dtype=torch.int64), 1)
    c = conv.PointNetConv(conv.DenseMLP([6, 8, 8]))
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        c(torch.rand(6, 4), (pos, pos[:2]), torch.zeros(2, 0, dtype=torch.int64))
    m = PointNet(4, 2, 3)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        m(torch.rand(6, 4), pos, torch.zeros(6, dtype=torch.int64), 1)


def test_unsupported_options_raise(monkeypatch):
    with pytest.raises(NotImplementedError, match="compile"):
        get_model(_config(compile=True))
    net = PointNet(4, 2, 3)
    with pytest.raises(NotImplementedError, match="SyncBatchNorm"):
        net.set_sync_bn(None)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="torch.distributed"):
        net(torch.rand(6, 4), torch.rand(6, 2), torch.zeros(6, dtype=torch.int64), 1)
    monkeypatch.undo()
    mlp = conv.DenseMLP([6, 8, 8])
    with pytest.raises(NotImplementedError, match="global_nn"):
        conv.PointNetConv(mlp, global_nn=conv.DenseMLP([8, 8]))
    with pytest.raises(NotImplementedError, match="add_self_loops"):
        conv.PointNetConv(mlp, add_self_loops=True)
    with pytest.raises(NotImplementedError, match="x=None"):
        conv.PointNetConv(mlp)((None, None), (torch.rand(3, 2), torch.rand(1, 2)), None)
    with pytest.raises(ValueError, match="ratio"):
        lesion_gnn_amd.fps(torch.rand(3, 2), ratio=0.0)


def test_sample_counts_are_torch_clusters():
    n = torch.tensor([10, 64, 65, 1, 0, 3])
    assert cluster.fps_counts(n, 0.3).tolist() == ref.fps_counts(n.tolist(), 0.3)
    assert cluster.fps_counts(n, 0.3).tolist() == [3, 20, 20, 1, 0, 1]
