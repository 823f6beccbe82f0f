"""Host-side surface of the SetTransformer addition (no GPU): the registry, the state_dict keys
of the model and of the aggregation (PyG 2.5.1's / the reference file's), the header entries and
the single-graph trace of the compiled model on meta tensors."""
import pytest
import torch

from lesion_gnn_amd import _lib, synth
from lesion_gnn_amd.conv import (InducedSetAttentionBlock, MultiheadAttentionBlock,
                                 PoolingByMultiheadAttention, SetAttentionBlock,
                                 SetTransformerAggregation)
from lesion_gnn_amd.models import (ModelConfig, OptimizerConfig, SetTransformer,
                                   SetTransformerModelConfig, SetTransformerModule, get_model)
from tests import set_transformer_cases as cases
from tests import set_transformer_ref as ref
from tests.test_compile import GLUE, VIEWS, trace

MAB_KEYS = ["attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
            "attn.out_proj.bias", "lin.weight", "lin.bias"]
LN_KEYS = ["layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"]


def _config(**kw):
    base = dict(inner_dim=64, num_inducing_points=3, num_seed_points=1, num_encoder_blocks=1,
                num_decoder_blocks=1, heads=4, layer_norm=True, dropout=0.0)
    base.update(kw)
    cfg = SetTransformerModelConfig(optimizer=OptimizerConfig(loss_type="MSE"), **base)
    cfg.input_features.value = 37
    cfg.num_classes.value = 5
    return cfg


def test_get_model_returns_the_module():
    cfg = _config()
    assert cfg.name == "SetTransformer" and cfg.compile is False
    assert isinstance(cfg, ModelConfig)
    m = get_model(cfg)
    assert isinstance(m, SetTransformerModule) and m.is_regression
    assert isinstance(m.model, SetTransformer)
    assert m.model.out_proj.out_features == 1  # regression -> one output (reference :90)
    assert m.model.concat is True  # the reference wrapper never passes concat
    assert "_dropout_rng" not in m.model.state_dict()
    assert m.model._dropout_rng.shape == (8,)
    cfg.compile = True
    assert isinstance(get_model(cfg).model, torch._dynamo.eval_frame.OptimizedModule)


def test_constructor_defaults_are_the_references():
    m = SetTransformer(8, 8, 2)
    assert len(m.encoders) == 1 and len(m.decoders) == 1 and m.concat is True
    assert m.encoders[0].ind.shape == (1, 1, 8) and m.pma.seed.shape == (1, 1, 8)
    assert m.pma.mab.layer_norm1 is None and m.pma.mab.heads == 1
    a = SetTransformerAggregation(8)
    assert a.concat is True and a.layer_norm is False and a.num_seed_points == 1
    assert MultiheadAttentionBlock(8).layer_norm1 is not None  # PyG: layer_norm=True there
    for blk in (SetAttentionBlock(8), InducedSetAttentionBlock(8, 2),
                PoolingByMultiheadAttention(8)):
        blk.reset_parameters()


def test_model_state_dict_keys():
    m = SetTransformer(**cases.MODEL_KW)
    mab = MAB_KEYS + LN_KEYS
    want = ["in_proj.weight", "in_proj.bias", "encoders.0.ind"] \
        + [f"encoders.0.mab1.{k}" for k in mab] + [f"encoders.0.mab2.{k}" for k in mab] \
        + ["pma.seed", "pma.lin.weight", "pma.lin.bias"] + [f"pma.mab.{k}" for k in mab] \
        + [f"decoders.0.mab.{k}" for k in mab] + ["out_proj.weight", "out_proj.bias"]
    assert sorted(m.state_dict()) == sorted(want)


def test_aggregation_state_dict_keys():
    a = SetTransformerAggregation(32, num_seed_points=16, num_encoder_blocks=2,
                                  num_decoder_blocks=2, heads=2, layer_norm=False)
    want = [f"{p}.{i}.mab.{k}" for p in ("encoders", "decoders") for i in (0, 1)
            for k in MAB_KEYS] + ["pma.seed", "pma.lin.weight", "pma.lin.bias"] \
        + [f"pma.mab.{k}" for k in MAB_KEYS]
    assert sorted(a.state_dict()) == sorted(want)
    assert a.state_dict()["pma.seed"].shape == (1, 16, 32)


def test_reference_state_dicts_load_strict():
    """State dicts of the torch-module builds of the reference file and of PyG's aggregation load
    with strict=True (same keys, same shapes), both ways."""
    kw = cases.MODEL_KW
    theirs = ref.PaddedSetTransformer(**kw)
    ours = SetTransformer(**kw)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    for akw in cases.AGG_VARIANTS.values():
        SetTransformerAggregation(**akw).load_state_dict(
            ref.PaddedAggregation(**akw).state_dict(), strict=True)


def test_header_entries_are_exported_and_bound():
    lib = _lib.load()
    for name in ("lgnn_set_attn_fwd", "lgnn_set_attn_bwd", "lgnn_set_attn_mask_offsets",
                 "lgnn_res_norm_fwd", "lgnn_res_norm_bwd", "lgnn_res_norm_bwd_partials",
                 "lgnn_set_readout_fwd", "lgnn_set_readout_bwd", "lgnn_add"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.LGNN_ABI_VERSION == 40 == lib.lgnn_abi_version()
    assert _lib.LGNN_SET_ATTN_QROWS > 0 and _lib.LGNN_SET_ATTN_KROWS > 0
    assert (_lib.LGNN_SET_ATTN_MAX_D, _lib.LGNN_SET_ATTN_MAX_HD) == (128, 512)
    # argument validation runs before any launch: no GPU needed
    assert lib.lgnn_set_attn_fwd(None, 0, None, 0, None, 0, None, 1, 0, None, 1, 1, 1, 129, None,
                                 None, None, None, None) == _lib.LGNN_EINVAL
    assert lib.lgnn_set_attn_fwd(None, 0, None, 0, None, 0, None, 1, 0, None, 1, 1, 5, 128, None,
                                 None, None, None, None) == _lib.LGNN_EINVAL
    assert lib.lgnn_res_norm_fwd(None, 0, None, 0, None, None, 1e-5, 4, 513, None, None, None,
                                 None) == _lib.LGNN_EINVAL
    assert lib.lgnn_res_norm_bwd_partials(0) == 1


def test_out_of_range_heads_raise_naming_the_limit():
    from lesion_gnn_amd import ops

    with pytest.raises(NotImplementedError, match="128"):
        ops.set_attn_plan(1, 129)
    with pytest.raises(NotImplementedError, match="512"):
        ops.set_attn_plan(8, 128)
    ops.set_attn_plan(4, 128)


def test_gat_readout_message_names_the_aggregation():
    from lesion_gnn_amd.models.gat import GAT

    with pytest.raises(NotImplementedError, match="SetTransformerAggregation"):
        GAT(8, [8, 8], 2, heads=2, dropout=0.0, num_st_seed_points=4)


@pytest.mark.parametrize("drop", [0.0, 0.35], ids=["nodrop", "drop"])
def test_model_traces_in_one_graph(drop):
    """fullgraph=True on meta tensors, symbolic sizes: one forward and one backward graph holding
    only lgnn ops and views."""
    torch.manual_seed(0)
    b = synth.make_batch(6, n=20, k=2, d_in=37, seed=1, sizes="lognormal")
    m = SetTransformer(**dict(cases.MODEL_KW, dropout=drop, num_seed_points=2, concat=False,
                              num_encoder_blocks=2)).train()
    out, fw, bw = trace(m.to("meta"), (b.x.to("meta"), b.batch.to("meta"), b.num_graphs))
    assert out.shape == (6, 5)
    extra = {t for t in (fw | bw) - GLUE - VIEWS if not t.startswith("<function sym_")}
    assert all(t.startswith("lgnn.") for t in extra), sorted(extra)
    assert {"lgnn.mab.default", "lgnn.res_norm.default", "lgnn.set_readout.default",
            "lgnn.batch_ptr.default"} <= fw, sorted(fw)
    assert {"lgnn.mab_bwd.default", "lgnn.res_norm_bwd.default",
            "lgnn.set_readout_bwd.default"} <= bw, sorted(bw)
    if drop:
        assert "auto_functionalized_v2" in fw or "lgnn.dropout_masks.default" in fw, sorted(fw)


def test_set_attention_op_traces():
    """ops.set_attention alone under torch.compile: lgnn::set_attn and its registered backward."""
    from lesion_gnn_amd import ops

    class Attn(torch.nn.Module):
        def forward(self, q, k, v, ptr):
            form = ops.AttnForm(None, 5, True, ptr, 0, ptr.shape[0] - 1)
            return ops.set_attention(q, k, v, form, 2)

    q = torch.empty(5, 8, device="meta", requires_grad=True)
    k = torch.empty(30, 8, device="meta", requires_grad=True)
    v = torch.empty(30, 8, device="meta", requires_grad=True)
    out, fw, bw = trace(Attn(), (q, k, v, torch.empty(5, dtype=torch.int32, device="meta")))
    assert out.shape == (20, 8)
    assert "lgnn.set_attn.default" in fw and "lgnn.set_attn_bwd.default" in bw
