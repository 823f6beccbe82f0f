"""The per-set restatement of the set-attention path (tests/set_transformer_ref.py) against PyG's
own composition — torch.nn.MultiheadAttention / LayerNorm / Linear on to_dense_batch-padded sets
with key-padding masks — in float64 to 1e-12, and its float32 run inside the GPU tests' bars on
their inputs (so those bars are known to be meetable by an fp32 evaluation)."""
import pytest
import torch

from tests import set_transformer_cases as cases
from tests import set_transformer_ref as ref

SIZES = [1, 7, 64, 300, 2]
SIZES_EMPTY = [1, 7, 0, 40, 2]


def _inputs(sizes, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(sum(sizes), C, generator=g, dtype=torch.float64)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return x, batch


def _sd(module):
    return {k: v.detach() for k, v in module.state_dict().items()}


def _unpad(dense, sizes):
    return torch.cat([dense[g, :n] for g, n in enumerate(sizes)])


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("block", ["sab", "isab", "pma"])
def test_blocks_match_padded(block, ln):
    C, H = 16, 4
    x, batch = _inputs(SIZES, C)
    dense, mask = ref.to_dense_batch(x, batch, len(SIZES))
    if block == "sab":
        m = ref.PaddedSAB(C, H, ln).double()
    elif block == "isab":
        m = ref.PaddedISAB(C, 3, H, ln).double()
    else:
        m = ref.PaddedPMA(C, 5, H, ln).double()
    ref.randomize_(m, 1)
    want = m(dense, mask)
    xs = ref.split_sets(x, SIZES)
    got = torch.cat(getattr(ref, block)(_sd(m), "", xs, H))
    want = want.flatten(0, 1) if block == "pma" else _unpad(want, SIZES)
    assert (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("sizes", [SIZES, SIZES_EMPTY], ids=["full", "empty"])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("concat", [False, True])
def test_aggregation_matches_padded(concat, ln, sizes):
    C, H = 16, 2
    x, batch = _inputs(sizes, C, 2)
    x.requires_grad_(True)
    m = ref.PaddedAggregation(C, 4, 2, 1, H, concat, ln).double()
    ref.randomize_(m, 3)
    want = m(x, batch, len(sizes))
    xr = x.detach().clone().requires_grad_(True)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    got = ref.aggregation(sd, ref.split_sets(xr, sizes), H, concat)
    assert got.shape == want.shape
    full = torch.tensor(sizes) > 0
    assert (got[full] - want[full]).abs().max().item() <= 1e-12
    if 0 in sizes:
        # PyG's nan_to_num leaves an all-zero row for a set without rows where the padded
        # softmax over no key is NaN (torch versions whose attention returns zeros there give
        # the seed's own path instead: the zero row is the specification)
        assert (got[~full] == 0).all()
        return
    w = torch.randn(want.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    (want * w).sum().backward()
    (got * w).sum().backward()
    # gradients: 1e-12 of each tensor's scale (they reach 1e2 here; float64 carries 1e-16)
    assert (xr.grad - x.grad).abs().max().item() <= 1e-12 * max(1.0, x.grad.abs().max().item())
    for k, p in m.named_parameters():
        bar = 1e-12 * max(1.0, p.grad.abs().max().item())
        assert (sd[k].grad - p.grad).abs().max().item() <= bar, k


@pytest.mark.parametrize("concat,S", [(True, 1), (False, 3)])
def test_model_matches_padded(concat, S):
    kw = dict(cases.MODEL_KW, num_seed_points=S, concat=concat, num_encoder_blocks=2)
    x, batch = _inputs(SIZES, kw["input_features"], 5)
    m = ref.PaddedSetTransformer(**kw).double()
    ref.randomize_(m, 6, 0.2)
    want = m(x, batch, len(SIZES))
    got = ref.model(_sd(m), ref.split_sets(x, SIZES), kw["heads"], concat)
    assert (got - want).abs().max().item() <= 1e-12


def _run(fn, sd, xs, dtype):
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    xs = [x.detach().to(dtype).requires_grad_(True) for x in xs]
    out = fn(sd, xs)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    (out * w.to(dtype)).sum().backward()
    dx = [x.grad if x.grad is not None else torch.zeros_like(x) for x in xs]  # None: no rows
    return out.detach(), {k: v.grad for k, v in sd.items()}, torch.cat(dx)


@pytest.mark.parametrize("variant", list(cases.AGG_VARIANTS))
def test_float32_restatement_meets_gpu_bars_aggregation(variant):
    kw = cases.AGG_VARIANTS[variant]
    b, sizes = cases.module_batch(kw["channels"])
    m = ref.PaddedAggregation(**kw).double()
    ref.randomize_(m, 8, 0.2)
    xs = ref.split_sets(b.x.double(), sizes)
    fn = lambda sd, xs: ref.aggregation(sd, xs, kw["heads"], kw["concat"])  # noqa: E731
    o64, g64, dx64 = _run(fn, m.state_dict(), xs, torch.float64)
    o32, g32, dx32 = _run(fn, m.state_dict(), xs, torch.float32)
    cases.assert_output(o32, o64)
    cases.assert_grad(dx32, dx64, "x")
    for k in g64:
        cases.assert_grad(g32[k], g64[k], k)


def test_float32_restatement_meets_gpu_bars_model():
    kw = cases.MODEL_KW
    b, sizes = cases.module_batch(kw["input_features"], empty=False)
    m = ref.PaddedSetTransformer(**kw).double()
    ref.randomize_(m, 9, 0.2)
    xs = ref.split_sets(b.x.double(), sizes)
    fn = lambda sd, xs: ref.model(sd, xs, kw["heads"], True)  # noqa: E731
    o64, g64, dx64 = _run(fn, m.state_dict(), xs, torch.float64)
    o32, g32, dx32 = _run(fn, m.state_dict(), xs, torch.float32)
    cases.assert_output(o32, o64)
    for k in g64:
        cases.assert_grad(g32[k], g64[k], k)
