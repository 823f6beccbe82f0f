"""Fused split-3 GCN backward with in_proj folded behind the first conv (stack3_bwd.hip k_s3_fbwd).

in_proj has no activation, so its weight gradient is dW_0 = W_1^T (G_1^T X) with G_1 = Â^T dZ_1:
the kernel accumulates T = sum over its tiles of G_1^T X and g = sum of colsum G_1, and multiplies
by W_1^T once per workgroup (dW_0 = W_1^T T, db_0 = W_1^T g) instead of forming dH_0 = G_1 W_1 per
tile. The order of the products differs from the layer-wise backward's, so the results are held to
float64: for every parameter
    max|grad_fused - ref64| <= 3 * max|grad_layerwise - ref64| + 2e-7 * max|ref64|
(the idiom of tests/test_gpu_s3.py: the layer-wise backward, ops.FUSED_BWD = False, is the fp32
yardstick on the same step; ref64 is the plain-torch oracle in float64). An fp32 emulation of both
orders stays within 1.3 x of the direct order's error, so the factor 3 leaves room without hiding
a wrong product. Every case also runs twice and must repeat bit for bit.

Cases: more tiles than workgroups (some accumulate two tiles), widths below 128 on every side of
W_1 (masks and zero padding), one conv, two graphs in one closed tile with a partial last tile,
closed and open tiles adding into the same slots (open tiles inside the launch and in separate
launches), and no closed tile at all.
"""
import functools

import pytest
import torch

import oracle.pyg_ref as ref
from lesion_gnn_amd import ops, synth
from lesion_gnn_amd.models import GCN
from tests import tile_width_cases as twc

pytestmark = pytest.mark.gpu

# name: (make_batch arguments, d_in, hidden, pool)
CASES = {
    "two_tiles_per_wg": (dict(num_graphs=300, n=64, k=8), 128, [128, 128, 128], "mean"),
    "narrow_in": (dict(num_graphs=40, n=64, k=8), 36, [64, 32, 128], "mean"),
    "narrow_mid": (dict(num_graphs=40, n=64, k=8), 128, [16, 128, 8], "mean"),
    "one_conv_add": (dict(num_graphs=40, n=64, k=8), 128, [128, 128], "add"),
    "shared_tile": (dict(num_graphs=6, k=8, sizes=[64, 64, 30, 34, 64, 17]), 128,
                    [128, 128, 128], "mean"),
    "open_and_closed": (dict(num_graphs=4, k=6, sizes=[64, 200, 64, 64]), 128, [128, 128, 128],
                        "mean"),
    "all_open": (dict(num_graphs=2, k=8, sizes=[200, 200]), 128, [128, 128, 128], "mean"),
}


@functools.lru_cache(maxsize=None)
def _batch(case):
    kw, d_in, _, _ = CASES[case]
    return synth.make_batch(d_in=d_in, seed=60 + list(CASES).index(case), **kw)


@functools.lru_cache(maxsize=None)
def _state(case):
    _, d_in, hidden, pool = CASES[case]
    torch.manual_seed(1234)
    m = GCN(d_in, hidden, 5, dropout=0.0, pool=pool)
    gen = torch.Generator().manual_seed(4321)
    with torch.no_grad():  # GCNConv's bias starts at zero: move every bias
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _model(case, oracle=False):
    _, d_in, hidden, pool = CASES[case]
    m = (ref.GCN if oracle else GCN)(d_in, hidden, 5, dropout=0.0, pool=pool)
    m.load_state_dict(_state(case))
    return m.train()


@functools.lru_cache(maxsize=None)
def _ref64(case):
    """The oracle's step in float64, computed once per case: {parameter: gradient}."""
    out = twc.step(_model(case, oracle=True), _batch(case), torch.float64)
    return {k[len("grad/"):]: v for k, v in out.items() if k.startswith("grad/")}


def _step(m, b, cuda, ce_entry=False):
    """One step's (logits, loss, gradients). ce_entry: model and criterion as one node
    (GCN.forward_loss: the backward's _ce entry), else model then ops.cross_entropy (the
    logits-gradient entry where the head is folded, the dP entry otherwise)."""
    x, ei, bt, y = (t.to(cuda) for t in (b.x, b.edge_index, b.batch, b.y))
    m.zero_grad(set_to_none=True)
    if ce_entry:
        logits, loss = m.forward_loss(x, ei, bt, y, None, b.num_graphs)
    else:
        logits = m(x, ei, bt, b.num_graphs)
        loss = ops.cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return (logits.detach().cpu(), loss.detach().cpu(),
            {k: p.grad.detach().cpu() for k, p in m.named_parameters()})


def _check(case, cuda, monkeypatch, open_in_fused=None, ce_entry=False):
    b, want = _batch(case), _ref64(case)
    m = _model(case).to(cuda)
    if open_in_fused is not None:
        monkeypatch.setattr(ops, "OPEN_IN_FUSED", open_in_fused)
        monkeypatch.setattr(ops, "OPEN_IN_FUSED_BWD", open_in_fused)
    monkeypatch.setattr(ops, "FUSED_BWD", True)
    lf, lossf, gf = _step(m, b, cuda)
    _, _, gf2 = _step(m, b, cuda)
    monkeypatch.setattr(ops, "FUSED_BWD", False)
    ll, _, gl = _step(m, b, cuda)
    monkeypatch.setattr(ops, "FUSED_BWD", True)
    assert torch.equal(lf, ll)
    assert gf.keys() == want.keys()
    bad = []
    for k, w64 in want.items():
        e_new = (gf[k].double() - w64).abs().max().item()
        e_lw = (gl[k].double() - w64).abs().max().item()
        scale = w64.abs().max().item()
        bound = 3 * e_lw + 2e-7 * scale
        print(f"{case} {k}: err_fused {e_new:.3e} err_layerwise {e_lw:.3e} scale {scale:.3e} "
              f"bound {bound:.3e}")
        if not (e_new <= bound and bool(torch.isfinite(gf[k]).all())):
            bad.append((k, e_new, e_lw, scale))
    assert not bad, bad
    for k in gf:
        assert torch.equal(gf[k], gf2[k]), f"{k}: not repeatable"
    if ce_entry:
        lc, lossc, gc = _step(m, b, cuda, ce_entry=True)
        _, _, gc2 = _step(m, b, cuda, ce_entry=True)
        assert torch.equal(lc, lf) and torch.equal(lossc, lossf)
        for k in gf:
            assert torch.equal(gc[k], gf[k]), f"{k}: the _ce entry differs from the dlog entry"
            assert torch.equal(gc[k], gc2[k]), f"{k}: not repeatable (_ce entry)"


def test_two_tiles_per_workgroup_both_entries(cuda, monkeypatch):
    """300 closed tiles on 256 workgroups; model + CE (the logits-gradient entry) and
    forward_loss (the _ce entry) must agree bit for bit."""
    _check("two_tiles_per_wg", cuda, monkeypatch, ce_entry=True)


@pytest.mark.parametrize("case", ["narrow_in", "narrow_mid", "one_conv_add", "shared_tile",
                                  "all_open"])
def test_fold_vs_float64(cuda, case, monkeypatch):
    _check(case, cuda, monkeypatch)


@pytest.mark.parametrize("open_in_fused", ["1", "0"])
def test_open_tiles_add_into_folded_slots(cuda, open_in_fused, monkeypatch):
    """Closed tiles are folded, open tiles add their direct dW_0 into the same slots, inside the
    launch (after the fold) or in separate launches."""
    _check("open_and_closed", cuda, monkeypatch, open_in_fused=open_in_fused)
