"""Fused split-3 GCN backward with the in_proj fold deferred (stack3_bwd.hip k_s3_fbwd, DF mode;
foldgrad.hip; loss.hip's `live` reduction).

in_proj has no activation, so with G_1 = Â^T dZ_1, T = G_1^T X and g = colsum G_1
    dW_0 = W_1^T T,   db_0 = W_1^T g,   dW_1 = T W_0^T + g b_0^T
are linear in (T, g): the closed tiles only sum T and g per workgroup, the slabs are reduced, and one
lgnn_gcn_fold_wgrad launch forms the three gradients per step. The open tiles' direct sums of those
three gradients go through slabs of their own whose reductions are skipped (`live` = the open-tile
count word) when no tile is open; the T / g slabs likewise when the launch has no closed tile (the
closed-tile count word the kernel writes behind the g slab).

The bar is tests/test_gpu_s3f_fold.py's, for every parameter
    max|grad_fused - ref64| <= 3 * max|grad_layerwise - ref64| + 2e-7 * max|ref64|
(the layer-wise backward, ops.FUSED_BWD = False, is the fp32 yardstick on the same step; ref64 the
plain-torch oracle in float64). Every case runs twice and must repeat bit for bit, through the
logits-gradient entry and through the _ce entry, which must agree bitwise. With ops.DEFER_FOLD off
against on, logits, loss and every gradient the fold does not form are bitwise equal. b_0 carries
an extra N(0, 1) term, so a missing g b_0^T term fails by orders of magnitude. Workspaces start as
NaN (the idiom of tests/test_gpu_tile_widths.py): a slot nobody wrote, or a dead slab that is read
all the same, shows.
"""
import functools

import pytest
import torch

import oracle.pyg_ref as ref
from lesion_gnn_amd import _lib, ops, synth
from lesion_gnn_amd.models import GCN
from tests import tile_width_cases as twc

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FE5C3A1  # a quiet NaN with a payload no kernel produces

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
# the gradients the fold launch forms (another summation order than the legacy mode's)
FOLDED = ("in_proj.weight", "in_proj.bias", "convs.0.lin.weight")


class _SentinelTorch:
    """`torch` as ops.py sees it, except that every float32 torch.empty on the device starts as a
    NaN pattern."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kw):
        t = torch.empty(*args, **kw)
        if t.dtype == torch.float32 and t.is_cuda:
            t.view(torch.int32).fill_(SENTINEL)
        return t


@pytest.fixture(autouse=True)
def poisoned_workspaces(monkeypatch):
    monkeypatch.setattr(ops, "torch", _SentinelTorch())


@functools.lru_cache(maxsize=None)
def _batch(case):
    kw, d_in, _, _ = CASES[case]
    return synth.make_batch(d_in=d_in, seed=80 + list(CASES).index(case), **kw)


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
        m.in_proj.bias.add_(torch.randn(m.in_proj.bias.shape, generator=gen))
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


class _Names:
    def __init__(self):
        self.names = []

    def __call__(self, name, args, launch):
        self.names.append(name)
        return launch()


def _check(case, cuda, monkeypatch, open_in_fused=None):
    b, want = _batch(case), _ref64(case)
    m = _model(case).to(cuda)
    assert set(FOLDED) <= set(want)
    if open_in_fused is not None:
        monkeypatch.setattr(ops, "OPEN_IN_FUSED", open_in_fused)
        monkeypatch.setattr(ops, "OPEN_IN_FUSED_BWD", open_in_fused)
    monkeypatch.setattr(ops, "FUSED_BWD", True)
    monkeypatch.setattr(ops, "DEFER_FOLD", True)
    tracer = _Names()
    _lib.set_tracer(tracer)
    try:
        lf, lossf, gf = _step(m, b, cuda)
    finally:
        _lib.set_tracer(None)
    assert "lgnn_gcn_fold_wgrad" in tracer.names, tracer.names  # the deferred route ran
    _, _, gf2 = _step(m, b, cuda)
    lc, lossc, gc = _step(m, b, cuda, ce_entry=True)
    _, _, gc2 = _step(m, b, cuda, ce_entry=True)
    monkeypatch.setattr(ops, "DEFER_FOLD", False)
    lo, losso, go = _step(m, b, cuda)
    monkeypatch.setattr(ops, "FUSED_BWD", False)
    ll, _, gl = _step(m, b, cuda)
    monkeypatch.setattr(ops, "FUSED_BWD", True)
    monkeypatch.setattr(ops, "DEFER_FOLD", True)
    assert torch.equal(lf, ll)
    assert gf.keys() == want.keys()
    bad = []
    for k, w64 in want.items():
        e_new = (gf[k].double() - w64).abs().max().item()
        e_lw = (gl[k].double() - w64).abs().max().item()
        scale = w64.abs().max().item()
        bound = 3 * e_lw + 2e-7 * scale
        print(f"{case} {k}: err_deferred {e_new:.3e} err_layerwise {e_lw:.3e} scale {scale:.3e} "
              f"bound {bound:.3e}")
        if not (e_new <= bound and bool(torch.isfinite(gf[k]).all())):
            bad.append((k, e_new, e_lw, scale))
    assert not bad, bad
    assert torch.equal(lc, lf) and torch.equal(lossc, lossf)
    assert torch.equal(lo, lf) and torch.equal(losso, lossf)
    for k in gf:
        assert torch.equal(gf[k], gf2[k]), f"{k}: not repeatable"
        assert torch.equal(gc[k], gf[k]), f"{k}: the _ce entry differs from the dlog entry"
        assert torch.equal(gc[k], gc2[k]), f"{k}: not repeatable (_ce entry)"
        if k not in FOLDED:
            assert torch.equal(go[k], gf[k]), f"{k}: differs from the legacy mode"


@pytest.mark.parametrize("case", ["two_tiles_per_wg", "narrow_in", "narrow_mid", "one_conv_add",
                                  "shared_tile", "all_open"])
def test_defer_vs_float64(cuda, case, monkeypatch):
    _check(case, cuda, monkeypatch)


@pytest.mark.parametrize("open_in_fused", ["1", "0"])
def test_open_tiles_with_deferred_fold(cuda, open_in_fused, monkeypatch):
    """Closed and open tiles together: the open-only slabs of layers 0 and 1 are live, written
    inside the launch or by separate launches, and the fold adds their totals."""
    _check("open_and_closed", cuda, monkeypatch, open_in_fused=open_in_fused)


# ---------------------------------------------------------------------------------------------
# the fold launch alone
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("widths", [(128, 128, 128), (36, 64, 32), (128, 16, 128)])
@pytest.mark.parametrize("with_open", [False, True])
def test_fold_entry_vs_float64(cuda, widths, with_open):
    """lgnn_gcn_fold_wgrad on random operands, (d_in, w1, w2) as the model cases have them. Each
    output element is one fp32 FMA chain of n <= 129 terms (+ one add of the open total), so
    |err| <= (n + 2) u sum|terms| with u = 2^-24 (the standard bound of a recursive sum), taken
    element by element from the float64 magnitudes."""
    d_in, w1, w2 = widths
    gen = torch.Generator().manual_seed(7 + d_in + w1 + w2)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float32)

    T, g, W0, b0, W1 = rnd(w2, d_in), rnd(w2), rnd(w1, d_in), rnd(w1), rnd(w2, w1)
    o0, ob, o1 = rnd(w1, d_in), rnd(w1), rnd(w2, w1)
    dev = [t.to(cuda) for t in (T, g, W0, b0, W1)]
    opens = [t.to(cuda) for t in (o0, ob, o1)] if with_open else [None, None, None]
    outs = []
    for _ in range(2):
        dW0 = torch.full((w1, d_in), float("nan"), device=cuda)
        db0 = torch.full((w1,), float("nan"), device=cuda)
        dW1 = torch.full((w2, w1), float("nan"), device=cuda)
        _lib.call("lgnn_gcn_fold_wgrad", *dev, d_in, w1, w2, *opens, None, dW0, db0, dW1,
                  _lib.stream(cuda))
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in (dW0, db0, dW1)])
    for a, c in zip(*outs):
        assert torch.equal(a, c), "not repeatable"
    T6, g6, W06, b06, W16 = (t.double() for t in (T, g, W0, b0, W1))
    z = torch.zeros((), dtype=torch.float64)
    add = [t.double() if with_open else z for t in (o0, ob, o1)]
    want = [W16.t() @ T6 + add[0], W16.t() @ g6 + add[1], T6 @ W06.t() + torch.outer(g6, b06) + add[2]]
    mag = [W16.abs().t() @ T6.abs() + add[0].abs(), W16.abs().t() @ g6.abs() + add[1].abs(),
           T6.abs() @ W06.abs().t() + torch.outer(g6.abs(), b06.abs()) + add[2].abs()]
    terms = [w2, w2, d_in + 1]
    for name, got, w, mg, n in zip(("dW0", "db0", "dW1"), outs[0], want, mag, terms):
        err = (got.double() - w).abs()
        bound = (n + 2) * 2.0 ** -24 * mg
        print(f"{widths} open={with_open} {name}: max err {err.max().item():.3e}, "
              f"max err / bound {(err / bound).max().item():.3f}")
        assert got.shape == w.shape and bool((err <= bound).all()), name


def test_fold_entry_dead_word(cuda):
    """live = 0: T and g (NaN here) are not used; the outputs are the open totals, bitwise (in
    place, as ops runs it), or zeros without them. live = 1: as without a word, bitwise."""
    d_in, w1, w2 = 36, 64, 32
    gen = torch.Generator().manual_seed(5)
    W0, b0, W1 = (torch.randn(*sh, generator=gen).to(cuda) for sh in ((w1, d_in), (w1,), (w2, w1)))
    T, g = torch.randn(w2, d_in, generator=gen).to(cuda), torch.randn(w2, generator=gen).to(cuda)
    nanT, nang = torch.full_like(T, float("nan")), torch.full_like(g, float("nan"))
    zero = torch.zeros(1, dtype=torch.int32, device=cuda)
    one = torch.ones(1, dtype=torch.int32, device=cuda)
    opens = [torch.randn(*sh, generator=gen).to(cuda) for sh in ((w1, d_in), (w1,), (w2, w1))]
    outs = [t.clone() for t in opens]
    _lib.call("lgnn_gcn_fold_wgrad", nanT, nang, W0, b0, W1, d_in, w1, w2, *outs, zero, *outs,
              _lib.stream(cuda))
    fresh = [torch.full_like(t, float("nan")) for t in opens]
    _lib.call("lgnn_gcn_fold_wgrad", nanT, nang, W0, b0, W1, d_in, w1, w2, None, None, None, zero,
              *fresh, _lib.stream(cuda))
    a = [torch.full_like(t, float("nan")) for t in opens]
    b = [torch.full_like(t, float("nan")) for t in opens]
    _lib.call("lgnn_gcn_fold_wgrad", T, g, W0, b0, W1, d_in, w1, w2, *opens, one, *a,
              _lib.stream(cuda))
    _lib.call("lgnn_gcn_fold_wgrad", T, g, W0, b0, W1, d_in, w1, w2, *opens, None, *b,
              _lib.stream(cuda))
    torch.cuda.synchronize()
    for o, w, f, x, y in zip(outs, opens, fresh, a, b):
        assert torch.equal(o, w) and torch.equal(f, torch.zeros_like(f)) and torch.equal(x, y)


# ---------------------------------------------------------------------------------------------
# the reduction with live words
# ---------------------------------------------------------------------------------------------

def test_reduce_live_words(cuda):
    """live = 0: the slab (NaN) is not read and out is exact zeros; live = 1 or no word: the sums
    of lgnn_reduce_jobs, bitwise. One long job (the 16-byte path) and short ones."""
    gen = torch.Generator().manual_seed(11)
    P = 37
    lens = [128 * 128, 100, 128 * 36, 7]
    slabs = [torch.randn(P * n, generator=gen).to(cuda) for n in lens]
    nan = [torch.full((P * n,), float("nan"), device=cuda) for n in lens]
    want = [torch.empty(n, device=cuda) for n in lens]
    _lib.call("lgnn_reduce_jobs", len(lens), slabs, None, None, [P] * len(lens), lens, want,
              _lib.stream(cuda))
    one = torch.ones(1, dtype=torch.int32, device=cuda)
    zero = torch.zeros(1, dtype=torch.int32, device=cuda)
    # jobs 0..3 live (word 1, or none), then the same shapes dead on NaN slabs
    parts = slabs + nan
    live = [one, None, None, one] + [zero] * len(lens)
    outs = [torch.full((n,), float("nan"), device=cuda) for n in lens + lens]
    _lib.call("lgnn_reduce_jobs_live", len(parts), parts, None, None, [P] * len(parts),
              lens + lens, outs, None, None, 0, live, _lib.stream(cuda))
    torch.cuda.synchronize()
    for j, n in enumerate(lens):
        assert torch.equal(outs[j], want[j]), f"live job {j}"
        dead = outs[len(lens) + j]
        assert torch.equal(dead, torch.zeros(n, device=cuda)), f"dead job {j}"
        assert not bool(torch.signbit(dead).any())

