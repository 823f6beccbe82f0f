"""CPU: tests/gat_ref.py and tests/gat_cases.py, what tests/test_gpu_gat_kernels.py stands on.

- the restated chain att -> fwd -> bwd_edge -> bwd_node (+ lin's backward) equals the float64
  autograd of oracle.pyg_ref.GATConv to 1e-10 relative, with and without a mask, with ELU and
  without, so the reference is pinned and not merely self-consistent;
- the CSR is what Graph.csr("gat") is documented to hold;
- the degree lists, the regime conditions and test f's logit margin hold for the committed seeds;
- the steadiness of the bar's scale (ref32 at one thread against the default thread count).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import oracle.pyg_ref as ref
from tests import gat_cases as gc
from tests import gat_ref as gr
from tests import trajectory_ref as tr

GRAPHS = ("degrees", "tiny")


class _Masks:
    """oracle.pyg_ref.DropoutMasks' interface around one given mask (flat, CSR order x head)."""

    def __init__(self, m):
        self.m = m

    def mask(self, stream, n):
        assert n == self.m.numel()
        return self.m.reshape(-1)


# three shapes: a narrow one-pass shape, a three-strip shape with a partial strip, NS = 2
@pytest.mark.parametrize("act", gc.ACTS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,C", [(3, 8), (5, 64), (2, 256)])
def test_chain_equals_oracle_autograd(H, C, masked, act):
    g = gc.graph("degrees")
    c = gc.e2e_case(H, C, "tiny")  # the conv's state; x below is drawn for `degrees`
    gen = torch.Generator().manual_seed(11 * H + C)
    x = torch.randn(g.n, gc.D_IN, generator=gen)
    dY = torch.randn(g.n, H * C, generator=gen)
    mask = gc.inputs(H, C, "degrees")["mask"] if masked else None
    conv = ref.GATConv(gc.D_IN, C, heads=H, dropout=gc.DROP_P if masked else 0.0)
    with torch.no_grad():
        conv.lin.weight.copy_(c["W"])
        conv.att_src.copy_(c["att_src"] * 3)
        conv.att_dst.copy_(c["att_dst"] * 3)
        conv.bias.copy_(c["bias"])
    conv = conv.double().train()
    xo = x.double().requires_grad_()
    y = conv(xo, g.edge_index, masks=_Masks(mask) if masked else None)
    if act == gr.ACT_ELU:
        y = F.elu(y)
    y.backward(dY.double())
    want = {"Y": y, "dx": xo.grad, "dW": conv.lin.weight.grad,
            "datt_src": conv.att_src.grad.view(-1), "datt_dst": conv.att_dst.grad.view(-1),
            "dbias": conv.bias.grad}
    got = gr.chain(x.double(), c["W"].double(), (c["att_src"] * 3).double().view(-1),
                   (c["att_dst"] * 3).double().view(-1), c["bias"].double(), g.csr, g.tcsr, H,
                   conv.negative_slope, None if mask is None else mask.double(), act, dY.double())
    for k, w in want.items():
        w = w.detach()
        err = (got[k] - w).abs().max().item()
        print(f"{k}: {err / w.abs().max().item():.3g} relative")
        assert err <= 1e-10 * w.abs().max().item(), k


@pytest.mark.parametrize("gname", GRAPHS)
def test_csr_layout(gname):
    """Rows by target; inside a row the edge list's order, explicit self loops removed, one self
    loop appended last; the transpose grouped by source with tmap into the target CSR."""
    g = gc.graph(gname)
    rows = [[] for _ in range(g.n)]
    for s, d in g.edge_index.t().tolist():
        if s != d:
            rows[d].append(s)
    for i in range(g.n):
        rows[i].append(i)
    assert g.csr.rowptr.tolist() == [0] + torch.tensor([len(r) for r in rows]).cumsum(0).tolist()
    assert g.csr.col.tolist() == [s for r in rows for s in r]
    assert g.csr.dst.tolist() == [i for i, r in enumerate(rows) for _ in r]
    t = g.tcsr
    nnz = g.csr.col.numel()
    assert sorted(t.tmap.tolist()) == list(range(nnz))
    assert torch.equal(g.csr.col[t.tmap], t.src) and torch.equal(g.csr.dst[t.tmap], t.tidx)
    assert torch.equal(t.src, torch.sort(t.src).values)
    assert gc.row_lengths(t.tptr) == torch.bincount(g.csr.col, minlength=g.n).tolist()


def test_degrees_graph():
    g = gc.graph("degrees")
    assert g.n == 347 and g.n % 8 != 0
    rl, tl = gc.row_lengths(g.csr.rowptr), gc.row_lengths(g.tcsr.tptr)
    for k, length in enumerate(gc.LENGTHS):
        assert rl[k] == length and tl[20 + k] == length
    assert rl[gc.HUB] == 301 and tl[gc.FEEDER] == 301
    assert len(set(g.tcsr.tidx[g.tcsr.tptr[gc.FEEDER]:g.tcsr.tptr[gc.FEEDER + 1]].tolist())) == 301
    row45 = g.csr.col[g.csr.rowptr[45]:g.csr.rowptr[46]].tolist()
    assert row45.count(41) == 2 and row45[-1] == 45           # the doubled edge counts twice
    ei = g.edge_index
    assert int(((ei[0] == 2) & (ei[1] == 2)).sum()) == 1       # the explicit self loop
    row2 = g.csr.col[g.csr.rowptr[2]:g.csr.rowptr[3]].tolist()
    assert row2.count(2) == 1 and row2[-1] == 2 and len(row2) == 3
    nnz = g.csr.col.numel()
    assert nnz <= 2700 and ei.size(1) + g.n == nnz + 1         # capacity: one row past nnz
    assert torch.bincount(g.batch, minlength=4).tolist() == [120, 0, 200, 27]
    assert g.gptr.tolist() == [0, 120, 120, 320, 347] and g.num_graphs == 4


def test_tiny_graph():
    g = gc.graph("tiny")
    assert g.n == 3 and g.edge_index.tolist() == [[0, 1], [1, 0]]
    assert g.csr.rowptr.tolist() == [0, 2, 4, 5] and g.csr.col.tolist() == [1, 0, 0, 1, 2]
    assert g.batch.tolist() == [0, 1, 1] and g.gptr.tolist() == [0, 1, 3]


def test_shape_groups():
    assert [gc.form(*s) for s in gc.SHAPES] == ["p1"] * 6 + ["p2"] * 3 + ["ps"] * 6 + ["row"] * 7
    assert [gc.ns_of(c) for _, c in gc.SHAPES_ROW] == [1, 1, 1, 1, 2, 2, 4]
    assert all(gc.form(*s, pipe=0) == "row" for s in gc.SHAPES)
    assert len(gc.PIPE_SHAPES) == 15 and len(gc.RUNS) == 37
    assert sorted(gc.form(*s) + str(gc.ns_of(s[1])) for s in gc.ALT_SLOPE_SHAPES) == \
        ["p11", "p21", "ps1", "row1", "row2", "row4"]
    for H, C in gc.SHAPES:  # what gat.hip's shape_ok accepts
        assert C >= 4 and C & (C - 1) == 0 and H * C <= 512


def _row_range(e, g):
    idx = g.csr.dst[:, None].expand_as(e)
    z = torch.zeros(g.n, e.size(1), dtype=e.dtype)
    return (z.scatter_reduce(0, idx, e, "amax", include_self=False) -
            z.scatter_reduce(0, idx, e, "amin", include_self=False))


@pytest.mark.parametrize("gname", GRAPHS)
@pytest.mark.parametrize("H,C", gc.SHAPES)
def test_regime_conditions(H, C, gname):
    g = gc.graph(gname)
    i = gc.inputs(H, C, gname)
    deg = torch.tensor(gc.row_lengths(g.csr.rowptr))
    lg = {r: gr.logits(*gc.cpu_scores(H, C, gname, r), g.csr, gc.SLOPE) for r in gc.REGIMES}
    # init: where the model tests live, no overflow without the max subtraction
    assert lg["init"].abs().max() < 20
    # peaked
    e = lg["peaked"]
    wide = (_row_range(e, g)[deg >= 2] > 88).double().mean().item()
    print(f"peaked: logits [{e.min():.1f}, {e.max():.1f}], {wide:.3f} of the (row, head) pairs "
          "with two or more entries range over more than 88")
    assert e.max() > 88.7 and e.min() < -20
    if gname == "degrees":
        assert wide >= 0.25
    else:  # two such rows: the fraction is a coin per head; some pair has the range
        assert wide > 0
    # negative: every logit negative; zero: every logit exactly 0 and alpha = 1 / deg
    assert lg["negative"].max() < 0
    assert torch.count_nonzero(lg["zero"]) == 0
    a_s, a_d = gc.cpu_scores(H, C, gname, "zero")
    alpha, _ = gr.fwd(i["XP"].double(), a_s, a_d, g.csr, gc.SLOPE, None, None, gr.ACT_NONE)
    torch.testing.assert_close(alpha, (1.0 / deg.double())[g.csr.dst][:, None].expand_as(alpha),
                               rtol=1e-15, atol=0)
    # the mask: [nnz, H] of 0 and 1 / (1 - p); one row wholly dropped, the hub partly
    m = i["mask"]
    assert m.shape == (g.csr.col.numel(), H)
    assert set(m.unique().tolist()) <= {0.0, gc.f32(1 / (1 - gc.DROP_P))}
    if gname == "degrees":
        hub = m[g.csr.rowptr[gc.HUB]:g.csr.rowptr[gc.HUB + 1]]
        assert 0 < torch.count_nonzero(hub) < hub.numel()
        assert torch.count_nonzero(m[g.csr.rowptr[gc.DROPPED_ROW]:
                                     g.csr.rowptr[gc.DROPPED_ROW + 1]]) == 0
        for act in gc.ACTS:  # the dropped row's output is act(bias)
            a_s, a_d = gc.cpu_scores(H, C, gname, "peaked")
            _, Y = gr.fwd(i["XP"].double(), a_s, a_d, g.csr, gc.SLOPE, m.double(),
                          i["bias"].double(), act)
            b = i["bias"].double()
            # (a vectorised and a scalar expm1 may differ in the last place)
            torch.testing.assert_close(Y[gc.DROPPED_ROW], F.elu(b) if act == gr.ACT_ELU else b,
                                       rtol=1e-15, atol=0)


@pytest.mark.parametrize("H,C", gc.SHAPES)
def test_e2e_logit_margin(H, C):
    """Test f's condition: in ref64 the smallest |logit| is at least 1e-4 x the largest."""
    for gname in gc.e2e_graphs(H, C):
        for regime in ("init", "peaked"):
            m = gc.e2e_oracle(H, C, gname, regime, None, torch.float64)["logit_margin"].item()
            print(f"({H}, {C}) {gname} {regime}: min|logit| / max|logit| = {m:.3g}")
            assert m >= gc.E2E_MARGIN
    assert gc.D_IN == 36


def test_ref32_thread_steadiness():
    """How steady the bar's scale is: ref32 at one CPU thread against ref32 at the default thread
    count, under the bar's formula, over every shape on `degrees` (init with a mask, peaked). A
    measurement (printed; recorded in tests/gat_cases.py), with a loose sanity bound."""
    threads = torch.get_num_threads()
    worst = (0.0, "")
    try:
        for H, C in gc.SHAPES:
            for regime, masked in (("init", True), ("peaked", False)):
                case = (H, C, "degrees", regime, masked, gr.ACT_ELU, gc.SLOPE)
                arrays = gc.host_arrays(*case)
                r64 = gc.stage_refs(*case, arrays, torch.float64)
                r32 = gc.stage_refs(*case, arrays, torch.float32)
                torch.set_num_threads(1)
                one = gc.stage_refs(*case, arrays, torch.float32)
                torch.set_num_threads(threads)
                r = gc.ratios(one, r64, r32)
                k = max(r, key=r.get)
                if r[k] > worst[0]:
                    worst = (r[k], f"({H}, {C}) {regime} {k}")
    finally:
        torch.set_num_threads(threads)
    print(f"ref32 at 1 thread vs {threads}: worst ratio {worst[0]:.3g} at {worst[1]}")
    assert math.isfinite(worst[0]) and worst[0] <= 16
