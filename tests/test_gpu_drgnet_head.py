"""The DRGNet head kernels (lgnn_drgnet_head_fwd / _bwd, csrc/drgnet_head.hip) on the GPU.

* Kernel against the float64 restatement of tests/drgnet_head_ref.py, on inputs built as sort
  pooling builds them (a random number of real rows per graph, one graph full, one with a single
  real row, zero rows after). The project's fp32 bar: logits 1e-4 absolute; dx and every parameter
  gradient 1e-4 x max|grad| of that tensor, floor 1e-6. Each case first asserts its own
  conditioning in float64: every pooled pair that is not two padding rows has
  |ELU(z1[2q]) - ELU(z1[2q + 1])| >= 1e-5, so no max-pool choice hangs on fp32 rounding.
* Exact properties: the dropped last row of an odd k has dx exactly 0; tied pairs send their
  whole gradient to the first row; two runs agree bit for bit.
* Dropout: DRGNet in train() against the oracle's GraphConv stack + sort_aggregation followed by
  the restated head under the mask regenerated from (seed, counter); the counter's advance.
* The compiled training-mode DRGNet is one graph and matches eager bit for bit, also at a second
  batch size. Unsupported shapes raise.
"""
import functools

import pytest
import torch

import oracle.pyg_ref as ref
from lesion_gnn_amd import _lib, dropout, ops, synth
from lesion_gnn_amd.models.drgnet import DRGNet
from tests import drgnet_head_ref as hr

pytestmark = pytest.mark.gpu

# (B, k, D, c0, c1, C) -> seed (chosen so that the conditioning assertion holds)
CASES = {
    (67, 30, 97, 16, 32, 5): 1,     # the reference shape; B no multiple of the graphs per pass
    (5, 10, 3, 16, 32, 1): 1,       # P = 1; D below one MFMA k-step; the regression head
    (9, 11, 9, 5, 7, 5): 1,         # odd k; channel counts that fill no tile
    (1, 12, 33, 16, 32, 5): 1,      # B = 1
    (16, 30, 1025, 16, 32, 5): 1,   # D streamed in chunks with a ragged last chunk
    # beyond the issue's five: enough graphs for three per pass (a conv1 tile spanning two
    # graphs, the last pass holding one) and for workgroups that add a second pass to their slab
    (2050, 10, 3, 16, 32, 5): 1,
}
H = 128


def _uniform(gen, *shape, fan_in):
    bound = fan_in ** -0.5
    return (torch.rand(*shape, generator=gen) * 2 - 1) * bound


def make_case(B, k, D, c0, c1, C, seed, hidden=H):
    """(x, real_rows, params, mask-free dlogits): fp32 values; x as SortAggregation leaves it."""
    gen = torch.Generator().manual_seed(seed)
    rows = torch.randint(1, k + 1, (B,), generator=gen)
    rows[0] = k
    if B > 1:
        rows[-1] = 1
    x = torch.randn(B, k, D, generator=gen)
    x = x * (torch.arange(k).view(1, k, 1) < rows.view(B, 1, 1))
    P = k // 2 - 4
    params = (_uniform(gen, c0, 1, D, fan_in=D), _uniform(gen, c0, fan_in=D),
              _uniform(gen, c1, c0, 5, fan_in=5 * c0), _uniform(gen, c1, fan_in=5 * c0),
              _uniform(gen, hidden, c1 * P, fan_in=c1 * P), _uniform(gen, hidden, fan_in=c1 * P),
              _uniform(gen, C, hidden, fan_in=hidden), _uniform(gen, C, fan_in=hidden))
    dlogits = torch.randn(B, C, generator=gen)
    return x.reshape(B, k * D).contiguous(), rows, params, dlogits


def reference(x, k, params, dlogits, mask=None):
    """float64 logits, dx and parameter gradients of the restated head."""
    xd = x.double().requires_grad_(True)
    pd = [p.double().requires_grad_(True) for p in params]
    out = hr.head(xd, k, *pd, mask=None if mask is None else mask.double())
    out.backward(dlogits.double())
    return out.detach(), xd.grad, [p.grad for p in pd]


@functools.lru_cache(maxsize=None)
def case_data(case):
    x, rows, params, dlogits = make_case(*case, seed=CASES[case])
    return x, rows, params, dlogits, reference(x, case[1], params, dlogits)


def run_gpu(dev, x, k, params, dlogits, mask=None):
    xg = x.to(dev).requires_grad_(True)
    pg = [p.to(dev).requires_grad_(True) for p in params]
    out = ops.drgnet_head(xg, k, *pg, mask=None if mask is None else mask.to(dev))
    out.backward(dlogits.to(dev))
    return out.detach().cpu(), xg.grad.cpu(), [p.grad.cpu() for p in pg]


def check(got, want, what):
    """Every figure is printed before the first assertion, so one run shows them all."""
    lo, dx, gp = got
    wlo, wdx, wgp = want
    err = (lo.double() - wlo).abs().max().item()
    print(f"{what}: logits max|err| {err:.3e}")
    figures = []
    for name, g, w in [("dx", dx, wdx)] + list(zip(hr.PARAM_NAMES, gp, wgp)):
        assert g.shape == w.shape, (what, name)
        s = w.abs().max().item()
        e = (g.double() - w).abs().max().item()
        print(f"{what}: {name} max|err| {e:.3e} of max|grad| {s:.3e} (rel {e / max(s, 1e-30):.2e})")
        figures.append((name, e, s))
    assert err <= 1e-4, (what, err)
    for name, e, s in figures:
        assert e <= max(1e-4 * s, 1e-6), (what, name, e, s)


@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "x".join(map(str, c)))
def test_head_vs_float64(cuda, case):
    B, k, D, c0, c1, C = case
    x, rows, params, dlogits, want = case_data(case)
    gap = hr.pair_gaps(x.double(), k, params[0].double(), params[1].double(), rows)
    print(f"{case}: smallest pooled-pair gap {gap:.3e}")
    assert gap >= 1e-5
    assert int(rows.max()) == k and (B == 1 or int(rows.min()) == 1)
    got = run_gpu(cuda, x, k, params, dlogits)
    check(got, want, str(case))
    if k % 2:  # the row MaxPool1d drops
        assert torch.count_nonzero(got[1].view(B, k, D)[:, k - 1]) == 0
    # rows past a graph's size sit in tied pairs (or behind a real first row): whatever reaches
    # them is what the float64 restatement routes there, checked above; the second row of a pair
    # of two padding rows gets nothing
    dx = got[1].view(B, k, D)
    for b in range(B):
        first_pad_pair = (int(rows[b]) + 1) // 2
        for q in range(first_pad_pair, k // 2):
            assert torch.count_nonzero(dx[b, 2 * q + 1]) == 0


@pytest.mark.parametrize("case", [(9, 11, 9, 5, 7, 5), (67, 30, 97, 16, 32, 5)],
                         ids=lambda c: "x".join(map(str, c)))
def test_ties_go_to_the_first_row(cuda, case):
    """conv1.weight = 0 makes every pair an exact tie (both rows give ELU(b1)); with a positive
    incoming gradient the routing shows in conv1.weight's gradient (it sums the rows the pool
    chose) and in dx (all zero: W1^T dz1). Then real weights on duplicated rows (x[2q + 1] =
    x[2q]): the same arithmetic on the same data ties exactly, and the second row's dx must be
    exactly 0 while the first carries the restatement's gradient."""
    B, k, D, c0, c1, C = case
    x, rows, params, dlogits, _ = case_data(case)
    pos = dlogits.abs() + 0.1
    zeroed = (torch.zeros_like(params[0]),) + params[1:]
    want = reference(x, k, zeroed, pos)
    got = run_gpu(cuda, x, k, zeroed, pos)
    check(got, want, f"{case} W1 = 0")
    assert want[2][0].abs().max() > 0  # the routing is visible in conv1.weight's gradient
    xv = x.view(B, k, D).clone()
    K2 = k // 2
    xv[:, 1:2 * K2:2] = xv[:, 0:2 * K2:2]
    xdup = xv.reshape(B, k * D)
    want = reference(xdup, k, params, pos)
    got = run_gpu(cuda, xdup, k, params, pos)
    check(got, want, f"{case} duplicated rows")
    dx = got[1].view(B, k, D)
    assert torch.count_nonzero(dx[:, 1:2 * K2:2]) == 0
    assert torch.count_nonzero(dx[:, 0:2 * K2:2]) > 0
    assert torch.count_nonzero(want[1].view(B, k, D)[:, 1:2 * K2:2]) == 0


@pytest.mark.parametrize("case", [(9, 11, 9, 5, 7, 5), (67, 30, 97, 16, 32, 5)],
                         ids=lambda c: "x".join(map(str, c)))
def test_two_runs_agree_bitwise(cuda, case):
    x, rows, params, dlogits, _ = case_data(case)
    mask = (torch.rand(case[0], H, generator=torch.Generator().manual_seed(3)) < 0.5).float() * 2
    a = run_gpu(cuda, x, case[1], params, dlogits, mask)
    b = run_gpu(cuda, x, case[1], params, dlogits, mask)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for name, ga, gb in zip(hr.PARAM_NAMES, a[2], b[2]):
        assert torch.equal(ga, gb), name
    check(a, reference(x, case[1], params, dlogits, mask), f"{case} masked")


def test_odd_hidden_width(cuda):
    """H odd: the weight-gradient GEMM runs on H + 1 padded columns; the gradients are the first H
    rows."""
    x, rows, params, dlogits = make_case(7, 12, 6, 4, 3, 2, seed=5, hidden=9)
    got = run_gpu(cuda, x, 12, params, dlogits)
    check(got, reference(x, 12, params, dlogits), "H = 9")


# ---- dropout: DRGNet in training mode against the oracle -----------------------------------------


def _key_margin(oref, b, ew, k):
    """Smallest gap between consecutive sort keys (last channel of the concatenated GraphConv
    outputs) among each graph's top k + 1 in the oracle: sort pooling is discontinuous in them."""
    x, xs = b.x.to(ew.dtype), []
    for c in oref.graph_convs:
        x = torch.nn.functional.elu(c(x, b.edge_index, ew))
        xs.append(x)
    key = torch.cat(xs, 1)[:, -1].detach()
    ptr, m = b.ptr.tolist(), float("inf")
    for g in range(len(ptr) - 1):
        kk = key[ptr[g]:ptr[g + 1]].sort(descending=True).values[:k + 1]
        if kk.numel() > 1:
            m = min(m, float((kk[:-1] - kk[1:]).min()))
    return m


def _oracle_step(oref, b, ew, k, mask, y):
    """Loss gradients of the oracle's GraphConv stack + sort_aggregation + the restated head."""
    oref.zero_grad(set_to_none=True)
    x, xs = b.x.double(), []
    for c in oref.graph_convs:
        x = torch.nn.functional.elu(c(x, b.edge_index, ew))
        xs.append(x)
    pooled = ref.sort_aggregation(torch.cat(xs, dim=1), b.batch, k, b.num_graphs)
    head = [oref.conv1.weight, oref.conv1.bias, oref.conv2.weight, oref.conv2.bias,
            oref.mlp.lins[0].weight, oref.mlp.lins[0].bias, oref.mlp.lins[1].weight,
            oref.mlp.lins[1].bias]
    logits = hr.head(pooled, k, *head, mask=mask)
    torch.nn.functional.cross_entropy(logits, y).backward()
    return logits.detach(), {n: p.grad.clone() for n, p in oref.named_parameters()}


def test_drgnet_training_step_with_dropout(cuda):
    d_in, hidden, layers, k, classes, B = 16, 8, 2, 10, 5, 20
    seed, counter = 0x1234ABCD, 7
    b = synth.make_batch(B, n=24, k=6, d_in=d_in, seed=32, sizes="lognormal")
    ew = ref.gaussian_distance(b.edge_index, b.pos, 0.1).double()
    torch.manual_seed(1234)
    ours = DRGNet(d_in, hidden, layers, k, classes)
    with torch.no_grad():  # out of ELU saturation, as tests/test_gpu_drgnet.py
        for c in ours.graph_convs:
            c.lin_rel.weight.mul_(0.25)
            c.lin_root.weight.mul_(0.25)
    oref = ref.DRGNet(d_in, hidden, layers, k, classes)
    oref.load_state_dict(ours.state_dict())
    oref = oref.double()
    assert _key_margin(oref, b, ew, k) >= 1e-5
    ours = ours.to(cuda).train()
    dropout.set_state(ours._dropout_rng, seed, counter)
    y = b.y % classes
    args = (b.x.to(cuda), b.edge_index.to(cuda), b.batch.to(cuda), ew.float().to(cuda),
            b.num_graphs)
    for step in range(2):  # the second step draws from counter + 1
        mask = ref.DropoutMasks(seed, counter + step, 0.5).mask(0, B * 128).view(B, 128).double()
        assert 0 < int((mask == 0).sum()) < mask.numel() and float(mask.max()) == 2.0
        want, wg = _oracle_step(oref, b, ew, k, mask, y)
        ours.zero_grad(set_to_none=True)
        lo = ours(*args)
        torch.nn.functional.cross_entropy(lo, y.to(cuda)).backward()
        assert dropout.get_state(ours._dropout_rng) == (seed, counter + step + 1)
        err = (lo.detach().cpu().double() - want).abs().max().item()
        print(f"step {step}: logits max|err| {err:.3e}")
        assert err <= 1e-4
        for (n1, g1), (n2, p2) in zip(wg.items(), ours.named_parameters()):
            assert n1 == n2
            s = g1.abs().max().item()
            e = (p2.grad.cpu().double() - g1).abs().max().item()
            print(f"step {step}: {n1} max|err| {e:.3e} of {s:.3e}")
            assert e <= max(1e-4 * s, 1e-6), (n1, e, s)
    ours.eval()
    with torch.no_grad():
        ev = ours(*args)
    assert dropout.get_state(ours._dropout_rng) == (seed, counter + 2)  # eval draws nothing
    want_eval, _ = _oracle_step(oref, b, ew, k, None, y)
    assert (ev.cpu().double() - want_eval).abs().max().item() <= 1e-4


# ---- compile --------------------------------------------------------------------------------------


def test_compiled_training_drgnet_matches_eager_bitwise(cuda):
    """Compiled (dynamic=True, fullgraph=True) DRGNet in train() against eager from the same
    generator state, at two batch sizes with one compilation: logits and every gradient bit for
    bit. That holds because no torch elementwise op is left between the lgnn ops: the sum of
    GraphConv's branches and the ELU after it are ops.add_elu (with torch's `rel + root` and
    F.elu there, Inductor's generated ELU differed from eager's in the last bits of some node
    rows, and the GraphConv weight gradients with it: up to 6e-8 of 1.0)."""
    import copy

    torch.manual_seed(1234)
    m = DRGNet(16, 8, 2, 10, 5).train()
    eager, comp = copy.deepcopy(m).to(cuda), copy.deepcopy(m).to(cuda)
    torch._dynamo.reset()
    torch._dynamo.utils.counters.clear()
    compiled = torch.compile(comp, dynamic=True, fullgraph=True)
    for i, B in enumerate((48, 21)):
        b = synth.make_batch(B, n=24, k=6, d_in=16, seed=32 + i, sizes="lognormal")
        ew = ref.gaussian_distance(b.edge_index, b.pos, 0.1).float()
        args = (b.x.to(cuda), b.edge_index.to(cuda), b.batch.to(cuda), ew.to(cuda), b.num_graphs)
        outs = []
        for model in (compiled, eager):
            dropout.set_state(model._dropout_rng, 99, 5 + i)
            model.zero_grad(set_to_none=True)
            lo = model(*args)
            torch.nn.functional.cross_entropy(lo, b.y.to(cuda)).backward()
            assert dropout.get_state(model._dropout_rng) == (99, 6 + i)
            outs.append((lo.detach().cpu(), [p.grad.cpu() for p in model.parameters()]))
        (lc, gc), (le, ge) = outs
        names = [n for n, _ in eager.named_parameters()]
        for n, a, e in zip(names, gc, ge):  # every figure before the first assertion
            print(f"B = {B}: {n} max|compiled - eager| {(a - e).abs().max().item():.3e} of "
                  f"{e.abs().max().item():.3e}")
        assert torch.equal(lc, le), (lc - le).abs().max()
        for n, a, e in zip(names, gc, ge):
            assert torch.equal(a, e), n
    assert torch._dynamo.utils.counters["stats"]["unique_graphs"] <= 2  # no per-size recompile


# ---- ELU(a + b): GraphConv's branch sum and activation ----------------------------------------------


def test_add_elu_vs_float64(cuda):
    """ops.add_elu against float64. Forward: one fp32 add (0.5 ulp) and expm1f (2 ulp) leave at
    most about 4 ulp = 5e-7 relative; backward dy * (y > 0 ? 1 : y + 1) inherits y's error and one
    product rounding. Sizes: below one block, a ragged tail, more than the grid's 4096 blocks."""
    for n, cols in ((3, 1), (24 * 17, 17), (4097 * 256 + 5, 1)):
        gen = torch.Generator().manual_seed(n)
        a = (torch.randn(n // cols, cols, generator=gen) * 2).requires_grad_(True)
        b = (torch.randn(n // cols, cols, generator=gen) * 2).requires_grad_(True)
        dy = torch.randn(n // cols, cols, generator=gen)
        ad, bd = a.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
        want = torch.nn.functional.elu(ad + bd)
        want.backward(dy.double())
        ag, bg = a.detach().to(cuda).requires_grad_(True), b.detach().to(cuda).requires_grad_(True)
        got = ops.add_elu(ag, bg)
        got.backward(dy.to(cuda))
        torch.testing.assert_close(got.detach().cpu().double(), want.detach(), rtol=1e-6, atol=1e-7)
        assert torch.equal(ag.grad, bg.grad)
        torch.testing.assert_close(ag.grad.cpu().double(), ad.grad, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("k_in,n_out", [(16, 8), (8, 8), (8, 1), (6, 3)])
def test_graph_conv_elu_matches_elu_of_graph_conv(cuda, k_in, n_out):
    """GraphConv(elu=True) against F.elu(GraphConv(...)) on each route (aggregate before lin_rel,
    after it with the bias moved onto lin_root's kernel, zero-padded input): the same sum in
    another order, so fp32 rounding apart (1e-5 of the largest value, gradients 1e-4 x max)."""
    from lesion_gnn_amd.conv import GraphConv

    b = synth.make_batch(5, n=24, k=6, d_in=k_in, seed=3, sizes="lognormal")
    ew = ref.gaussian_distance(b.edge_index, b.pos, 0.1).float().to(cuda)
    torch.manual_seed(5)
    conv = GraphConv(k_in, n_out).to(cuda)
    x, ei = b.x.to(cuda), b.edge_index.to(cuda)
    gy = torch.randn(x.size(0), n_out, generator=torch.Generator().manual_seed(1)).to(cuda)
    outs = []
    for fused in (True, False):
        conv.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y = conv(xg, ei, ew, elu=True) if fused else torch.nn.functional.elu(conv(xg, ei, ew))
        y.backward(gy)
        outs.append([y.detach(), xg.grad] + [p.grad.clone() for p in conv.parameters()])
    for got, want in zip(*outs):
        s = max(want.abs().max().item(), 1e-3)
        torch.testing.assert_close(got, want, rtol=0, atol=1e-4 * s)


# ---- unsupported shapes -----------------------------------------------------------------------------


def test_unsupported_shapes_raise(cuda):
    x, rows, params, dlogits = make_case(3, 12, 6, 4, 3, 17, seed=2)  # C = 17 > 16
    with pytest.raises(ValueError, match="C = 17"):
        ops.drgnet_head(x.to(cuda), 12, *[p.to(cuda) for p in params])
    x, rows, params, dlogits = make_case(3, 12, 6, 65, 3, 2, seed=2)  # c0 = 65 > 64
    with pytest.raises(ValueError, match="c0 = 65"):
        ops.drgnet_head(x.to(cuda), 12, *[p.to(cuda) for p in params])
    x, rows, params, dlogits = make_case(3, 12, 6, 4, 3, 2, seed=2)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.drgnet_head(x, 12, *params)  # CPU tensors: no fallback
    # the C entry itself refuses what the op would have refused
    with pytest.raises(ValueError):
        ops.drgnet_head(x.to(cuda), 6, *[p.to(cuda) for p in params])
