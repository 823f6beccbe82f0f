"""The set-attention kernels (csrc/setattn.hip) against the float64 per-set restatement
(tests/set_transformer_ref.py): segmented multi-head attention forward and backward in its four
query forms, with and without attention dropout, and the residual + activation + LayerNorm kernel.
Bars: tests/set_transformer_cases.py; two runs agree bit for bit."""
import pytest
import torch

from oracle.pyg_ref import DropoutMasks
from tests import set_transformer_cases as cases
from tests import set_transformer_ref as ref

pytestmark = pytest.mark.gpu

SIZES = cases.KERNEL_SIZES
P_DROP = 0.35
SEED = 1234

# (name, shared query rows S or None, query layout, key layout); layouts: "ragged" (SIZES) or a
# number of rows per set
FORMS = [("self", None, "ragged", "ragged"), ("shared1", 1, 1, "ragged"),
         ("shared5", 5, 5, "ragged"), ("shared64", 64, 64, "ragged"),
         ("ragged_q_dense_k", None, "ragged", 3), ("dense", None, 5, 5)]


def _ptr(sizes, dev):
    return torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32,
                        device=dev)


def _layout(kind, dev):
    """(per-set sizes, ptr tensor or None, rows per set)."""
    if kind == "ragged":
        return SIZES, _ptr(SIZES, dev), 0
    return [kind] * len(SIZES), None, kind


def _case(form, H, D, dev, dropout):
    from lesion_gnn_amd import dropout as lgnn_dropout
    from lesion_gnn_amd import ops

    name, shared, qkind, kkind = form
    C = H * D
    B = len(SIZES)
    qsizes, qptr, q_rows = _layout(qkind, dev)
    ksizes, kptr, k_rows = _layout(kkind, dev)
    g = torch.Generator().manual_seed(H * 1000 + D)
    Mq = shared if shared is not None else sum(qsizes)
    q = torch.randn(Mq, C, generator=g, dtype=torch.float64)
    k = torch.randn(sum(ksizes), C, generator=g, dtype=torch.float64)
    v = torch.randn(sum(ksizes), C, generator=g, dtype=torch.float64)
    aform = ops.AttnForm(qptr, q_rows, shared is not None, kptr, k_rows, B)
    numel = H * sum(a * b for a, b in zip(qsizes, ksizes))
    mask_dev = mask_cpu = None
    if dropout:
        state = lgnn_dropout.new_state(seed=SEED).to(dev)
        lgnn_dropout.set_state(state, SEED, 7)
        mask_dev = lgnn_dropout.masks(state, [(numel,)], repr(P_DROP))[0]
        mask_cpu = DropoutMasks(SEED, 7, P_DROP).mask(0, numel)
        assert torch.equal(mask_dev.cpu(), mask_cpu)
        assert ops.set_attn_mask_numel(aform, H, Mq, k.size(0)) in (numel, None)
    return q, k, v, aform, qsizes, ksizes, mask_dev, mask_cpu


def _reference(q, k, v, H, shared, qsizes, ksizes, mask):
    q = q.clone().requires_grad_(True)
    k = k.clone().requires_grad_(True)
    v = v.clone().requires_grad_(True)
    qs = [q] * len(ksizes) if shared else ref.split_sets(q, qsizes)
    ks, vs = ref.split_sets(k, ksizes), ref.split_sets(v, ksizes)
    outs, off = [], 0
    for a, b, c in zip(qs, ks, vs):
        n = H * a.shape[0] * b.shape[0]
        outs.append(ref.attention(a, b, c, H, mask[off:off + n] if mask is not None else None))
        off += n
    out = torch.cat(outs)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    (out * w).sum().backward()
    return out.detach(), w, q.grad, k.grad, v.grad


@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("H,D", cases.HEAD_SHAPES)
def test_attention_matches_restatement(cuda, H, D, form, dropout):
    from lesion_gnn_amd import ops

    q, k, v, aform, qsizes, ksizes, mask_dev, mask_cpu = _case(form, H, D, cuda, dropout)
    want, w, dq, dk, dv = _reference(q, k, v, H, form[1] is not None, qsizes, ksizes, mask_cpu)

    def run():
        ts = [t.float().to(cuda).requires_grad_(True) for t in (q, k, v)]
        out = ops.set_attention(*ts, aform, H, mask_dev)
        out.backward(w.float().to(cuda))
        return [out.detach()] + [t.grad for t in ts]

    got = run()
    assert torch.isfinite(got[0]).all()
    cases.assert_output(got[0], want)
    for name, a, b in zip(("dq", "dk", "dv"), got[1:], (dq, dk, dv)):
        assert torch.isfinite(a).all(), name
        cases.assert_grad(a, b, name)
    again = run()
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_attention_packed_projection_views(cuda):
    """q, k, v as column blocks of one [M, 3C] tensor and gradients written into the column
    blocks of one [M, 3C] gradient (the layout ops.mab uses) equal the contiguous run bit for
    bit."""
    from lesion_gnn_amd import ops

    H, D = 2, 20
    C = H * D
    q, k, v, aform, *_ = _case(FORMS[0], H, D, cuda, False)
    packed = torch.cat([q, k, v], 1).float().to(cuda)
    out, sv = ops.set_attn_fwd(packed[:, :C], packed[:, C:2 * C], packed[:, 2 * C:], aform, H)
    out2, sv2 = ops.set_attn_fwd(*[t.float().to(cuda) for t in (q, k, v)], aform, H)
    assert torch.equal(out, out2)
    dout = torch.randn_like(out)
    dp = torch.full_like(packed, float("nan"))
    ops.set_attn_bwd(sv, dout, dp[:, :C], dp[:, C:2 * C], dp[:, 2 * C:])
    grads = ops.set_attn_bwd(sv2, dout)
    assert torch.equal(dp, torch.cat(grads, 1))


def test_dropout_mask_layout_element_by_element(cuda):
    """With q = 0 the probabilities are 1 / n_k, and with one-hot value rows output column j of
    head h is the dropped-out probability of key j: out * n_k reads the mask back element by
    element in the layout [set][head][query][key]."""
    from lesion_gnn_amd import dropout as lgnn_dropout
    from lesion_gnn_amd import ops

    H, D = 2, 8
    C = H * D
    sizes = [3, 0, 5, 8]
    ptr = _ptr(sizes, cuda)
    M = sum(sizes)
    q = torch.zeros(M, C, device=cuda)
    kk = torch.randn(M, C, device=cuda)
    v = torch.zeros(M, C, device=cuda)
    row = 0
    for n in sizes:
        for j in range(n):
            for h in range(H):
                v[row + j, h * D + j] = 1.0
        row += n
    numel = H * sum(n * n for n in sizes)
    state = lgnn_dropout.new_state(seed=SEED).to(cuda)
    lgnn_dropout.set_state(state, SEED, 3)
    # the mask as the second span of a launch: stream 1
    mask = lgnn_dropout.masks(state, [(5,), (numel,)], repr(P_DROP))[1]
    want = DropoutMasks(SEED, 3, P_DROP).mask(1, numel)
    form = ops.AttnForm(ptr, 0, False, ptr, 0, len(sizes))
    out, _ = ops.set_attn_fwd(q, kk, v, form, H, mask)
    out = out.cpu()
    off, row = 0, 0
    for n in sizes:
        for h in range(H):
            for i in range(n):
                for j in range(n):
                    got = out[row + i, h * D + j].item() * n
                    assert abs(got - want[off].item()) <= 1e-5, (n, h, i, j)
                    off += 1
        row += n
    assert off == numel
    moff = ops.set_attn_mask_offsets(form, H, cuda).cpu().tolist()
    assert moff == [0] + torch.tensor([H * n * n for n in sizes]).cumsum(0).tolist()


@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_mask_offsets_scan_lengths(cuda, B):
    """k_mask_offsets (one workgroup of 256 threads) at the wave edge, the tile edge and with a
    carry over two tiles: ragged query and key sets, some empty; and keys of a fixed size."""
    from lesion_gnn_amd import ops

    H = 3
    gen = torch.Generator().manual_seed(B)
    nq = torch.randint(0, 6, (B,), generator=gen)
    nk = torch.randint(0, 9, (B,), generator=gen)
    zero = torch.zeros(1, dtype=torch.int64)
    qptr, kptr = _ptr(nq.tolist(), cuda), _ptr(nk.tolist(), cuda)
    moff = ops.set_attn_mask_offsets(ops.AttnForm(qptr, 0, False, kptr, 0, B), H, cuda)
    assert torch.equal(moff.cpu(), torch.cat([zero, H * (nq * nk).cumsum(0)]))
    moff = ops.set_attn_mask_offsets(ops.AttnForm(qptr, 0, False, None, 7, B), H, cuda)
    assert torch.equal(moff.cpu(), torch.cat([zero, H * (nq * 7).cumsum(0)]))


@pytest.mark.parametrize("H,D", [(1, 129), (5, 128), (3, 171)])
def test_out_of_range_shapes_raise(cuda, H, D):
    from lesion_gnn_amd import ops

    ptr = _ptr([2, 3], cuda)
    x = torch.zeros(5, H * D, device=cuda)
    with pytest.raises(NotImplementedError, match="head_dim"):
        ops.set_attn_fwd(x, x, x, ops.AttnForm(ptr, 0, False, ptr, 0, 2), H)


def test_cpu_tensor_raises():
    from lesion_gnn_amd import _lib, ops

    x = torch.zeros(5, 8)
    ptr = torch.tensor([0, 2, 5], dtype=torch.int32)
    with pytest.raises(_lib.LgnnError):
        ops.set_attn_fwd(x, x, x, ops.AttnForm(ptr, 0, False, ptr, 0, 2), 2)
    with pytest.raises(_lib.LgnnError):
        ops.res_norm_fwd(x, 0, x, 0)


# ----------------------------------------------------------------------------------------------
# residual + activation + LayerNorm
# ----------------------------------------------------------------------------------------------


def _res_norm_ref(a, b, relu, gamma, beta, S):
    a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ps = [p.clone().requires_grad_(True) for p in (gamma, beta)] if gamma is not None else []
    au = a.repeat(b.shape[0] // S, 1) if S else a
    u = au + (torch.relu(b) if relu else b)
    y = ref.layer_norm(u, *ps) if ps else u
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    (y * w).sum().backward()
    return y.detach(), w, a.grad, b.grad, [p.grad for p in ps]


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("ln", [False, True], ids=["noln", "ln"])
@pytest.mark.parametrize("C", [3, 8, 96, 128, 512])
@pytest.mark.parametrize("M,S", [(0, 0), (1, 0), (333, 0), (335, 5)])
def test_res_norm_matches_restatement(cuda, M, S, C, ln, relu):
    from lesion_gnn_amd import _lib, ops

    g = torch.Generator().manual_seed(M + C)
    a = torch.randn(S if S else M, C, generator=g, dtype=torch.float64)
    b = torch.randn(M, C, generator=g, dtype=torch.float64)
    if M > 1 and not S:  # a row of constant values: variance 0
        a[M // 2] = 0.25
        b[M // 2] = 0.5
    gamma = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64) if ln else None
    beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64) if ln else None
    want, w, da, db, dps = _res_norm_ref(a, b, relu, gamma, beta, S)
    act = _lib.LGNN_ACT_RELU if relu else _lib.LGNN_ACT_NONE

    def run():
        ts = [t.float().to(cuda).requires_grad_(True) for t in (a, b)]
        ps = [t.float().to(cuda).requires_grad_(True) for t in (gamma, beta)] if ln else \
            [None, None]
        y = ops.res_norm(ts[0], ts[1], act, ps[0], ps[1], S)
        y.backward(w.float().to(cuda))
        return [y.detach()] + [t.grad for t in ts] + [p.grad for p in ps if p is not None]

    got = run()
    cases.assert_output(got[0], want)
    for name, x, y in zip(("da", "db", "dgamma", "dbeta"), got[1:], [da, db] + dps):
        # a constant row's LayerNorm gradient is amplified by rstd = eps^-1/2 = 316 in both
        # evaluations alike: the bar is the tensor's own scale, as everywhere
        cases.assert_grad(x, y, name)
    for x, y in zip(got, run()):
        assert torch.equal(x, y)


def test_relu_alone(cuda):
    """a = None: y = relu(b), PoolingByMultiheadAttention's lin(x).relu()."""
    from lesion_gnn_amd import _lib, ops

    b = torch.randn(37, 24, device=cuda, requires_grad=True)
    y = ops.res_norm(None, b, _lib.LGNN_ACT_RELU)
    assert torch.equal(y, torch.relu(b.detach()))
    y.backward(torch.ones_like(y))
    assert torch.equal(b.grad, (b.detach() > 0).float())


@pytest.mark.parametrize("mean", [False, True])
def test_set_readout(cuda, mean):
    from lesion_gnn_amd import ops

    B, S, C = 4, 3, 10
    ptr = _ptr([2, 0, 5, 1], cuda)
    x = torch.randn(B * S, C, device=cuda, requires_grad=True)
    out = ops.set_readout(x, ptr, B, S, mean)
    xd = x.detach().view(B, S, C).double()
    want = xd.mean(1) if mean else xd.flatten(1)
    want[1] = 0
    cases.assert_output(out.detach(), want.cpu())
    w = torch.randn_like(out)
    out.backward(w)
    wd = w.double().clone()
    wd[1] = 0
    gw = (wd.view(B, 1, C).expand(B, S, C) / S).reshape(B * S, C) if mean else wd.view(B * S, C)
    cases.assert_grad(x.grad, gw.cpu(), "dx")
