"""GPU: the fused split-3 GCN forward with in_proj folded into conv 1 (stack3.hip k_s3_fwd,
has_in_proj = LGNN_S3_FWD_FOLD / LGNN_S3_FWD_FOLD_H0; ops.FWD_FOLD).

in_proj has no activation, so H_0 W_1^T = X (W_1 W_0)^T + 1 (W_1 b_0)^T: the plane job writes the
planes of W_10 = W_1 W_0 and b_10 = W_1 b_0 once per step (the fold slot) and the closed tiles
start at conv 1; mode 2 never forms H_0 of a closed tile, mode 3 also stores it as mode 1 does.

Kernel level (ops.stack_fwd_planes, modes 1 / 2 / 3 on buffers that start as a NaN pattern):
  * H_1..H_L of modes 2 and 3 are the same bits; H_0 of mode 3 is mode 1's, bit for bit;
  * mode 2 leaves H_0's closed rows unwritten and writes its open rows as mode 1 does;
  * every run repeats bit for bit;
  * against the float64 dense reference, per layer, err_fold <= 3 err_f32mode + 2e-7 scale: the
    bar tests/test_gpu_s3.py holds the split-3 forward to, the fp32-MFMA kernels as yardstick;
  * the fold slot and b_10 are the same bits from every launch that can write them.
Model level (GCN, one step through forward_loss and through model + ops.cross_entropy):
  * FWD_FOLD on: logits, loss and gradients within 3 x the unfolded layer-wise step's error
    + 2e-7 scale of the float64 oracle (tests/test_gpu_s3f_fold.py's bar), repeatable, and the
    logits the same bits under every FUSED_BWD / DEFER_FOLD / OPEN_IN_FUSED setting;
  * a captured step replays with weights loaded between replays (a W_10 kept from capture fails).

b_0 carries an extra N(0, 1) term everywhere, and one case has unequal degrees (about 30 % of
the non-loop edges of a k-NN batch deleted): on k-regular graphs every row of Â sums to 1 and a
b_10 added on the wrong side of the aggregation would pass unnoticed.

The 300-tile case has more tiles than the backward's 256 workgroups; the forward's grid holds up
to 512, so `two_per_wg_fwd` (520 tiles) is the one where a forward workgroup takes two tiles.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import oracle.pyg_ref as ref
from lesion_gnn_amd import _lib, ops, optim, synth
from lesion_gnn_amd.graph import Graph
from lesion_gnn_amd.models import GCN
from tests import tile_width_cases as twc

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FE5C3A1  # a quiet NaN with a payload no kernel produces


class _SentinelTorch:
    """`torch` as ops.py sees it, every float32 torch.empty starting as SENTINEL (the idiom of
    tests/test_gpu_tile_widths.py)."""

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


class _Names:
    def __init__(self):
        self.names = []

    def __call__(self, name, args, launch):
        self.names.append(name)
        return launch()


def thin(b: synth.Batch, seed: int, frac: float = 0.3) -> synth.Batch:
    """b without a seeded `frac` of its non-loop edges: unequal degrees (order kept)."""
    ei = b.edge_index
    gen = torch.Generator().manual_seed(seed)
    drop = (ei[0] != ei[1]) & (torch.rand(ei.size(1), generator=gen) < frac)
    return dataclasses.replace(b, edge_index=ei[:, ~drop].contiguous())


# name: (make_batch arguments, [d_in, w1, .., w_{L+1}], thinned)
CASES = {
    "one_tile": (dict(num_graphs=1, n=64, k=8), [128, 128, 128, 128], False),
    "shared_partial": (dict(num_graphs=4, k=8, sizes=[64, 30, 34, 17]), [128, 128, 128, 128],
                       False),
    "tiles_300": (dict(num_graphs=300, n=64, k=8), [128, 128, 128, 128], False),
    "two_per_wg_fwd": (dict(num_graphs=520, n=64, k=6), [128, 128, 128, 128], False),
    "open_and_closed": (dict(num_graphs=4, k=6, sizes=[64, 200, 64, 64]), [128, 128, 128, 128],
                        False),
    "all_open": (dict(num_graphs=2, k=8, sizes=[200, 200]), [128, 128, 128, 128], False),
    "narrow_in": (dict(num_graphs=40, n=64, k=8), [36, 64, 32, 128], False),
    "narrow_mid": (dict(num_graphs=40, n=64, k=8), [128, 16, 128, 8], False),
    "one_conv": (dict(num_graphs=40, n=64, k=8), [128, 128, 128], False),
    "unequal_degrees": (dict(num_graphs=40, n=64, k=8), [128, 128, 128, 128], True),
    "unequal_open": (dict(num_graphs=5, k=8, sizes=[64, 200, 64, 30, 34]), [128, 64, 128, 128],
                     True),
}


@functools.lru_cache(maxsize=None)
def _batch(case):
    kw, widths, thinned = CASES[case]
    b = synth.make_batch(d_in=widths[0], seed=80 + list(CASES).index(case), **kw)
    return thin(b, 7) if thinned else b


@functools.lru_cache(maxsize=None)
def _params(case):
    """([W_0..W_L], [b_0..b_L]) on the CPU; b_0 with an N(0, 1) term."""
    wd = CASES[case][1]
    gen = torch.Generator().manual_seed(5)
    Ws = [torch.randn(wd[i + 1], wd[i], generator=gen) / wd[i] ** 0.5 for i in range(len(wd) - 1)]
    bs = [torch.randn(wd[i + 1], generator=gen) * 0.1 for i in range(len(wd) - 1)]
    bs[0] = bs[0] + torch.randn(wd[1], generator=gen)
    return Ws, bs


@functools.lru_cache(maxsize=None)
def _ref64(case):
    b = _batch(case)
    Ws, bs = _params(case)
    return twc.ref_stack64(b.x, b.edge_index, b.num_nodes, Ws, bs)


def _run(case, cuda, mode, monkeypatch, open_in="auto", mfma="s3"):
    """One forward on a fresh Graph: ([H_l] on the CPU, closed-row mask, launch names)."""
    b = _batch(case)
    Ws, bs = _params(case)
    monkeypatch.setattr(ops, "MFMA_MODE", mfma)
    monkeypatch.setattr(ops, "OPEN_IN_FUSED", open_in)
    g = Graph(b.edge_index.to(cuda), b.num_nodes)
    tr = _Names()
    _lib.set_tracer(tr)
    try:
        hs = ops.stack_fwd_planes(b.x.to(cuda), g, [W.to(cuda) for W in Ws],
                                  [v.to(cuda) for v in bs], fold=mode >= 2,
                                  keep_h0=mode != 2)[0]
    finally:
        _lib.set_tracer(None)
    torch.cuda.synchronize()
    assert g.barrier_timeouts("gcn") == 0
    nt = (b.num_nodes + 63) // 64
    flags = torch.tensor(g.tile_open("gcn").cpu().tolist()[:nt]) != 0
    closed = (~flags).repeat_interleave(64)[:b.num_nodes]
    return [h.cpu() for h in hs], closed, tr.names


def _bits(t):
    return t.view(torch.int32)


def _check_kernel(case, cuda, monkeypatch, open_in="auto"):
    want = _ref64(case)
    L = len(want) - 1
    h1, closed, names1 = _run(case, cuda, 1, monkeypatch, open_in)
    h2, closed2, names2 = _run(case, cuda, 2, monkeypatch, open_in)
    h3, _, names3 = _run(case, cuda, 3, monkeypatch, open_in)
    assert torch.equal(closed, closed2)
    entry = [n for n in names2 if n.startswith("lgnn_gcn_stack_fwd")]
    assert entry == [n for n in names1 if n.startswith("lgnn_gcn_stack_fwd")] == \
        [n for n in names3 if n.startswith("lgnn_gcn_stack_fwd")] and len(entry) == 1, entry
    if open_in in ("0", "1"):
        assert entry == ["lgnn_gcn_stack_fwd_s3_all" if open_in == "1" else
                         "lgnn_gcn_stack_fwd_s3"], entry
    assert "lgnn_graph_build_planes" in names2 and "lgnn_weight_planes" not in names2
    print(f"{case} open_in_fused={open_in}: {entry[0]}, {int(closed.sum())} closed rows of "
          f"{closed.numel()}")
    # modes 2 and 3: the same H_1..H_L; mode 3's H_0 is mode 1's
    for l in range(1, L + 1):
        assert torch.equal(_bits(h2[l]), _bits(h3[l])), f"H_{l}: modes 2 and 3 differ"
    assert torch.equal(_bits(h3[0]), _bits(h1[0])), "H_0: mode 3 differs from mode 1"
    # mode 2: closed rows of H_0 untouched, open rows as mode 1
    assert bool((_bits(h2[0])[closed] == SENTINEL).all()), "mode 2 wrote H_0 of a closed tile"
    assert torch.equal(_bits(h2[0])[~closed], _bits(h1[0])[~closed]), "H_0 open rows"
    for hs in (h1, h3):
        for l, h in enumerate(hs):
            assert not bool((_bits(h) == SENTINEL).any()), f"H_{l} has unwritten elements"
    for l in range(1, L + 1):
        assert not bool((_bits(h2[l]) == SENTINEL).any()), f"H_{l} has unwritten elements"
    # every run repeats
    for mode, first in ((1, h1), (2, h2), (3, h3)):
        again = _run(case, cuda, mode, monkeypatch, open_in)[0]
        for l, (a, c) in enumerate(zip(first, again)):
            assert torch.equal(_bits(a), _bits(c)), f"mode {mode} H_{l}: not repeatable"
    # the float64 bar, the fp32-MFMA kernels as yardstick
    f32 = _run(case, cuda, 1, monkeypatch, open_in, mfma="f32")[0]
    bad = []
    for l in range(1, L + 1):
        w64 = want[l]
        e_fold = (h2[l].double() - w64).abs().max().item()
        e_s3 = (h1[l].double() - w64).abs().max().item()
        e_f32 = (f32[l].double() - w64).abs().max().item()
        scale = w64.abs().max().item()
        bound = 3 * e_f32 + 2e-7 * scale
        print(f"{case} H_{l}: err_fold {e_fold:.3e} err_unfolded {e_s3:.3e} err_f32mode "
              f"{e_f32:.3e} scale {scale:.3e} bound {bound:.3e}")
        if not e_fold <= bound:
            bad.append((l, e_fold, e_f32, scale))
    # H_0 of mode 3 (= mode 1's) against the same bar
    e0 = (h3[0].double() - want[0]).abs().max().item()
    e0f = (f32[0].double() - want[0]).abs().max().item()
    assert e0 <= 3 * e0f + 2e-7 * want[0].abs().max().item()
    assert not bad, bad


@pytest.mark.parametrize("case", [c for c in CASES if c not in ("open_and_closed",
                                                                "unequal_open")])
def test_folded_forward(cuda, case, monkeypatch):
    _check_kernel(case, cuda, monkeypatch)


@pytest.mark.parametrize("open_in", ["1", "0"])
@pytest.mark.parametrize("case", ["open_and_closed", "unequal_open"])
def test_folded_forward_with_open_tiles(cuda, case, open_in, monkeypatch):
    """Closed and open tiles together: the open phase inside the launch (_all) and in separate
    launches."""
    _check_kernel(case, cuda, monkeypatch, open_in)


def test_has_unequal_degrees():
    """The thinned cases really have rows of Â that do not sum to 1."""
    for case in ("unequal_degrees", "unequal_open"):
        b = _batch(case)
        ei, w = ref.gcn_norm(b.edge_index, b.num_nodes)
        rows = torch.zeros(b.num_nodes, dtype=torch.float64).index_add_(0, ei[1], w.double())
        assert (rows - 1).abs().max().item() > 0.05


# ----------------------------------------------------------------------------------------------
# the fold slot
# ----------------------------------------------------------------------------------------------


def _bf16_f64(u: np.ndarray) -> np.ndarray:
    return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _perm16(k: np.ndarray) -> np.ndarray:
    return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1)


@pytest.mark.parametrize("widths", [[128, 128, 128, 128], [36, 64, 32, 128], [128, 16, 128]])
def test_fold_slot_same_bits_from_every_launch(cuda, widths):
    gen = torch.Generator().manual_seed(9)
    nl = len(widths) - 1
    Ws = [(torch.randn(widths[i + 1], widths[i], generator=gen) / widths[i] ** 0.5).to(cuda)
          for i in range(nl)]
    b0 = torch.randn(widths[1], generator=gen).to(cuda)
    b = synth.make_batch(12, n=64, k=8, d_in=widths[0], seed=2)
    ei = b.edge_index.to(cuda)
    shuffled = ei[:, torch.randperm(ei.size(1), generator=gen).to(cuda)].contiguous()
    got = {}

    def job():
        planes, _ = ops.plane_buffers(Ws, fold=True)
        planes.fill_(0x7A7A)
        return planes, ops.plane_job(Ws, widths[0], planes, None, b0)

    planes, j = job()
    ops.run_plane_job(j, cuda)
    got["lgnn_weight_planes"] = planes
    # the build's first launch: k_prep_sorted (lazy build; taken, then refused by an unsorted
    # edge_index) and k_prep (the non-lazy build, and the lazy one with the sorted path off)
    for name, edges, kind, sorted_on in (("sorted", ei, "gcn_lazy", 1),
                                         ("sorted launch, unsorted edges", shuffled, "gcn_lazy", 1),
                                         ("k_prep", ei, "gcn", 1),
                                         ("k_prep lazy", shuffled, "gcn_lazy", 0)):
        planes, j = job()
        with _lib.path_option(_lib.LGNN_OPT_GRAPH_SORTED, sorted_on):
            _, done = Graph(edges, b.num_nodes).csr_planes(kind, j)
        assert done, name
        got[name] = planes
    torch.cuda.synchronize()
    first = got["lgnn_weight_planes"].cpu()
    for name, p in got.items():
        assert torch.equal(p.cpu(), first), f"{name}: the plane buffer differs"
    # the layers' slots are what the unflagged job writes
    plain, _ = ops.weight_planes(Ws, widths[0])
    assert torch.equal(first[:nl * 3 * 128 * 128], plain.cpu().flatten())
    # the fold slot holds W_1 W_0 and b_10 = W_1 b_0 (fp32 sums of at most 128 terms)
    raw = first.numpy().view(np.uint16)
    slot = raw[nl * 49152:(nl + 1) * 49152].reshape(3, 4, 8, 2, 32, 8)
    slot = slot.transpose(0, 1, 4, 2, 3, 5).reshape(3, 128, 128)  # [plane][row][phys position]
    rec = sum(_bf16_f64(slot[i]) for i in range(3))[:, _perm16(np.arange(128))]
    W10 = (Ws[1].double() @ Ws[0].double()).cpu().numpy()
    absW = (Ws[1].double().abs() @ Ws[0].double().abs()).cpu().numpy()
    w2, d_in = W10.shape
    assert np.all(np.abs(rec[:w2, :d_in] - W10) <= 130 * 2.0 ** -24 * absW)
    assert not rec[w2:].any() and not rec[:, d_in:].any()
    b10 = raw[(nl + 1) * 49152:].view(np.float32).astype(np.float64)
    assert b10.shape == (128,)
    wb = (Ws[1].double() @ b0.double()).cpu().numpy()
    absb = (Ws[1].double().abs() @ b0.double().abs()).cpu().numpy()
    assert np.all(np.abs(b10[:w2] - wb) <= 130 * 2.0 ** -24 * absb)
    assert not b10[w2:].any()


# ----------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------

MODEL_CASES = ["one_tile", "shared_partial", "tiles_300", "open_and_closed", "all_open",
               "narrow_in", "narrow_mid", "one_conv", "unequal_degrees", "unequal_open"]


@functools.lru_cache(maxsize=None)
def _state(case):
    wd = CASES[case][1]
    torch.manual_seed(1234)
    m = GCN(wd[0], wd[1:], 5, dropout=0.0)
    gen = torch.Generator().manual_seed(4321)
    with torch.no_grad():  # GCNConv's bias starts at zero: move every bias
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
        m.in_proj.bias.add_(torch.randn(m.in_proj.bias.shape, generator=gen))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _model(case, oracle=False):
    wd = CASES[case][1]
    m = (ref.GCN if oracle else GCN)(wd[0], wd[1:], 5, dropout=0.0)
    m.load_state_dict(_state(case))
    return m.train()


@functools.lru_cache(maxsize=None)
def _step64(case):
    return twc.step(_model(case, oracle=True), _batch(case), torch.float64)


def _step(m, b, cuda, ce_entry):
    x, ei, bt, y = (t.to(cuda) for t in (b.x, b.edge_index, b.batch, b.y))
    m.zero_grad(set_to_none=True)
    tr = _Names()
    _lib.set_tracer(tr)
    try:
        if ce_entry:
            logits, loss = m.forward_loss(x, ei, bt, y, None, b.num_graphs)
        else:
            logits = m(x, ei, bt, b.num_graphs)
            loss = ops.cross_entropy(logits, y)
        loss.backward()
    finally:
        _lib.set_tracer(None)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in twc.named_step(logits, loss, m).items()}
    return out, tr.names


@pytest.mark.parametrize("ce_entry", [False, True])
@pytest.mark.parametrize("case", MODEL_CASES)
def test_model_step_folded(cuda, case, ce_entry, monkeypatch):
    b, want = _batch(case), _step64(case)
    m = _model(case).to(cuda)
    assert ops.FWD_FOLD
    on, names = _step(m, b, cuda, ce_entry)
    on2, _ = _step(m, b, cuda, ce_entry)
    fwd = [n for n in names if n.startswith("lgnn_gcn_stack_fwd")]
    assert len(fwd) == 1 and fwd[0] in ("lgnn_gcn_stack_fwd_s3", "lgnn_gcn_stack_fwd_s3_all")
    assert "lgnn_graph_build_planes" in names and "lgnn_weight_planes" not in names
    for k in on:
        assert torch.equal(on[k], on2[k]), f"{k}: not repeatable"
    # the fp32 yardstick: the unfolded forward with the layer-wise backward
    monkeypatch.setattr(ops, "FWD_FOLD", False)
    monkeypatch.setattr(ops, "FUSED_BWD", False)
    lw, _ = _step(m, b, cuda, ce_entry)
    monkeypatch.setattr(ops, "FWD_FOLD", True)
    assert on.keys() == want.keys() == lw.keys()
    bad = []
    for k, w64 in want.items():
        e_on = (on[k] - w64).abs().max().item()
        e_lw = (lw[k] - w64).abs().max().item()
        scale = w64.abs().max().item()
        bound = 3 * e_lw + 2e-7 * scale
        print(f"{case} {k}: err_fold {e_on:.3e} err_layerwise {e_lw:.3e} scale {scale:.3e} "
              f"bound {bound:.3e}")
        if not (e_on <= bound and bool(torch.isfinite(on[k]).all())):
            bad.append((k, e_on, e_lw, scale))
    # the logits do not depend on the backward that follows
    for sw in (dict(FUSED_BWD=False), dict(FUSED_BWD=True, DEFER_FOLD=False),
               dict(FUSED_BWD=True, DEFER_FOLD=True, OPEN_IN_FUSED="0", OPEN_IN_FUSED_BWD="0"),
               dict(OPEN_IN_FUSED="1", OPEN_IN_FUSED_BWD="1"),
               dict(DEFER_FOLD=False, OPEN_IN_FUSED="1", OPEN_IN_FUSED_BWD="0")):
        for name, v in sw.items():
            monkeypatch.setattr(ops, name, v)
        other, _ = _step(m, b, cuda, ce_entry)
        assert torch.equal(other["logits"], on["logits"]), f"logits differ under {sw}"
        assert torch.equal(other["loss"], on["loss"]), f"loss differs under {sw}"
        for k, w64 in want.items():  # and every backward behind the folded forward holds the bar
            e = (other[k] - w64).abs().max().item()
            e_lw = (lw[k] - w64).abs().max().item()
            if not e <= 3 * e_lw + 2e-7 * w64.abs().max().item():
                bad.append((str(sw), k, e, e_lw))
    assert not bad, bad


def test_backward_recomputes_h0_when_the_switches_change(cuda, monkeypatch):
    """Forward under the deferred backward (H_0's closed rows unwritten), backward after
    DEFER_FOLD went off: the gradients are those of a step run with DEFER_FOLD off throughout
    within the bar (H_0 comes from linear_fwd then, not from the unwritten rows)."""
    case = "unequal_degrees"
    b, want = _batch(case), _step64(case)
    m = _model(case).to(cuda)
    x, ei, bt, y = (t.to(cuda) for t in (b.x, b.edge_index, b.batch, b.y))
    m.zero_grad(set_to_none=True)
    logits = m(x, ei, bt, b.num_graphs)
    loss = ops.cross_entropy(logits, y)
    monkeypatch.setattr(ops, "DEFER_FOLD", False)
    loss.backward()
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in twc.named_step(logits, loss, m).items()}
    monkeypatch.setattr(ops, "FWD_FOLD", False)
    monkeypatch.setattr(ops, "FUSED_BWD", False)
    lw, _ = _step(m, b, cuda, False)
    for k, w64 in want.items():
        e, e_lw = (got[k] - w64).abs().max().item(), (lw[k] - w64).abs().max().item()
        assert torch.isfinite(got[k]).all(), k
        assert e <= 3 * e_lw + 2e-7 * w64.abs().max().item(), (k, e, e_lw)


def test_captured_step_folds_the_live_weights(cuda):
    """The C2-shaped step captured in a HIP graph: W_10 / b_10 are remade by every replay."""
    torch.manual_seed(0)
    m = GCN(128, [128, 128, 128], 5, 0.0).to(cuda).train()
    b = synth.make_batch(128, n=64, k=8, d_in=128, seed=3)
    x, ei, bt, y = (t.to(cuda) for t in (b.x, b.edge_index, b.batch, b.y))
    B = b.num_graphs
    opt = optim.Adam(m.parameters(), lr=1e-2, weight_decay=2e-6)
    out = {}

    def step():
        logits, loss = m.forward_loss(x, ei, bt, y, None, B)
        loss.backward()
        opt.step()
        out["logits"], out["loss"] = logits, loss

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(cuda).wait_stream(side)
    opt.zero_grad(set_to_none=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    g.replay()
    torch.manual_seed(1)
    fresh = GCN(128, [128, 128, 128], 5, 0.0)
    with torch.no_grad():  # a b_0 that matters
        fresh.in_proj.bias.add_(torch.randn(128))
    m.load_state_dict(fresh.state_dict())  # in-place copies, outside the graph
    g.replay()
    torch.cuda.synchronize()
    oref = ref.GCN(128, [128, 128, 128], 5, 0.0)
    oref.load_state_dict(fresh.state_dict())
    want = oref(b.x, b.edge_index, b.batch, B)
    want_loss = torch.nn.functional.cross_entropy(want, b.y)
    torch.testing.assert_close(out["logits"].cpu(), want, rtol=0, atol=1e-4)
    torch.testing.assert_close(out["loss"].cpu(), want_loss, rtol=0, atol=1e-5)
