"""GPU: the 64-node tile kernels (tile.hip, tile_lw.h, tile_util.h), the fused GCN stacks
(stack3.hip, stack3_bwd.hip) and the BN-fused GIN linears at the layer widths and node counts where
their padding predicates decide something, against the float64 oracle.

Every layer of width <= 128 that is a multiple of 4 runs on these kernels, which compute on a
128-wide padded image; the rest of the suite reaches them at widths from {32, 64, 96, 128} only.
The cases are tests/tile_width_cases.py's: widths 4, 12, 20, 36, 60, 68, 100, 124 and 128, growing
and shrinking between layers; batches that are one partial tile (1, 63 rows), two open tiles the
second of one row (65), a one-row open last tile (193), a 37-row closed last tile (229) and the
444-node mix of closed, two-graph, open and partial tiles with a 1-node graph and graphs below k.

a. test_stack_fwd_layers: ops.stack_fwd's H_0..H_L per layer, MFMA_MODE x OPEN_IN_FUSED, every
   row of every layer written (the buffers start as a NaN bit pattern).
b. test_gcn_step_*: one training step of the GCN model, every backward variant on `mixed`, the
   default switches and BWD_MODE = "f32" on the other sizes; default-switch runs twice, bit-equal.
c. test_gin_step: one training step of the GIN model, BN_FUSED x STACK x pool, the BatchNorm
   running statistics and an eval-mode forward on the moved statistics.
d. test_node_linear_autograd: ops.node_linear through autograd, Y, dX, dW and db.
e. test_guard_bands: lgnn_node_linear_fwd (with S_out) and lgnn_spmm at the C ABI into views of a
   larger buffer: not a byte before the view or after its M x N (M x K) floats changes.

Each variant asserts which kernel entry ran (the launches traced through _lib.set_tracer, against
ops._open_in_fused / ops.head_in_stack_bwd / ops.gcn_plan / ops.gin_bn_fused), so a switch
combination that falls back to another kernel at these shapes cannot pass as coverage. Which
entry each setting reaches (w_d is the L = 3 case):
  lgnn_gcn_stack_fwd             a (MFMA_MODE "f32", + lgnn_node_linear_fwd_tiles)
  lgnn_gcn_stack_fwd_s3          a (s3, OPEN_IN_FUSED "0"), b (OPEN_IN_FUSED "0" and the default
                                 "auto" on every size but `one`; + lgnn_node_linear_fwd_tiles)
  lgnn_gcn_stack_fwd_s3_all      a (s3, OPEN_IN_FUSED "1"), b (OPEN_IN_FUSED "1"; default on `one`)
  lgnn_gcn_stack_bwd             b BWD_MODE "f32", w_a / w_b / w_c (+ lgnn_node_linear_bwd_tiles)
  lgnn_gcn_stack_bwd_s3          b BWD_MODE "s3"; BWD_MODE "s3f" on w_d with the open tiles
                                 outside the launch, which is w_d's default on every size but
                                 `one` (+ lgnn_node_linear_bwd_tiles)
  lgnn_gcn_stack_bwd_s3f         b default and OPEN_IN_FUSED_BWD "0", w_a / w_b / w_c, ADJT on and
                                 off (+ lgnn_node_linear_bwd_tiles, accumulate = 2)
  lgnn_gcn_stack_bwd_s3f_all     b OPEN_IN_FUSED_BWD "1", HEAD_FOLD on (dP formed in the launch)
                                 and off, ADJT on and off; the default on `one`; forward_loss
                                 with HEAD_FOLD off
  lgnn_gcn_stack_bwd_s3f_ce      b GCN.forward_loss, OPEN_IN_FUSED_BWD "1", HEAD_FOLD on
  lgnn_node_linear_bwd (chain)   b FUSED_BWD = False; BWD_MODE "f32" on w_d (no fp32 fused L = 3)
  lgnn_node_linear_fwd / _bwd    d; c (in_proj, and every linear with BN_FUSED off)
  lgnn_node_linear_fwd_bn, lgnn_node_linear_bwd_bn, lgnn_node_linear_bwd_bn_pool
                                 c BN_FUSED on (the last conv's readout backward is _pool with
                                 STACK on and off)
  lgnn_node_linear_bwd_bn_gather c BN_FUSED on and STACK on, w_a / w_b (w_c has one conv)

Every test runs ops.py on workspaces that start as NaN (poisoned_workspaces): torch.empty hands
out recycled memory, so what a kernel reads from a row or a slot nobody wrote otherwise depends on
what ran before. That is how this file found that the layer-wise tile bodies multiplied global
row 0 of the open tiles' gradient buffer, a closed tile's row nobody writes, by their zero-weight
padding entries (fixed in tile_util.h idx_store): on the parent's kernels every
fused-backward variant of b fails on `mixed` and `tail_open`, the two cases with a closed tile 0 in
front of open tiles, with NaN gradients below the last conv.

The bar (tests/tile_width_cases.py, the one of tests/trajectory_ref.py): for every tensor
    max|got - ref64| <= C x max(max|ref32 - ref64|, 1e-6 max|ref64|).
C is measured, not guessed, by the method of tests/test_gpu_trajectory.py: this file run once with
C = inf on one MI355X, every test printing its largest ratios; the largest ratio of the whole file
doubled and rounded up to a power of two. Measured maxima (err / scale):
  a stack forward   0.48      b GCN step   0.80      d node_linear   0.51
  e guard bands     0.30 (lgnn_node_linear_fwd), 0.12 (lgnn_spmm)
  c GIN step        2.205 (w_a tail_open, grad/convs.0.nn.lins.1.bias: err 7.8e-9 on a scale of
                    3.6e-9 with pool mean, 5.6e-7 on 2.5e-7 with add; the same figure with
                    BN_FUSED and STACK on and off)
so C = 8 (2 x 2.205 = 4.41, rounded up), half the six-step trajectories' 16. GIN's vanishing
gradients (tile_width_cases.ZERO_GRAD_FLOOR = 5e-6 absolute) measured 9.6e-7 at the most
(in_proj.bias, pool add). The scale is one float32 run of plain torch, so a ratio is only as steady
as that run: the same oracle at one CPU thread reaches 7.1 x against itself on GIN w_b tail_open
(tests/test_tile_width_cases.py), a column sum that cancels; every case of a, b, d and e stays
below 1.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from lesion_gnn_amd import _lib, ops
from lesion_gnn_amd.graph import Graph
from lesion_gnn_amd.models import gin as gin_mod
from tests import tile_width_cases as tw
from tests import trajectory_ref as tr

pytestmark = pytest.mark.gpu

C = tw.C

SENTINEL = 0x7FE5C3A1  # a quiet NaN with a payload no kernel produces
GUARD = 4096           # floats on either side of a guarded view (16 KiB: views stay aligned)

STACK_BWD_ENTRIES = ("lgnn_gcn_stack_bwd", "lgnn_gcn_stack_bwd_s3", "lgnn_gcn_stack_bwd_s3f",
                     "lgnn_gcn_stack_bwd_s3f_all", "lgnn_gcn_stack_bwd_s3f_ce")
STACK_FWD_ENTRIES = ("lgnn_gcn_stack_fwd", "lgnn_gcn_stack_fwd_s3", "lgnn_gcn_stack_fwd_s3_all")


class _Names:
    """_lib tracer: the entry names of every launch, in order."""

    def __init__(self):
        self.names = []

    def __call__(self, name, args, launch):
        self.names.append(name)
        return launch()


@contextlib.contextmanager
def traced():
    t = _Names()
    _lib.set_tracer(t)
    try:
        yield t.names
    finally:
        _lib.set_tracer(None)


class _SentinelTorch:
    """`torch` as ops.py sees it, except that every float32 torch.empty starts as SENTINEL (and
    every float64 one as NaN): a row or a column a kernel leaves unwritten keeps the pattern, and
    a kernel that reads what nobody wrote, even times a zero weight, turns its result into NaN.
    torch.empty hands out recycled memory, so outside this file that depends on what ran before."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kw):
        t = torch.empty(*args, **kw)
        if t.dtype == torch.float32 and t.is_cuda:
            t.view(torch.int32).fill_(SENTINEL)
        elif t.dtype == torch.float64 and t.is_cuda:
            t.fill_(float("nan"))
        return t


@pytest.fixture(autouse=True)
def poisoned_workspaces(monkeypatch):
    """Every test of this file runs ops.py on buffers that start as NaN."""
    monkeypatch.setattr(ops, "torch", _SentinelTorch())


def report(what: str, r: dict, detail: dict | None = None) -> None:
    top = sorted(r.items(), key=lambda kv: -kv[1])[:3]
    more = ", ".join(f"{k} {v:.3g}" + (f" (err {detail[k][0]:.3g}, scale {detail[k][1]:.3g})"
                                       if detail and k in detail else "") for k, v in top)
    v, k = tw.worst(r)
    print(f"{what}: max ratio {v:.4g} ({k}) over {len(r)} tensors; {more}")


def held(what: str, got: dict, r64: dict, r32: dict, family: str = "") -> None:
    """Print the largest ratios, then assert the bar (and GIN's floor)."""
    exclude = tr.GIN_EXCLUDED if family == "gin" else None
    detail = {}
    report(what, tw.ratios(got, r64, r32, family, exclude, detail), detail)
    if family == "gin":
        z = tw.zero_grad_errors(got, r64, family)
        print(f"{what}: vanishing gradients off by " +
              ", ".join(f"{k[5:]} {v:.3g}" for k, v in z.items()))
    tw.check(got, r64, r32, C, family, exclude, what)


def assert_one_of(names: list, family: tuple, want: str, what: str) -> None:
    ran = [n for n in family if n in names]
    assert ran == [want], f"{what}: expected {want}, launched {ran}"


def device_flags(g: Graph, kind: str = "gcn") -> list:
    nt = (g.num_nodes + 63) // 64
    return g.tile_open(kind).cpu().tolist()[:nt + 1]


# ----------------------------------------------------------------------------------------------
# a. the fused GCN stack forward, layer by layer
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scase", list(tw.SIZE_CASES))
@pytest.mark.parametrize("wcase", list(tw.WIDTH_CASES))
def test_stack_fwd_layers(cuda, wcase, scase, monkeypatch):
    b = tw.batch(wcase, scase)
    M = b.num_nodes
    Ws, bs = tw.stack_params(wcase)
    r64 = {f"H/{l}": tr.to64(h) for l, h in
           enumerate(tw.ref_stack64(b.x, b.edge_index, M, Ws, bs))}
    r32 = {f"H/{l}": tr.to64(h) for l, h in
           enumerate(tw.ref_stack32(b.x, b.edge_index, M, Ws, bs))}
    xd, ei = b.x.to(cuda), b.edge_index.to(cuda)
    Wd, bd = [W.to(cuda) for W in Ws], [v.to(cuda) for v in bs]
    written = {}
    for mode in ("s3", "f32"):
        for open_in in ("0", "1"):
            what = f"stack_fwd {wcase} {scase} {mode} open_in_fused={open_in}"
            monkeypatch.setattr(ops, "MFMA_MODE", mode)
            monkeypatch.setattr(ops, "OPEN_IN_FUSED", open_in)
            g = Graph(ei, M)
            with traced() as names:
                hs, _ = ops.stack_fwd(xd, g, Wd, bd)
            torch.cuda.synchronize()
            flags = device_flags(g)
            assert flags == tw.FLAGS[scase] + [sum(tw.FLAGS[scase])], what
            one_launch = mode == "s3" and ops._open_in_fused(open_in, g, "fwd")
            assert one_launch == (mode == "s3" and open_in == "1"), what
            want = "lgnn_gcn_stack_fwd" if mode == "f32" else \
                "lgnn_gcn_stack_fwd_s3_all" if one_launch else "lgnn_gcn_stack_fwd_s3"
            assert_one_of(names, STACK_FWD_ENTRIES, want, what)
            assert ("lgnn_node_linear_fwd_tiles" in names) == (not one_launch), what
            assert g.barrier_timeouts("gcn") == 0, what
            assert [tuple(h.shape) for h in hs] == [(M, W.size(0)) for W in Ws]
            written[mode, open_in] = [(h.view(torch.int32) != SENTINEL).cpu() for h in hs]
            for l, w in enumerate(written[mode, open_in]):
                missing = (~w).nonzero()
                assert missing.numel() == 0, f"{what}: H_{l} unwritten at {missing[:4].tolist()}"
            held(what, {f"H/{l}": h for l, h in enumerate(hs)}, r64, r32)
    for key, w in written.items():  # s3 and f32 agree on which rows are written
        for a, c in zip(w, written["f32", "0"]):
            assert torch.equal(a, c), key


# ----------------------------------------------------------------------------------------------
# b. the GCN model, one training step
# ----------------------------------------------------------------------------------------------


def model_step(model, b, forward_loss: bool = False, eval_after: bool = False,
               graph: Graph | None = None) -> dict:
    """One training step on the device (b: the batch on the device; graph: a Graph to run on in
    place of b.edge_index) -> tw.named_step."""
    model.zero_grad(set_to_none=True)
    ei = graph if graph is not None else b.edge_index
    if forward_loss:
        logits, loss = model.forward_loss(b.x, ei, b.batch, b.y, None, b.num_graphs)
    else:
        logits = model(b.x, ei, b.batch, b.num_graphs)
        loss = F.cross_entropy(logits, b.y)
    loss.backward()
    eval_logits = None
    if eval_after:
        model.eval()
        with torch.no_grad():
            eval_logits = model(b.x, b.edge_index, b.batch, b.num_graphs)
        model.train()
    torch.cuda.synchronize()
    return tw.named_step(logits, loss, model, eval_logits)


def gcn_expected(g: Graph, wcase: str, ce: bool) -> tuple:
    """(forward entry, backward entry, open tiles layer-wise in the backward) under the
    switches as they stand, from the plan predicates the ops themselves use."""
    _, hidden, classes = tw.WIDTH_CASES[wcase]
    L = len(hidden) - 1
    plan = ops.gcn_plan(tw.layer_shapes(wcase), L, lazy_ok=True)
    assert plan.fused
    fwd = "lgnn_gcn_stack_fwd" if ops.MFMA_MODE != "s3" else \
        "lgnn_gcn_stack_fwd_s3_all" if ops._open_in_fused(ops.OPEN_IN_FUSED, g, "fwd") else \
        "lgnn_gcn_stack_fwd_s3"
    if not plan.fused_bwd:
        return fwd, "lgnn_node_linear_bwd", False
    if not plan.keeps_planes:
        return fwd, "lgnn_gcn_stack_bwd", True
    open_bwd = ops._open_in_fused(ops.OPEN_IN_FUSED_BWD, g, "bwd")
    if not (ops._s3f(L) and (L <= 2 or open_bwd)):
        return fwd, "lgnn_gcn_stack_bwd_s3", True
    if not open_bwd:
        return fwd, "lgnn_gcn_stack_bwd_s3f", True
    if ce and ops.head_in_stack_bwd(g, L, classes, True):
        return fwd, "lgnn_gcn_stack_bwd_s3f_ce", False
    return fwd, "lgnn_gcn_stack_bwd_s3f_all", False


def run_gcn_variant(cuda, wcase, scase, switches: dict, ce: bool, monkeypatch, model, bd, g,
                    label: str) -> dict:
    for k, v in switches.items():
        monkeypatch.setattr(ops, k, v)
    what = f"gcn {wcase} {scase} {label}"
    fwd, bwd, tiles = gcn_expected(g, wcase, ce)
    fresh = Graph(bd.edge_index, bd.num_nodes, bd.batch, bd.num_graphs)  # built by the forward
    with traced() as names:
        got = model_step(model, bd, forward_loss=ce, graph=fresh)
    for kind in ("gcn", "gcn_lazy"):  # no grid barrier of an open-tile phase gave up
        assert fresh.barrier_timeouts(kind) == 0, what
    assert_one_of(names, STACK_FWD_ENTRIES, fwd, what)
    if bwd == "lgnn_node_linear_bwd":  # the layer-wise chain: one launch per layer
        assert not [n for n in STACK_BWD_ENTRIES if n in names], what
        assert names.count(bwd) == len(tw.WIDTH_CASES[wcase][1]), what
    else:
        assert_one_of(names, STACK_BWD_ENTRIES, bwd, what)
        assert "lgnn_node_linear_bwd" not in names, what
    assert ("lgnn_node_linear_bwd_tiles" in names) == tiles, what
    print(f"{what}: {fwd} / {bwd}" + (" + lgnn_node_linear_bwd_tiles" if tiles else ""))
    r64, r32 = tw.oracle_pair("gcn", wcase, scase, tw.POOL[wcase])
    held(what, got, r64, r32)
    return got


def gcn_setup(cuda, wcase, scase):
    b = tw.batch(wcase, scase)
    bd = b.to(cuda)
    g = Graph(bd.edge_index, b.num_nodes, bd.batch, b.num_graphs)  # for the plan predicates
    model = tw.build("gcn", wcase, tw.POOL[wcase]).to(cuda)
    return model, bd, g


def assert_bit_equal(a: dict, b: dict, what: str) -> None:
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs between two runs"


GROUPS = ("default", "f32", "s3", "s3f", "layerwise", "ce")


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("wcase", list(tw.WIDTH_CASES))
def test_gcn_step_mixed(cuda, wcase, group, monkeypatch):
    """`mixed`, every backward variant. f32 / s3 / s3f: BWD_MODE (BWD_S3 with it) x open tiles
    inside the fused launches or layer-wise x HEAD_FOLD x ADJT; layerwise: FUSED_BWD = False, the
    lgnn_node_linear_bwd chain; ce: GCN.forward_loss (ops.gcn_stack_ce), open tiles inside the
    launch (the CE-fused entry) and outside it, HEAD_FOLD on and off."""
    model, bd, g = gcn_setup(cuda, wcase, "mixed")
    L = len(tw.WIDTH_CASES[wcase][1]) - 1
    classes = tw.WIDTH_CASES[wcase][2]

    def run(switches, ce=False):
        label = group + " " + " ".join(f"{k}={v}" for k, v in switches.items())
        return run_gcn_variant(cuda, wcase, "mixed", switches, ce, monkeypatch, model, bd, g,
                               label)

    if group == "default":
        first, second = run({}), run({})
        assert_bit_equal(first, second, f"gcn {wcase} mixed default")
        return
    if group == "layerwise":
        run(dict(FUSED_BWD=False))
        assert not ops.gcn_plan(tw.layer_shapes(wcase), L, lazy_ok=True).fused_bwd
        return
    if group == "ce":
        for open_in in ("0", "1"):
            for fold in (True, False):
                run(dict(OPEN_IN_FUSED=open_in, OPEN_IN_FUSED_BWD=open_in, HEAD_FOLD=fold),
                    ce=True)
                # the CE-fused entry is the one that ran exactly when the head folds
                assert ops.head_in_stack_bwd(g, L, classes, True) == (open_in == "1" and fold)
        return
    for open_in in ("0", "1"):
        for fold in (True, False):
            for adjt in (True, False):
                run(dict(BWD_MODE=group, BWD_S3=group != "f32", OPEN_IN_FUSED=open_in,
                         OPEN_IN_FUSED_BWD=open_in, HEAD_FOLD=fold, ADJT=adjt))
                if group == "s3f":  # the fold needs the single launch: assert which ran
                    assert ops.head_in_stack_bwd(g, L, classes, True) == \
                        (open_in == "1" and fold)
                else:
                    assert not ops.head_in_stack_bwd(g, L, classes, True)


@pytest.mark.parametrize("scase", [s for s in tw.SIZE_CASES if s != "mixed"])
@pytest.mark.parametrize("wcase", list(tw.WIDTH_CASES))
def test_gcn_step_sizes(cuda, wcase, scase, monkeypatch):
    """The other size cases: the default switches (twice, bit-equal) and BWD_MODE = "f32"."""
    model, bd, g = gcn_setup(cuda, wcase, scase)
    runs = [run_gcn_variant(cuda, wcase, scase, {}, False, monkeypatch, model, bd, g, "default")
            for _ in range(2)]
    assert_bit_equal(runs[0], runs[1], f"gcn {wcase} {scase} default")
    run_gcn_variant(cuda, wcase, scase, dict(BWD_MODE="f32", BWD_S3=False), False, monkeypatch,
                    model, bd, g, "BWD_MODE=f32")
    gl = Graph(bd.edge_index, bd.num_nodes)
    assert device_flags(gl, "gcn_lazy") == tw.FLAGS[scase] + [sum(tw.FLAGS[scase])]


# ----------------------------------------------------------------------------------------------
# c. the GIN model, one training step
# ----------------------------------------------------------------------------------------------


GIN_BN_ENTRIES = ("lgnn_node_linear_fwd_bn", "lgnn_node_linear_bwd_bn",
                  "lgnn_node_linear_bwd_bn_pool", "lgnn_node_linear_bwd_bn_gather")


@pytest.mark.parametrize("pool", ["add", "mean"])
@pytest.mark.parametrize("scase", list(tw.GIN_SIZE_CASES))
@pytest.mark.parametrize("wcase", list(tw.GIN_WIDTH_CASES))
def test_gin_step(cuda, wcase, scase, pool, monkeypatch):
    _, hidden, _ = tw.WIDTH_CASES[wcase]
    convs = len(hidden) - 1
    bd = tw.batch(wcase, scase).to(cuda)
    model = tw.build("gin", wcase, pool).to(cuda)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    r64, r32 = tw.oracle_pair("gin", wcase, scase, pool)
    for bn_fused in (True, False):
        for stack in (True, False):
            what = f"gin {wcase} {scase} {pool} BN_FUSED={bn_fused} STACK={stack}"
            monkeypatch.setattr(ops, "BN_FUSED", bn_fused)
            monkeypatch.setattr(gin_mod, "STACK", stack)
            model.load_state_dict(sd)
            model.train()
            assert all(ops.gin_bn_fused(a, c, c) == bn_fused for a, c in zip(hidden, hidden[1:]))
            with traced() as names:
                got = model_step(model, bd, eval_after=True)
            ran = [n for n in GIN_BN_ENTRIES if n in names]
            if not bn_fused:  # the separate BatchNorm passes around the plain tile linears
                assert ran == [] and "lgnn_bn_stats" in names, (what, ran)
                assert "lgnn_node_linear_fwd" in names and "lgnn_node_linear_bwd" in names
            else:
                gather = stack and convs > 1  # a conv below the last gathers its gradient
                want = list(GIN_BN_ENTRIES[:3]) + ([GIN_BN_ENTRIES[3]] if gather else [])
                assert ran == want, (what, ran)
                assert names.count("lgnn_node_linear_bwd_bn_pool") == 1
                assert names.count("lgnn_node_linear_bwd_bn_gather") == (convs - 1) * gather
            print(f"{what}: {', '.join(ran) or 'lgnn_node_linear_fwd / lgnn_node_linear_bwd'}")
            held(what, got, r64, r32, "gin")


# ----------------------------------------------------------------------------------------------
# d. ops.node_linear through autograd
# ----------------------------------------------------------------------------------------------


def linear_case(K, N, M):
    gen = torch.Generator().manual_seed(1000 * K + 10 * N + M)
    b = tw.linear_batch(M, K)
    W = torch.randn(N, K, generator=gen) / K ** 0.5
    bias = torch.randn(N, generator=gen) * 0.5
    dy = torch.randn(M, N, generator=gen)
    return b, W, bias, dy


@pytest.mark.parametrize("M", list(tw.LINEAR_M))
@pytest.mark.parametrize("K,N", tw.LINEAR_KN)
def test_node_linear_autograd(cuda, K, N, M):
    b, W, bias, dy = linear_case(K, N, M)
    for gather in (True, False):
        g = Graph(b.edge_index.to(cuda), M) if gather else None
        for elu in (True, False):
            what = f"node_linear K={K} N={N} M={M} gather={gather} elu={elu}"
            ei = b.edge_index if gather else None
            r64 = tw.ref_linear(b.x, W, bias, ei, elu, dy, torch.float64)
            r32 = tw.ref_linear(b.x, W, bias, ei, elu, dy, torch.float32)
            xg, Wg, bg = (t.to(cuda).requires_grad_() for t in (b.x, W, bias))
            with traced() as names:
                y = ops.node_linear(xg, Wg, bg, g, "gcn", 0.0,
                                    _lib.LGNN_ACT_ELU if elu else _lib.LGNN_ACT_NONE)
                y.backward(dy.to(cuda))
            torch.cuda.synchronize()
            assert "lgnn_node_linear_fwd" in names and "lgnn_node_linear_bwd" in names, what
            held(what, {"Y": y, "dX": xg.grad, "dW": Wg.grad, "db": bg.grad}, r64, r32)


# ----------------------------------------------------------------------------------------------
# e. guard bands at the C ABI
# ----------------------------------------------------------------------------------------------


def guarded(numel: int, device) -> torch.Tensor:
    return torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=torch.int32, device=device)


def assert_guards(buf: torch.Tensor, numel: int, what: str) -> torch.Tensor:
    """The bands around the view are untouched bit for bit; returns the view's floats."""
    host = buf.cpu()
    for name, band in (("before", host[:GUARD]), ("after", host[GUARD + numel:])):
        hit = (band != SENTINEL).nonzero()
        assert hit.numel() == 0, f"{what}: wrote {name} the view, at {hit[:4].flatten().tolist()}"
    return host[GUARD:GUARD + numel].view(torch.float32)


@pytest.mark.parametrize("M", list(tw.LINEAR_M))
@pytest.mark.parametrize("K,N", tw.LINEAR_KN)
def test_guard_bands(cuda, K, N, M):
    b, W, bias, _ = linear_case(K, N, M)
    g = Graph(b.edge_index.to(cuda), M)
    c = g.csr("gcn")
    xd, Wd, bd = b.x.to(cuda), W.to(cuda), bias.to(cuda)
    refs = {}
    for dt in (torch.float64, torch.float32):
        S = tw.aggregate(b.x.to(dt), b.edge_index)
        Z = S @ W.to(dt).T + bias.to(dt)
        refs[dt] = {"S": tr.to64(S), "Y/none": tr.to64(Z), "Y/elu": tr.to64(F.elu(Z))}
    for elu in (True, False):
        what = f"lgnn_node_linear_fwd K={K} N={N} M={M} elu={elu}"
        ybuf, sbuf = guarded(M * N, cuda), guarded(M * K, cuda)
        _lib.call("lgnn_node_linear_fwd", xd, M, K, c.rowptr, c.col, c.w, 0.0, Wd, bd, N,
                  _lib.LGNN_ACT_ELU if elu else _lib.LGNN_ACT_NONE,
                  ybuf.data_ptr() + 4 * GUARD, sbuf.data_ptr() + 4 * GUARD, _lib.stream())
        torch.cuda.synchronize()
        key = "Y/elu" if elu else "Y/none"
        got = {"Y": assert_guards(ybuf, M * N, what + " Y").view(M, N),
               "S": assert_guards(sbuf, M * K, what + " S_out").view(M, K)}
        held(what, got, *({"Y": refs[dt][key], "S": refs[dt]["S"]}
                          for dt in (torch.float64, torch.float32)))
    what = f"lgnn_spmm D={K} M={M}"
    buf = guarded(M * K, cuda)
    _lib.call("lgnn_spmm", c.rowptr, c.col, c.w, 0.0, xd, M, K, buf.data_ptr() + 4 * GUARD,
              _lib.stream())
    torch.cuda.synchronize()
    got = {"S": assert_guards(buf, M * K, what).view(M, K)}
    held(what, got, *({"S": refs[dt]["S"]} for dt in (torch.float64, torch.float32)))
