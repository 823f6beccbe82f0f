"""Shared cases, CPU restatements and the bar of the tile-width tests (tests/test_tile_width_cases.py
on the CPU, tests/test_gpu_tile_widths.py on the device). Test-only; next to tests/trajectory_ref.py.

Every linear layer of width <= 128 that is a multiple of 4 runs on the 64-node tile kernels
(ops.fast_shape / lgnn_tile_fits). Those kernels compute on a 128-wide padded image and keep the
padding out of the result with per-lane predicates; the cases here put the widths and the node
counts where those predicates decide something.

Width cases (d_in, hidden, classes): the minimum width 4, widths below 16 (12, 4), just past 32
(36) and 64 (68), just below 128 (124, 100), widths that grow and shrink between layers, and 128
next to 4 and 68. Size cases (graph sizes of synth.make_batch, k = 6): the tile structure each one
has is stated in FLAGS / NODES and asserted on the CPU.

The bar is tests/trajectory_ref.py's: for every compared tensor
    max|got - ref64| <= C x max(max|ref32 - ref64|, 1e-6 max|ref64|),
ref64 / ref32 the plain-torch oracle (oracle/pyg_ref.py, or the restatements below) in float64 and
float32 on the same inputs. GIN only: the gradients of the tensors trajectory_ref.GIN_EXCLUDED
names (a bias in front of BatchNorm: analytically zero) are left out of the ratio and held to
|got - ref64| <= 5e-6 absolute instead, the floor tests/test_gpu_gin.py::test_gin_stack_node uses.
On `mixed` the gradient of in_proj.bias does not vanish (0.013 to 0.06 in float64: graphs smaller
than k give their rows other aggregation weights, so the constant survives BatchNorm); the floor
is then a 1e-4 relative check of a real gradient, still far below a leaked lane. Nothing else may be
left out: in particular every BatchNorm running statistic is under the ratio bar here (one step
from the initial statistics is well conditioned).
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

import oracle.pyg_ref as ref
from lesion_gnn_amd import models, synth
from tests import trajectory_ref as tr

K_NN = 6

# name: (d_in, hidden_channels, classes)
WIDTH_CASES = {
    "w_a": (20, [36, 100, 12], 3),
    "w_b": (124, [4, 68, 128], 8),
    "w_c": (12, [124, 36], 5),             # one conv
    "w_d": (100, [60, 60, 60, 60], 5),     # three convs: the L = 3 entry of the fused backward
}
GIN_WIDTH_CASES = ("w_a", "w_b", "w_c")
# GCN readout per width case (GIN runs both)
POOL = {"w_a": "mean", "w_b": "add", "w_c": "mean", "w_d": "add"}

SIZE_CASES = {
    "mixed": [64, 30, 34, 1, 5, 70, 52, 64, 17, 3, 64, 40],
    "tail_open": [64, 100, 29],
    "tail_closed": [64, 30, 34, 64, 37],
    "m63": [63],
    "m65": [65],
    "one": [1],                            # GCN only: BatchNorm in training needs > 1 row
}
NODES = {"mixed": 444, "tail_open": 193, "tail_closed": 229, "m63": 63, "m65": 65, "one": 1}
# per 64-node tile: 1 = an edge leaves the tile (open), 0 = closed
FLAGS = {
    "mixed": [0, 0, 1, 1, 0, 1, 1],
    "tail_open": [0, 1, 1, 1],
    "tail_closed": [0, 0, 0, 0],
    "m63": [0],
    "m65": [1, 1],
    "one": [0],
}
GIN_SIZE_CASES = ("mixed", "tail_open", "m63")

# single-op cases (ops.node_linear, the C ABI guard bands)
LINEAR_KN = [(4, 4), (12, 124), (36, 68), (100, 36), (124, 12), (68, 128), (128, 4)]
LINEAR_M = {1: [1], 63: [63], 65: [65], 193: [64, 100, 29]}

ZERO_GRAD_FLOOR = 5e-6

# the bar's constant: twice the largest ratio measured on one MI355X, rounded up to a power of
# two (2 x 2.205 -> 8), see tests/test_gpu_tile_widths.py
C = 8


def open_flags(edge_index: torch.Tensor, num_nodes: int) -> list:
    """Per 64-node tile: does an edge cross the tile's boundary (the graph build's tile flags,
    below its 2048-entry capacity rule)."""
    src, dst = edge_index
    want = torch.zeros((num_nodes + 63) // 64, dtype=torch.int64)
    cross = (src // 64) != (dst // 64)
    want[src[cross] // 64] = 1
    want[dst[cross] // 64] = 1
    return want.tolist()


def layer_shapes(wcase: str) -> list:
    """(N, K) of in_proj and every conv's weight."""
    d_in, hidden, _ = WIDTH_CASES[wcase]
    widths = [d_in] + list(hidden)
    return [(widths[i + 1], widths[i]) for i in range(len(hidden))]


@functools.lru_cache(maxsize=None)
def batch(wcase: str, scase: str) -> synth.Batch:
    d_in, _, classes = WIDTH_CASES[wcase]
    sizes = SIZE_CASES[scase]
    seed = 200 + 10 * list(WIDTH_CASES).index(wcase) + list(SIZE_CASES).index(scase)
    return synth.make_batch(len(sizes), k=K_NN, d_in=d_in, num_classes=classes, seed=seed,
                            sizes=sizes)


@functools.lru_cache(maxsize=None)
def linear_batch(M: int, K: int) -> synth.Batch:
    sizes = LINEAR_M[M]
    return synth.make_batch(len(sizes), k=K_NN, d_in=K, seed=300 + M, sizes=sizes)


def ref_stack64(x, edge_index, n, Ws, bs):
    """float64 restatement of in_proj + L x ELU(GCNConv) (PyG order: lin, propagate, bias)."""
    ei, w = ref.gcn_norm(edge_index, n)
    h = x.double() @ Ws[0].double().T + bs[0].double()
    out = [h]
    for W, b in zip(Ws[1:], bs[1:]):
        p = h @ W.double().T
        agg = torch.zeros_like(p).index_add_(0, ei[1], w.double()[:, None] * p[ei[0]])
        h = torch.nn.functional.elu(agg + b.double())
        out.append(h)
    return out


def ref_stack32(x, edge_index, n, Ws, bs):
    """ref_stack64's expressions in float32 (plain torch): the bar's scale."""
    ei, w = ref.gcn_norm(edge_index, n)
    h = x @ Ws[0].T + bs[0]
    out = [h]
    for W, b in zip(Ws[1:], bs[1:]):
        p = h @ W.T
        agg = torch.zeros_like(p).index_add_(0, ei[1], w[:, None] * p[ei[0]])
        h = torch.nn.functional.elu(agg + b)
        out.append(h)
    return out


def stack_params(wcase: str):
    """The stack-forward test's weights: ([W_0..W_L], [b_0..b_L]), float32 on the CPU."""
    torch.manual_seed(5)
    shapes = layer_shapes(wcase)
    Ws = [torch.randn(N, K) / K ** 0.5 for N, K in shapes]
    bs = [torch.randn(N) * 0.1 for N, _ in shapes]
    return Ws, bs


def ref_linear(x, W, b, edge_index, act_elu: bool, dy, dtype):
    """Y = act(P(x) W^T + b) and its autograd in `dtype` (P = the GCN aggregation when edge_index
    is given): {"Y", "dX", "dW", "db"} as float64."""
    x, W, b = (t.detach().to(dtype, copy=True).requires_grad_() for t in (x, W, b))
    h = aggregate(x, edge_index) if edge_index is not None else x
    y = h @ W.T + b
    if act_elu:
        y = F.elu(y)
    y.backward(dy.to(dtype))
    return {"Y": tr.to64(y), "dX": tr.to64(x.grad), "dW": tr.to64(W.grad), "db": tr.to64(b.grad)}


def aggregate(x, edge_index):
    """Â x in x's dtype (gcn_norm's float32 edge weights, as the device reads them)."""
    e, w = ref.gcn_norm(edge_index, x.size(0))
    return ref.scatter_sum(w.to(x.dtype).view(-1, 1) * x.index_select(0, e[0]), e[1], x.size(0))


# ----------------------------------------------------------------------------------------------
# models
# ----------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _initial_state(family: str, wcase: str, pool: str) -> dict:
    d_in, hidden, classes = WIDTH_CASES[wcase]
    torch.manual_seed(1234)
    m = getattr(models, family.upper())(d_in, hidden, classes, 0.0, pool=pool)
    # GCNConv's bias starts at zero and BatchNorm at (1, 0): move every bias and every BatchNorm
    # weight, so that a bias or a scale read from (or added to) a padding lane shows
    gen = torch.Generator().manual_seed(4321)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def build(family: str, wcase: str, pool: str, oracle: bool = False) -> torch.nn.Module:
    """The HIP package's model (on the CPU: move it with .to(device)) or the oracle's, on the
    same state."""
    d_in, hidden, classes = WIDTH_CASES[wcase]
    m = getattr(ref if oracle else models, family.upper())(d_in, hidden, classes, 0.0, pool=pool)
    m.load_state_dict(_initial_state(family, wcase, pool))
    return m.train()


def named_step(logits, loss, model, eval_logits=None) -> dict:
    """One step's compared tensors under one key each: logits, loss, grad/<parameter>,
    state/<BatchNorm buffer> and (GIN) eval_logits, floating tensors as float64."""
    out = {"logits": tr.to64(logits), "loss": tr.to64(loss)}
    for k, p in model.named_parameters():
        out[f"grad/{k}"] = tr.to64(p.grad)
    for k, v in model.state_dict().items():
        if "running_" in k or "num_batches_tracked" in k:
            out[f"state/{k}"] = tr.to64(v)
    if eval_logits is not None:
        out["eval_logits"] = tr.to64(eval_logits)
    return out


def step(model, b: synth.Batch, dtype: torch.dtype, eval_after: bool = False) -> dict:
    """One training step of an oracle model in `dtype` on the CPU: logits, loss and every
    parameter gradient (and the BatchNorm statistics it moved) as float64 tensors, see
    named_step. eval_after: an eval-mode forward on the moved statistics follows."""
    model = model.to(dtype).train()
    x = b.x.to(dtype)
    model.zero_grad(set_to_none=True)
    logits = model(x, b.edge_index, b.batch, b.num_graphs)
    loss = F.cross_entropy(logits, b.y)
    loss.backward()
    eval_logits = None
    if eval_after:
        model.eval()
        with torch.no_grad():
            eval_logits = model(x, b.edge_index, b.batch, b.num_graphs)
        model.train()
    return named_step(logits, loss, model, eval_logits)


@functools.lru_cache(maxsize=None)
def oracle_pair(family: str, wcase: str, scase: str, pool: str) -> tuple:
    """(ref64, ref32): the oracle's step in float64 and float32, computed once."""
    b = batch(wcase, scase)
    return tuple(step(build(family, wcase, pool, oracle=True), b, dt, eval_after=family == "gin")
                 for dt in (torch.float64, torch.float32))


# ----------------------------------------------------------------------------------------------
# the bar
# ----------------------------------------------------------------------------------------------


def zero_grad_keys(family: str, keys) -> list:
    """GIN: the gradients that vanish analytically (trajectory_ref.GIN_EXCLUDED)."""
    return [k for k in keys if k.startswith("grad/") and tr.excluded(family, k)]


def _refuse(family: str, exclude: tuple | None) -> None:
    if exclude is not None:
        allowed = tr.GIN_EXCLUDED if family == "gin" else ()
        extra = [e for e in exclude if e not in allowed]
        if extra:
            raise ValueError(f"check({family!r}) refuses to leave out {extra}")


def zero_grad_errors(got: dict, ref64: dict, family: str) -> dict:
    """key -> max|got - ref64| (inf when got is not finite) of GIN's vanishing gradients."""
    out = {}
    for k in zero_grad_keys(family, ref64):
        g = got[k].detach().cpu().double()
        err = (g - ref64[k]).abs().max().item()
        out[k] = err if bool(torch.isfinite(g).all()) and math.isfinite(err) else math.inf
    return out


def ratios(got: dict, ref64: dict, ref32: dict, family: str = "", exclude: tuple | None = None,
           detail: dict | None = None) -> dict:
    """key -> err / scale (trajectory_ref.ratios) for every tensor but GIN's vanishing gradients
    (zero_grad_errors holds those). `exclude` is trajectory_ref.GIN_EXCLUDED for GIN or nothing;
    any other exclusion is refused."""
    _refuse(family, exclude)
    if not (got.keys() == ref64.keys() == ref32.keys()):
        raise AssertionError(f"tensor sets differ: {sorted(set(got) ^ set(ref64))}")
    zero = zero_grad_keys(family, ref64) if exclude is not None else []

    def rest(d):
        return {k: v for k, v in d.items() if k not in zero}
    # family "": trajectory_ref.ratios leaves nothing else out
    return tr.ratios(rest(got), rest(ref64), rest(ref32), "", detail)


def check(got: dict, ref64: dict, ref32: dict, C: float, family: str = "",
          exclude: tuple | None = None, what: str = "") -> dict:
    """Assert the bar for every compared tensor, and the absolute floor for GIN's vanishing
    gradients, and report all violations at once. Returns the ratios."""
    r = ratios(got, ref64, ref32, family, exclude)
    bad = [f"{k} {v:.3g}x" for v, k in
           sorted(((v, k) for k, v in r.items() if not (v <= C and math.isfinite(v))),
                  reverse=True)]
    if exclude is not None:
        bad += [f"{k} {v:.3g} absolute (floor {ZERO_GRAD_FLOOR})"
                for k, v in zero_grad_errors(got, ref64, family).items()
                if not v <= ZERO_GRAD_FLOOR]
    if bad:
        raise AssertionError(f"{what or family}: {len(bad)} of {len(ref64)} tensors beyond {C} x "
                             "the float32 oracle's error: " + ", ".join(bad))
    return r


def worst(r: dict) -> tuple:
    """(largest ratio, its key)."""
    if not r:
        return 0.0, ""
    k = max(r, key=lambda key: (math.inf if math.isnan(r[key]) else r[key]))
    return r[k], k
