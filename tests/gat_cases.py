"""Shapes, graphs, regimes and the bar of the GATConv kernel tests (tests/test_gat_ref.py on the
CPU, tests/test_gpu_gat_kernels.py on the device). Test-only; the formulas are tests/gat_ref.py's.

Shapes (H, C), grouped by the kernel form each takes under the default path option
(LGNN_OPT_GAT_PIPE = 1), derived from gat.hip's pipe2_ok / pipe_ok in that order (form()):
  "ps"   two-strip form          128 < H*C <= 512 and 32 <= C <= 128
  "p1"   row-pipelined, 1 slot   H*C <= 128 and H <= 4
  "p2"   row-pipelined, 2 slots  H*C <= 128 and 5 <= H <= 8
  "row"  per-row kernels         everything else: H > 8 at H*C <= 128, C < 32 at H*C > 128
                                 (NS = 1), C = 256 (NS = 2), C = 512 (NS = 4)
With LGNN_OPT_GAT_PIPE = 0 every shape takes the per-row kernels; the first fifteen shapes (the
p1, p2 and ps groups) run a second time that way, which holds the per-row kernels to the same bar
at the shapes where they are the reference of tests/test_gpu_gat_pipe.py's bitwise pairs.

Graphs: `degrees` (347 nodes, not a multiple of the 8 rows per block; the row lengths LENGTHS in
the target and in the transposed CSR, a hub gathering 300 sources and a source feeding 300
targets, an edge present twice, an explicit self loop, graph sizes [120, 0, 200, 27]) and `tiny`
(3 nodes, edges 0->1 and 1->0, node 2 isolated, graph sizes [1, 2]).

Regimes (XP unit normal float32; a_s and a_d are kernel inputs, so a regime may set them):
  init      a_s, a_d from glorot-scale attention vectors (glorot_att: the bound of one head)
  peaked    the same vectors x 40: logits past expf's overflow (88.7), below -20, row ranges > 88
  negative  a_s = -30 |n1|, a_d = -30 |n2|: every logit negative, every edge on the slope branch
  zero      a_s = a_d = 0: every logit exactly 0, alpha = 1 / deg, leaky' at 0 is the slope
The quarter of (row, head) pairs ranging over 88 is asserted on `degrees` only: `tiny` has two
multi-entry rows of two entries, a pair there ranges over 88 with a probability near 0.1 to 0.3,
and at 16 heads or more no seed reaches a quarter (none in 400 at (32, 4) and (128, 4)); on `tiny`
the test asserts that some pair does, besides the logit above 88.7 and the one below -20.
init and peaked also run with an edge mask (Bernoulli keep, p = 0.35, scaled 1 / (1 - p), [cap, H]
in CSR order; one whole row dropped, the hub row partly dropped).

The bar is the project's (tests/trajectory_ref.py, tests/tile_width_cases.py), per compared tensor:
    max|got - ref64| <= CG x max(max|ref32 - ref64|, 1e-6 max|ref64|),
ref64 / ref32 tests/gat_ref.py in float64 and float32 on the same inputs. CG (and CG_E2E, for the
whole conv against the oracle) is measured on the device; the figures are in the docstring of
tests/test_gpu_gat_kernels.py.

da_d where it vanishes. da_d[i] = sum_j alpha_ij (dal_ij - s_i) leaky'_ij, and s_i = sum_j alpha_ij
dal_ij with sum_j alpha_ij = 1: for a (row, head) whose entries are all on one leaky-ReLU branch
the sum is analytically 0 (one_branch; the branch is the sign of a_s[j] + a_d[i], which the two
sides share). In `zero` and `negative` that is every row, on `tiny` it can be every row in any
regime. ref32 can then cancel exactly (alpha = 1/2 twice, or a saturated alpha = 1: a scale of 0,
so that one unit in the last place of a term is an infinite ratio), which makes its error no
measure of anything. As the tile tests do for GIN's vanishing gradients
(tests/tile_width_cases.py), those entries of da_d are left out of the ratio (set to 0 on all three
sides) and held to an absolute floor instead, the first-order rounding bound of the sum in float32
(da_d_floor): the dot products' errors cancel in the sum as the exact terms do, what is left is
one rounding per accumulation of s_i and of da_d and four per term, each relative to
alpha_ij (|dal_ij| + |s_i|) |leaky'_ij|:
    |da_d[i] - ref64| <= (deg_i + 4) (2^-24 sum_j alpha_ij (|dal_ij| + |s_i|) |leaky'_ij| + 2^-149).
The 2^-149 is float32's subnormal spacing: in `peaked` a mask can leave a row only entries with
alpha near 1e-40, whose terms are subnormal and round by that spacing, not relatively.
The other entries of da_d, and da_e everywhere, stay under the ratio bar.

Steadiness of the bar's scale: ref32 at torch.set_num_threads(1) against ref32 at the default
thread count, under the bar's formula (tests/test_gat_ref.py::test_ref32_thread_steadiness): the
worst ratio over every shape, regime and tensor is recorded in STEADINESS below (a ratio of 1
means the two runs agree bit for bit: the formula then divides ref32's error by itself).
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import torch

from tests import gat_ref as gr
from tests import trajectory_ref as tr

SHAPES_P1 = [(1, 4), (3, 8), (3, 32), (2, 64), (4, 32), (1, 128)]
SHAPES_P2 = [(8, 4), (5, 16), (8, 16)]
SHAPES_PS = [(2, 128), (8, 32), (5, 64), (3, 128), (4, 128), (16, 32)]
SHAPES_ROW = [(16, 8), (32, 4), (16, 16), (128, 4), (1, 256), (2, 256), (1, 512)]
SHAPES = SHAPES_P1 + SHAPES_P2 + SHAPES_PS + SHAPES_ROW
PIPE_SHAPES = SHAPES[:15]  # these also run under LGNN_OPT_GAT_PIPE = 0
# (shape, pipe) of every kernel run
RUNS = [(s, 1) for s in SHAPES] + [(s, 0) for s in PIPE_SHAPES]
# one shape per kernel form also runs at this slope
SLOPE = 0.2
SLOPE_ALT = 0.05
ALT_SLOPE_SHAPES = [(3, 32), (5, 16), (5, 64), (16, 16), (2, 256), (1, 512)]

REGIMES = ("init", "peaked", "negative", "zero")
MASKED = ("init", "peaked")
ACTS = (gr.ACT_ELU, gr.ACT_NONE)
DROP_P = 0.35
PEAK = 40.0
D_IN = 36  # test f's input width

LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 301)
M_DEGREES = 347
SIZES = {"degrees": [120, 0, 200, 27], "tiny": [1, 2]}
HUB = LENGTHS.index(301)       # the target gathering 300 sources (node id = its index)
DROPPED_ROW = LENGTHS.index(5)  # the target whose whole row the mask drops
FEEDER = 20 + LENGTHS.index(301)  # the source feeding 300 targets

# worst ref32(1 thread) vs ref32(default threads) ratio under the bar's formula, as printed by
# tests/test_gat_ref.py::test_ref32_thread_steadiness
# (8 threads by default): 1.0, that is, bit-identical. The restatement's sums are scatter_add_
# and single-row reductions, which the CPU runs in one fixed order at any thread count, so the
# scale does not move between runs; the margin of 2 in CG is then a margin only.
STEADINESS = 1.0

# the bar's constants (tests/test_gpu_gat_kernels.py documents the measurement): CG for the
# kernels one by one (twice the largest ratio measured on one MI355X, rounded up to a power of
# two: 2 x 2.45 -> 8), CG_E2E for the whole conv against the oracle's autograd (2 x 8.42 -> 32)
CG = 8
CG_E2E = 32


def form(H: int, C: int, pipe: int = 1) -> str:
    """The kernel form of gat.hip's launchers: pipe2_ok, then pipe_ok, else the per-row kernels."""
    HC = H * C
    if pipe and 128 < HC <= 512 and 32 <= C <= 128:
        return "ps"
    if pipe and H <= 8 and HC <= 128:
        return "p1" if H <= 4 else "p2"
    return "row"


def ns_of(C: int) -> int:
    """Strips per pass of the per-row kernels."""
    return 1 if C <= 128 else C // 128


class GraphCase(NamedTuple):
    name: str
    n: int
    edge_index: torch.Tensor  # [2, E] int64 (source, target), as given to Graph
    batch: torch.Tensor       # [n] int64
    num_graphs: int
    gptr: torch.Tensor        # [num_graphs + 1] int64
    csr: gr.Csr
    tcsr: gr.TCsr


def _batch(sizes: list) -> tuple:
    batch = torch.cat([torch.full((s,), g, dtype=torch.int64) for g, s in enumerate(sizes)])
    gptr = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
    return batch, gptr


@functools.lru_cache(maxsize=None)
def graph(name: str) -> GraphCase:
    sizes = SIZES[name]
    batch, gptr = _batch(sizes)
    if name == "tiny":
        n = 3
        ei = torch.tensor([[0, 1], [1, 0]], dtype=torch.int64)
    else:
        # nodes 0..13: targets of LENGTHS[k] - 1 fillers each; nodes 20..33: sources feeding
        # LENGTHS[k] - 1 fillers each; nodes 40..346: the 307 fillers, which also carry 500
        # random filler -> filler edges. Nothing else points at a special target or leaves a
        # special source, so their row lengths (with the self loop) are exactly LENGTHS.
        n = M_DEGREES
        g = torch.Generator().manual_seed(347)
        fill = torch.arange(40, n)
        src, dst = [], []
        for k, length in enumerate(LENGTHS):
            pick = fill[torch.randperm(fill.numel(), generator=g)[:length - 1]]
            src.append(pick)
            dst.append(torch.full((length - 1,), k))
            pick = fill[torch.randperm(fill.numel(), generator=g)[:length - 1]]
            src.append(torch.full((length - 1,), 20 + k))
            dst.append(pick)
        rs = fill[torch.randint(fill.numel(), (500,), generator=g)]
        rd = fill[torch.randint(fill.numel(), (500,), generator=g)]
        keep = rs != rd
        src += [rs[keep], torch.tensor([41, 41, 2])]  # 41 -> 45 twice; the self loop 2 -> 2
        dst += [rd[keep], torch.tensor([45, 45, 2])]
        ei = torch.stack([torch.cat(src), torch.cat(dst)])
        ei = ei[:, torch.randperm(ei.size(1), generator=g)]  # no order the build could lean on
    csr, tcsr = gr.gat_csr(ei, n)
    return GraphCase(name, n, ei, batch, len(sizes), gptr, csr, tcsr)


def row_lengths(ptr: torch.Tensor) -> list:
    return (ptr[1:] - ptr[:-1]).tolist()


# ----------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------

# seeds chosen so that the regime conditions (tests/test_gat_ref.py) hold; (H, C, graph) -> seed,
# where the default 1000 H + C (+ 500000 on `tiny`) does not satisfy them
SEEDS: dict = {
    (1, 4, "degrees"): 1006, (3, 8, "degrees"): 3010, (8, 4, "degrees"): 8007,
    (16, 8, "degrees"): 16009, (128, 4, "degrees"): 128007,
    (3, 8, "tiny"): 503077, (2, 64, "tiny"): 502068, (4, 32, "tiny"): 504034,
    (1, 128, "tiny"): 501152, (8, 4, "tiny"): 508012, (5, 16, "tiny"): 505024,
    (8, 16, "tiny"): 508037, (2, 128, "tiny"): 502174, (8, 32, "tiny"): 508060,
    (5, 64, "tiny"): 505067, (3, 128, "tiny"): 503129, (4, 128, "tiny"): 504149,
    (16, 32, "tiny"): 516079, (16, 8, "tiny"): 516122, (16, 16, "tiny"): 516105,
    (1, 256, "tiny"): 501263, (2, 256, "tiny"): 502268, (1, 512, "tiny"): 501518,
}


def seed_of(H: int, C: int, gname: str) -> int:
    return SEEDS.get((H, C, gname), 1000 * H + C + (500000 if gname == "tiny" else 0))


def glorot_att(H: int, C: int, g: torch.Generator) -> torch.Tensor:
    """H * C values uniform in (-a, a), a = sqrt(6 / (1 + C)): glorot's bound for one head's
    vector [1, C]. PyG draws the [1, H, C] parameter with a = sqrt(6 / (H + C)), which shrinks
    with H: at (128, 4) the x 40 logits then stay below 72 and `peaked` could not reach expf's
    overflow, whatever the seed. Per head, every shape sees the same regime."""
    a = math.sqrt(6.0 / (1 + C))
    return ((torch.rand(H * C, generator=g) * 2 - 1) * a).float()


@functools.lru_cache(maxsize=None)
def inputs(H: int, C: int, gname: str) -> dict:
    """The float32 inputs every regime of a (shape, graph) shares."""
    gc = graph(gname)
    g = torch.Generator().manual_seed(seed_of(H, C, gname))
    M, HC, nnz = gc.n, H * C, gc.csr.col.numel()
    out = {
        "XP": torch.randn(M, HC, generator=g),
        "att_src": glorot_att(H, C, g),
        "att_dst": glorot_att(H, C, g),
        "n1": torch.randn(M, H, generator=g),
        "n2": torch.randn(M, H, generator=g),
        "bias": torch.randn(HC, generator=g) * 0.5,
        "dY": torch.randn(M, HC, generator=g),
    }
    keep = (torch.rand(nnz, H, generator=g) >= DROP_P).float() / (1.0 - DROP_P)
    if gname == "degrees":
        keep[gc.csr.rowptr[DROPPED_ROW]:gc.csr.rowptr[DROPPED_ROW + 1]] = 0.0
    out["mask"] = keep
    for nc in (1, 5):
        out[f"dlogits{nc}"] = torch.randn(gc.num_graphs, nc, generator=g)
        out[f"Wout{nc}"] = torch.randn(nc, HC, generator=g) / HC ** 0.5
    return out


def att_vectors(H: int, C: int, gname: str, regime: str) -> tuple:
    """(att_src, att_dst) float32 of `init` / `peaked`."""
    i = inputs(H, C, gname)
    k = PEAK if regime == "peaked" else 1.0
    return i["att_src"] * k, i["att_dst"] * k


def scores(H: int, C: int, gname: str, regime: str):
    """(a_s, a_d) float32 of the regimes that set them directly; None for init / peaked (there
    they are lgnn_gat_att's output on the device, gat_ref.att on the CPU)."""
    i = inputs(H, C, gname)
    if regime == "negative":
        return -30.0 * i["n1"].abs(), -30.0 * i["n2"].abs()
    if regime == "zero":
        return torch.zeros_like(i["n1"]), torch.zeros_like(i["n2"])
    return None


def cpu_scores(H: int, C: int, gname: str, regime: str, dtype=torch.float64):
    """(a_s, a_d) in `dtype` as the CPU restatement forms them (the regime conditions)."""
    s = scores(H, C, gname, regime)
    if s is not None:
        return s[0].to(dtype), s[1].to(dtype)
    a_src, a_dst = att_vectors(H, C, gname, regime)
    return gr.att(inputs(H, C, gname)["XP"].to(dtype), a_src.to(dtype), a_dst.to(dtype), H)


def slopes(H: int, C: int) -> tuple:
    return (SLOPE, SLOPE_ALT) if (H, C) in ALT_SLOPE_SHAPES else (SLOPE,)


def f32(v: float) -> float:
    """A float as the C ABI's `float` parameter receives it."""
    return torch.tensor(v, dtype=torch.float32).item()


# ----------------------------------------------------------------------------------------------
# the whole conv (test f): ops.gat_conv / ops.gat_conv_head against the oracle's autograd
# ----------------------------------------------------------------------------------------------

E2E_MARGIN = 1e-4  # smallest |logit| >= E2E_MARGIN x largest |logit| in ref64
E2E_CLASSES = 5
# Here the two sides form their own logits, so a logit within rounding of 0 could take the other
# leaky-ReLU branch on the device. The margin rules that out, and it has to be found by seed.
# `tiny` has 5 H logits and every shape runs on it. `degrees` has 1941 H logits: searching up from
# the default seed, every shape with 4 heads or fewer meets the margin within 302 seeds (within
# 15 at one head), and none of 600 does at 5 heads or more (9705 logits and up), so `degrees`
# runs every shape with H <= 4: every one-slot pipelined shape (the reference config's (2, 64) and the widths the GEMM
# epilogue scores), the two-strip form at (2, 128), (3, 128) and (4, 128), and the per-row
# kernels at NS = 2 and 4. Tests b to e hold the forms with more heads to the bar on `degrees`.
E2E_DEGREES = [(1, 4), (3, 8), (3, 32), (2, 64), (4, 32), (1, 128), (2, 128), (3, 128), (4, 128),
               (1, 256), (2, 256), (1, 512)]
# (H, C, graph) -> seed where the default (7 + the inputs' seed) misses the margin
E2E_SEEDS: dict = {
    (1, 4, "degrees"): 1015, (3, 8, "degrees"): 3179, (3, 32, "degrees"): 3341,
    (2, 64, "degrees"): 2072, (4, 32, "degrees"): 4184, (1, 128, "degrees"): 1150,
    (2, 128, "degrees"): 2141, (3, 128, "degrees"): 3218, (4, 128, "degrees"): 4372,
    (1, 256, "degrees"): 1266, (2, 256, "degrees"): 2265, (1, 512, "degrees"): 1519,
    (16, 32, "tiny"): 516088, (16, 8, "tiny"): 516132, (128, 4, "tiny"): 628017,
}


def e2e_graphs(H: int, C: int) -> tuple:
    return ("tiny", "degrees") if (H, C) in E2E_DEGREES else ("tiny",)


@functools.lru_cache(maxsize=None)
def e2e_case(H: int, C: int, gname: str) -> dict:
    """The oracle conv's float32 state at init (att_src / att_dst as PyG draws them), x, the
    readout's Linear and the cotangents."""
    import oracle.pyg_ref as ref
    gc = graph(gname)
    seed = E2E_SEEDS.get((H, C, gname), 7 + seed_of(H, C, gname))
    torch.manual_seed(seed)
    conv = ref.GATConv(D_IN, C, heads=H)
    g = torch.Generator().manual_seed(seed)
    HC = H * C
    return {
        "x": torch.randn(gc.n, D_IN, generator=g),
        "W": conv.lin.weight.detach().clone(),
        "att_src": conv.att_src.detach().clone(),
        "att_dst": conv.att_dst.detach().clone(),
        "bias": torch.randn(HC, generator=g) * 0.5,
        "W_out": torch.randn(E2E_CLASSES, HC, generator=g) / HC ** 0.5,
        "b_out": torch.randn(E2E_CLASSES, generator=g) * 0.1,
        "dY": torch.randn(gc.n, HC, generator=g),
        "dlogits": torch.randn(gc.num_graphs, E2E_CLASSES, generator=g),
    }


def e2e_oracle(H: int, C: int, gname: str, regime: str, head: str | None, dtype,
               slope: float = SLOPE) -> dict:
    """ELU(oracle GATConv) (+ global pool `head` + Linear) and its autograd in `dtype`, as
    float64 tensors; "logit_margin" is min|logit| / max|logit| of the conv's attention logits."""
    import oracle.pyg_ref as ref
    gc = graph(gname)
    c = e2e_case(H, C, gname)
    k = PEAK if regime == "peaked" else 1.0
    conv = ref.GATConv(D_IN, C, heads=H, negative_slope=slope)
    with torch.no_grad():
        conv.lin.weight.copy_(c["W"])
        conv.att_src.copy_(c["att_src"] * k)
        conv.att_dst.copy_(c["att_dst"] * k)
        conv.bias.copy_(c["bias"])
    conv = conv.to(dtype)
    x = c["x"].to(dtype, copy=True).requires_grad_()
    y = torch.nn.functional.elu(conv(x, gc.edge_index))
    out = {}
    if head is None:
        y.backward(c["dY"].to(dtype))
        out["Y"] = y
    else:
        lin = torch.nn.Linear(H * C, E2E_CLASSES).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(c["W_out"])
            lin.bias.copy_(c["b_out"])
        pool = ref.global_mean_pool if head == "mean" else ref.global_add_pool
        logits_ = lin(pool(y, gc.batch, gc.num_graphs))
        logits_.backward(c["dlogits"].to(dtype))
        out.update({"logits": logits_, "dW_out": lin.weight.grad, "db_out": lin.bias.grad})
    out.update({"dx": x.grad, "dW": conv.lin.weight.grad, "datt_src": conv.att_src.grad.view(-1),
                "datt_dst": conv.att_dst.grad.view(-1), "dbias": conv.bias.grad})
    out = {k_: tr.to64(v) for k_, v in out.items()}
    with torch.no_grad():
        a_s, a_d = gr.att(c["x"].to(dtype) @ conv.lin.weight.T, conv.att_src.view(-1),
                          conv.att_dst.view(-1), H)
        e = gr.logits(a_s, a_d, gc.csr, slope).abs()
    out["logit_margin"] = (e.min() / e.max()).double()
    return out


# ----------------------------------------------------------------------------------------------
# the bar
# ----------------------------------------------------------------------------------------------


def ratios(got: dict, ref64: dict, ref32: dict, detail: dict | None = None) -> dict:
    """key -> err / scale, trajectory_ref.ratios with nothing left out."""
    r32 = {k: tr.to64(v) for k, v in ref32.items()}
    return tr.ratios(got, ref64, r32, "", detail)


# ----------------------------------------------------------------------------------------------
# one case through the four kernels: the reference of each stage from that stage's inputs
# ----------------------------------------------------------------------------------------------


def cast(a, dtype):
    return a.to(dtype) if isinstance(a, torch.Tensor) and a.is_floating_point() else a


def in_dtype(fn, dtype, *args):
    return fn(*[cast(a, dtype) for a in args])


STAGES = ("att", "fwd", "edge", "node")


def stage_refs(H: int, C: int, gname: str, regime: str, masked: bool, act: str, slope: float,
               arrays: dict, dtype, dY: torch.Tensor | None = None, stages=STAGES) -> dict:
    """The compared tensors of a case's `stages` in `dtype`, as float64: each stage restated
    from the float32 arrays its kernel reads. arrays: a_s, a_d, alpha, Y, dZ, da_e, da_d as the
    previous stage produced them (the device's own on the device, host_arrays on the CPU).
    dY: the edge stage's output gradient (default: the case's)."""
    gc = graph(gname)
    i = inputs(H, C, gname)
    mask = i["mask"] if masked else None
    s = f32(slope)
    out = {}
    direct = scores(H, C, gname, regime) is not None
    a_src, a_dst = att_vectors(H, C, gname, "init" if direct else regime)
    if "att" in stages and not direct:
        out["att/a_s"], out["att/a_d"] = in_dtype(gr.att, dtype, i["XP"], a_src, a_dst, H)
    if "fwd" in stages:
        alpha, Y = in_dtype(gr.fwd, dtype, i["XP"], arrays["a_s"], arrays["a_d"], gc.csr, s,
                            mask, i["bias"], act)
        out["fwd/alpha"], out["fwd/Y"] = alpha, Y
        out["fwd/alpha_rowsum"] = gr.ref.scatter_sum(alpha, gc.csr.dst, gc.n)
    if "edge" in stages:
        out["edge/dZ"], out["edge/da_e"], out["edge/da_d"] = in_dtype(
            gr.bwd_edge, dtype, i["XP"], arrays["a_s"], arrays["a_d"], arrays["alpha"], mask,
            i["dY"] if dY is None else dY, arrays["Y"], act, s, gc.csr)
    if "node" in stages:
        out["node/dXP"], out["node/datt_src"], out["node/datt_dst"], out["node/dbias"] = \
            in_dtype(gr.bwd_node, dtype, arrays["alpha"], mask, arrays["da_e"], arrays["da_d"],
                     arrays["dZ"], i["XP"], a_src, a_dst, gc.tcsr)
    return {k: tr.to64(v) for k, v in out.items()}


def one_branch(gname: str, arrays: dict) -> torch.Tensor:
    """[M, H] bool: every entry of the (row, head) is on one leaky-ReLU branch, so its da_d
    vanishes analytically (module docstring)."""
    gc = graph(gname)
    pos = ((arrays["a_s"][gc.csr.col] + arrays["a_d"][gc.csr.dst]) > 0).double()
    n_pos = gr.ref.scatter_sum(pos, gc.csr.dst, gc.n)
    deg = (gc.csr.rowptr[1:] - gc.csr.rowptr[:-1]).double().unsqueeze(-1)
    return (n_pos == 0) | (n_pos == deg)


def da_d_floor(H: int, C: int, gname: str, regime: str, masked: bool, act: str, slope: float,
               arrays: dict, dY: torch.Tensor | None = None) -> torch.Tensor:
    """[M, H] float64: the rounding bound of da_d where it vanishes (module docstring), from the
    float32 arrays the edge kernel reads. dY: the output gradient in float64 (default: the
    case's)."""
    gc = graph(gname)
    i = inputs(H, C, gname)
    s = f32(slope)
    XP, Y = i["XP"].double(), arrays["Y"].double()
    dY = i["dY"].double() if dY is None else dY
    alpha = arrays["alpha"].double()
    dZ = dY * torch.where(Y > 0, torch.ones_like(Y), Y + 1) if act == gr.ACT_ELU else dY
    dal = (dZ.reshape(gc.n, H, C)[gc.csr.dst] * XP.reshape(gc.n, H, C)[gc.csr.col]).sum(-1)
    if masked:
        dal = dal * i["mask"].double()
    s_i = gr.ref.scatter_sum(alpha * dal, gc.csr.dst, gc.n)
    pre = arrays["a_s"].double()[gc.csr.col] + arrays["a_d"].double()[gc.csr.dst]
    g = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, s))
    terms = alpha * (dal.abs() + s_i.abs()[gc.csr.dst]) * g
    deg = (gc.csr.rowptr[1:] - gc.csr.rowptr[:-1]).double().unsqueeze(-1)
    # (+ one subnormal spacing per rounding: where a mask leaves a row only entries with
    # alpha ~ 1e-40, the terms are float32 subnormals and round absolutely, not relatively)
    return (deg + 4) * (2.0 ** -24 * gr.ref.scatter_sum(terms, gc.csr.dst, gc.n) + 2.0 ** -149)


def split_da_d(case: tuple, arrays: dict, got: dict, r64: dict, r32: dict,
               dY: torch.Tensor | None = None) -> tuple:
    """The edge stage's tensors with da_d's vanishing entries taken out of the ratio: (got, r64,
    r32) for the ratio bar, and the largest |da_d - ref64| / floor over the vanishing entries
    (0.0 when there are none)."""
    ob = one_branch(case[2], arrays)
    fl = da_d_floor(*case, arrays, dY)
    err = (got["edge/da_d"].double() - r64["edge/da_d"]).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / fl)  # (a floor of 0 admits no error)
    frac = q[ob].max().item() if bool(ob.any()) else 0.0
    if not bool(torch.isfinite(got["edge/da_d"]).all()):
        frac = math.inf
    out = []
    for d in (got, r64, r32):
        d = dict(d)
        d["edge/da_d"] = torch.where(ob, torch.zeros_like(d["edge/da_d"]), d["edge/da_d"])
        out.append(d)
    return out[0], out[1], out[2], frac


def host_arrays(H: int, C: int, gname: str, regime: str, masked: bool, act: str,
                slope: float) -> dict:
    """The float32 arrays the kernels hand from stage to stage, formed by the restatement in
    float32 on the CPU (what stands in for the device's arrays where there is no device)."""
    gc = graph(gname)
    i = inputs(H, C, gname)
    mask = i["mask"] if masked else None
    s = f32(slope)
    a_s, a_d = cpu_scores(H, C, gname, regime, torch.float32)
    alpha, Y = gr.fwd(i["XP"], a_s, a_d, gc.csr, s, mask, i["bias"], act)
    dZ, da_e, da_d = gr.bwd_edge(i["XP"], a_s, a_d, alpha, mask, i["dY"], Y, act, s, gc.csr)
    return {"a_s": a_s, "a_d": a_d, "alpha": alpha, "Y": Y, "dZ": dZ, "da_e": da_e, "da_d": da_d}


def variants(H: int, C: int) -> list:
    """(regime, masked, act, slope) of every kernel case of a shape."""
    out = []
    for slope in slopes(H, C):
        for act in ACTS:
            for regime in REGIMES:
                out.append((regime, False, act, slope))
                if regime in MASKED:
                    out.append((regime, True, act, slope))
    return out
