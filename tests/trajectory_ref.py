"""Multi-step training trajectories of the CPU oracle (oracle/pyg_ref.py) in float32 and float64,
and the bar a HIP trajectory is held to. Test-only; next to tests/dense_ref.py.

A trajectory is: build the model, then for every batch of a schedule zero the gradients, run
forward + cross-entropy + backward, step Adam and step the LR scheduler; one eval-mode no_grad
forward sits between two of the steps. What comes out is every per-step loss, the final
state_dict, the eval logits and Adam's first moments.

The default schedule has six steps whose batches differ in shape as well as in data:
closed 64-node tiles (steps 0, 2, 4), graphs that cross tile boundaries, a 1-node graph, graphs
with fewer than k nodes, a graph larger than 256 nodes, and two steps (0 and 4) with the same
shapes and different data (a cache keyed on shape would hand step 4 the structures of step 0).

The bar (check): for every compared tensor t,
    max|got - ref64| <= C * max(max|ref32 - ref64|, 1e-6 * max|ref64|),
i.e. C times the error the same trajectory picks up when plain torch runs it in float32, with a
floor of 1e-6 relative for tensors the float32 oracle happens to hit exactly.

Adam runs with eps = 1e-4 here, see DESIGN.md ("Adam's eps in the trajectory tests").
"""
from __future__ import annotations

import dataclasses
import math

import torch
import torch.nn.functional as F

import oracle.pyg_ref as ref
from lesion_gnn_amd import models, synth
from lesion_gnn_amd.optim import LinearWarmupCosineAnnealingLR

SIZES = [[64] * 12, [1, 3, 70, 64, 17, 130, 2, 40], [64] * 5, [33, 64, 200, 9], [64] * 12,
         [5, 5, 300]]
STEPS = len(SIZES)
EVAL_AFTER = 3  # the eval forward runs after step 3's update, before step 4
EVAL_SEED, EVAL_SIZES = 99, [64, 7, 130]
DROPOUT_P = 0.35
CPU_MASK_SEED = 777  # on CPU the GAT masks come from ref.DropoutMasks(777, t, 0.35)

ADAM = dict(lr=1e-2, weight_decay=2e-6, eps=1e-4)
SCHED = dict(warmup_epochs=2, max_epochs=6, warmup_start_lr=1e-3)

# The captured-replay schedule (tests/test_gpu_trajectory.py part c): seven steps at one fixed
# shape, every step on other data and topology. bench.make_step runs the first three eagerly
# before it captures; replay i runs on seed 60 + i. The three eager steps get batches of their
# own (57..59) and the constant learning rate is bench.py's 1e-3, both for the bar's sake: this
# float32 oracle run at another CPU thread count stays within 1.1x (gcn, gat) and 5.5x (gin) of
# itself under the bar below, while three warm-ups on batch 60 itself, or lr = 1e-2 with no
# warm-up, overfit or blow up GIN's loss (9e-4, or 8 -> 95) until plain torch float32 misses
# C = 16 against itself (13x to 21x), whatever the device computes.
CAPTURE_SIZES = [64] * 16
CAPTURE_WARMUPS, CAPTURE_REPLAYS = 3, 4
CAPTURE_SEEDS = [57, 58, 59] + [60 + i for i in range(CAPTURE_REPLAYS)]
CAPTURE_ADAM = dict(lr=1e-3, weight_decay=2e-6, eps=1e-4)

FAMILIES = {
    # name: (model class name, positional args, keyword args, batch k, d_in, last_channel_class)
    "gcn": ("GCN", (128, [128] * 3, 5, 0.0), dict(pool="mean"), 8, 128, False),
    "gin": ("GIN", (128, [128] * 3, 5, 0.0), dict(pool="add"), 8, 128, False),
    "gat": ("GAT", (1025, [128] * 4, 5), dict(heads=2, dropout=DROPOUT_P, precision="fp32"),
            6, 1025, True),
    # bitwise (HIP against HIP) families only: no oracle bar
    "gcn_drop": ("GCN", (128, [128] * 3, 5, DROPOUT_P), dict(pool="mean"), 8, 128, False),
    "gat_bf16": ("GAT", (1025, [128] * 4, 5), dict(heads=4, dropout=0.0, precision="bf16"),
                 6, 1025, True),
}

# GIN only: a constant in front of BatchNorm is a gauge direction, so these tensors' gradients are
# analytically zero (or nearly so: in_proj.bias reaches the first BatchNorm through the sum
# aggregation, whose row weights differ) and their trajectories are rounding noise normalised by
# Adam. They are a condition of the bar, not a measurement; nothing else may be left out.
GIN_EXCLUDED = ("in_proj.bias", ".nn.lins.0.bias", "convs.0.nn.norms.0.module.running_mean")


def excluded(family: str, key: str) -> bool:
    if family != "gin":
        return False
    name = key.split("/", 1)[-1]
    return (name == GIN_EXCLUDED[0] or name.endswith(GIN_EXCLUDED[1])
            or name == GIN_EXCLUDED[2])


def build(family: str, oracle: bool = False) -> torch.nn.Module:
    """The family's model under torch.manual_seed(1234): the HIP package's (built on the CPU,
    move it with .to(device)) or the oracle's."""
    cls, args, kw, _, _, _ = FAMILIES[family]
    torch.manual_seed(1234)
    return getattr(ref if oracle else models, cls)(*args, **kw)


def make_batch(family: str, seed: int, sizes: list[int]) -> synth.Batch:
    _, _, _, k, d_in, lcc = FAMILIES[family]
    return synth.make_batch(len(sizes), k=k, d_in=d_in, seed=seed, sizes=sizes,
                            last_channel_class=lcc)


def batch(family: str, t: int) -> synth.Batch:
    """Step t's batch of the six-step schedule."""
    return make_batch(family, 50 + t, SIZES[t])


def capture_batches(family: str) -> list:
    return [make_batch(family, s, CAPTURE_SIZES) for s in CAPTURE_SEEDS]


def eval_batch(family: str) -> synth.Batch:
    return make_batch(family, EVAL_SEED, EVAL_SIZES)


def cpu_masks(t: int) -> ref.DropoutMasks:
    return ref.DropoutMasks(CPU_MASK_SEED, t, DROPOUT_P)


@dataclasses.dataclass
class Trajectory:
    losses: list            # one 0-d tensor per step
    state: dict             # final state_dict, floating tensors as float64
    eval_logits: torch.Tensor | None
    exp_avg: dict           # Adam's first moment per parameter name, float64

    def named(self, exp_avg: tuple = ()) -> dict:
        """Every compared tensor under one key: loss/<t>, state/<name>, eval_logits and
        exp_avg/<name> for the names asked for."""
        out = {f"loss/{t}": v for t, v in enumerate(self.losses)}
        out.update({f"state/{k}": v for k, v in self.state.items()})
        if self.eval_logits is not None:
            out["eval_logits"] = self.eval_logits
        out.update({f"exp_avg/{k}": self.exp_avg[k] for k in exp_avg})
        return out


def to64(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu()
    return t.double() if t.is_floating_point() else t.clone()


def initial_state(family: str) -> dict:
    """The state_dict the HIP model starts from (the oracle is loaded from it)."""
    return {k: v.detach().clone() for k, v in build(family).state_dict().items()}


def run_oracle(family: str, dtype: torch.dtype, masks_for_step=None, *, state: dict | None = None,
               batches: list | None = None, eval_after: int | None = EVAL_AFTER,
               adam: dict | None = None, scheduler: bool = True,
               stale: tuple | None = None) -> Trajectory:
    """The oracle's trajectory in `dtype` (torch.float32 or torch.float64).

    masks_for_step(t) -> ref.DropoutMasks | None: the dropout masks of step t (families with
    dropout; the masks the device drew, or cpu_masks on the CPU).
    state: the initial state_dict (default: the HIP model's under seed 1234).
    batches: the schedule (default: the six steps above); eval_after: the step after which the
    eval forward runs (None: none). adam: torch.optim.Adam's arguments (default ADAM);
    scheduler: step LinearWarmupCosineAnnealingLR(**SCHED) after every optimizer step.
    stale = (step, name): the mutant. At that step only, forward and backward see parameter
    `name` as it was one step earlier (the update then lands on the current value): what a
    kernel reading last step's copy of a weight computes."""
    model = build(family, oracle=True)
    model.load_state_dict(initial_state(family) if state is None else
                          {k: v.detach().cpu() for k, v in state.items()})
    model = model.to(dtype).train()
    names = {p: n for n, p in model.named_parameters()}
    opt = torch.optim.Adam(model.parameters(), foreach=False, **(ADAM if adam is None else adam))
    sched = LinearWarmupCosineAnnealingLR(opt, **SCHED) if scheduler else None
    if batches is None:
        batches = [batch(family, t) for t in range(STEPS)]
    stale_p = dict(model.named_parameters())[stale[1]] if stale is not None else None
    previous = None
    losses, eval_logits = [], None
    for t, b in enumerate(batches):
        kw = {}
        if masks_for_step is not None and masks_for_step(t) is not None:
            kw["masks"] = masks_for_step(t)
        current = None
        if stale is not None and t == stale[0]:
            current = stale_p.data
            stale_p.data = previous
        if stale is not None:
            previous = (stale_p.data if current is None else current).clone()
        opt.zero_grad(set_to_none=True)
        logits = model(b.x.to(dtype), b.edge_index, b.batch, b.num_graphs, **kw)
        loss = F.cross_entropy(logits, b.y)
        loss.backward()
        if current is not None:
            stale_p.data = current
        opt.step()
        if sched is not None:
            sched.step()
        losses.append(to64(loss))
        if eval_after is not None and t == eval_after:
            eb = eval_batch(family)
            model.eval()
            with torch.no_grad():
                eval_logits = to64(model(eb.x.to(dtype), eb.edge_index, eb.batch, eb.num_graphs))
            model.train()
    return Trajectory(losses, {k: to64(v) for k, v in model.state_dict().items()}, eval_logits,
                      {names[p]: to64(s["exp_avg"]) for p, s in opt.state.items()})


def ratios(got: dict, ref64: dict, ref32: dict, family: str, detail: dict | None = None) -> dict:
    """key -> max|got - ref64| / max(max|ref32 - ref64|, 1e-6 max|ref64|) for every compared
    floating tensor (the tensors excluded() names left out); integer tensors must be equal.
    `detail` (optional) receives key -> (err, scale)."""
    if not (got.keys() == ref64.keys() == ref32.keys()):
        raise AssertionError(f"tensor sets differ: {sorted(set(got) ^ set(ref64))} "
                             f"{sorted(set(ref32) ^ set(ref64))}")
    out = {}
    for k, r64 in ref64.items():
        g, r32 = got[k].detach().cpu(), ref32[k]
        if g.shape != r64.shape:
            raise AssertionError(f"{k}: shape {tuple(g.shape)} != {tuple(r64.shape)}")
        if not r64.is_floating_point():
            if not (torch.equal(g.to(r64.dtype), r64) and torch.equal(r32, r64)):
                raise AssertionError(f"{k}: {g.tolist()} != {r64.tolist()}")
            continue
        if excluded(family, k):
            continue
        scale = max((r32 - r64).abs().max().item(), 1e-6 * r64.abs().max().item())
        err = (g.double() - r64).abs().max().item()
        if detail is not None:
            detail[k] = (err, scale)
        if not math.isfinite(err):
            out[k] = math.inf
        elif scale == 0.0:  # an all-zero tensor on both oracles: any difference is a violation
            out[k] = 0.0 if err == 0.0 else math.inf
        else:
            out[k] = err / scale
    return out


def check(got: dict, ref64: dict, ref32: dict, C: float, family: str = "",
          exclude: tuple | None = None) -> dict:
    """Assert the bar for every compared tensor, every per-step loss and the eval logits, and
    report all violations at once with their ratios. Returns the ratios (key -> err / scale).
    `exclude` is the GIN condition above or nothing: any other exclusion is refused."""
    if exclude is not None:
        allowed = GIN_EXCLUDED if family == "gin" else ()
        extra = [e for e in exclude if e not in allowed]
        if extra:
            raise ValueError(f"check({family!r}) refuses to leave out {extra}")
    r = ratios(got, ref64, ref32, family)
    bad = sorted(((v, k) for k, v in r.items() if not v <= C), reverse=True)
    if bad:
        raise AssertionError(f"{family}: {len(bad)} of {len(r)} tensors beyond {C} x the float32 "
                             "oracle's error: " + ", ".join(f"{k} {v:.3g}x" for v, k in bad))
    return r
