"""GPU: part c of tests/test_gpu_trajectory.py (bench.make_step(("graph:step",)): three eager
steps, capture, four replays on refilled inputs) with the learning-rate schedule switched ON.
lesion_gnn_amd.optim.Adam(capturable=True) keeps the rate in a device tensor that the captured
lgnn_adam_step_dlr launch reads, and LinearWarmupCosineAnnealingLR(**SCHED) is stepped after
every step, replays included: the seven steps run at 1, 1, 1, 0.854, 0.5, 0.146, 0 x 1e-3.

Held to the CPU oracle run with the same scheduler in float64 and float32, the project's bar and
C = 16 (tests/trajectory_ref.check; GIN's gauge tensors left out, nothing else). On the CPU the
float32 oracle stays within 1.01x (gcn), 1.2x (gat) and 4.1x (gin) of itself at other thread
counts (1, 3, 7 against 8) under this bar, and its float32 error is at most 2.5e-5 x max|p|.

The test also runs the oracle with the rate FROZEN at the value the capture saw (0.854e-3 for
the four replays: what a launch-argument rate computes) and asserts that the bar refuses it: on
the CPU it lands at 2.8e5 x (gcn), 3.9e5 x (gin) and 2.4e5 x (gat), flagged on 12 of 17, 20 of
27 and 20 of 25 compared tensors; among those below the bar are the losses of steps 0 to 4,
which the frozen rate has not reached yet (it first differs in step 4's update).

Measured maxima (err / scale) on one MI355X:
  gcn 1.80 (convs.1.bias)   gin 1.91 (convs.1.nn.lins.1.weight)   gat 2.45 (convs.1.bias)
"""
import math

import pytest
import torch

import bench
from lesion_gnn_amd import dropout, optim
from tests import trajectory_ref as tr
from tests.test_gpu_trajectory import C, fwd_loss, got_named, masks_from, report

pytestmark = pytest.mark.gpu

RATES = [1.0, 1.0, 1.0, 0.854, 0.5, 0.146, 0.0]  # x 1e-3: SCHED on CAPTURE_ADAM's base rate


class FrozenAfterCapture(optim.LinearWarmupCosineAnnealingLR):
    """The schedule a captured launch-argument rate follows: it stops at the capture."""

    def get_lr(self):
        if self.last_epoch > tr.CAPTURE_WARMUPS:
            return [g["lr"] for g in self.optimizer.param_groups]
        return super().get_lr()


@pytest.mark.parametrize("family", ["gcn", "gin", "gat"])
def test_captured_replays_follow_the_schedule(cuda, family, monkeypatch):
    W, R = tr.CAPTURE_WARMUPS, tr.CAPTURE_REPLAYS
    batches = tr.capture_batches(family)
    static = batches[0].to(cuda)  # the captured step's static input buffers
    model = tr.build(family).to(cuda).train()
    init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    opt = optim.Adam(model.parameters(), capturable=True, **tr.CAPTURE_ADAM)
    sched = optim.LinearWarmupCosineAnnealingLR(opt, **tr.SCHED)
    held = opt.param_groups[0]["lr"]
    rates = []  # the rate in force at every step (device copies, read once the run is over)

    class ScheduledStep:
        """What make_step steps: the optimizer, with the scheduler stepped after every eager
        (warm-up) step. The capture records the optimizer's launch alone."""
        zero_grad = staticmethod(opt.zero_grad)

        @staticmethod
        def step():
            if torch.cuda.is_current_stream_capturing():
                return opt.step()
            rates.append(held.clone())
            opt.step()
            sched.step()

    one = torch.ones((), device=cuda)
    seen = []  # every executed (or captured) step's loss tensor
    feed = iter(batches)

    def refill():
        nb = next(feed)
        static.x.copy_(nb.x)
        static.y.copy_(nb.y)
        static.edge_index.copy_(nb.edge_index)

    def fwd_bwd():
        if not torch.cuda.is_current_stream_capturing():
            refill()
        _, loss = fwd_loss(family, model, static)
        seen.append(loss.detach())
        loss.backward(one)

    rng0 = dropout.get_state(model._dropout_rng)
    step = bench.make_step(("graph:step",), fwd_bwd, None, ScheduledStep, cuda)
    assert len(seen) == W + 1 and sched.last_epoch == W
    losses = [tr.to64(v) for v in seen[:W]]
    states = [(rng0[0], rng0[1] + i) for i in range(W)]
    for i in range(R):
        refill()
        states.append(dropout.get_state(model._dropout_rng))
        rates.append(held.clone())
        step()
        sched.step()  # between replays: fills the tensor the captured launch reads
        losses.append(tr.to64(seen[-1]))
    assert next(feed, None) is None and opt.param_groups[0]["lr"] is held
    steps = W + R
    assert [float(v) / tr.CAPTURE_ADAM["lr"] for v in rates] == pytest.approx(RATES, abs=5e-4)
    assert sched.last_epoch == steps
    got, ends = got_named(model, opt, losses, None)
    masks = masks_from(states) if family == "gat" else None
    kw = dict(masks_for_step=masks, state=init, batches=batches, eval_after=None,
              adam=tr.CAPTURE_ADAM, scheduler=True)
    r64, r32 = (tr.run_oracle(family, dt, **kw) for dt in (torch.float64, torch.float32))
    detail = {}
    ratios = tr.ratios(got, r64.named(ends), r32.named(ends), family, detail)
    report("captured+sched", family, ratios, detail)
    assert {float(opt.state[p]["step"].item()) for p in model.parameters()} == {float(steps)}
    tr.check(got, r64.named(ends), r32.named(ends), C, family)
    assert math.isfinite(sum(v.item() for v in losses))

    # the bar tells a frozen rate apart: the same oracle, its schedule stopped at the capture
    monkeypatch.setattr(tr, "LinearWarmupCosineAnnealingLR", FrozenAfterCapture)
    frozen = tr.run_oracle(family, torch.float64, **kw)
    with pytest.raises(AssertionError, match="beyond"):
        tr.check(frozen.named(ends), r64.named(ends), r32.named(ends), C, family)
