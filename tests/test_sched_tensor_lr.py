"""CPU: the schedulers the reference draws (scripts/sweep.py: LinearWarmupCosineAnnealingLR,
CosineAnnealingWarmRestarts) driving a TENSOR lr, which is what a capturable optimizer holds
(lesion_gnn_amd.optim, capturable=True): torch's schedulers fill_ the tensor in place, and the
recursive forms then step the rate in fp32 instead of Python floats.

Bar: every epoch's value within 1e-5 x base_lr of the same scheduler on a float lr. fp32 carries
6e-8 relative per operation and the recursive form compounds one or two per epoch; measured
worst case over the cases below: 8e-7 x base, at 500 epochs.
"""
import pytest
import torch

from lesion_gnn_amd.optim import LinearWarmupCosineAnnealingLR

BASE = 1e-3
WARMUP_COSINE = [(10, 100, 0.0, 0.0), (5, 40, 1e-4, 1e-5), (3, 7, 0.0, 1e-6), (0, 20, 1e-4, 0.0),
                 (1, 20, 1e-4, 0.0), (0, 9, 0.0, 1e-6), (10, 500, 0.0, 0.0)]


def _rates(lr, make, epochs):
    """(rates per epoch, the optimizer's lr object at the end) under scheduler make(opt)."""
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.Adam([p], lr=lr, foreach=False)
    held = opt.param_groups[0]["lr"]
    sch = make(opt)
    out = []
    for _ in range(epochs):
        out.append(float(opt.param_groups[0]["lr"]))
        p.grad = torch.ones(2)
        opt.step()
        sch.step()
    return out, held, opt.param_groups[0]["lr"]


def _check(make, epochs):
    want, _, _ = _rates(BASE, make, epochs)
    got, held, last = _rates(torch.tensor(BASE), make, epochs)
    assert isinstance(held, torch.Tensor) and last is held  # filled in place, never replaced
    assert held.dtype == torch.float32
    worst = max(abs(g - w) for g, w in zip(got, want))
    print(f"worst |tensor - float| = {worst / BASE:.3g} x base over {epochs} epochs")
    for e, (g, w) in enumerate(zip(got, want)):
        assert abs(g - w) <= 1e-5 * BASE, (e, g, w)
    assert len(set(want)) > 1  # the schedule moved


@pytest.mark.parametrize("warmup,max_epochs,start,eta", WARMUP_COSINE)
def test_warmup_cosine_drives_a_tensor_lr(warmup, max_epochs, start, eta):
    _check(lambda opt: LinearWarmupCosineAnnealingLR(opt, warmup_epochs=warmup,
                                                     max_epochs=max_epochs, warmup_start_lr=start,
                                                     eta_min=eta), max_epochs + 1)


def test_cosine_warm_restarts_drives_a_tensor_lr():
    _check(lambda opt: torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=7, T_mult=2),
           50)
