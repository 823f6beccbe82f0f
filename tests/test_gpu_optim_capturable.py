"""GPU: capturable=True, the learning rate as a device tensor the launch reads
(lgnn_adam_step_dlr, lgnn_sgd_step's lr_dev), so that an LR scheduler acts on the replays of a
captured step. Tolerances against torch.optim.*(foreach=False) are tests/test_gpu_optim.py's
(rtol 1e-5, atol 1e-7); capturable against the default path is bitwise."""
import warnings

import pytest
import torch

from lesion_gnn_amd import optim

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-7
SHAPES = [(128, 128), (128,), (5, 128), (5,), (3, 7, 2), (0,), (1,), (130,)] * 3  # 24: 2 launches
SCHED = dict(warmup_epochs=2, max_epochs=8, warmup_start_lr=1e-3)  # base 1e-2
KINDS = {
    "adam": (optim.Adam, torch.optim.Adam, dict(lr=1e-2, betas=(0.8, 0.95), weight_decay=1e-3)),
    "adamw": (optim.AdamW, torch.optim.AdamW, dict(lr=1e-2, betas=(0.8, 0.95))),
    "sgd": (optim.SGD, torch.optim.SGD, dict(lr=1e-2, momentum=0.9, dampening=0.3,
                                             weight_decay=1e-3)),
}


def _params(cuda, shapes, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(*s, generator=g).to(cuda).requires_grad_() for s in shapes]


def _grads(cuda, shapes, seed, steps):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [[torch.randn(s, generator=g).to(cuda) for s in shapes] for _ in range(steps)]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)  # in place: a captured step reads these tensors


def _close(ours, ref):
    for a, b in zip(ours, ref):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=RTOL, atol=ATOL)


def _captured(cuda, opt, params, grads0):
    """One eager step of `opt` on a side stream, then its step captured: the graph."""
    _set_grads(params, grads0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        opt.step()  # warm-up: allocates the state outside capture
    torch.cuda.current_stream().wait_stream(s)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        opt.step()
    return gph


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_capturable_is_bitwise_the_default_path(cuda, kind):
    cls, _, kw = KINDS[kind]
    a, b = _params(cuda, SHAPES, 0), _params(cuda, SHAPES, 0)
    oa, ob = cls(a, capturable=True, **kw), cls(b, **kw)
    lr = oa.param_groups[0]["lr"]
    assert isinstance(lr, torch.Tensor) and lr.is_cuda and lr.dim() == 0
    assert lr.dtype == torch.float32 and isinstance(ob.param_groups[0]["lr"], float)
    for grads in _grads(cuda, SHAPES, 1, 6):
        _set_grads(a, grads)
        _set_grads(b, grads)
        oa.step()
        ob.step()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"])
        assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])
    assert float(oa.state[a[0]]["step"]) == float(ob.state[b[0]]["step"]) == 6.0
    assert oa.param_groups[0]["lr"] is lr


def test_a_device_tensor_lr_is_taken_as_it_is(cuda):
    p = _params(cuda, [(4,)], 0)
    lr = torch.full((1,), 1e-2, device=cuda)
    for cls in (optim.Adam, optim.AdamW, optim.SGD):
        assert cls(p, lr=lr, capturable=True).param_groups[0]["lr"] is lr
    with pytest.raises(ValueError):
        optim.Adam(p, lr=torch.tensor(1e-2), capturable=True)  # not on the parameters' device
    o = optim.SGD(p, lr=1e-2, capturable=True)
    held = o.param_groups[0]["lr"]
    o.add_param_group({"params": _params(cuda, [(3,)], 1), "lr": 5e-3})
    assert o.param_groups[0]["lr"] is held and float(held) == pytest.approx(1e-2)
    new = o.param_groups[1]["lr"]
    assert new is not held and new.is_cuda and float(new) == pytest.approx(5e-3)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_scheduler_acts_on_replays(cuda, kind):
    """One captured step, scheduler.step() before each of 6 replays, against torch's optimizer
    under the same scheduler stepped eagerly; and against torch's with the rate held at the
    captured value, which this test must be able to tell apart."""
    cls, tcls, kw = KINDS[kind]
    steps = 7
    grads = _grads(cuda, SHAPES, 1, steps)
    p, q, z = (_params(cuda, SHAPES, 0) for _ in range(3))
    o = cls(p, capturable=True, **kw)
    r, f = tcls(q, foreach=False, **kw), tcls(z, foreach=False, **kw)
    so = optim.LinearWarmupCosineAnnealingLR(o, **SCHED)
    sr = optim.LinearWarmupCosineAnnealingLR(r, **SCHED)
    f.param_groups[0]["lr"] = SCHED["warmup_start_lr"]  # what the capture saw, held
    held = o.param_groups[0]["lr"]
    gph = _captured(cuda, o, p, grads[0])
    rates = [float(held)]
    for t in range(1, steps):
        so.step()
        rates.append(float(held))
        _set_grads(p, grads[t])
        gph.replay()
    for t in range(steps):
        _set_grads(q, grads[t])
        _set_grads(z, grads[t])
        r.step()
        f.step()
        if t + 1 < steps:
            sr.step()
    torch.cuda.synchronize()
    assert o.param_groups[0]["lr"] is held
    assert rates[:3] == [pytest.approx(v) for v in (1e-3, 1e-2, 1e-2)], rates
    assert all(x > y > 0 for x, y in zip(rates[2:], rates[3:])), rates  # then the cosine
    _close(p, q)
    assert float(o.state[p[0]]["step"]) == float(steps)
    # a frozen rate lands far outside the tolerance: on every tensor of some size (a lone
    # element may have met small gradients), hence on the parameters as a whole
    for a, b in zip(p, z):
        if a.numel() >= 100:
            excess = ((a - b).abs() / (ATOL + RTOL * b.abs())).max().item()
            assert excess > 100.0, (tuple(a.shape), excess)


def test_scheduler_step_and_replay_read_nothing_on_the_host(cuda):
    p = _params(cuda, SHAPES, 0)
    o = optim.Adam(p, lr=1e-2, capturable=True)
    sched = optim.LinearWarmupCosineAnnealingLR(o, **SCHED)
    gph = _captured(cuda, o, p, _grads(cuda, SHAPES, 1, 1)[0])
    sched.step()
    gph.replay()  # warm: the scheduler's and the replay's allocations are made
    torch.cuda.synchronize()
    before = float(o.param_groups[0]["lr"])
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            for _ in range(3):  # warm-up's end and two cosine steps
                sched.step()
                gph.replay()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()]
    assert not syncs, syncs
    assert float(o.param_groups[0]["lr"]) != before and float(o.state[p[0]]["step"]) == 5.0


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_loaded_rate_reaches_the_captured_step(cuda, kind):
    """load_state_dict after capture copies the loaded rate into the tensor the graph reads."""
    cls, tcls, kw = KINDS[kind]
    grads = _grads(cuda, SHAPES, 1, 1)[0]
    p, q = _params(cuda, SHAPES, 0), _params(cuda, SHAPES, 0)
    o, r = cls(p, capturable=True, **kw), tcls(q, foreach=False, **kw)
    gph = _captured(cuda, o, p, grads)
    gph.replay()
    _set_grads(q, grads)
    r.step()
    r.step()
    held = o.param_groups[0]["lr"]
    ptr = held.data_ptr()
    for loaded in (5e-3, torch.tensor(2e-3)):  # a float, and a saved tensor
        sd = o.state_dict()
        sd["param_groups"][0]["lr"] = loaded
        o.load_state_dict(sd)
        assert o.param_groups[0]["lr"] is held and held.data_ptr() == ptr
        assert float(held) == pytest.approx(float(loaded))
        gph.replay()
        r.param_groups[0]["lr"] = float(loaded)
        r.step()
    torch.cuda.synchronize()
    _close(p, q)
    assert float(o.state[p[0]]["step"]) == 4.0
