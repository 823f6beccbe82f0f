"""GPU: lesion_gnn_amd.optim.SGD (lgnn_sgd_step, one HIP launch per 16 tensors) vs
torch.optim.SGD(foreach=False) on the same parameters and gradients. fp32; the same operations,
fused differently in the last bits only (tests/test_gpu_optim.py's rtol 1e-5, atol 1e-7)."""
import copy

import pytest
import torch

from lesion_gnn_amd import _lib, optim

pytestmark = pytest.mark.gpu

FIVE = [(128, 128), (128,), (5, 128), (5,), (3, 7, 2)]
# numel 0, 1, 3 and 130; more than 16 tensors, so three launches per step
FORTY = [(3,), (0,), (17, 5), (1,), (64,), (0, 4), (130,), (2, 2)] * 5
CASES = {
    "plain_wd": dict(weight_decay=0.01),  # the reference's call
    "momentum": dict(momentum=0.9),
    "dampening": dict(momentum=0.9, dampening=0.3),  # first step: buf = g, not (1 - 0.3) g
    "nesterov": dict(momentum=0.9, nesterov=True, weight_decay=1e-3),
    "maximize": dict(momentum=0.5, maximize=True, weight_decay=0.01),
}


# The momentum buffer is a signed sum of up to six gradient terms that may cancel, and each of its
# operations rounds at the size of its operands (2^-24 relative), not of the sum: its absolute
# bound is 6 steps x 3 roundings (the weight decay, the scaled buffer, the sum) of the largest
# gradient element. The parameters, which the buffer reaches scaled by lr, keep 1e-5 / 1e-7.
BUF_ULPS = 6 * 3


def _params(cuda, shapes, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(*s, generator=g).to(cuda).requires_grad_() for s in shapes]


def _close(ours, ref):
    for a, b in zip(ours, ref):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("shapes", [FIVE, FORTY], ids=["five", "forty"])
@pytest.mark.parametrize("case", list(CASES))
def test_sgd_matches_torch(cuda, case, shapes):
    kw = CASES[case]
    ours, ref = _params(cuda, shapes, 0), _params(cuda, shapes, 0)
    o = optim.SGD(ours, lr=1e-2, **kw)
    r = torch.optim.SGD(ref, lr=1e-2, foreach=False, **kw)
    gen = torch.Generator(device="cpu").manual_seed(1)
    gmax = 0.0
    for _ in range(6):
        for a, b in zip(ours, ref):
            gr = torch.randn(a.shape, generator=gen).to(cuda)
            a.grad, b.grad = gr.clone(), gr.clone()
            gmax = max(gmax, gr.abs().max().item() if gr.numel() else 0.0)
        o.step()
        r.step()
    _close(ours, ref)
    if kw.get("momentum"):
        for a, b in zip(ours, ref):
            torch.testing.assert_close(o.state[a]["momentum_buffer"],
                                       r.state[b]["momentum_buffer"], rtol=1e-5,
                                       atol=BUF_ULPS * 2.0 ** -24 * gmax)
        assert {float(o.state[a]["step"]) for a in ours} == {6.0}
    else:
        assert not any(o.state[a] for a in ours)  # as torch: no state without momentum


def test_sgd_captured_replays_no_host_sync(cuda):
    """One momentum step captured after one eager step, replayed 12 times back to back: the
    device step count keeps the first-step rule out of the replays and reads 13."""
    p, q = _params(cuda, FORTY, 11), _params(cuda, FORTY, 11)
    gen = torch.Generator(device="cpu").manual_seed(2)
    for a, b in zip(p, q):
        g = torch.randn(a.shape, generator=gen).to(cuda)
        a.grad, b.grad = g.clone(), g.clone()
    kw = dict(lr=3e-3, momentum=0.9, dampening=0.3, weight_decay=1e-3)
    o = optim.SGD(p, **kw)
    r = torch.optim.SGD(q, foreach=False, **kw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        o.step()  # warm-up: allocates the state outside capture
    torch.cuda.current_stream().wait_stream(s)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        o.step()
    for _ in range(12):
        gph.replay()
    for _ in range(13):
        r.step()
    torch.cuda.synchronize()
    assert float(o.state[p[0]]["step"]) == 13.0
    _close(p, q)


def test_sgd_refusals(cuda):
    w = torch.zeros(2, requires_grad=True)
    w.grad = torch.zeros(2)
    with pytest.raises(_lib.LgnnError):
        optim.SGD([w], lr=0.1).step()  # no CPU path
    h = torch.zeros(4, device=cuda, dtype=torch.float64, requires_grad=True)
    h.grad = torch.zeros_like(h)
    with pytest.raises(_lib.LgnnError):
        optim.SGD([h], lr=0.1).step()  # fp32 only
    t = torch.zeros(4, 4, device=cuda).t().requires_grad_()
    t.grad = torch.zeros(4, 4, device=cuda).t()
    with pytest.raises(_lib.LgnnError):
        optim.SGD([t], lr=0.1).step()  # contiguous only
    g = [torch.zeros(2, device=cuda, requires_grad=True)]
    with pytest.raises(ValueError):
        optim.SGD(g, lr=0.1, nesterov=True)  # needs momentum > 0
    with pytest.raises(ValueError):
        optim.SGD(g, lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)  # and no dampening


def test_sgd_continues_from_a_torch_state(cuda):
    """torch.optim.SGD's state has a momentum_buffer and no step: loaded here it continues from
    the buffer (no first-step rule on the next step), and a parameter that joins later takes
    its own first step as torch's would."""
    kw = dict(lr=1e-2, momentum=0.9, dampening=0.3)
    shapes = FIVE + [(9,)]
    ours, ref = _params(cuda, shapes, 4), _params(cuda, shapes, 4)
    r = torch.optim.SGD(ref, foreach=False, **kw)
    gen = torch.Generator(device="cpu").manual_seed(5)

    def grads(n):
        for a, b in list(zip(ours, ref))[:n]:
            gr = torch.randn(a.shape, generator=gen).to(cuda)
            a.grad, b.grad = gr.clone(), gr.clone()

    for _ in range(2):  # torch alone; the last parameter has no gradient yet, so no state
        grads(len(FIVE))
        r.step()
    for a, b in zip(ours, ref):
        a.data.copy_(b.data)
    o = optim.SGD(ours, **kw)
    o.load_state_dict(copy.deepcopy(r.state_dict()))  # state_dict() hands out r's own buffers
    assert "step" not in o.state[ours[0]] and not o.state[ours[-1]]
    for _ in range(3):
        grads(len(shapes))
        o.step()
        r.step()
    _close(ours, ref)
    for a, b in zip(ours, ref):  # gradients of at most 6 here: BUF_ULPS' bound at that size
        torch.testing.assert_close(o.state[a]["momentum_buffer"], r.state[b]["momentum_buffer"],
                                   rtol=1e-5, atol=BUF_ULPS * 2.0 ** -24 * 6.0)
    assert {float(o.state[a]["step"]) for a in ours} == {4.0}  # 1 (a loaded buffer) + 3


def test_configure_optimizers_sgd_steps_on_the_gpu(cuda):
    from lesion_gnn_amd.models import GCNConfig, OptimizerConfig, get_model
    from lesion_gnn_amd.models.base import OptimizerAlgo

    cfg = GCNConfig(optimizer=OptimizerConfig(algo=OptimizerAlgo.SGD, loss_type="MSE"),
                    hidden_channels=[16, 16], dropout=0.0, compile=False)
    cfg.num_classes.value, cfg.input_features.value = 5, 8
    module = get_model(cfg).to(cuda)
    opt = module.configure_optimizers(capturable=True)
    assert type(opt) is optim.SGD
    lr = opt.param_groups[0]["lr"]
    assert lr.is_cuda and lr.dim() == 0 and lr.dtype == torch.float32
    before = [p.detach().clone() for p in module.parameters()]
    for p in module.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    for p, b in zip(module.parameters(), before):  # the reference's call: lr 1e-3, wd 1e-2
        torch.testing.assert_close(p.detach(), b - 1e-3 * (1 + 1e-2 * b), rtol=1e-5, atol=1e-7)
