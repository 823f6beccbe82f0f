"""Training-step time of DRGNet on the HIP path, and the head's share of it: milliseconds per eager
step (forward, backward, Adam), and HIP-event times of the head's forward and backward
(lgnn_drgnet_head_fwd / _bwd) against the torch composition of the same head on the same
parameters and the same pooled rows, in one process. The composition (F.conv1d / F.max_pool1d /
F.linear, i.e. MIOpen + hipBLAS + elementwise launches) is what DRGNet ran before the head kernels
and is written here only: the package holds no such route. The step is also timed with the
composition substituted for the head (the rest of the model as it is), on the same box.

The two heads alternate round by round past the clock ramp; the medians over the rounds are
reported, with the largest difference between the two heads' logits and gradients at this shape.
Figures are recorded in DESIGN §4.13, not asserted.

    timeout -k 10 300 python tools/time_drgnet.py [--graphs 1024] [--nodes 64] [--d-in 1025] \\
        [--hidden 32] [--layers 3] [--k 30] [--seconds 2]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lesion_gnn_amd import _lib, ops, synth  # noqa: E402
from lesion_gnn_amd.models import DRGNetModelConfig, OptimizerAlgo, OptimizerConfig  # noqa: E402
from lesion_gnn_amd.models import get_model  # noqa: E402
from lesion_gnn_amd.transforms import gaussian_distance  # noqa: E402


def torch_head(x, k, w1, b1, w2, b2, l0w, l0b, l1w, l1b, mask=None):
    """The head as torch modules compute it (reference drgnet.py:60-64), dropout as a mask."""
    D = x.size(1) // k
    y = F.max_pool1d(F.elu(F.conv1d(x.unsqueeze(1), w1, b1, stride=D)), 2, 2)
    y = F.elu(F.conv1d(y, w2, b2)).view(x.size(0), -1)
    h = F.elu(F.linear(y, l0w, l0b))
    if mask is not None:
        h = h * mask
    return F.linear(h, l1w, l1b)


def event_ms(fn, reps: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def step_ms(step, seconds: float) -> float:
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        n += 5
    return (time.perf_counter() - t0) / n * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--d-in", type=int, default=1025)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = DRGNetModelConfig(optimizer=OptimizerConfig(algo=OptimizerAlgo.ADAM),
                            gnn_hidden_dim=a.hidden, num_layers=a.layers, sortpool_k=a.k)
    cfg.input_features.value = a.d_in
    cfg.num_classes.value = 5
    cfg.optimizer.class_weights.value = torch.ones(5)
    torch.manual_seed(0)
    module = get_model(cfg).to(dev).train()
    opt = module.configure_optimizers()
    b = synth.make_batch(a.graphs, n=a.nodes, k=6, d_in=a.d_in, seed=1).to(dev)
    data = SimpleNamespace(x=b.x, edge_index=b.edge_index, batch=b.batch, y=b.y,
                           edge_weight=gaussian_distance(b.edge_index, b.pos, 0.1),
                           num_graphs=b.num_graphs)

    def step():
        module.zero_grad(set_to_none=True)
        module.training_step(data).backward()
        opt.step()

    # the head's input at this shape: what SortAggregation hands it in a training forward
    pooled = []
    hook = module.model.sort_pool.register_forward_hook(lambda m, i, o: pooled.append(o.detach()))
    step()
    hook.remove()
    x = pooled[0].contiguous()
    m = module.model
    params = [p.detach() for p in (m.conv1.weight, m.conv1.bias, m.conv2.weight, m.conv2.bias,
                                   *(q for lin in m.mlp.lins for q in (lin.weight, lin.bias)))]
    gen = torch.Generator().manual_seed(2)
    mask = ((torch.rand(x.size(0), params[4].size(0), generator=gen) >= 0.5).float() * 2).to(dev)
    dlogits = torch.randn(x.size(0), params[6].size(0), generator=gen).to(dev)

    # the step, with the HIP head and with the torch composition in its place, alternating
    hip_step, torch_step = [], []
    for _ in range(3):
        hip_step.append(step_ms(step, a.seconds / 3))
        ops.drgnet_head, keep = torch_head, ops.drgnet_head
        try:
            torch_step.append(step_ms(step, a.seconds / 3))
        finally:
            ops.drgnet_head = keep

    # head alone: forward and backward, HIP entries against autograd of the composition
    saved = ops.drgnet_head_fwd(x, a.k, params, mask)[1]
    xt = x.clone().requires_grad_(True)
    pt = [p.clone().requires_grad_(True) for p in params]
    leaves = [xt] + pt

    def torch_fwd():
        return torch_head(xt, a.k, *pt, mask=mask)

    out_t = torch_fwd()

    def torch_bwd():
        return torch.autograd.grad(out_t, leaves, dlogits, retain_graph=True)

    times = {"hip_fwd": [], "hip_bwd": [], "torch_fwd": [], "torch_bwd": []}
    fns = {"hip_fwd": lambda: ops.drgnet_head_fwd(x, a.k, params, mask),
           "hip_bwd": lambda: ops.drgnet_head_bwd(saved, dlogits),
           "torch_fwd": torch_fwd, "torch_bwd": torch_bwd}
    # the C entries alone, outputs and workspace allocated once: what the GPU spends on the head
    # (the op times above also hold the host's allocations and marshalling)
    w1, b1, w2, b2, l0w, l0b, l1w, l1b = params
    B, D, c0, c1, (H, dense), C = x.size(0), x.size(1) // a.k, w1.size(0), w2.size(0), \
        l0w.shape, l1w.size(0)
    lo0 = torch.empty(B, C, device=dev)
    nws = _lib.query("lgnn_drgnet_head_workspace_bytes", B, a.k, D, c0, c1, H, C)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    dxo, dho = torch.empty_like(x), torch.empty(B, H + H % 2, device=dev)
    grads = [torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2),
             torch.empty_like(b2), torch.empty(H + H % 2, dense, device=dev),
             torch.empty(H + H % 2, device=dev), torch.empty_like(l1w), torch.empty_like(l1b)]
    st = _lib.stream(dev)
    fns["entry_fwd"] = lambda: _lib.call(
        "lgnn_drgnet_head_fwd", x, B, a.k, D, w1, b1, c0, w2, b2, c1, l0w, l0b, H, dense, l1w,
        l1b, C, mask, lo0, saved.a1, saved.sel, saved.a2, saved.h, st)
    fns["entry_bwd"] = lambda: _lib.call(
        "lgnn_drgnet_head_bwd", dlogits, x, B, a.k, D, w1, c0, w2, c1, l0w, H, dense, l1w, C,
        mask, saved.a1, saved.sel, saved.a2, saved.h, dxo, dho, *grads, ws, nws, st)
    times["entry_fwd"], times["entry_bwd"] = [], []
    for fn in fns.values():  # warm every shape
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in fns.items():
            times[name].append(event_ms(fn, 50))
    med = {k: statistics.median(v) for k, v in times.items()}

    # the two heads compute the same thing at this shape
    lo_h, sv = ops.drgnet_head_fwd(x, a.k, params, mask)
    dx_h, dp_h = ops.drgnet_head_bwd(sv, dlogits)
    g_t = torch_bwd()
    diffs = {"logits": (lo_h - out_t.detach()).abs().max().item()}
    for name, g, w in zip(["dx", "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias",
                           "lins.0.weight", "lins.0.bias", "lins.1.weight", "lins.1.bias"],
                          [dx_h] + dp_h, g_t):
        diffs[name] = ((g - w).abs().max() / w.abs().max().clamp_min(1e-30)).item()
    print(json.dumps({
        "box": torch.cuda.get_device_name(0), "graphs": a.graphs, "nodes": b.x.size(0),
        "d_in": a.d_in, "k": a.k, "D": x.size(1) // a.k,
        "step_ms": round(statistics.median(hip_step), 3),
        "step_ms_torch_head": round(statistics.median(torch_step), 3),
        "head_fwd_us": round(med["hip_fwd"] * 1e3, 2), "head_bwd_us": round(med["hip_bwd"] * 1e3, 2),
        "torch_head_fwd_us": round(med["torch_fwd"] * 1e3, 2),
        "torch_head_bwd_us": round(med["torch_bwd"] * 1e3, 2),
        "head_fwd_bwd_us": round((med["hip_fwd"] + med["hip_bwd"]) * 1e3, 2),
        "entry_fwd_us": round(med["entry_fwd"] * 1e3, 2),
        "entry_bwd_us": round(med["entry_bwd"] * 1e3, 2),
        "torch_head_fwd_bwd_us": round((med["torch_fwd"] + med["torch_bwd"]) * 1e3, 2),
        "spread_us": {k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in times.items()},
        "max_difference_hip_vs_torch": {k: float(f"{v:.3e}") for k, v in diffs.items()}}))


if __name__ == "__main__":
    main()
