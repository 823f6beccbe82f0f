"""Training-step time of the PointNet++ model on the HIP path, and where it goes: milliseconds per
eager step (forward, backward, Adam) and per-entry HIP-event times of one step. There is no
earlier PointNet here and PyG does not run on this stack, so nothing to compare against: the
figures are recorded in DESIGN §4.9, not asserted.

The step is eager (FPS and the radius search size their outputs from the data: three host reads
per forward, no graph capture); it is run for `--seconds` past the clock ramp.

    python tools/time_pointnet.py [--graphs 1024] [--nodes 64] [--d-in 1025] [--seconds 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from collections import defaultdict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lesion_gnn_amd import _lib, synth  # noqa: E402
from lesion_gnn_amd.models import OptimizerAlgo, OptimizerConfig  # noqa: E402
from lesion_gnn_amd.models import PointNetModelConfig, get_model  # noqa: E402


class EntryTimes:
    """_lib tracer: every library entry of a step bracketed by HIP events on its stream."""

    def __init__(self):
        self.spans = []

    def __call__(self, name, args, launch):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        status = launch()
        b.record()
        self.spans.append((name, a, b))
        return status

    def totals(self) -> dict:
        torch.cuda.synchronize()
        ms, calls = defaultdict(float), defaultdict(int)
        for name, a, b in self.spans:
            ms[name] += a.elapsed_time(b)
            calls[name] += 1
        return {k: {"ms": round(v, 4), "calls": calls[k]}
                for k, v in sorted(ms.items(), key=lambda kv: -kv[1])}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--d-in", type=int, default=1025)
    ap.add_argument("--seconds", type=float, default=3.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = PointNetModelConfig(optimizer=OptimizerConfig(algo=OptimizerAlgo.ADAM), pos_dim=2)
    cfg.input_features.value = a.d_in
    cfg.num_classes.value = 5
    cfg.optimizer.class_weights.value = torch.ones(5)
    torch.manual_seed(0)
    module = get_model(cfg).to(dev).train()
    opt = module.configure_optimizers()
    b = synth.make_batch(a.graphs, n=a.nodes, k=2, d_in=a.d_in, seed=1).to(dev)

    def step():
        module.zero_grad(set_to_none=True)
        module.training_step(b).backward()
        opt.step()

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        n += 5
    step_ms = (time.perf_counter() - t0) / n * 1e3

    tracer = EntryTimes()
    _lib.set_tracer(tracer)
    try:
        step()
        entries = tracer.totals()
    finally:
        _lib.set_tracer(None)
    print(json.dumps({"box": torch.cuda.get_device_name(0), "graphs": a.graphs,
                      "nodes": b.x.size(0), "d_in": a.d_in, "step_ms": round(step_ms, 3),
                      "entries_ms": round(sum(e["ms"] for e in entries.values()), 3),
                      "entries": entries}))


if __name__ == "__main__":
    main()
