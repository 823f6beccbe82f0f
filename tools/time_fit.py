"""Time of a training epoch of `lesion_gnn_amd.training.Trainer` at the reference experiment's
shape (configs/config.py: GAT [128] * 4, heads 2, KNNGraph(k=6, loop=True), one full-batch step
per epoch) with the per-graph transforms hoisted into the stores (DataModule(hoist=True): the
loader collates stored edges, lgnn_collate_edges) and with the per-batch chain (hoist=False: the
loader rebuilds the k-NN graph of the collated batch every step, which is what the loader did
before stores kept edges). Recorded in DESIGN §4.12.

One process, one model and optimizer; the two loaders take turns epoch by epoch, so both modes
see the same clocks and the same neighbours on the machine. Per mode, after `--warmup` epochs of
each: the median and the quartiles of the epoch time (host clock around an epoch that ends in a
device synchronise: the epoch has host work), and the median HIP-event time of every library
entry the loader calls (events recorded around the launch by the _lib tracer, in separate epochs
from the timed ones: the tracer synchronises nothing but costs host time).

    python tools/time_fit.py [--graphs 6000] [--d-in 1025] [--epochs 50] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOADER_ENTRIES = ("lgnn_collate", "lgnn_collate_edges", "lgnn_batch_ptr", "lgnn_knn_graph")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=6000)
    ap.add_argument("--d-in", type=int, default=1025)
    ap.add_argument("--batch-size", type=int, default=10000)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--traced", type=int, default=10, help="epochs per mode under the tracer")
    a = ap.parse_args()

    import torch

    from lesion_gnn_amd import _lib, synth
    from lesion_gnn_amd.datasets import DataConfig, DataModule, GraphStore
    from lesion_gnn_amd.datasets.base import BaseDatasetConfig
    from lesion_gnn_amd.models import GATConfig, OptimizerConfig, get_model
    from lesion_gnn_amd.training import Trainer
    from lesion_gnn_amd.transforms import TransformConfig

    if not torch.cuda.is_available():
        sys.exit("time_fit: no GPU; a CPU run says nothing about these times")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    sizes = torch.tensor(synth.graph_sizes(a.graphs, "lognormal", gen), dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    rows = int(ptr[-1])
    torch.manual_seed(0)
    x = torch.randn(rows, a.d_in, dtype=torch.float32, device=dev)
    x[:, -1] = torch.randint(0, 5, (rows,), device=dev).float()  # the lesion class channel
    pos = torch.rand(rows, 2, dtype=torch.float64, device=dev)
    y = torch.randint(0, 5, (a.graphs,), generator=gen)
    stores = {"train": GraphStore(x, pos, y, ptr)}

    data = DataConfig(train_datasets=[BaseDatasetConfig(name="train", root="", nodes=None)],
                      val_datasets=[], test_datasets=[],
                      transforms=[TransformConfig(name="KNNGraph", kwargs=dict(k=6, loop=True))],
                      batch_size=a.batch_size, num_workers=0)
    model_cfg = GATConfig(optimizer=OptimizerConfig(lr=1e-3), hiddden_channels=[128] * 4, heads=2,
                          dropout=0.0, compile=False)
    loaders = {}
    for mode, hoist in (("hoist", True), ("per_batch", False)):
        dm = DataModule(data, compile=False, stores=stores, hoist=hoist)
        dm.generator = torch.Generator().manual_seed(1)
        dm.setup("fit")
        loaders[mode] = dm.train_dataloader()
        if hoist:
            model_cfg.optimizer.class_weights.value = dm.get_class_weights()
            model_cfg.num_classes.value = dm.num_classes
            model_cfg.input_features.value = dm.num_features
            edges = dm.train_datasets.edge_index.size(1)
    module = get_model(model_cfg).to(dev)
    total = 2 * (a.warmup + a.epochs + a.traced)
    trainer = Trainer(max_epochs=total, check_val_every_n_epoch=total + 1)
    trainer.prepare(module)

    epoch = 0

    def run_epoch(mode: str) -> float:
        nonlocal epoch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.train_epoch(module, loaders[mode], epoch)
        torch.cuda.synchronize()
        epoch += 1
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        for mode in loaders:
            run_epoch(mode)
    wall = {mode: [] for mode in loaders}
    for _ in range(a.epochs):
        for mode in loaders:  # the modes alternate
            wall[mode].append(run_epoch(mode))

    spans = {mode: {} for mode in loaders}
    current = [None]

    def tracer(name, args, launch):
        if name not in LOADER_ENTRIES:
            return launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        status = launch()
        e1.record()
        spans[current[0]].setdefault(name, []).append((e0, e1))
        return status

    _lib.set_tracer(tracer)
    try:
        for _ in range(a.traced):
            for mode in loaders:
                current[0] = mode
                run_epoch(mode)
    finally:
        _lib.set_tracer(None)
    torch.cuda.synchronize()

    out = {"box": torch.cuda.get_device_name(0), "graphs": a.graphs, "rows": rows, "edges": edges,
           "d_in": a.d_in, "steps_per_epoch": len(loaders["hoist"]), "epochs": a.epochs,
           "warmup": a.warmup}
    for mode in loaders:
        q = statistics.quantiles(wall[mode], n=4)
        out[mode] = {"epoch_ms": round(q[1], 3), "epoch_ms_q1": round(q[0], 3),
                     "epoch_ms_q3": round(q[2], 3),
                     "entries_ms": {name: round(statistics.median(e0.elapsed_time(e1)
                                                                  for e0, e1 in ev), 4)
                                    for name, ev in sorted(spans[mode].items())}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
