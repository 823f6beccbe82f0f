"""Time of one collated batch out of a GPU-resident GraphStore at the reference experiment's
shape (d_in 1025, lognormal graph sizes, 1024 or 10000 graphs per batch), three figures per batch
size, recorded in DESIGN §4.10:

  a  lgnn_collate on preallocated buffers, and its effective bandwidth (bytes read plus bytes
     written over time) as a fraction of the measured float4-copy rate of the part (6.29 TB/s);
  b  the torch composition that produces the same tensors (two index_selects, y[ids],
     repeat_interleave, cumsum), its per-row source index built outside the timed region;
  c  one GraphLoader step: ids to the device, collate, KNNGraph(k=6, loop=True).

Medians over `--iters` different batches after `--warmup`, by HIP events (c: wall clock around a
synchronised step, since the step has host work). Every figure is measured in a child process of
its own under `timeout`; the first one that fails ends the run.

    python tools/time_loader.py [--batches 1024,10000] [--store-graphs 12000] [--iters 50]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_TBPS = 6.29


def make_store(num_graphs: int, d_in: int, dev):
    import torch

    from lesion_gnn_amd import synth
    from lesion_gnn_amd.datasets import GraphStore

    gen = torch.Generator().manual_seed(0)
    sizes = torch.tensor(synth.graph_sizes(num_graphs, "lognormal", gen), dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    rows = int(ptr[-1])
    torch.manual_seed(0)
    x = torch.randn(rows, d_in, dtype=torch.float32, device=dev)
    pos = torch.rand(rows, 2, dtype=torch.float64, device=dev)
    y = torch.randint(0, 5, (num_graphs,), generator=gen)
    return GraphStore.from_tensors(x, pos, y, ptr)


def selections(store, batch: int, count: int):
    import torch

    gen = torch.Generator().manual_seed(1)
    return [torch.randperm(len(store), generator=gen)[:batch] for _ in range(count)]


def event_ms(fn, jobs, warmup: int) -> list[float]:
    import torch

    for j in jobs[:warmup]:
        fn(j)
    torch.cuda.synchronize()
    spans = []
    for j in jobs:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(j)
        b.record()
        spans.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in spans]


def part(a) -> dict:
    import torch

    from lesion_gnn_amd import _lib
    from lesion_gnn_amd.datasets import GraphLoader
    from lesion_gnn_amd.knn import KNNGraph

    dev = torch.device("cuda:0")
    store = make_store(a.store_graphs, a.d_in, dev)
    B, C = a.batch, a.d_in
    sels = selections(store, B, a.iters)
    totals = [int((store.ptr_host[s + 1] - store.ptr_host[s]).sum()) for s in sels]
    cap = max(totals)
    out = {"part": a.part, "box": torch.cuda.get_device_name(0), "graphs": B, "d_in": C,
           "store_graphs": len(store), "store_rows": store.x.size(0),
           "rows_median": int(statistics.median(totals))}
    if a.part == "a":
        ox = torch.empty(cap, C, dtype=torch.float32, device=dev)
        op = torch.empty(cap, 2, dtype=torch.float64, device=dev)
        ob = torch.empty(cap, dtype=torch.int64, device=dev)
        oy = torch.empty(B, dtype=torch.int64, device=dev)
        optr = torch.empty(B + 1, dtype=torch.int64, device=dev)
        err = torch.empty(1, dtype=torch.int32, device=dev)
        nws = _lib.load().lgnn_collate_workspace_bytes(B)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        ids = [s.to(dev) for s in sels]
        stream = _lib.stream(dev)

        def run(k):
            _lib.call("lgnn_collate", ids[k], B, store.ptr, len(store), store.x, C, store.pos, 2,
                      store.y, ox, op, oy, ob, optr, cap, err, ws, nws, stream)

        ms = event_ms(run, list(range(len(sels))), a.warmup)
        # bytes read + written: x and pos both ways, batch, and the per-graph words
        byt = [2 * t * (4 * C + 16) + 8 * t + B * 48 for t in totals]
        tbps = statistics.median(b / (m * 1e-3) / 1e12 for b, m in zip(byt, ms))
        out.update(collate_ms=round(statistics.median(ms), 4), tbps=round(tbps, 3),
                   fraction_of_copy_rate=round(tbps / HBM_COPY_TBPS, 3), err=int(err.item()))
    elif a.part == "b":
        jobs = []
        for s in sels:  # the per-row source index and the sizes: given, not timed
            sizes = (store.ptr_host[s + 1] - store.ptr_host[s])
            starts = torch.repeat_interleave(store.ptr_host[s], sizes)
            optr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
            within = torch.arange(int(optr[-1])) - torch.repeat_interleave(optr[:-1], sizes)
            jobs.append((s.to(dev), (starts + within).to(dev), sizes.to(dev), int(optr[-1])))
        gids = torch.arange(B, device=dev)
        zero = torch.zeros(1, dtype=torch.int64, device=dev)

        def run(j):
            ids, rows, sizes, total = j
            return (store.x.index_select(0, rows), store.pos.index_select(0, rows),
                    store.y[ids], torch.repeat_interleave(gids, sizes, output_size=total),
                    torch.cat([zero, sizes.cumsum(0)]))

        ms = event_ms(run, jobs, a.warmup)
        out.update(torch_ms=round(statistics.median(ms), 4))
    else:
        loader = GraphLoader(store, B, shuffle=True, drop_last=True,
                             transform=KNNGraph(k=6, loop=True),
                             generator=torch.Generator().manual_seed(2))

        def epochs():
            while True:
                yield from loader

        ms = []
        it = epochs()
        for k in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch = next(it)
            torch.cuda.synchronize()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        out.update(loader_step_ms=round(statistics.median(ms), 4), steps=len(ms),
                   edges=batch.edge_index.size(1))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,10000")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--store-graphs", type=int, default=12000)
    ap.add_argument("--d-in", type=int, default=1025)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=150, help="seconds per figure")
    ap.add_argument("--part", choices=["a", "b", "c"], default=None)
    a = ap.parse_args()
    if a.part is not None:
        print(json.dumps(part(a)), flush=True)
        return
    for batch in (int(b) for b in a.batches.split(",")):
        for p in "abc":
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__),
                   "--part", p, "--batch", str(batch), "--store-graphs", str(a.store_graphs),
                   "--d-in", str(a.d_in), "--iters", str(a.iters), "--warmup", str(a.warmup)]
            status = subprocess.run(cmd).returncode
            if status != 0:
                sys.exit(f"time_loader: part {p} at {batch} graphs ended with status {status}")


if __name__ == "__main__":
    main()
