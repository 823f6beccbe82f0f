#!/usr/bin/env python3
"""HIP-event timing of the evaluation path against the same metrics from plain torch GPU ops
(DESIGN.md §4.5): one GradingMetrics.update at B = 1024, C = 5, and one compute launch sequence
at N = 16,384 stored scores (no host read on either side). Prints one JSON line.

    python tools/time_metrics.py [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lesion_gnn_amd.metrics import GradingMetrics  # noqa: E402

C, B, N = 5, 1024, 16384


def timed(fn, iters, warmup):
    """Mean microseconds per call of fn over `iters` calls between two events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def torch_update(state, z, y):
    """What torchmetrics' updates do per batch, as torch ops: argmax, confusion matrix, the
    referable probabilities and counts, the criterion; scores and targets appended."""
    pred = torch.argmax(z, dim=1)
    state["conf"] += torch.bincount(y * C + pred, minlength=C * C)
    score = torch.softmax(z, dim=-1)[:, 2:].sum(dim=-1)
    rt, rp = y >= 2, score > 0.5
    state["ref"] += torch.bincount(rt.long() * 2 + rp.long(), minlength=4)
    state["loss"] += torch.nn.functional.cross_entropy(z, y, reduction="sum")
    state["scores"].append(score)
    state["positive"].append(rt)


def torch_compute(conf, ref, scores, positive):
    """Every metric from the accumulated state with torch ops; AUROC / AUPRC by a device sort and
    cumulative sums over the distinct thresholds (torchmetrics' thresholds=None path)."""
    conf = conf.double()
    n = conf.sum()
    rows, cols, tp = conf.sum(1), conf.sum(0), conf.diagonal()
    idx = torch.arange(C, device=conf.device, dtype=torch.float64)
    w = (idx[:, None] - idx[None, :]) ** 2
    kappa = 1 - (w * conf).sum() / ((w * torch.outer(rows, cols)).sum() / n)
    fp, fn = cols - tp, rows - tp
    present = (tp + fp + fn) > 0

    def macro(num, den):
        return torch.where(den > 0, num / den, torch.zeros_like(num))[present].mean()

    tn_, fp_, fn_, tp_ = ref.double().unbind()
    s, order = torch.sort(scores, descending=True)
    pos = positive[order].double()
    tps, fps = torch.cumsum(pos, 0), torch.cumsum(1 - pos, 0)
    last = torch.cat([s[1:] != s[:-1], torch.ones(1, dtype=torch.bool, device=s.device)])
    tps, fps = tps[last], fps[last]
    zero = torch.zeros(1, dtype=torch.float64, device=s.device)
    tpr, fpr = torch.cat([zero, tps]) / tps[-1], torch.cat([zero, fps]) / fps[-1]
    auroc = torch.trapezoid(tpr, fpr)
    auprc = ((tpr[1:] - tpr[:-1]) * (tps / (tps + fps))).sum()
    return torch.stack([tp.sum() / n, kappa, macro(2 * tp, 2 * tp + fp + fn),
                        macro(tp, tp + fp), macro(tp, tp + fn), (tp_ + tn_) / n,
                        2 * tp_ / (2 * tp_ + fp_ + fn_), tp_ / (tp_ + fp_), tp_ / (tp_ + fn_),
                        auroc, auprc])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(N, C, generator=g) * 2).to(dev)
    y = torch.randint(0, C, (N,), generator=g).to(dev)
    zb, yb = z[:B].contiguous(), y[:B].contiguous()

    ev = GradingMetrics(C, False, "CE", capacity=B * (a.iters + a.warmup + 1))
    t_update = timed(lambda: ev.update(zb, yb), a.iters, a.warmup)
    ev = GradingMetrics(C, False, "CE")  # the default capacity, N rows stored
    for lo in range(0, N, B):
        ev.update(z[lo:lo + B], y[lo:lo + B])
    t_compute = timed(ev._launch_compute, a.iters, a.warmup)
    ours = ev.compute()

    def fresh():
        return {"conf": torch.zeros(C * C, dtype=torch.int64, device=dev),
                "ref": torch.zeros(4, dtype=torch.int64, device=dev),
                "loss": torch.zeros((), device=dev), "scores": [], "positive": []}

    st = fresh()
    t_update_torch = timed(lambda: torch_update(st, zb, yb), a.iters, a.warmup)
    st = fresh()
    for lo in range(0, N, B):
        torch_update(st, z[lo:lo + B], y[lo:lo + B])
    conf, scores = st["conf"].view(C, C), torch.cat(st["scores"])
    positive = torch.cat(st["positive"])
    t_compute_torch = timed(lambda: torch_compute(conf, st["ref"], scores, positive), a.iters,
                            a.warmup)
    theirs = torch_compute(conf, st["ref"], scores, positive).tolist()
    names = ("micro_acc", "kappa", "macro_f1", "macro_precision", "macro_recall", "acc", "f1",
             "precision", "recall", "auroc", "auprc")
    diff = max(abs(ours[k] - v) for k, v in zip(names, theirs))
    pairs = float(N) * N
    print(json.dumps({
        "update_us": round(t_update, 2), "update_torch_us": round(t_update_torch, 2),
        "compute_us": round(t_compute, 2), "compute_torch_us": round(t_compute_torch, 2),
        "B": B, "C": C, "N": N, "iters": a.iters, "rank_pairs": pairs,
        "pairs_per_us": round(pairs / t_compute, 1), "max_abs_diff_vs_torch": diff}))


if __name__ == "__main__":
    main()
