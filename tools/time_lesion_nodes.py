"""Time of the lesion-node chain on the HIP path (csrc/ccl.hip + lgnn_cc_pool): HIP-event
milliseconds per call of `label_pool`, `ccl`, `ccl_stats` and the whole
`LesionsExtractor.nodes_from_maps`, at the reference's size (a 512 x 512 map, 1024 feature
channels), for a map of blobs and, labelling only, for noise at p = 0.41 (near the 8-connected
percolation point: the most tangled components). Nothing here ran on the GPU before, so there is
nothing to compare against: the figures are recorded in DESIGN §4.5, not asserted.

Each figure is the mean over `--iters` calls between two events after `--warmup` calls.
nodes_from_maps reads the component count on the host once per call (it sizes the outputs).

    python tools/time_lesion_nodes.py [--size 512] [--channels 1024] [--blobs 300] [--iters 2000]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lesion_gnn_amd import ops  # noqa: E402
from lesion_gnn_amd.datasets.nodes import lesions  # noqa: E402


def blob_classes(size: int, n: int, gen: torch.Generator) -> torch.Tensor:
    cls = torch.zeros(size, size, dtype=torch.int64)
    for _ in range(n):
        h, w = (int(v) for v in torch.randint(1, max(2, size // 16), (2,), generator=gen))
        y0 = int(torch.randint(0, size - h + 1, (1,), generator=gen))
        x0 = int(torch.randint(0, size - w + 1, (1,), generator=gen))
        cls[y0:y0 + h, x0:x0 + w] = int(torch.randint(1, 5, (1,), generator=gen))
    return cls


def event_ms(fn, warmup: int, iters: int) -> float:
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / iters, 4)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--blobs", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=2000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    S = a.size
    # the segmentation output at twice the feature resolution
    cls = blob_classes(2 * S, a.blobs, gen)
    logits = (torch.rand(1, 5, 2 * S, 2 * S, generator=gen)
              + 8.0 * torch.nn.functional.one_hot(cls, 5).permute(2, 0, 1)[None]).to(dev)
    feats = torch.randn(1, a.channels, S, S, device=dev)
    noise = (torch.rand(S, S, generator=gen) < 0.41).to(torch.uint8).to(dev)

    blobs = ops.label_pool(logits[0], (S, S))
    cc, num = ops.ccl(blobs)
    nlabel = int(num)
    ex = lesions.LesionsExtractor(lesions.LesionsNodesConfig(
        feature_source=lesions.SegmentationEncoderFeatures(layer=4)))
    out = {
        "box": torch.cuda.get_device_name(0), "size": S, "channels": a.channels,
        "iters": a.iters, "nlabel_blobs": nlabel, "nlabel_noise": int(ops.ccl(noise)[1]),
        "label_pool_ms": event_ms(lambda: ops.label_pool(logits[0], (S, S)), a.warmup, a.iters),
        "ccl_blobs_ms": event_ms(lambda: ops.ccl(blobs), a.warmup, a.iters),
        "ccl_noise_ms": event_ms(lambda: ops.ccl(noise), a.warmup, a.iters),
        "ccl_stats_ms": event_ms(lambda: ops.ccl_stats(cc, nlabel, validate=False), a.warmup,
                                 a.iters),
        "nodes_from_maps_ms": event_ms(lambda: ex.nodes_from_maps(logits, feats, 0), 5,
                                       max(1, a.iters // 10)),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
