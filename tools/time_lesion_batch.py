"""Time of building the store of a batch of images' lesion nodes, two ways, at the reference's
setting (`reinterpolation=(512, 512)`, configs/config.py; 1024 encoder channels at 16 x 16;
five-class 1024 x 1024 logits with 300 blobs per image; B = 16):

- batch: `LesionsExtractor.nodes_from_batch` + `LesionNodesBatch.to_store()`: the reinterpolation
  is evaluated inside the pooling (lgnn_cc_pool_resample), one host read per batch;
- loop: `nodes_from_maps` per image + `GraphStore.from_list`: F.interpolate writes a 1 x 1024 x
  512 x 512 map per image, lgnn_cc_pool reads it back, one host read per image.

HIP-event milliseconds per batch (mean over `--iters` builds after `--warmup`), and the peak of
torch's allocator over one build of each (`torch.cuda.max_memory_allocated` above what the inputs
hold), then the batch route's entries one by one. Figures are recorded in DESIGN §4.5, not
asserted; run it twice for the spread between processes.

    python tools/time_lesion_batch.py [--batch 16] [--size 512] [--channels 1024] [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lesion_gnn_amd import ops  # noqa: E402
from lesion_gnn_amd.datasets import GraphStore  # noqa: E402
from lesion_gnn_amd.datasets.nodes import lesions  # noqa: E402
from tools.time_lesion_nodes import blob_classes, event_ms  # noqa: E402


def peak_mb(fn) -> float:
    """Peak allocator bytes of one call above what is held before it, in MB."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - held) / 1e6, 1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--source", type=int, default=16)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--blobs", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    B, S = a.batch, a.size
    logits = torch.empty(B, 5, 2 * S, 2 * S, device=dev)
    for b in range(B):  # the segmentation output at twice the pooled resolution
        cls = blob_classes(2 * S, a.blobs, gen)
        logits[b] = (torch.rand(5, 2 * S, 2 * S, generator=gen)
                     + 8.0 * torch.nn.functional.one_hot(cls, 5).permute(2, 0, 1)).to(dev)
    feats = torch.randn(B, a.channels, a.source, a.source, device=dev)
    labels = list(range(B))
    ex = lesions.LesionsExtractor(lesions.LesionsNodesConfig(
        feature_source=lesions.SegmentationEncoderFeatures(layer=4), reinterpolation=(S, S)))

    def batch():
        return ex.nodes_from_batch(logits, feats, labels).to_store()

    def loop():
        return GraphStore.from_list(
            ex.nodes_from_maps(logits[b:b + 1], feats[b:b + 1], labels[b]) for b in range(B))

    new, old = batch(), loop()
    assert torch.equal(new.ptr_host, old.ptr_host) and torch.equal(new.pos, old.pos)
    # the batch route's launches one by one (no host read between them here)
    classes = ops.label_pool_batch(logits, (S, S))
    cc, _, ptr = ops.ccl_batch(classes)
    total = int(new.ptr_host[-1])
    nmax = int((new.ptr_host[1:] - new.ptr_host[:-1]).max())
    cls = classes.view(B, 1, S, S).float()
    parts = {
        "label_pool_batch_ms": lambda: ops.label_pool_batch(logits, (S, S)),
        "ccl_batch_ms": lambda: ops.ccl_batch(classes),
        "ccl_stats_batch_ms": lambda: ops.ccl_stats_batch(cc, ptr, total, validate=False),
        "pool_features_ms": lambda: ops.cc_pool_resample(feats, cc, ptr, total, False, nmax,
                                                         validate=False),
        "pool_classes_ms": lambda: ops.cc_pool_resample(cls, cc, ptr, total, False, nmax,
                                                        validate=False),
    }
    out = {
        "box": torch.cuda.get_device_name(0), "batch": B, "size": S, "source": a.source,
        "channels": a.channels, "iters": a.iters, "nodes": int(new.ptr_host[-1]),
        "max_abs_diff_x": float((new.x - old.x).abs().max()),
        "batch_ms": event_ms(batch, a.warmup, a.iters),
        "loop_ms": event_ms(loop, a.warmup, a.iters),
        "batch_peak_mb": peak_mb(batch), "loop_peak_mb": peak_mb(loop),
        **{k: event_ms(fn, a.warmup, a.iters) for k, fn in parts.items()},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
