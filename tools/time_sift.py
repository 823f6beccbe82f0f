"""Time of the SIFT nodes of a batch of images (`SiftExtractor.nodes_from_batch`) against one
`nodes_from_image` call per image, and of the batch route's stages one by one: 8 seeded 512 x 512
textures (filtered noise at two scales), `num_keypoints = 512`, sigma 1.6.

HIP-event milliseconds (mean over `--iters` runs after `--warmup`). The scale space is the
bandwidth-bound stage: `pyramid_gbs` is the bytes it must move at least (every Gaussian level
written once and read once by the next blur, every DoG level written once, the gray image
written and read) over its time, `pyramid_hbm_fraction` that rate over the 8.0 TB/s HBM peak
DESIGN §4 uses. The keypoint and descriptor stages are float64 per-keypoint work, not bandwidth.
Figures are recorded in DESIGN §4.11, not asserted; run it twice for the spread between
processes.

    python tools/time_sift.py [--batch 8] [--size 512] [--keypoints 512] [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lesion_gnn_amd import ops  # noqa: E402
from lesion_gnn_amd.datasets.nodes.sift import SiftExtractor  # noqa: E402
from tools.time_lesion_nodes import event_ms  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def textures(batch: int, size: int, dev) -> torch.Tensor:
    """(batch, size, size, 3) uint8: noise smoothed at two scales, scaled to 0..255."""
    gen = torch.Generator().manual_seed(0)

    def smooth(t, s):
        r = int(3 * s)
        x = torch.arange(-r, r + 1, dtype=torch.float32)
        w = torch.exp(-x * x / (2 * s * s))
        w = (w / w.sum()).view(1, 1, -1)
        t = torch.nn.functional.pad(t, (r, r, r, r), mode="reflect")
        n, c = t.shape[:2]
        t = torch.nn.functional.conv2d(t.reshape(n * c, 1, *t.shape[2:]), w.unsqueeze(2))
        t = torch.nn.functional.conv2d(t, w.unsqueeze(3))
        return t.reshape(n, c, size, size)

    noise = torch.randn(2, batch, 3, size, size, generator=gen)
    t = smooth(noise[0], 1.2) + 3.0 * smooth(noise[1], 2.5)
    lo = t.amin((2, 3), keepdim=True)
    hi = t.amax((2, 3), keepdim=True)
    return ((t - lo) / (hi - lo) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1) \
        .contiguous().to(dev)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--keypoints", type=int, default=512)
    ap.add_argument("--sigma", type=float, default=1.6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    imgs = textures(B, S, dev)
    labels = list(range(B))
    ex = SiftExtractor(a.keypoints, a.sigma)

    def batch():
        return ex.nodes_from_batch(imgs, labels)

    def loop():
        return [ex.nodes_from_image(imgs[b], labels[b]) for b in range(B)]

    new, old = batch(), loop()
    assert torch.equal(new.x, torch.cat([o.x for o in old]))
    assert torch.equal(new.pos, torch.cat([o.pos for o in old]))
    pyr = ops.sift_pyramid(imgs, a.sigma)
    cand = ops.sift_candidates(pyr)
    kf, ki, _, ptr_host = ops.sift_keypoints(pyr, cand, a.sigma, a.keypoints)
    parts = {
        "pyramid_ms": lambda: ops.sift_pyramid(imgs, a.sigma),
        "candidates_ms": lambda: ops.sift_candidates(pyr),     # one host read inside
        "keypoints_ms": lambda: ops.sift_keypoints(pyr, cand, a.sigma, a.keypoints),  # likewise
        "descriptors_ms": lambda: ops.sift_descriptors(pyr, kf, ki),
    }
    times = {k: event_ms(fn, a.warmup, a.iters) for k, fn in parts.items()}
    gauss, dog = pyr.gauss_flat.numel() * 4, pyr.dog_flat.numel() * 4
    # five of six levels are read again by the next blur, level 3 also by the next octave's
    # sampling (a quarter of it); the doubled base is formed from the gray image in LDS
    pyramid_bytes = gauss + gauss * 5 // 6 + dog + 2 * B * S * S + imgs.numel()
    rate = pyramid_bytes / (times["pyramid_ms"] * 1e-3)
    out = {
        "box": torch.cuda.get_device_name(0), "batch": B, "size": S, "keypoints": a.keypoints,
        "sigma": a.sigma, "iters": a.iters, "octaves": len(pyr.gauss),
        "candidates": int(cand.size(0)), "nodes": int(ptr_host[-1]),
        "batch_ms": event_ms(batch, a.warmup, a.iters),
        "loop_ms": event_ms(loop, a.warmup, a.iters),
        **times,
        "pyramid_mb": round(pyramid_bytes / 1e6, 1), "pyramid_gbs": round(rate / 1e9, 1),
        "pyramid_hbm_fraction": round(rate / HBM_PEAK, 4),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
