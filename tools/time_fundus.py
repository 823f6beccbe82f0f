"""Time of the fundus preprocessing (`FundusPreprocess`, csrc/fundus.hip) on a batch of
photograph-sized images: 8 seeded synthetic 2848 x 4288 uint8 RGB images (a bright noisy disc on
a dark noisy border, centre and radius varying per image), to S = 512 and S = 1536.

HIP-event milliseconds (mean over `--iters` calls after `--warmup`) of each of the two entries
(`ops.fundus_bbox`, `ops.fundus_preprocess`) and of the whole call, eager (`*_ms`: the host's
marshalling and enqueueing run ahead of the device) and as replays of a captured HIP graph
(`*_graph_ms`: the launches alone, no host work between them). The box pass reads every byte of every
image once: `bbox_gbs` is those bytes over its replay time, `bbox_hbm_fraction` that rate over
the 8.0 TB/s HBM peak DESIGN §4 uses (a float4 copy reaches 6.3 TB/s). Two sets of images
alternate from call to call, so that a call's 293 MB were not left in the 256 MiB Infinity Cache
by the call before it. `torch_ms` is the same work composed from torch ops on the same GPU, image
by image: mask, `any`, index min / max with their host reads, crop, `F.interpolate(bilinear,
align_corners=False)`, pad, normalise (float arithmetic: close to, not bitwise, the integer
resize). Figures are recorded in DESIGN §4.15, not asserted; run it twice for the spread between
processes.

    python tools/time_fundus.py [--batch 8] [--height 2848] [--width 4288] [--iters 50]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lesion_gnn_amd import ops  # noqa: E402
from lesion_gnn_amd.datasets.fundus import IMAGENET_DEFAULT_MEAN  # noqa: E402
from lesion_gnn_amd.datasets.fundus import IMAGENET_DEFAULT_STD, FundusPreprocess  # noqa: E402
from tools.time_lesion_nodes import event_ms  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
HBM_COPY = 6.3e12  # what a float4 copy reaches


def photographs(batch: int, H: int, W: int, seed: int, dev) -> list[torch.Tensor]:
    """`batch` (H, W, 3) uint8 images: a disc of 60..255 on a border of 0..20."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    host = torch.Generator().manual_seed(seed)
    ys = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xs = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    out = []
    for _ in range(batch):
        cy, cx, rad = (torch.rand(3, generator=host) * 0.06 + torch.tensor([0.47, 0.47, 0.42])) \
            * torch.tensor([H, W, H])
        disc = ((ys - cy) ** 2 + (xs - cx) ** 2 <= rad ** 2)[:, :, None]
        bright = torch.randint(60, 256, (H, W, 3), generator=gen, device=dev, dtype=torch.uint8)
        border = torch.randint(0, 21, (H, W, 3), generator=gen, device=dev, dtype=torch.uint8)
        out.append(torch.where(disc, bright, border))
    return out


def torch_boxes(images, threshold: float) -> list[tuple[int, int, int, int]]:
    boxes = []
    for img in images:
        H, W = img.shape[:2]
        mask = img[:, :, 0] > threshold
        if not bool(mask.any()):
            boxes.append((0, W, 0, H))
            continue
        cols = mask.any(0).nonzero()
        rows = mask.any(1).nonzero()
        x0, x1, y0, y1 = int(cols.min()), int(cols.max()), int(rows.min()), int(rows.max())
        boxes.append((0, W, 0, H) if x0 == x1 or y0 == y1 else (x0, x1, y0, y1))
    return boxes


def torch_chain(images, S: int, threshold: float, mean: torch.Tensor, std: torch.Tensor):
    out = []
    for img, (x0, x1, y0, y1) in zip(images, torch_boxes(images, threshold)):
        crop = img[y0:y1, x0:x1].permute(2, 0, 1)[None].float()
        h, w = crop.shape[2:]
        scale = S / float(max(h, w))
        nh, nw = max(1, round(h * scale)), max(1, round(w * scale))
        small = torch.nn.functional.interpolate(crop, size=(nh, nw), mode="bilinear",
                                                align_corners=False)
        top, left = (S - nh) // 2, (S - nw) // 2
        small = torch.nn.functional.pad(small, (left, S - nw - left, top, S - nh - top))
        out.append((small - mean) / std)
    return torch.cat(out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=2848)
    ap.add_argument("--width", type=int, default=4288)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1536])
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    sets = [photographs(B, H, W, seed, dev) for seed in (0, 1)]
    turn = [0]

    def images():
        turn[0] ^= 1
        return sets[turn[0]]

    def replays(fn):
        """fn(k) on set k captured once per set; the returned call replays the sets in turn."""
        graphs = []
        side = torch.cuda.Stream()
        for k in range(len(sets)):
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn(k)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep = fn(k)
            graphs.append((g, keep))

        def replay():
            turn[0] ^= 1
            graphs[turn[0]][0].replay()

        return replay

    thr = 25.0
    mean = torch.tensor(IMAGENET_DEFAULT_MEAN, device=dev).view(1, 3, 1, 1) * 255.0
    std = torch.tensor(IMAGENET_DEFAULT_STD, device=dev).view(1, 3, 1, 1) * 255.0
    boxes = [ops.fundus_bbox(s, thr) for s in sets]
    for s, b in zip(sets, boxes):  # the box pass against torch's index min / max
        assert b.cpu().tolist() == [list(t) for t in torch_boxes(s, thr)]
    image_bytes = B * H * W * 3
    bbox_ms = event_ms(lambda: ops.fundus_bbox(images(), thr), a.warmup, a.iters)
    bbox_graph_ms = event_ms(replays(lambda k: ops.fundus_bbox(sets[k], thr)), a.warmup, a.iters)
    rate = image_bytes / (bbox_graph_ms * 1e-3)
    out = {
        "box": torch.cuda.get_device_name(0), "batch": B, "height": H, "width": W,
        "iters": a.iters, "image_mb": round(image_bytes / 1e6, 1), "bbox_ms": bbox_ms,
        "bbox_graph_ms": bbox_graph_ms,
        "bbox_gbs": round(rate / 1e9, 1), "bbox_hbm_fraction": round(rate / HBM_PEAK, 4),
        "bbox_copy_fraction": round(rate / HBM_COPY, 4),
    }
    for S in a.sizes:
        fp = FundusPreprocess(S, threshold=thr)

        def resize():
            return ops.fundus_preprocess(sets[turn[0]], boxes[turn[0]], S,
                                         IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)

        got = fp(sets[0]).image
        want = torch_chain(sets[0], S, thr, mean, std)
        r = {
            "preprocess_ms": event_ms(lambda: (images(), resize()), a.warmup, a.iters),
            "preprocess_graph_ms": event_ms(replays(lambda k: ops.fundus_preprocess(
                sets[k], boxes[k], S, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)),
                a.warmup, a.iters),
            "call_ms": event_ms(lambda: fp(images()), a.warmup, a.iters),
            "call_graph_ms": event_ms(replays(lambda k: fp(sets[k])), a.warmup, a.iters),
            "torch_ms": event_ms(lambda: torch_chain(images(), S, thr, mean, std), 2,
                                 max(2, a.iters // 5)),
            "written_mb": round(B * S * S * 12 / 1e6, 1),
            "max_abs_diff_to_torch": round((got - want).abs().max().item(), 4),
        }
        r["torch_over_call"] = round(r["torch_ms"] / r["call_ms"], 1)
        out[f"s{S}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
