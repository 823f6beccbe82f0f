"""Forward + backward time of SetTransformerAggregation on the HIP path against the padded
torch.nn.MultiheadAttention build (tests/set_transformer_ref.py PaddedAggregation, moved to the
same GPU): what a user would run without the HIP path. Recorded in DESIGN §4.8, not asserted.

Each side's step is captured in a HIP graph after warm-up and replayed for `--seconds` (past the
clock ramp); the figure is the mean replay time.

    python tools/time_set_attention.py [--sets 1024] [--rows 64] [--seconds 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lesion_gnn_amd import synth  # noqa: E402
from lesion_gnn_amd.conv import SetTransformerAggregation  # noqa: E402
from tests import set_transformer_ref as ref  # noqa: E402


def timed(step, seconds: float) -> float:
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            step()
        run = g.replay
    except RuntimeError as e:  # a step that cannot be captured is timed as eager launches
        print(f"not captured ({str(e).splitlines()[0]}): eager timing", file=sys.stderr)
        torch.cuda.synchronize()
        run = step
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        n += 10
    return (time.perf_counter() - t0) / n * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(channels=128, num_seed_points=64, num_encoder_blocks=2, num_decoder_blocks=2,
              heads=2, layer_norm=True, concat=False)
    torch.manual_seed(0)
    ours = SetTransformerAggregation(**kw).to(dev)
    theirs = ref.PaddedAggregation(**kw)
    theirs.load_state_dict(ours.state_dict())
    theirs = theirs.to(dev)
    # to_dense_batch of the padded build indexes with host-made positions: made once, outside
    total = a.sets * a.rows
    gen = torch.Generator().manual_seed(1)
    layouts = {"fixed": [a.rows] * a.sets}
    ln = synth.graph_sizes(a.sets, "lognormal", gen)
    scale = total / sum(ln)
    layouts["lognormal"] = [max(1, round(s * scale)) for s in ln]
    result = {"box": torch.cuda.get_device_name(0), "sets": a.sets, "channels": 128}
    for name, sizes in layouts.items():
        M, B = sum(sizes), len(sizes)
        x = torch.randn(M, 128, device=dev, requires_grad=True)
        batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).to(dev)
        w = torch.randn(B, 128, device=dev)
        nmax = max(sizes)
        pos = (torch.arange(M) - torch.repeat_interleave(
            torch.tensor([0] + sizes[:-1]).cumsum(0), torch.tensor(sizes))).to(dev)
        mask = torch.zeros(B, nmax, dtype=torch.bool, device=dev)
        mask[batch, pos] = True

        def hip_step():
            ours.zero_grad(set_to_none=True)
            x.grad = None
            ours(x, batch, dim_size=B).backward(w)

        def padded_step():
            theirs.zero_grad(set_to_none=True)
            x.grad = None
            h = x.new_zeros(B, nmax, 128).index_put((batch, pos), x)
            for e in theirs.encoders:
                h = e(h, mask)
            h = theirs.pma(h, mask)
            for d in theirs.decoders:
                h = d(h)
            h.mean(dim=1).backward(w)

        result[name] = {"rows": M, "max_rows": nmax,
                        "hip_ms": round(timed(hip_step, a.seconds), 4),
                        "padded_torch_ms": round(timed(padded_step, a.seconds), 4)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
