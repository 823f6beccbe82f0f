"""The collate of tests/test_gpu_loader.py restated in plain CPU torch, and its cases.

`collate_ref` is PyG's Collater / Batch.from_data_list for x, pos, y, batch and ptr: `torch.cat`
of the selected graphs' row slices, `repeat_interleave` for batch, `cumsum` for ptr. Copies are
exact, so every comparison against it is `torch.equal`.
"""
from __future__ import annotations

import torch

# graph sizes of the stores: one graph, two, and 37 with the sizes around the 64-row tile, the
# smallest graphs and one of the largest the workload has (512)
_EDGE_SIZES = [1, 2, 63, 64, 65, 512]
STORE_SIZES = {
    1: [65],
    2: [1, 64],
    37: _EDGE_SIZES + [3 + (7 * i) % 23 for i in range(37 - len(_EDGE_SIZES))],
}
CHANNELS = [1, 3, 4, 128, 1025]   # 1, 3 and 1025: graph starts at every 4-byte offset mod 16
DIMS = [2, 3, 0]                  # 0: a store without pos


def make_store_tensors(num_graphs: int, channels: int, dims: int, seed: int = 0):
    """(x, pos or None, y, ptr) on the host for STORE_SIZES[num_graphs]."""
    gen = torch.Generator().manual_seed(seed + 1000 * num_graphs + channels)
    sizes = torch.tensor(STORE_SIZES[num_graphs], dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    rows = int(ptr[-1])
    x = torch.randn(rows, channels, generator=gen, dtype=torch.float32)
    pos = torch.rand(rows, dims, generator=gen, dtype=torch.float64) if dims else None
    y = torch.randint(0, 5, (num_graphs,), generator=gen)
    return x, pos, y, ptr


def id_cases(num_graphs: int) -> dict[str, list[int]]:
    """The selections every store is collated with."""
    G = num_graphs
    perm = torch.randperm(G, generator=torch.Generator().manual_seed(G)).tolist()
    return {
        "identity": list(range(G)),
        "reversed": list(range(G - 1, -1, -1)),
        "shuffled_subset": perm[:max(1, (2 * G) // 3)],
        "repeats": [perm[0], perm[-1], perm[0], perm[G // 2], perm[0]],
        "single": [perm[G // 2]],
        "empty": [],
    }


def collate_ref(x, pos, y, ptr, ids):
    """(x, pos or None, y, batch, ptr) of the graphs `ids`, all host tensors."""
    ids = [int(i) for i in ids]
    sizes = torch.tensor([int(ptr[i + 1] - ptr[i]) for i in ids], dtype=torch.int64)
    rows = [slice(int(ptr[i]), int(ptr[i + 1])) for i in ids]
    out_x = torch.cat([x[r] for r in rows]) if ids else x[:0]
    out_pos = None
    if pos is not None:
        out_pos = torch.cat([pos[r] for r in rows]) if ids else pos[:0]
    out_y = y[torch.tensor(ids, dtype=torch.int64)]
    batch = torch.repeat_interleave(torch.arange(len(ids)), sizes)
    out_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    return out_x, out_pos, out_y, batch, out_ptr
