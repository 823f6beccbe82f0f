"""GPU k-NN graph construction (liblgnn lgnn_knn_graph via lesion_gnn_amd.knn) vs the CPU
restatement of torch_cluster.knn_graph: oracle.pyg_ref.knn_graph (per graph, pure Python) for
small cases, and synth.knn_edges (vectorised; pinned to the oracle by
tests/test_oracle.py::test_synth_knn_matches_oracle_bitexact) for batch-sized ones.

Bar: edge_index bit-exact (same neighbours, same order). Cases: k-regular C2 graphs, log-normal
(C3) and power-law (C5) sizes including graphs smaller than k, loop=False, exact duplicate
positions (distance ties broken by node index), 3-D positions, one graph larger than the LDS
candidate chunk, k = 1 and k = 32, and the KNNGraph transform on a collated batch. loop=False
follows torch_cluster (k + 1 neighbours, self dropped) except when k + 1 other nodes share a
node's exact position with lower indices (self not among the k + 1): not exercised.
"""
import pytest
import torch

import oracle.pyg_ref as ref
from lesion_gnn_amd import synth
from lesion_gnn_amd.knn import KNNGraph, knn_graph

pytestmark = pytest.mark.gpu


def oracle_batch(pos, sizes, k, loop):
    out, off = [], 0
    for n in sizes:
        out.append(ref.knn_graph(pos[off:off + n], k, loop=loop) + off)
        off += n
    return torch.cat(out, dim=1) if out else torch.empty(2, 0, dtype=torch.long)


def synth_batch(pos, sizes, k, loop):
    out, off = [], 0
    for n in sizes:
        out.append(synth.knn_edges(pos[off:off + n][None], k, loop)[0] + off)
        off += n
    return torch.cat(out, dim=1)


def run(pos, sizes, k, loop, cuda):
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    got = knn_graph(pos.to(cuda), k, batch.to(cuda), loop=loop, num_graphs=len(sizes))
    torch.cuda.synchronize()
    return got.cpu()


@pytest.mark.parametrize("k,loop", [(8, True), (6, True), (5, False), (1, True), (32, True)])
def test_knn_small_vs_oracle(cuda, k, loop):
    gen = torch.Generator().manual_seed(k)
    sizes = [1, 2, 5, 64, 33, 7, 40]
    pos = torch.rand(sum(sizes), 2, generator=gen, dtype=torch.float64)
    assert torch.equal(run(pos, sizes, k, loop, cuda), oracle_batch(pos, sizes, k, loop))


def test_knn_ties_and_3d_vs_oracle(cuda):
    gen = torch.Generator().manual_seed(1)
    sizes = [30, 20]
    pos = torch.rand(50, 3, generator=gen, dtype=torch.float64)
    pos[5] = pos[2]
    pos[7] = pos[2]
    pos[12] = pos[3]  # exact duplicates: distance ties, index order decides
    pos[40] = pos[33]
    pos2 = torch.round(torch.rand(50, 2, generator=gen, dtype=torch.float64) * 4) / 4  # a grid
    for p, k in ((pos, 6), (pos2, 9)):
        assert torch.equal(run(p, sizes, k, True, cuda), oracle_batch(p, sizes, k, True))


@pytest.mark.parametrize("dist,k", [("fixed", 8), ("lognormal", 6), ("powerlaw", 16),
                                    ("powerlaw", 4)])
def test_knn_batches_vs_restatement(cuda, dist, k):
    b = synth.make_batch(1024 if dist == "fixed" else 300, n=64, k=k, d_in=4, seed=21,
                         sizes=dist)
    sizes = (b.ptr[1:] - b.ptr[:-1]).tolist()
    got = run(b.pos, sizes, k, True, cuda)
    assert torch.equal(got, b.edge_index)  # make_batch's own k-NN (synth.knn_edges)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_knn_offsets_scan_lengths(cuda, B):
    """k_knn_offsets at the wave edge, the tile edge (1024 graphs) and with a carry over two
    tiles: graphs of 1 to 3 nodes, so k is clamped in every one and a single node has no edge."""
    gen = torch.Generator().manual_seed(B)
    sizes = torch.randint(1, 4, (B,), generator=gen).tolist()
    pos = torch.rand(sum(sizes), 2, generator=gen, dtype=torch.float64)
    assert torch.equal(run(pos, sizes, 2, False, cuda), oracle_batch(pos, sizes, 2, False))


def test_knn_large_graph_chunks(cuda):
    gen = torch.Generator().manual_seed(2)
    sizes = [3000, 5, 2500]
    pos = torch.rand(sum(sizes), 2, generator=gen, dtype=torch.float64)
    for k, loop in ((16, True), (3, False)):
        assert torch.equal(run(pos, sizes, k, loop, cuda), synth_batch(pos, sizes, k, loop))


def test_knn_transform_and_defaults(cuda):
    b = synth.make_batch(64, n=64, k=6, d_in=4, seed=22).to(cuda)
    want = b.edge_index.clone()
    b.edge_index = None
    out = KNNGraph(k=6, loop=True)(b)
    assert torch.equal(out.edge_index, want)
    # single graph, torch_cluster defaults (loop=False), target_to_source flips the rows
    pos = b.pos[:64]
    e = knn_graph(pos, 4)
    assert torch.equal(e.cpu(), ref.knn_graph(pos.cpu(), 4, loop=False))
    assert torch.equal(knn_graph(pos, 4, flow="target_to_source"), e.flip(0))
    with pytest.raises(NotImplementedError):
        KNNGraph(k=3, force_undirected=True)
    with pytest.raises(ValueError):
        knn_graph(pos, 33)
