"""GPU: a GraphStore that keeps each graph's edges (GraphStore.with_edges) and their collation
(ops.collate -> lgnn_collate_edges) against the torch composition tests/fit_ref.collate_edges_ref.
Copies and integer offsets only: every comparison is exact.

The store has 12 graphs of 1, 1, 2, 3, 7, 64, 65, 130, 300, 5, 4 and 1 nodes with KNNGraph(k=6)
edges, with and without self loops (a one-node graph then has 1 or 0 edges); graph 10 has nodes
and no edge. 300 nodes x 6 = 1800 edges span two of the gather's 1024-edge workgroups."""
import pytest
import torch

from lesion_gnn_amd import _lib, ops
from lesion_gnn_amd.datasets import ConcatGraphs, GraphStore
from tests import fit_ref as fr
from tests.loader_ref import collate_ref

pytestmark = pytest.mark.gpu

SIZES = [1, 1, 2, 3, 7, 64, 65, 130, 300, 5, 4, 1]
NO_EDGES = 10
G = len(SIZES)
ID_CASES = {
    "in_order": list(range(G)),
    "reversed": list(range(G - 1, -1, -1)),
    "repeats": [8, 0, 8, 10, 5, 8, 11, 11],
    "single": [7],
    "none_with_edges": [NO_EDGES, NO_EDGES],
    "empty": [],
}
WEIGHTS = {"f32": torch.float32, "f64": torch.float64, "none": None}


def host_store(loop: bool, wdtype, seed: int = 0):
    """(x, pos, y, ptr, edge_index, edge_weight or None, edge_ptr) on the host."""
    gen = torch.Generator().manual_seed(seed)
    ptr = torch.tensor([0] + SIZES, dtype=torch.int64).cumsum(0)
    rows = int(ptr[-1])
    x = torch.randn(rows, 3, generator=gen)
    pos = torch.rand(rows, 2, generator=gen, dtype=torch.float64)
    y = torch.arange(G) % 5
    ei, eptr = fr.store_edges(pos, ptr, 6, loop)
    keep = torch.ones(ei.size(1), dtype=torch.bool)
    keep[int(eptr[NO_EDGES]):int(eptr[NO_EDGES + 1])] = False
    counts = eptr[1:] - eptr[:-1]
    counts[NO_EDGES] = 0
    ei = ei[:, keep].contiguous()
    eptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    w = None if wdtype is None else torch.randn(ei.size(1), generator=gen, dtype=wdtype)
    return x, pos, y, ptr, ei, w, eptr


def device_store(h, cuda) -> GraphStore:
    x, pos, y, ptr, ei, w, _ = h
    return GraphStore(x.to(cuda), pos.to(cuda), y, ptr).with_edges(
        ei.to(cuda), None if w is None else w.to(cuda))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def assert_edges(batch, h, ids):
    x, pos, y, ptr, ei, w, eptr = h
    want_ei, want_w, want_eptr = fr.collate_edges_ref(ei, w, eptr, ptr, ids)
    assert batch.edge_index.dtype == torch.int64 and batch.edge_index.is_contiguous()
    assert batch.edge_index.shape == want_ei.shape
    assert torch.equal(batch.edge_index.cpu(), want_ei)
    assert torch.equal(batch.edge_ptr.cpu(), want_eptr)
    if w is None:
        assert not hasattr(batch, "edge_weight")
    else:
        assert batch.edge_weight.dtype == w.dtype
        assert torch.equal(bits(batch.edge_weight), bits(want_w))
    # the rows are the collate's, as before
    want = collate_ref(x, pos, y, ptr, ids)
    assert torch.equal(batch.x.cpu(), want[0]) and torch.equal(batch.ptr.cpu(), want[4])
    n = batch.x.size(0)
    assert want_ei.numel() == 0 or (0 <= int(batch.edge_index.min())
                                    and int(batch.edge_index.max()) < n)


@pytest.mark.parametrize("loop", [True, False])
@pytest.mark.parametrize("weights", list(WEIGHTS))
def test_collate_with_edges(cuda, loop, weights):
    h = host_store(loop, WEIGHTS[weights])
    store = device_store(h, cuda)
    assert torch.equal(store.edge_ptr_host, h[6]) and torch.equal(store.edge_ptr.cpu(), h[6])
    assert torch.equal(store.edge_index.cpu(), h[4])
    ones = [0, 1, 11]  # one-node graphs: one edge each with self loops, none without
    assert [int(h[6][g + 1] - h[6][g]) for g in ones] == [1 if loop else 0] * 3
    for name, ids in ID_CASES.items():
        batch = ops.collate(store, ids, validate=True)
        assert batch.num_graphs == len(ids), name
        assert_edges(batch, h, ids)
    if not loop:
        batch = ops.collate(store, ones, validate=True)
        assert batch.edge_index.shape == (2, 0) and batch.edge_ptr.tolist() == [0, 0, 0, 0]


class Call:
    """Output buffers with a canary behind `capacity` edges, and one lgnn_collate_edges call."""

    CANARY = -7

    def __init__(self, store, h, ids, capacity, cuda):
        ptr = h[3]
        ok = [i for i in ids if 0 <= i < G]
        sizes = [int(ptr[i + 1] - ptr[i]) if 0 <= i < G else 0 for i in ids]
        self.out_ptr = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0).to(cuda)
        self.ok, B = ok, len(ids)
        self.capacity = capacity
        self.ei = torch.full((2 * capacity + 16,), self.CANARY, dtype=torch.int64, device=cuda)
        w = store.edge_weight
        self.w = None if w is None else torch.full((capacity + 16,), float(self.CANARY),
                                                   dtype=w.dtype, device=cuda)
        self.eptr = torch.full((B + 1,), self.CANARY, dtype=torch.int64, device=cuda)
        self.err = torch.full((1,), self.CANARY, dtype=torch.int32, device=cuda)
        nws = _lib.load().lgnn_collate_edges_workspace_bytes(B)
        ws = torch.empty(nws, dtype=torch.uint8, device=cuda)
        ids_dev = torch.tensor(ids, dtype=torch.int64, device=cuda)
        _lib.call("lgnn_collate_edges", ids_dev if B else None, B, store.ptr, store.edge_ptr, G,
                  store.edge_index, store.edge_index.size(1), w,
                  0 if w is None else w.element_size(), self.out_ptr, self.ei, self.w, self.eptr,
                  capacity, self.err, ws, nws, _lib.stream(cuda))
        torch.cuda.synchronize()


@pytest.mark.parametrize("weights", ["f32", "none"])
def test_capacity_below_the_total(cuda, weights):
    h = host_store(True, WEIGHTS[weights])
    store = device_store(h, cuda)
    ids = [8, 4, 7]  # 1800 + 42 + 780 edges
    want_ei, want_w, want_eptr = fr.collate_edges_ref(h[4], h[5], h[6], h[3], ids)
    total = int(want_eptr[-1])
    for cap in (total - 1, 1500, 1024, 1):
        c = Call(store, h, ids, cap, cuda)
        assert int(c.err.item()) == _lib.LGNN_COLLATE_OVERFLOW
        assert torch.equal(c.eptr.cpu(), want_eptr)  # complete all the same
        ei = c.ei.cpu()
        assert torch.equal(ei[:cap], want_ei[0, :cap])
        assert torch.equal(ei[cap:2 * cap], want_ei[1, :cap])
        assert bool((ei[2 * cap:] == Call.CANARY).all())
        if c.w is not None:
            assert torch.equal(bits(c.w[:cap]), bits(want_w[:cap]))
            assert bool((c.w[cap:].cpu() == float(Call.CANARY)).all())
    # the exact capacity and a larger one: no flag, nothing beyond the total
    for cap in (total, total + 5):
        c = Call(store, h, ids, cap, cuda)
        assert int(c.err.item()) == 0
        ei = c.ei.cpu()
        assert torch.equal(ei[:total], want_ei[0]) and torch.equal(ei[cap:cap + total], want_ei[1])
        assert bool((ei[total:cap] == Call.CANARY).all())
        assert bool((ei[cap + total:] == Call.CANARY).all())


def test_ids_out_of_range_count_as_graphs_without_edges(cuda):
    h = host_store(True, torch.float32)
    store = device_store(h, cuda)
    ids = [5, G, 2, -1, 9, 1 << 40]
    want_ei, want_w, _ = fr.collate_edges_ref(h[4], h[5], h[6], h[3], [5, 2, 9])
    m = [int(h[6][i + 1] - h[6][i]) if 0 <= i < G else 0 for i in ids]
    total = sum(m)
    c = Call(store, h, ids, total, cuda)
    assert int(c.err.item()) == 3
    assert c.eptr.tolist() == torch.tensor([0] + m).cumsum(0).tolist()
    ei = c.ei.cpu()
    assert torch.equal(ei[:total], want_ei[0]) and torch.equal(ei[total:2 * total], want_ei[1])
    assert torch.equal(bits(c.w[:total]), bits(want_w))
    assert bool((ei[2 * total:] == Call.CANARY).all())
    # no selection at all: out_edge_ptr[0] and err are written, nothing else
    c = Call(store, h, [], 4, cuda)
    assert c.eptr.tolist() == [0] and int(c.err.item()) == 0
    assert bool((c.ei == Call.CANARY).all())
    with pytest.raises(IndexError):  # through ops.collate the ids are checked on the host
        ops.collate(store, [0, G])


def test_with_edges_checks_and_groups(cuda):
    h = host_store(True, torch.float64)
    x, pos, y, ptr, ei, w, eptr = h
    plain = GraphStore(x.to(cuda), pos.to(cuda), y, ptr)
    assert plain.edge_index is None and plain.edge_ptr is None and plain.edge_ptr_host is None
    rows = int(ptr[-1])
    crossing = ei.clone()
    crossing[0, 5] = int(ptr[6])      # a source in graph 6 for a target in graph 2
    crossing[0, 100] = int(ptr[2])
    with pytest.raises(ValueError, match="2 edge"):
        plain.with_edges(crossing.to(cuda))
    outside = ei.clone()
    outside[1, 7], outside[0, 8], outside[0, 9] = rows, -1, rows + 5
    with pytest.raises(ValueError, match="3 endpoint"):
        plain.with_edges(outside.to(cuda))
    with pytest.raises(ValueError):
        plain.with_edges(ei.to(cuda).to(torch.int32))
    with pytest.raises(ValueError):
        plain.with_edges(ei.to(cuda), w[:-1].to(cuda))
    # ungrouped: the graphs' blocks in reverse graph order, each block's own order kept; the
    # stable sort by graph gives the grouped input back
    graph = torch.bucketize(ei[1], ptr[1:], right=True)
    order = torch.sort(-graph, stable=True).indices
    assert not torch.equal(order, torch.arange(order.numel()))
    grouped = plain.with_edges(ei.to(cuda), w.to(cuda))
    regrouped = plain.with_edges(ei[:, order].to(cuda), w[order].to(cuda))
    assert torch.equal(regrouped.edge_index, grouped.edge_index)
    assert torch.equal(bits(regrouped.edge_weight), bits(grouped.edge_weight))
    assert torch.equal(regrouped.edge_ptr_host, eptr)
    assert regrouped.x.data_ptr() == plain.x.data_ptr()  # shared, not copied
    assert regrouped.pos.data_ptr() == plain.pos.data_ptr() and regrouped.ptr is plain.ptr
    assert_edges(ops.collate(regrouped, [8, 3, 0], validate=True), h, [8, 3, 0])


def test_save_and_load_carry_the_edges(cuda, tmp_path):
    h = host_store(False, torch.float32)
    store = device_store(h, cuda)
    store.save(tmp_path / "s.pt")
    back = GraphStore.load(tmp_path / "s.pt", cuda)
    assert torch.equal(back.edge_index, store.edge_index)
    assert torch.equal(bits(back.edge_weight), bits(store.edge_weight))
    assert torch.equal(back.edge_ptr_host, store.edge_ptr_host)
    plain = GraphStore(h[0].to(cuda), h[1].to(cuda), h[2], h[3])
    plain.save(tmp_path / "p.pt")
    assert GraphStore.load(tmp_path / "p.pt", cuda).edge_index is None


def test_concat_graphs_with_edges(cuda):
    a, b = host_store(True, torch.float32, seed=1), host_store(False, torch.float32, seed=2)
    both = ConcatGraphs([device_store(a, cuda), device_store(b, cuda)])
    rows_a, edges_a = int(a[3][-1]), int(a[6][-1])
    h = (torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]), torch.cat([a[2], b[2]]),
         torch.cat([a[3], b[3][1:] + rows_a]), torch.cat([a[4], b[4] + rows_a], dim=1),
         torch.cat([a[5], b[5]]), torch.cat([a[6], b[6][1:] + edges_a]))
    assert torch.equal(both.edge_index.cpu(), h[4]) and torch.equal(both.edge_ptr_host, h[6])
    for ids in ([G + 8, 3, 8, G + NO_EDGES, 2 * G - 1, 0], list(range(2 * G))):
        assert_edges(ops.collate(both, ids, validate=True), h, ids)
    plain = GraphStore(b[0].to(cuda), b[1].to(cuda), b[2], b[3])
    with pytest.raises(ValueError, match="edges"):
        ConcatGraphs([device_store(a, cuda), plain])
    with pytest.raises(ValueError, match="weights"):
        ConcatGraphs([device_store(a, cuda),
                      device_store(host_store(True, torch.float64, seed=2), cuda)])
    with pytest.raises(ValueError, match="weights"):
        ConcatGraphs([device_store(a, cuda), device_store(host_store(True, None, seed=2), cuda)])


def test_store_without_edges_is_as_before(cuda):
    h = host_store(True, None)
    plain = GraphStore(h[0].to(cuda), h[1].to(cuda), h[2], h[3])
    calls = []
    _lib.set_tracer(lambda name, args, launch: (calls.append(name), launch())[1])
    try:
        batch = ops.collate(plain, [3, 8], validate=True)
    finally:
        _lib.set_tracer(None)
    assert calls == ["lgnn_collate"]
    assert batch.edge_index.shape == (2, 0) and batch.edge_index.dtype == torch.int64
    assert not hasattr(batch, "edge_ptr") and not hasattr(batch, "edge_weight")
