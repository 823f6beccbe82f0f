"""The GPU graph dataset and loader (datasets/memory.py, ops.collate, lgnn_collate) against the
plain-torch collate of tests/loader_ref.py. Copies are exact: every comparison is torch.equal."""
import functools

import pytest
import torch

from lesion_gnn_amd import _lib, ops, synth
from lesion_gnn_amd.datasets import (ConcatGraphs, DataConfig, DataModule, GraphLoader,
                                     GraphStore)
from lesion_gnn_amd.knn import KNNGraph
from lesion_gnn_amd.utils import ClassWeights
from tests import loader_ref as lr

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def _host(G, channels, dims):
    return lr.make_store_tensors(G, channels, dims)


def _store(cuda, G, channels, dims):
    x, pos, y, ptr = _host(G, channels, dims)
    return GraphStore.from_tensors(x.to(cuda), None if pos is None else pos.to(cuda), y, ptr)


def _assert_batch(batch, want, num_graphs):
    wx, wpos, wy, wbatch, wptr = want
    assert batch.num_graphs == num_graphs
    assert batch.x.dtype == torch.float32 and torch.equal(batch.x.cpu(), wx)
    if wpos is None:
        assert batch.pos is None
    else:
        assert batch.pos.dtype == torch.float64 and torch.equal(batch.pos.cpu(), wpos)
    assert batch.y.dtype == torch.int64 and torch.equal(batch.y.cpu(), wy)
    assert batch.batch.dtype == torch.int64 and torch.equal(batch.batch.cpu(), wbatch)
    assert batch.ptr.dtype == torch.int64 and torch.equal(batch.ptr.cpu(), wptr)


# 1 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", lr.DIMS)
@pytest.mark.parametrize("channels", lr.CHANNELS)
@pytest.mark.parametrize("G", sorted(lr.STORE_SIZES))
def test_collate_parity(cuda, G, channels, dims):
    host = _host(G, channels, dims)
    store = _store(cuda, G, channels, dims)
    assert len(store) == G and store.num_features == channels
    for name, ids in lr.id_cases(G).items():
        batch = ops.collate(store, ids, validate=True)
        _assert_batch(batch, lr.collate_ref(*host, ids), len(ids))
        assert batch.edge_index.shape == (2, 0) and batch.edge_index.dtype == torch.int64
        assert batch.x.is_cuda and batch.edge_index.is_cuda, name
    # a host tensor of ids is taken as a list is
    ids = lr.id_cases(G)["reversed"]
    _assert_batch(ops.collate(store, torch.tensor(ids)), lr.collate_ref(*host, ids), len(ids))


# 2, 3: the C entry on buffers of its caller ------------------------------------------------------

class _Buffers:
    """Output buffers of `rows` rows filled with a sentinel, and one lgnn_collate call on them."""

    def __init__(self, store, max_sel, rows):
        dev = store.x.device
        self.store, self.rows = store, rows
        C = store.num_features
        self.x = torch.full((rows, C), SENTINEL, dtype=torch.float32, device=dev)
        self.dims = 0 if store.pos is None else store.pos.size(1)
        self.pos = torch.full((rows, max(self.dims, 1)), SENTINEL, dtype=torch.float64,
                              device=dev)
        self.batch = torch.full((rows,), int(SENTINEL), dtype=torch.int64, device=dev)
        self.y = torch.full((max_sel,), int(SENTINEL), dtype=torch.int64, device=dev)
        self.ptr = torch.full((max_sel + 1,), int(SENTINEL), dtype=torch.int64, device=dev)
        self.err = torch.full((1,), 99, dtype=torch.int32, device=dev)
        self.ids = torch.zeros(max_sel, dtype=torch.int64, device=dev)
        self.nws = _lib.load().lgnn_collate_workspace_bytes(max_sel)
        self.ws = torch.empty(self.nws, dtype=torch.uint8, device=dev)

    def call(self, num_sel, capacity):
        s = self.store
        _lib.call("lgnn_collate", self.ids, num_sel, s.ptr, len(s), s.x, s.num_features, s.pos,
                  self.dims, s.y, self.x, self.pos if self.dims else None, self.y, self.batch,
                  self.ptr, capacity, self.err, self.ws, self.nws, _lib.stream(s.x.device))

    def check(self, want, written):
        """Rows [0, written) equal the reference, rows from `written` on are still sentinel."""
        wx, wpos, wy, wbatch, wptr = want
        B = wy.numel()
        assert torch.equal(self.x[:written].cpu(), wx[:written])
        assert torch.equal(self.batch[:written].cpu(), wbatch[:written])
        if self.dims:
            assert torch.equal(self.pos[:written].cpu(), wpos[:written])
        assert bool((self.x[written:] == SENTINEL).all())
        assert bool((self.pos[written:] == SENTINEL).all())
        assert bool((self.batch[written:] == int(SENTINEL)).all())
        assert torch.equal(self.ptr[:B + 1].cpu(), wptr) and torch.equal(self.y[:B].cpu(), wy)
        assert bool((self.y[B:] == int(SENTINEL)).all())
        assert bool((self.ptr[B + 1:] == int(SENTINEL)).all())


@pytest.mark.parametrize("channels,dims", [(1025, 2), (3, 3), (1, 0)])
def test_capacity(cuda, channels, dims):
    host = _host(37, channels, dims)
    store = _store(cuda, 37, channels, dims)
    ids = lr.id_cases(37)["shuffled_subset"]
    want = lr.collate_ref(*host, ids)
    total = int(want[4][-1])
    for capacity in (total, total - 1, total // 2, 1, 0):
        buf = _Buffers(store, len(ids) + 3, total + 70)
        buf.ids[:len(ids)] = torch.tensor(ids)
        buf.call(len(ids), capacity)
        err = int(buf.err.item())
        if capacity == total:
            assert err == 0
        else:
            assert err == _lib.LGNN_COLLATE_OVERFLOW
        buf.check(want, capacity)


def test_out_of_range_id(cuda):
    host = _host(37, 1025, 2)
    x, pos, y, ptr = host
    store = _store(cuda, 37, 1025, 2)
    ids = [5, 37, 0, -1, 36, 1 << 40, 4]
    good = [i for i in ids if 0 <= i < 37]
    buf = _Buffers(store, len(ids), int(ptr[-1]))
    buf.ids[:] = torch.tensor(ids)
    wx, wpos, wy, wbatch, wptr = lr.collate_ref(*host, good)
    total = int(wptr[-1])
    buf.call(len(ids), total)
    assert int(buf.err.item()) == 3
    # a bad id is an empty graph: the good ones keep their batch positions
    where = torch.tensor([k for k, i in enumerate(ids) if 0 <= i < 37])
    sizes = torch.zeros(len(ids), dtype=torch.int64)
    sizes[where] = wptr[1:] - wptr[:-1]
    assert torch.equal(buf.ptr.cpu(), torch.cat([torch.zeros(1, dtype=torch.int64),
                                                 sizes.cumsum(0)]))
    assert torch.equal(buf.x[:total].cpu(), wx) and torch.equal(buf.pos[:total].cpu(), wpos)
    assert torch.equal(buf.batch[:total].cpu(), where[wbatch])
    assert torch.equal(buf.y.cpu()[where], wy)
    assert bool((buf.x[total:] == SENTINEL).all())
    # through ops.collate the ids are checked on the host, before any launch
    calls = []
    _lib.set_tracer(lambda name, args, launch: calls.append(name) or launch())
    try:
        for bad in ([0, 37], [-1], torch.tensor([3, 1 << 40])):
            with pytest.raises(IndexError):
                ops.collate(store, bad)
    finally:
        _lib.set_tracer(None)
    assert calls == []


@pytest.mark.parametrize("num_sel", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_scan_lengths(cuda, num_sel):
    """k_collate_scan at the wave edge, the tile edge (1024 ids) and with a carry over two tiles:
    ids drawn with repetition from the 37 graphs and three empty ones, every 61st one (and the ids
    on both sides of the first tile edge) outside the dataset, so the count in err crosses a tile
    as the offsets do."""
    x, pos, y, ptr = _host(37, 3, 2)
    ptr = torch.cat([ptr, ptr[-1:].expand(3)])  # graphs 37, 38, 39: no rows
    y = torch.cat([y, torch.tensor([0, 1, 2])])
    host, G = (x, pos, y, ptr), 40
    store = GraphStore.from_tensors(x.to(cuda), pos.to(cuda), y, ptr)
    ids = torch.randint(0, G, (num_sel,), generator=torch.Generator().manual_seed(num_sel))
    bad = [k for k in range(num_sel) if k % 61 == 60 or k in (1023, 1024)]
    for j, k in enumerate(bad):
        ids[k] = (G, -1, 1 << 40)[j % 3]
    where = torch.tensor([k for k in range(num_sel) if k not in bad], dtype=torch.int64)
    assert num_sel < 100 or bool((ids[where] >= 37).any())  # an empty graph is selected
    wx, wpos, wy, wbatch, wptr = lr.collate_ref(*host, ids[where].tolist())
    total = int(wptr[-1])
    buf = _Buffers(store, num_sel, total + 8)
    buf.ids[:] = ids
    buf.call(num_sel, total)
    assert int(buf.err.item()) == len(bad) < _lib.LGNN_COLLATE_OVERFLOW
    # a bad id is an empty graph: the good ones keep their batch positions
    sizes = torch.zeros(num_sel, dtype=torch.int64)
    sizes[where] = wptr[1:] - wptr[:-1]
    assert torch.equal(buf.ptr.cpu(), torch.cat([torch.zeros(1, dtype=torch.int64),
                                                 sizes.cumsum(0)]))
    assert torch.equal(buf.x[:total].cpu(), wx) and torch.equal(buf.pos[:total].cpu(), wpos)
    assert torch.equal(buf.batch[:total].cpu(), where[wbatch])
    assert torch.equal(buf.y.cpu()[where], wy)
    assert bool((buf.x[total:] == SENTINEL).all())
    assert bool((buf.batch[total:] == int(SENTINEL)).all())


# 4 ---------------------------------------------------------------------------------------------

def test_offsets_past_4gib(cuda):
    """A resident x of just over 2^32 bytes at 1025 channels; the last two graphs' rows lie past
    byte 2^32 and are the only ones filled."""
    C = 1025
    rows = (1 << 32) // (4 * C) + 200
    nbytes = rows * C * 4
    assert nbytes > 1 << 32
    if torch.cuda.mem_get_info(cuda)[0] < 3 * nbytes:
        pytest.skip("not enough free device memory for a > 4 GiB store")
    n1, n2 = 65, 64
    first = rows - n1 - n2
    assert first * C * 4 > 1 << 32
    x = torch.empty(rows, C, dtype=torch.float32, device=cuda)
    gen = torch.Generator().manual_seed(4)
    tail = torch.randn(n1 + n2, C, generator=gen)
    x[first:] = tail.to(cuda)
    pos = torch.zeros(rows, 2, dtype=torch.float64, device=cuda)
    tail_pos = torch.rand(n1 + n2, 2, generator=gen, dtype=torch.float64)
    pos[first:] = tail_pos.to(cuda)
    store = GraphStore.from_tensors(x, pos, torch.tensor([0, 1, 2]),
                                    torch.tensor([0, first, first + n1, rows]))
    batch = ops.collate(store, [2, 1], validate=True)
    assert torch.equal(batch.x.cpu(), torch.cat([tail[n1:], tail[:n1]]))
    assert torch.equal(batch.pos.cpu(), torch.cat([tail_pos[n1:], tail_pos[:n1]]))
    assert batch.ptr.tolist() == [0, n2, n1 + n2] and batch.y.tolist() == [2, 1]
    assert torch.equal(batch.batch.cpu(), torch.repeat_interleave(torch.arange(2),
                                                                  torch.tensor([n2, n1])))


# 5 ---------------------------------------------------------------------------------------------

def test_captured_call_replays_on_refilled_ids(cuda):
    host = _host(37, 1025, 2)
    store = _store(cuda, 37, 1025, 2)
    B = 6
    sizes = host[3][1:] - host[3][:-1]
    capacity = int(sizes.sort(descending=True).values[:B].sum())  # any B distinct graphs fit
    buf = _Buffers(store, B, capacity + 8)
    buf.ids[:] = torch.arange(B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buf.call(B, capacity)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.call(B, capacity)
    order = sizes.argsort(descending=True).tolist()
    selections = [order[:B], order[-B:], [0, 5, 1, 4, 2, 3], order[3:3 + B][::-1], [1] * B]
    totals = set()
    for ids in selections:
        want = lr.collate_ref(*host, ids)
        total = int(want[4][-1])
        assert total <= capacity
        totals.add(total)
        buf.x.fill_(SENTINEL), buf.pos.fill_(SENTINEL), buf.batch.fill_(int(SENTINEL))
        buf.ids.copy_(torch.tensor(ids))
        graph.replay()
        assert int(buf.err.item()) == 0
        buf.check(want, total)
    assert len(totals) == len(selections)


# 6 ---------------------------------------------------------------------------------------------

def _knn_edges_of(pos, ptr, k=6):
    """synth.knn_edges per graph at its row offset."""
    out = []
    for a, b in zip(ptr[:-1].tolist(), ptr[1:].tolist()):
        out.append(synth.knn_edges(pos[a:b][None], k, True)[0] + a)
    return torch.cat(out, dim=1)


def test_loader_epoch(cuda):
    host = _host(37, 128, 2)
    store = _store(cuda, 37, 128, 2)
    loader = GraphLoader(store, 8, shuffle=True, transform=KNNGraph(k=6, loop=True),
                         generator=torch.Generator().manual_seed(1))
    assert len(loader) == 5
    epochs = []
    for _ in range(2):
        seen = []
        for batch in loader:
            ids = batch.ids
            assert ids.dtype == torch.int64 and not ids.is_cuda
            want = lr.collate_ref(*host, ids.tolist())
            _assert_batch(batch, want, ids.numel())
            assert torch.equal(batch.edge_index.cpu(), _knn_edges_of(want[1], want[4]))
            seen += ids.tolist()
        assert sorted(seen) == list(range(37))
        epochs.append(seen)
    assert epochs[0] != epochs[1]
    assert len(GraphLoader(store, 8, drop_last=True)) == 4
    assert [b.ids.tolist() for b in GraphLoader(store, 16)] == \
        [list(range(16)), list(range(16, 32)), list(range(32, 37))]


def _data_config(batch_size):
    from lesion_gnn_amd.datasets.aptos import AptosConfig
    from lesion_gnn_amd.datasets.ddr import DDRConfig, DDRVariant
    from lesion_gnn_amd.datasets.nodes import lesions
    from lesion_gnn_amd.transforms import TransformConfig

    nodes = lesions.LesionsNodesConfig(feature_source=lesions.SegmentationEncoderFeatures(layer=4))
    valid = DDRConfig(root="", nodes=nodes, variant=DDRVariant.VALID)
    test = DDRConfig(root="", nodes=nodes, variant=DDRVariant.TEST)
    valid.name, test.name = "DDR-valid", "DDR-test"  # every DDRConfig is born "DDR"
    return DataConfig(
        train_datasets=[DDRConfig(root="", nodes=nodes, variant=DDRVariant.TRAIN),
                        AptosConfig(root="", nodes=nodes)],
        val_datasets=[valid, AptosConfig(root="", nodes=nodes)],
        test_datasets=[test],
        transforms=[TransformConfig(name="KNNGraph", kwargs={"k": 6, "loop": True})],
        batch_size=batch_size, num_workers=0)


def test_data_module(cuda):
    big, small = _store(cuda, 37, 128, 2), _store(cuda, 2, 128, 2)
    x, pos, y, ptr = _host(37, 128, 2)
    y5 = torch.arange(37) % 5
    train = GraphStore.from_tensors(x.to(cuda), pos.to(cuda), y5, ptr)
    stores = {"DDR": train, "DDR-valid": big, "Aptos": train, "DDR-test": small}
    dm = DataModule(_data_config(16), stores=stores)
    with pytest.raises(NotImplementedError):
        dm.setup("predict")
    dm.setup("fit")
    assert dm.num_features == 128 and dm.num_classes == 5
    assert torch.equal(dm.get_class_weights(ClassWeights.INVERSE),
                       1 / (2 * torch.unique(y5, return_counts=True)[1]))
    tl = dm.train_dataloader()
    assert tl.shuffle and len(tl.store) == 74 and len(tl) == 5
    val = dm.val_dataloader()
    assert list(val) == ["DDR-valid", "Aptos"] and not val["DDR-valid"].shuffle
    host = _host(37, 128, 2)
    got = list(val["DDR-valid"])
    assert [b.ids.tolist() for b in got] == [list(range(16)), list(range(16, 32)),
                                             list(range(32, 37))]
    for b in got:
        want = lr.collate_ref(*host, b.ids.tolist())
        _assert_batch(b, want, b.ids.numel())
        assert torch.equal(b.edge_index.cpu(), _knn_edges_of(want[1], want[4]))
    dm.setup("test")
    assert len(dm.test_dataloader()["DDR-test"].store) == 2
    with pytest.raises(KeyError, match="Aptos"):
        DataModule(_data_config(16), stores={"DDR": small}).setup("fit")


# 7 ---------------------------------------------------------------------------------------------

def test_training_step_on_loader_batches(cuda):
    from lesion_gnn_amd.models import get_model
    from lesion_gnn_amd.models.base import OptimizerConfig
    from lesion_gnn_amd.models.gat import GATConfig

    host = _host(37, 1025, 2)
    store = _store(cuda, 37, 1025, 2)
    cfg = GATConfig(optimizer=OptimizerConfig(), hiddden_channels=[32, 32], heads=2, dropout=0.0,
                    compile=False)
    cfg.num_classes.value = 5
    cfg.input_features.value = store.num_features
    cfg.optimizer.class_weights.value = torch.ones(5)
    torch.manual_seed(0)
    module = get_model(cfg).to(cuda).train()
    loader = GraphLoader(store, 16, shuffle=True, transform=KNNGraph(k=6, loop=True),
                         generator=torch.Generator().manual_seed(2))
    for k, batch in enumerate(loader):
        if k == 2:
            break
        wx, wpos, wy, wbatch, wptr = lr.collate_ref(*host, batch.ids.tolist())
        ref_batch = synth.Batch(wx, _knn_edges_of(wpos, wptr), wbatch, wptr, wy, wpos,
                                batch.ids.numel()).to(cuda)
        got = module.training_step(batch)
        want = module.training_step(ref_batch)
        assert got.item() > 0 and torch.equal(got, want)


# 8 ---------------------------------------------------------------------------------------------

def test_concat_graphs(cuda):
    a, b = _store(cuda, 37, 4, 2), _store(cuda, 2, 4, 2)
    with pytest.raises(ValueError, match="features"):
        ConcatGraphs([a, _store(cuda, 2, 3, 2)])
    x, pos, y, ptr = _host(2, 4, 2)
    ya = torch.arange(37) % 5
    a = GraphStore.from_tensors(a.x, a.pos, ya, a.ptr_host)
    with pytest.raises(ValueError, match="classes"):
        ConcatGraphs([a, GraphStore.from_tensors(b.x, b.pos, torch.tensor([0, 1]), b.ptr_host)])
    b = GraphStore.from_tensors(b.x, b.pos, torch.tensor([4, 4]), b.ptr_host)
    both = ConcatGraphs([a, b])
    assert len(both) == 39 and both.num_features == 4 and both.num_classes == 5
    counts = torch.unique(ya, return_counts=True)[1]
    # reference ConcatDataset: the per-dataset counts summed position by position
    assert torch.equal(both.classes_counts, counts + torch.tensor([2]))
    summed = counts + 2
    want = {ClassWeights.UNIFORM: torch.ones(5), ClassWeights.INVERSE: 1 / summed,
            ClassWeights.QUADRATIC_INVERSE: 1 / summed ** 2,
            ClassWeights.INVERSE_FREQUENCY: summed.sum() / (5 * summed)}
    for mode in ClassWeights:
        assert torch.equal(both.get_class_weights(mode), want[mode])
    ha = _host(37, 4, 2)
    host = (torch.cat([ha[0], x]), torch.cat([ha[1], pos]), torch.cat([ya, torch.tensor([4, 4])]),
            torch.cat([ha[3], ptr[1:] + ha[3][-1]]))
    ids = [38, 0, 37, 36, 5]
    _assert_batch(ops.collate(both, ids), lr.collate_ref(*host, ids), 5)


def test_store_from_lesion_nodes_round_trip(cuda, tmp_path):
    from lesion_gnn_amd.datasets.nodes import lesions
    from tests import ccl_cases as cases

    ex = lesions.LesionsExtractor(lesions.LesionsNodesConfig(
        feature_source=lesions.SegmentationEncoderFeatures(layer=4)))
    items = []
    for seed, label in ((21, 3), (22, 0)):
        cls = cases.blob_classes(64, 64, 12, seed=seed)
        feats = torch.randn(1, 8, 32, 32, generator=torch.Generator().manual_seed(seed))
        items.append(ex.nodes_from_maps(cases.logits_of(cls, 5, seed=seed).to(cuda),
                                        feats.to(cuda), label))
    store = GraphStore.from_list(items)
    n = [it.x.size(0) for it in items]
    assert len(store) == 2 and store.num_features == 9 and store.num_classes == 4
    assert store.ptr_host.tolist() == [0, n[0], n[0] + n[1]] and store.y_host.tolist() == [3, 0]
    assert store.classes_counts.tolist() == [1, 1]
    host = (torch.cat([it.x for it in items]).cpu(), torch.cat([it.pos for it in items]).cpu(),
            store.y_host, store.ptr_host)
    _assert_batch(ops.collate(store, [1, 0]), lr.collate_ref(*host, [1, 0]), 2)
    path = tmp_path / "store.pt"
    store.save(path)
    raw = torch.load(path, weights_only=True)
    assert sorted(raw) == ["pos", "ptr", "x", "y"] and not raw["x"].is_cuda
    back = GraphStore.load(path, cuda)
    assert back.x.is_cuda and torch.equal(back.x, store.x) and torch.equal(back.pos, store.pos)
    assert torch.equal(back.y, store.y) and torch.equal(back.ptr, store.ptr)
    _assert_batch(ops.collate(back, [1, 0]), lr.collate_ref(*host, [1, 0]), 2)
    # the (data, slices) layout of a processed data.pt
    sliced = GraphStore.from_slices(store.x, store.pos, store.y,
                                    {"x": store.ptr_host, "pos": store.ptr_host,
                                     "y": torch.arange(3)})
    assert torch.equal(sliced.ptr, store.ptr) and len(sliced) == 2
