"""GPU: DataModule(hoist=True) — the per-graph transforms run once per store, the loader collates
their edges — against the per-batch chain of hoist=False on the same stores and the same epoch
order. k-NN and radius neighbours are found per graph and in node order, and the Gaussian weight
is a function of an edge's two positions, so the hoisted batches equal the per-batch chain's in
the order of the edges too (no sort is needed): asserted bit for bit."""
import pytest
import torch

from lesion_gnn_amd import _lib
from lesion_gnn_amd.datasets import DataConfig, DataModule, GraphStore
from lesion_gnn_amd.transforms import TransformConfig
from tests import fit_ref as fr

pytestmark = pytest.mark.gpu

KNN = TransformConfig(name="KNNGraph", kwargs=dict(k=6, loop=True))
MAX_NEIGHBORS = 8
# pos ~ U[0, 1)^2: the 300-node graph has about 300 pi r^2 = 21 nodes in range of each node, more
# than MAX_NEIGHBORS, and the one-node graph has nobody
RADIUS = TransformConfig(name="RadiusGraph", kwargs=dict(r=0.15, max_num_neighbors=MAX_NEIGHBORS))
WEIGHT = TransformConfig(name="GaussianDistance", kwargs=dict(sigma=0.3))
CHAINS = {"knn": [KNN], "radius": [RADIUS], "knn_gaussian": [KNN, WEIGHT]}


@pytest.fixture(scope="module")
def stores(cuda):
    out = {}
    for name, (x, pos, y, ptr) in fr.fixture_tensors().items():
        out[name] = GraphStore(x.to(cuda), pos.to(cuda), y, ptr)
    return out


def modules(chain, batch_size, stores):
    """(hoisted, per batch): two DataModules over the same stores, the train loaders' generators
    seeded alike."""
    out = []
    for hoist in (True, False):
        cfg = DataConfig(train_datasets=[fr._dataset("train")],
                         val_datasets=[fr._dataset("valA")], test_datasets=[],
                         transforms=list(CHAINS[chain]), batch_size=batch_size, num_workers=0)
        dm = DataModule(cfg, compile=False, stores=stores, hoist=hoist)
        dm.generator = torch.Generator().manual_seed(11)
        dm.setup("fit")
        out.append(dm)
    return out


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("batch_size", [5, 10000])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_hoisted_batches_equal_the_per_batch_chain(cuda, stores, chain, batch_size):
    hoisted, per_batch = modules(chain, batch_size, stores)
    assert hoisted.train_datasets.edge_index is not None
    assert per_batch.train_datasets.edge_index is None and stores["train"].edge_index is None
    if chain == "radius":
        eptr = hoisted.train_datasets.edge_ptr_host
        counts = eptr[1:] - eptr[:-1]
        indegree = torch.bincount(hoisted.train_datasets.edge_index[1])
        # the cap: max_num_neighbors in-range nodes in index order, one more when the node itself
        # is not among them (torch_cluster drops the self pair after the cut, include/lgnn.h)
        assert int(counts.min()) == 0
        assert int(indegree.max()) in (MAX_NEIGHBORS, MAX_NEIGHBORS + 1)
    for loaders in ((hoisted.train_dataloader(), per_batch.train_dataloader()),
                    (hoisted.val_dataloader()["valA"], per_batch.val_dataloader()["valA"])):
        n = 0
        for a, b in zip(*loaders, strict=True):
            assert torch.equal(a.ids, b.ids)
            assert torch.equal(a.edge_index, b.edge_index)  # the order too
            assert torch.equal(a.x, b.x) and torch.equal(a.batch, b.batch)
            assert torch.equal(a.y, b.y) and torch.equal(a.ptr, b.ptr)
            if chain == "knn_gaussian":
                assert a.edge_weight.dtype == b.edge_weight.dtype == torch.float32
                assert torch.equal(bits(a.edge_weight), bits(b.edge_weight))
            else:
                assert not hasattr(a, "edge_weight") and not hasattr(b, "edge_weight")
            n += 1
        assert n == len(loaders[0]) >= 1


def test_stores_that_are_not_hoisted_keep_the_chain(cuda, stores):
    edged = stores["valA"].with_edges(torch.zeros(2, 0, dtype=torch.int64, device=cuda))
    cfg = DataConfig(train_datasets=[fr._dataset("train")], val_datasets=[fr._dataset("valA")],
                     test_datasets=[], transforms=[KNN], batch_size=7, num_workers=0)
    dm = DataModule(cfg, stores=dict(stores, valA=edged), hoist=True)
    dm.setup("fit")
    assert dm.val_datasets["valA"] is edged  # a store with edges is left as it is ...
    plain = DataModule(cfg, stores=stores)   # ... and today's arguments mean today's behaviour
    plain.setup("fit")
    assert plain.hoist is False and plain.train_datasets.edge_index is None
    for a, b in zip(dm.val_dataloader()["valA"], plain.val_dataloader()["valA"], strict=True):
        assert torch.equal(a.edge_index, b.edge_index) and a.edge_index.size(1) > 0
    # a chain that does not start with a graph builder: nothing is hoisted
    attr = TransformConfig(name="GaussianDistance", kwargs=dict(sigma=0.3, save_as="edge_attr_cat"))
    cfg2 = DataConfig(train_datasets=[fr._dataset("train")], val_datasets=[], test_datasets=[],
                      transforms=[attr], batch_size=7, num_workers=0)
    dm2 = DataModule(cfg2, stores=stores, hoist=True)
    dm2.setup("fit")
    assert dm2.train_datasets.edge_index is None
    # train datasets of which only some come with edges: refused by name, nothing is hoisted
    cfg3 = DataConfig(train_datasets=[fr._dataset("train"), fr._dataset("valA")], val_datasets=[],
                      test_datasets=[], transforms=[KNN], batch_size=7, num_workers=0)
    with pytest.raises(ValueError, match=r"\['valA'\] already have edges and \['train'\] have"):
        DataModule(cfg3, stores=dict(stores, valA=edged), hoist=True).setup("fit")


def test_hoisted_epoch_launches_no_graph_builder_and_reads_nothing_back(cuda, stores, monkeypatch):
    hoisted, per_batch = modules("knn_gaussian", 5, stores)
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])

    def epoch(dm):
        names.clear()
        batches = list(dm.train_dataloader())
        for loader in dm.val_dataloader().values():
            batches += list(loader)
        return batches, sorted(set(names))

    _, per_batch_names = epoch(per_batch)
    assert {"lgnn_collate", "lgnn_knn_graph", "lgnn_gaussian_distance"} <= set(per_batch_names)
    assert "lgnn_collate_edges" not in per_batch_names
    _, hoisted_names = epoch(hoisted)  # also the warm-up of the guarded epoch below
    assert hoisted_names == ["lgnn_collate", "lgnn_collate_edges"]
    torch.cuda.synchronize()
    # does this build honour the sync debug mode at all?
    probe = torch.ones(1, device=cuda)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            batches, _ = epoch(hoisted)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not stop a .item() here")
    assert len(batches) == len(hoisted.train_dataloader()) + len(hoisted.val_dataloader()["valA"])
    assert all(b.edge_index.size(1) > 0 for b in batches)
