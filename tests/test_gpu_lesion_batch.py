"""LesionsExtractor.nodes_from_batch (reference lesions.py:147-176 for a batch of images, the
reinterpolation fused into the pooling) against the CPU restatement
tests/ccl_ref.lesion_nodes_ref per image, against a loop of nodes_from_maps, and through
GraphStore / GraphLoader / KNNGraph against the oracle's k-NN on the reference positions.

ptr and pos are exact. x is held per node to the rule of
tests/test_gpu_lesion_batch_kernels.py (the restatement interpolates with torch on the CPU, in
fp32 and in float64); with reinterpolation=None nothing is resampled and max is exact."""
import functools

import pytest
import torch
import torch.nn.functional as F

import oracle.pyg_ref as ref
from lesion_gnn_amd.datasets import GraphLoader, GraphStore
from lesion_gnn_amd.datasets.nodes import lesions
from lesion_gnn_amd.knn import KNNGraph
from tests import ccl_cases as cases
from tests import ccl_ref

pytestmark = pytest.mark.gpu

LABELS = [3, 0, 4]
NAMES = ["a", "b", "c"]


def _extractor(reduce, reinterpolation=None):
    return lesions.LesionsExtractor(lesions.LesionsNodesConfig(
        feature_source=lesions.SegmentationEncoderFeatures(layer=4), features_reduction=reduce,
        reinterpolation=reinterpolation))


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(logits (B, 5, Horg, Worg), features (B, C, h, w), reinterpolation)"""
    if case == "interp":  # B = 3, image 1 all background, 16 features at 24 x 24 -> 48 x 48
        cls = [cases.blob_classes(96, 96, 30, seed=11), torch.zeros(96, 96, dtype=torch.int64),
               cases.blob_classes(96, 96, 20, seed=13)]
        C, fsize, re = 16, (24, 24), (48, 48)
    else:  # "plain": B = 2, the reference's channel width at 32 x 32, nothing resampled
        cls = [cases.blob_classes(64, 64, 20, seed=14), cases.blob_classes(64, 64, 9, seed=15)]
        C, fsize, re = 1024, (32, 32), None
    logits = torch.cat([cases.logits_of(c, 5, seed=k) for k, c in enumerate(cls)])
    feats = torch.randn(len(cls), C, *fsize, generator=torch.Generator().manual_seed(C))
    return logits, feats, re


@functools.lru_cache(maxsize=None)
def _expected(case, reduce):
    """Per image (pos, x32, x64) of the restatement, torch's interpolate on the CPU before it."""
    logits, feats, re = _inputs(case)
    out = []
    for b in range(logits.size(0)):
        f32, f64 = feats[b:b + 1], feats[b:b + 1].double()
        if re is not None:
            kw = dict(size=re, mode="bilinear", align_corners=False)
            f32, f64 = F.interpolate(f32, **kw), F.interpolate(f64, **kw)
        pos, x32, _ = ccl_ref.lesion_nodes_ref(logits[b:b + 1], f32, 0, reduce)
        _, x64, _ = ccl_ref.lesion_nodes_ref(logits[b:b + 1], f64, 0, reduce,
                                             dtype=torch.float64)
        out.append((pos, x32, x64))
    return out


def _assert_rule(got, x32, x64, what):
    ref_err = (x32.double() - x64).abs()
    err = (got.double() - x64).abs()
    bound = torch.clamp(2 * ref_err.amax(1, keepdim=True), min=1e-6 * float(x64.abs().max()))
    print(f"{what}: max err {float(err.max()):.3e}, restatement's {float(ref_err.max()):.3e}, "
          f"largest err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (float(err.max()), float(ref_err.max()))


def _loop(ex, logits, feats, cuda, labels):
    return [ex.nodes_from_maps(logits[b:b + 1].to(cuda), feats[b:b + 1].to(cuda), labels[b])
            for b in range(logits.size(0))]


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_nodes_from_batch(cuda, reduce):
    logits, feats, re = _inputs("interp")
    want = _expected("interp", reduce)
    ex = _extractor(reduce, re)
    batch = ex.nodes_from_batch(logits.to(cuda), feats.to(cuda), LABELS, NAMES)
    sizes = [w[0].size(0) for w in want]
    ptr = [0, sizes[0], sizes[0] + sizes[1], sum(sizes)]
    assert sizes[1] == 1 and len(batch) == 3
    assert batch.ptr.is_cuda and batch.ptr.dtype == torch.int64 and batch.ptr.tolist() == ptr
    assert batch.pos.is_cuda and batch.pos.dtype == torch.float64
    assert torch.equal(batch.pos.cpu(), torch.cat([w[0] for w in want]))
    singles = _loop(ex, logits, feats, cuda, LABELS)
    assert torch.equal(batch.pos, torch.cat([s.pos for s in singles]))
    assert batch.y.tolist() == LABELS and batch.names == NAMES
    assert batch.x.is_cuda and batch.x.dtype == torch.float32
    assert batch.x.shape == (sum(sizes), 17)
    x32, x64 = torch.cat([w[1] for w in want]), torch.cat([w[2] for w in want])
    _assert_rule(batch.x.cpu(), x32, x64, f"nodes_from_batch {reduce}")
    for b in range(3):
        one = batch[b]
        assert torch.equal(one.x, batch.x[ptr[b]:ptr[b + 1]])
        assert torch.equal(one.pos, batch.pos[ptr[b]:ptr[b + 1]])
        assert one.y.tolist() == [LABELS[b]] and one.name == NAMES[b]
        assert one.x.data_ptr() == batch.x[ptr[b]:].data_ptr()  # a view, not a copy
    # the all-background image: one node, the global mean also under max
    mean = F.interpolate(feats[1:2].double(), size=re, mode="bilinear",
                         align_corners=False).mean((2, 3))
    assert torch.allclose(batch[1].x[:, :16].cpu().double(), mean, rtol=0, atol=1e-6)
    assert batch[1].x[0, 16].item() == 0.0


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_nodes_from_batch_without_reinterpolation(cuda, reduce):
    logits, feats, re = _inputs("plain")
    want = _expected("plain", reduce)
    ex = _extractor(reduce, re)
    batch = ex.nodes_from_batch(logits.to(cuda), feats.to(cuda), [1, 2])
    assert batch.names is None and batch[0].name is None
    assert torch.equal(batch.pos.cpu(), torch.cat([w[0] for w in want]))
    if reduce == "max":
        singles = _loop(ex, logits, feats, cuda, [1, 2])
        assert torch.equal(batch.x, torch.cat([s.x for s in singles]))
    x32, x64 = torch.cat([w[1] for w in want]), torch.cat([w[2] for w in want])
    _assert_rule(batch.x.cpu(), x32, x64, f"nodes_from_batch, no reinterpolation, {reduce}")


def test_one_host_read_per_batch(cuda, monkeypatch):
    logits, feats, re = _inputs("interp")
    ex = _extractor("max", re)  # max: image 1's lone node takes the second, mean, pass too
    zl, zf = logits.to(cuda), feats.to(cuda)
    ex.nodes_from_batch(zl, zf, LABELS)  # nothing left to load or allocate lazily
    reads = []
    for name in ("item", "tolist", "cpu"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **kw):
            if self.is_cuda:
                reads.append((_name, tuple(self.shape)))
            return _orig(self, *a, **kw)

        monkeypatch.setattr(torch.Tensor, name, counted)
    batch = ex.nodes_from_batch(zl, zf, LABELS)
    monkeypatch.undo()
    assert reads == [("cpu", (4,))], reads
    assert batch.ptr_host.tolist() == batch.ptr.tolist()


def test_store_and_loader(cuda):
    logits, feats, re = _inputs("interp")
    want = _expected("interp", "mean")
    batch = _extractor("mean", re).nodes_from_batch(logits.to(cuda), feats.to(cuda), LABELS)
    store = batch.to_store()
    assert isinstance(store, GraphStore) and len(store) == 3
    assert torch.equal(store.ptr_host, batch.ptr.cpu())
    assert store.x.data_ptr() == batch.x.data_ptr()  # no copy, no torch.cat
    assert store.pos.data_ptr() == batch.pos.data_ptr()
    assert store.y_host.tolist() == LABELS
    loader = GraphLoader(store, batch_size=2, transform=KNNGraph(k=6, loop=True))
    seen = []
    for got in loader:
        ids = got.ids.tolist()
        edges, base = [], 0
        for g in ids:
            edges.append(ref.knn_graph(want[g][0], 6, loop=True) + base)
            base += want[g][0].size(0)
        assert torch.equal(got.edge_index.cpu(), torch.cat(edges, dim=1))
        assert torch.equal(got.pos.cpu(), torch.cat([want[g][0] for g in ids]))
        seen += ids
    assert seen == [0, 1, 2]
