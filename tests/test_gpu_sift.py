"""SiftExtractor (reference sift.py:17-70 on the GPU) end to end: `nodes_from_image` over the
cases of tests/sift_cases.py against the float64 restatement tests/sift_ref.py, `nodes_from_batch`
against the per-image results bit for bit (an empty segment included), repeatability, the host
reads, and the nodes through GraphStore / GraphLoader / KNNGraph into a SetTransformer."""
import warnings

import numpy as np
import pytest
import torch

from lesion_gnn_amd import ops
from lesion_gnn_amd.datasets import GraphLoader, GraphStore
from lesion_gnn_amd.datasets.nodes.sift import SiftExtractor, SiftNodes, SiftNodesBatch
from lesion_gnn_amd.knn import KNNGraph, RadiusGraph
from lesion_gnn_amd.models.set_transformer import SetTransformer
from lesion_gnn_amd.transforms import GaussianDistance, SaveAs
from tests import sift_cases as cases
from tests import sift_ref

pytestmark = pytest.mark.gpu

LABELS = [3, 0, 4]
NAMES = ["a", "b", "c"]


def _dev(image, cuda):
    return torch.from_numpy(np.array(image)).to(cuda)  # a writable copy of the shared case


def _check_nodes(nodes, n=None):
    assert isinstance(nodes, SiftNodes)
    n = nodes.x.size(0) if n is None else n
    assert nodes.x.shape == (n, 128) and nodes.x.dtype == torch.float32
    assert nodes.pos.shape == (n, 2) and nodes.pos.dtype == torch.float64
    assert nodes.score.shape == (n,) and nodes.score.dtype == torch.float64
    assert nodes.edge_index is None and nodes.edge_attr is None
    x = nodes.x.cpu()
    assert torch.equal(x, x.round()) and (n == 0 or (x.min() >= 0 and x.max() <= 255))
    s = nodes.score.cpu()
    assert (s[:-1] >= s[1:]).all()  # strongest first


@pytest.mark.parametrize("num_keypoints", cases.NUM_KEYPOINTS)
@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_nodes_from_image(cuda, name, num_keypoints):
    _, image, sigma = cases.case(name)
    ex = SiftExtractor(num_keypoints, sigma)
    dev_image = _dev(image, cuda)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        nodes = ex.nodes_from_image(dev_image, 2, name="img")
    _check_nodes(nodes)
    n = nodes.x.size(0)
    assert nodes.y.tolist() == [2] and nodes.name == "img"
    messages = [str(w.message) for w in caught]
    if n < num_keypoints:
        assert messages == [f"Image img has less than {num_keypoints} keypoints."]
    else:
        assert messages == []
    # the device's own pyramid handed to the oracle: the same nodes
    pyr = ops.sift_pyramid(_dev(image, cuda)[None], sigma)
    gauss = [t[0].cpu().numpy() for t in pyr.gauss]
    dog = [t[0].cpu().numpy() for t in pyr.dog]
    kf, ki = sift_ref.keypoints(gauss, dog, sigma, num_keypoints)
    print(f"{name} num_keypoints {num_keypoints}: {n} nodes")
    assert n == len(kf) >= min(num_keypoints, 16)
    assert torch.equal(nodes.pos.cpu(), torch.from_numpy(kf[:, :2].astype(np.float64)))
    assert torch.equal(nodes.score.cpu(), torch.from_numpy(kf[:, 4].astype(np.float64)))
    diff = (nodes.x.cpu() - torch.from_numpy(sift_ref.descriptors(gauss, kf, ki))).abs()
    assert diff.max() <= 1 and (diff > 0).sum() <= diff.numel() * 1e-4


def test_no_keypoints(cuda):
    ex = SiftExtractor(16, 1.6)
    with pytest.warns(UserWarning, match="^Image flat has no keypoints.$"):
        nodes = ex.nodes_from_image(_dev(cases.constant(), cuda), 1, name="flat")
    _check_nodes(nodes, 0)


@pytest.mark.parametrize("num_keypoints", cases.NUM_KEYPOINTS)
def test_batch_equals_images(cuda, num_keypoints):
    imgs = _dev(cases.batch3(), cuda)
    ex = SiftExtractor(num_keypoints, 1.6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = ex.nodes_from_batch(imgs, LABELS, NAMES)
        singles = [ex.nodes_from_image(imgs[b], LABELS[b], NAMES[b]) for b in range(3)]
        again = ex.nodes_from_batch(imgs, LABELS, NAMES)
    assert isinstance(batch, SiftNodesBatch) and len(batch) == 3
    sizes = [s.x.size(0) for s in singles]
    assert sizes[1] == 0 and sizes[0] >= 16 and sizes[2] >= 16
    assert batch.ptr_host.tolist() == [0, sizes[0], sizes[0], sizes[0] + sizes[2]]
    assert torch.equal(batch.ptr.cpu(), batch.ptr_host) and batch.y.tolist() == LABELS
    for field in ("x", "pos", "score"):
        assert torch.equal(getattr(batch, field), torch.cat([getattr(s, field) for s in singles]))
        assert torch.equal(getattr(batch, field), getattr(again, field))  # two runs, the same bits
    for b in range(3):
        one = batch[b]
        _check_nodes(one, sizes[b])
        assert one.y.tolist() == [LABELS[b]] and one.name == NAMES[b]
        assert torch.equal(one.x, singles[b].x)
    assert batch[-1].x.data_ptr() == batch.x[batch.ptr_host[2]:].data_ptr()  # a view


def test_gray_batch(cuda):
    imgs = _dev(np.stack([cases.texture(37, 41, 3, channels=0),
                          cases.texture(37, 41, 4, channels=0)]), cuda)
    ex = SiftExtractor(10000, 1.6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = ex.nodes_from_batch(imgs, [0, 1])
        rgb = ex.nodes_from_batch(imgs[..., None].expand(-1, -1, -1, 3).contiguous(), [0, 1])
    assert int(batch.ptr_host[1]) >= 16 and int(batch.ptr_host[2] - batch.ptr_host[1]) >= 16
    # equal channels: (1868 + 9617 + 4899) v + 8192 >> 14 is v, so the gray image is the same
    assert torch.equal(batch.x, rgb.x) and torch.equal(batch.pos, rgb.pos)


def test_two_host_reads_per_batch(cuda, monkeypatch):
    imgs = _dev(cases.batch3(), cuda)
    ex = SiftExtractor(16, 1.6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ex.nodes_from_batch(imgs, LABELS)  # nothing left to load or allocate lazily
        reads = []
        for name in ("item", "tolist", "cpu"):
            orig = getattr(torch.Tensor, name)

            def counted(self, *a, _orig=orig, _name=name, **kw):
                if self.is_cuda:
                    reads.append((_name, tuple(self.shape)))
                return _orig(self, *a, **kw)

            monkeypatch.setattr(torch.Tensor, name, counted)
        ex.nodes_from_batch(imgs, LABELS)
        monkeypatch.undo()
    assert reads == [("item", ()), ("cpu", (4,))], reads


def test_store_loader_and_model(cuda):
    imgs = _dev(np.stack([cases.texture(48, 64, s) for s in (1, 2, 3)]), cuda)
    batch = SiftExtractor(32, 1.6).nodes_from_batch(imgs, LABELS)
    store = batch.to_store()
    assert isinstance(store, GraphStore) and len(store) == 3
    assert store.x.data_ptr() == batch.x.data_ptr() and store.pos.data_ptr() == batch.pos.data_ptr()
    assert store.y_host.tolist() == LABELS
    listed = GraphStore.from_list([batch[b] for b in range(3)])
    assert torch.equal(listed.x, store.x) and torch.equal(listed.pos, store.pos)
    assert torch.equal(listed.ptr_host, store.ptr_host)
    torch.manual_seed(0)
    model = SetTransformer(128, 32, 5, num_inducing_points=4, heads=2).to(cuda).eval()
    seen = []
    for got in GraphLoader(store, 2, transform=KNNGraph(k=6, loop=True)):
        n = got.x.size(0)
        assert got.edge_index.shape == (2, 6 * n) and got.x.shape == (n, 128)
        assert int(got.edge_index.max()) < n
        with torch.no_grad():
            logits = model(got.x, got.batch, got.num_graphs)
        assert logits.shape == (got.num_graphs, 5) and torch.isfinite(logits).all()
        seen += got.ids.tolist()
    assert seen == [0, 1, 2]


def test_graph_transforms_take_sift_nodes(cuda):
    nodes = SiftExtractor(32, 1.6).nodes_from_image(_dev(cases.texture(48, 64, 1), cuda), 1)
    n = nodes.x.size(0)
    nodes = KNNGraph(k=4, loop=False)(nodes)
    assert nodes.edge_index.shape == (2, 4 * n)
    nodes = GaussianDistance(sigma=10.0, save_as=SaveAs.EDGE_ATTR_REPLACE)(nodes)
    assert nodes.edge_attr is not None and nodes.edge_attr.size(0) == 4 * n
    other = SiftExtractor(32, 1.6).nodes_from_image(_dev(cases.texture(48, 64, 1), cuda), 1)
    other = RadiusGraph(r=12.0)(other)
    assert other.edge_index.size(0) == 2 and int(other.edge_index.max()) < n


def test_call_decodes_with_pil(cuda, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    image = cases.texture(48, 64, 1)
    path = tmp_path / "fundus_7.png"
    Image.fromarray(image).save(path)
    ex = SiftExtractor(16, 1.6)
    got = ex(path, 3)
    want = ex.nodes_from_image(_dev(image, cuda), 3, name="fundus_7")
    assert got.name == "fundus_7" and got.y.tolist() == [3]
    for field in ("x", "pos", "score"):
        assert torch.equal(getattr(got, field), getattr(want, field))
