"""Host-side surface of the batched lesion-node entries (no GPU): the header declarations and
their binding, the argument checks that run before any launch, and what raises in Python."""
import pytest
import torch

from lesion_gnn_amd import _lib, ops
from lesion_gnn_amd.datasets.nodes import lesions

ENTRIES = ("lgnn_label_pool_batch", "lgnn_ccl_batch", "lgnn_ccl_batch_workspace_bytes",
           "lgnn_ccl_stats_batch", "lgnn_cc_pool_resample",
           "lgnn_cc_pool_resample_workspace_bytes")


def test_header_entries_are_exported_and_bound():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 40  # additions only
    assert _lib.LGNN_CC_POOL_RESAMPLE_MAX_SOURCE_BYTES == 65536
    assert [n for _, n in _lib.PARAMS["lgnn_ccl_batch"]] == [
        "image", "batch", "height", "width", "connectivity", "labels", "num_labels", "node_ptr",
        "workspace", "workspace_bytes", "stream"]
    assert [c for c, n in _lib.PARAMS["lgnn_cc_pool_resample"] if n == "node_ptr"] == \
        ["const int64_t*"]


def test_bad_arguments_return_einval_before_any_launch():
    lib = _lib.load()
    E = _lib.LGNN_EINVAL
    b = torch.zeros(1 << 16, dtype=torch.uint8)  # host memory: never dereferenced
    p, n = b.data_ptr(), b.numel()
    # lgnn_label_pool_batch(logits, B, K, Hin, Win, out, H, W, stream)
    assert lib.lgnn_label_pool_batch(p, 0, 5, 4, 4, p, 2, 2, None) == E
    assert lib.lgnn_label_pool_batch(p, 2, 256, 4, 4, p, 2, 2, None) == E
    assert lib.lgnn_label_pool_batch(p, 2, 5, 4, 4, p, 1 << 15, 1 << 15, None) == E  # B*H*W = 2^31
    assert lib.lgnn_label_pool_batch(None, 2, 5, 4, 4, p, 2, 2, None) == E
    assert lib.lgnn_label_pool_batch(p, 2, 5, 4, 4, None, 2, 2, None) == E
    # lgnn_ccl_batch(image, B, H, W, connectivity, labels, num_labels, node_ptr, ws, bytes, stream)
    assert lib.lgnn_ccl_batch(p, 2, 4, 4, 6, p, p, p, p, n, None) == E
    assert lib.lgnn_ccl_batch(p, 0, 4, 4, 8, p, p, p, p, n, None) == E
    assert lib.lgnn_ccl_batch(p, 2, 0, 4, 8, p, p, p, p, n, None) == E
    assert lib.lgnn_ccl_batch(p, 1 << 11, 1 << 10, 1 << 10, 8, p, p, p, p, n, None) == E
    assert lib.lgnn_ccl_batch(None, 2, 4, 4, 8, p, p, p, p, n, None) == E
    assert lib.lgnn_ccl_batch(p, 2, 4, 4, 8, None, p, p, p, n, None) == E
    assert lib.lgnn_ccl_batch(p, 2, 4, 4, 8, p, None, p, p, n, None) == E
    assert lib.lgnn_ccl_batch(p, 2, 4, 4, 8, p, p, None, p, n, None) == E
    assert lib.lgnn_ccl_batch(p, 2, 4, 4, 8, p, p, p, None, n, None) == E
    assert lib.lgnn_ccl_batch(p, 2, 4, 4, 8, p, p, p, p, 8, None) == E  # workspace too small
    # lgnn_ccl_stats_batch(labels, B, H, W, node_ptr, total, stats, centroids, err, stream)
    assert lib.lgnn_ccl_stats_batch(p, 0, 4, 4, p, 2, p, p, p, None) == E
    assert lib.lgnn_ccl_stats_batch(p, 2, 4, 4, p, 0, p, p, p, None) == E
    assert lib.lgnn_ccl_stats_batch(p, 2, 4, 4, None, 2, p, p, p, None) == E
    assert lib.lgnn_ccl_stats_batch(None, 2, 4, 4, p, 2, p, p, p, None) == E
    assert lib.lgnn_ccl_stats_batch(p, 2, 4, 4, p, 2, None, p, p, None) == E
    assert lib.lgnn_ccl_stats_batch(p, 2, 4, 4, p, 2, p, None, p, None) == E
    assert lib.lgnn_ccl_stats_batch(p, 2, 4, 4, p, 2, p, p, None, None) == E

    # lgnn_cc_pool_resample(features, B, C, h, w, labels, H, W, node_ptr, total, max_nodes,
    #                       reduce_max, out, counts_out, err, workspace, bytes, stream)
    def pool(f=p, B=2, C=3, h=4, w=4, lab=p, H=8, W=8, ptr=p, total=5, nmax=4, out=p, err=p,
             ws=p, nb=n):
        return lib.lgnn_cc_pool_resample(f, B, C, h, w, lab, H, W, ptr, total, nmax, 0, out,
                                         None, err, ws, nb, None)

    for bad in (dict(B=0), dict(C=0), dict(h=0), dict(W=-1), dict(total=0), dict(nmax=0),
                dict(nmax=4033), dict(f=None), dict(lab=None), dict(ptr=None), dict(out=None),
                dict(err=None), dict(ws=None), dict(nb=8),
                dict(h=129, w=128, H=256, W=256),   # a source map over the LDS budget to stage
                dict(B=1 << 11, H=1 << 10, W=1 << 10)):
        assert pool(**bad) == E, bad


def test_workspace_bytes():
    lib = _lib.load()
    assert lib.lgnn_ccl_batch_workspace_bytes(1, 37, 53) == lib.lgnn_ccl_workspace_bytes(37, 53)
    assert lib.lgnn_ccl_batch_workspace_bytes(3, 37, 53) >= 3 * 2 * 4 * 37 * 53
    assert lib.lgnn_ccl_batch_workspace_bytes(0, 4, 4) == 0
    assert lib.lgnn_ccl_batch_workspace_bytes(1 << 11, 1 << 10, 1 << 10) == 0
    ws = lib.lgnn_cc_pool_resample_workspace_bytes
    assert ws(2, 48, 40, 30) >= 30 * 4 + 2 * 48 * 40 * 2 + (48 + 40) * 16
    assert ws(0, 4, 4, 3) == 0 and ws(2, 4, 4, 0) == 0


def test_cpu_tensors_raise():
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.label_pool_batch(torch.zeros(2, 5, 4, 4), (2, 2))
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.ccl_batch(torch.zeros(2, 4, 4, dtype=torch.uint8))
    ptr = torch.tensor([0, 1, 2])
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.ccl_stats_batch(torch.zeros(2, 4, 4, dtype=torch.int64), ptr, 2)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.cc_pool_resample(torch.zeros(2, 3, 2, 2), torch.zeros(2, 4, 4, dtype=torch.int64),
                             ptr, 2, False)


def _extractor(**kw):
    cfg = lesions.LesionsNodesConfig(
        feature_source=lesions.SegmentationEncoderFeatures(layer=4), **kw)
    return lesions.LesionsExtractor(cfg)


def test_nodes_from_batch_raises(monkeypatch):
    ex = _extractor()
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ex.nodes_from_batch(torch.zeros(2, 5, 8, 8), torch.zeros(2, 3, 4, 4), [0, 1])
    # the shape checks, past the device check
    monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)
    with pytest.raises(ValueError, match=r"label_maps must be \(B, K, H, W\)"):
        ex.nodes_from_batch(torch.zeros(5, 8, 8), torch.zeros(2, 3, 4, 4), [0, 1])
    with pytest.raises(ValueError, match="2 images, features 3"):
        ex.nodes_from_batch(torch.zeros(2, 5, 8, 8), torch.zeros(3, 3, 4, 4), [0, 1])
    with pytest.raises(ValueError, match="3 labels for 2 images"):
        ex.nodes_from_batch(torch.zeros(2, 5, 8, 8), torch.zeros(2, 3, 4, 4), [0, 1, 2])
    with pytest.raises(ValueError, match="1 names for 2 images"):
        ex.nodes_from_batch(torch.zeros(2, 5, 8, 8), torch.zeros(2, 3, 4, 4), [0, 1], ["a"])


def test_nodes_from_maps_on_cpu_tensors_still_raises():
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        _extractor().nodes_from_maps(torch.zeros(1, 5, 8, 8), torch.zeros(1, 3, 4, 4), 0)


def test_lesion_nodes_batch_indexing():
    ptr = torch.tensor([0, 2, 2, 5])
    batch = lesions.LesionNodesBatch(
        x=torch.arange(15.).view(5, 3), pos=torch.zeros(5, 2, dtype=torch.float64),
        y=torch.tensor([4, 0, 1]), ptr=ptr, names=["a", "b", "c"])
    assert len(batch) == 3 and batch.ptr_host.tolist() == [0, 2, 2, 5]
    assert batch[0].x.tolist() == [[0., 1., 2.], [3., 4., 5.]] and batch[0].name == "a"
    assert batch[1].x.shape == (0, 3) and batch[1].y.tolist() == [0]
    assert batch[-1].x.shape == (3, 3) and batch[-1].name == "c"
    assert batch[2].x.data_ptr() == batch.x[2:].data_ptr()
    with pytest.raises(IndexError):
        batch[3]
