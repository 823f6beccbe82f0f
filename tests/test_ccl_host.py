"""Host-side surface of the lesion-node addition (no GPU): the header entries, their argument
checks (which run before any launch), the workspace size, and what raises."""
import pytest
import torch

from lesion_gnn_amd import _lib, ops
from lesion_gnn_amd.datasets.nodes import lesions

ENTRIES = ("lgnn_label_pool", "lgnn_ccl", "lgnn_ccl_workspace_bytes", "lgnn_ccl_stats")


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 40
    assert _lib.load().lgnn_abi_version() == 40


def test_header_entries_are_exported_and_bound():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert [c for c, _ in _lib.PARAMS["lgnn_ccl"]][:1] == ["const uint8_t*"]
    assert _lib.LGNN_CC_POOL_MAX_SEGMENTS == 4032


def test_uint8_pointers_take_uint8_tensors_only():
    img = torch.zeros(4, 4, dtype=torch.uint8)
    assert _lib.marshal("lgnn_ccl", (img, 4, 4, 8, None, None, None, 0, None))[0] == img.data_ptr()
    with pytest.raises(_lib.LgnnError, match="uint8_t"):
        _lib.marshal("lgnn_ccl", (img.float(), 4, 4, 8, None, None, None, 0, None))


def test_bad_arguments_return_einval_before_any_launch():
    lib = _lib.load()
    E = _lib.LGNN_EINVAL
    assert E == -22
    b = torch.zeros(1 << 16, dtype=torch.uint8)  # host memory: never dereferenced
    p, n = b.data_ptr(), b.numel()
    # lgnn_ccl(image, H, W, connectivity, labels, num_labels, workspace, bytes, stream)
    assert lib.lgnn_ccl(p, 4, 4, 6, p, p, p, n, None) == E          # connectivity
    assert lib.lgnn_ccl(p, 0, 4, 8, p, p, p, n, None) == E          # H = 0
    assert lib.lgnn_ccl(p, 4, -1, 8, p, p, p, n, None) == E         # W < 0
    assert lib.lgnn_ccl(p, 1 << 16, 1 << 15, 8, p, p, p, n, None) == E  # H * W = 2^31
    assert lib.lgnn_ccl(None, 4, 4, 8, p, p, p, n, None) == E
    assert lib.lgnn_ccl(p, 4, 4, 8, None, p, p, n, None) == E
    assert lib.lgnn_ccl(p, 4, 4, 8, p, None, p, n, None) == E
    assert lib.lgnn_ccl(p, 4, 4, 8, p, p, None, n, None) == E
    assert lib.lgnn_ccl(p, 4, 4, 4, p, p, p, 8, None) == E          # workspace too small
    # lgnn_ccl_stats(labels, H, W, num_labels, stats, centroids, err, stream)
    assert lib.lgnn_ccl_stats(p, 0, 4, 2, p, p, p, None) == E
    assert lib.lgnn_ccl_stats(p, 1 << 15, 1 << 16, 2, p, p, p, None) == E
    assert lib.lgnn_ccl_stats(p, 4, 4, 0, p, p, p, None) == E       # no label at all
    assert lib.lgnn_ccl_stats(None, 4, 4, 2, p, p, p, None) == E
    assert lib.lgnn_ccl_stats(p, 4, 4, 2, None, p, p, None) == E
    assert lib.lgnn_ccl_stats(p, 4, 4, 2, p, None, p, None) == E
    assert lib.lgnn_ccl_stats(p, 4, 4, 2, p, p, None, None) == E
    # lgnn_label_pool(logits, K, Hin, Win, out, H, W, stream)
    assert lib.lgnn_label_pool(p, 0, 4, 4, p, 2, 2, None) == E
    assert lib.lgnn_label_pool(p, 256, 4, 4, p, 2, 2, None) == E    # a class must fit a byte
    assert lib.lgnn_label_pool(p, 5, 0, 4, p, 2, 2, None) == E
    assert lib.lgnn_label_pool(p, 5, 4, 4, p, 2, 0, None) == E
    assert lib.lgnn_label_pool(p, 5, 4, 4, p, 1 << 16, 1 << 15, None) == E
    assert lib.lgnn_label_pool(None, 5, 4, 4, p, 2, 2, None) == E
    assert lib.lgnn_label_pool(p, 5, 4, 4, None, 2, 2, None) == E


def test_workspace_bytes_positive_and_monotone():
    ws = _lib.load().lgnn_ccl_workspace_bytes
    sizes = [1, 2, 31, 64, 65, 512, 1000]
    for h in sizes:
        for w in sizes:
            assert ws(h, w) >= 2 * 4 * h * w  # the parent and root-label words
    for a, b in zip(sizes, sizes[1:]):
        for o in sizes:
            assert ws(a, o) <= ws(b, o) and ws(o, a) <= ws(o, b)
    assert ws(0, 4) == 0 and ws(1 << 16, 1 << 15) == 0  # sizes lgnn_ccl refuses


def test_cpu_tensors_raise():
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.label_pool(torch.zeros(5, 4, 4), (2, 2))
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.ccl(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.ccl_stats(torch.zeros(4, 4, dtype=torch.int64), 1)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        lesions.connected_components_with_stats(torch.zeros(4, 4))


def _extractor(**kw):
    cfg = lesions.LesionsNodesConfig(
        feature_source=lesions.SegmentationEncoderFeatures(layer=4), **kw)
    return lesions.LesionsExtractor(cfg)


def test_extractor_constructor_and_repr():
    ex = _extractor(features_reduction="max", reinterpolation=(512, 512), compile=True)
    assert ex.features_reduction is lesions.FeaturesReduction.MAX
    assert ex.reinterpolation == (512, 512)
    assert repr(ex) == ("LesionsExtractor(feature_source="
                        "SegmentationEncoderFeatures(layer=4))")
    assert _extractor().features_reduction is lesions.FeaturesReduction.MEAN


def test_extractor_call_points_to_nodes_from_maps():
    with pytest.raises(NotImplementedError, match="nodes_from_maps"):
        _extractor()("image.png", 0)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        _extractor().nodes_from_maps(torch.zeros(1, 5, 8, 8), torch.zeros(1, 3, 4, 4), 0)


def test_lesion_nodes_is_the_transforms_duck_type():
    d = lesions.LesionNodes(pos=torch.zeros(2, 2, dtype=torch.float64), x=torch.zeros(2, 3),
                            y=torch.tensor([1]))
    assert d.name is None and d.edge_index is None and d.edge_attr is None
    assert hasattr(d, "edge_attr") and not hasattr(d, "batch")
