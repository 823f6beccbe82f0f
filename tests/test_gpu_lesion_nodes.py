"""LesionsExtractor.nodes_from_maps (reference lesions.py:147-176 on the GPU) against the CPU
restatement tests/ccl_ref.lesion_nodes_ref, and the reference config's transform
(KNNGraph(k=6, loop=True)) on its result against the oracle's k-NN on the reference's positions.

pos is exact. x is exact for max; for mean it is held to the bound of
tests/test_gpu_drgnet.py::test_extract_features_by_cc: the error against the float64 restatement
is at most 2x the fp32 restatement's own error, or 1e-6 of the largest value (the sums run over up
to thousands of pixels in a different order). The restatement gets the same reinterpolated feature
tensor, so only the pooling is compared."""
import functools

import pytest
import torch
import torch.nn.functional as F

import oracle.pyg_ref as ref
from lesion_gnn_amd.datasets.nodes import lesions
from lesion_gnn_amd.knn import KNNGraph
from tests import ccl_cases as cases
from tests import ccl_ref

pytestmark = pytest.mark.gpu


def _extractor(reduce, reinterpolation=None):
    return lesions.LesionsExtractor(lesions.LesionsNodesConfig(
        feature_source=lesions.SegmentationEncoderFeatures(layer=4), features_reduction=reduce,
        reinterpolation=reinterpolation))


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(logits (1, 5, Horg, Worg), features (1, C, h, w), reinterpolation)"""
    if case == "interp":  # 96 x 96 logits, 16 features at 24 x 24 -> 48 x 48
        cls, C, fsize, re = cases.blob_classes(96, 96, 30, seed=11), 16, (24, 24), (48, 48)
    elif case == "wide":  # the reference's d_in = 1025 at 64 x 64, 40 blobs
        cls, C, fsize, re = cases.blob_classes(128, 128, 40, seed=12), 1024, (64, 64), None
    else:  # "background": nothing but class 0
        cls, C, fsize, re = torch.zeros(32, 32, dtype=torch.int64), 8, (16, 16), None
    feats = torch.randn(1, C, *fsize, generator=torch.Generator().manual_seed(C))
    return cases.logits_of(cls, 5, seed=C + 1), feats, re


@functools.lru_cache(maxsize=None)
def _expected(case, reduce, cuda):
    """The restatement in fp32 and float64 on the feature tensor the GPU interpolated."""
    logits, feats, re = _inputs(case)
    if re is not None:
        feats = F.interpolate(feats.to(cuda), size=re, mode="bilinear", align_corners=False).cpu()
    pos, x32, y = ccl_ref.lesion_nodes_ref(logits, feats, 3, reduce)
    _, x64, _ = ccl_ref.lesion_nodes_ref(logits, feats, 3, reduce, dtype=torch.float64)
    return pos, x32, x64, y


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("case", ["interp", "wide", "background"])
def test_nodes_from_maps(cuda, case, reduce):
    logits, feats, re = _inputs(case)
    pos, x32, x64, y = _expected(case, reduce, cuda)
    data = _extractor(reduce, re).nodes_from_maps(logits.to(cuda), feats.to(cuda), 3, name="im")
    n, C = pos.size(0), feats.size(1)
    assert (n == 1) == (case == "background") and n <= 4032
    assert data.pos.is_cuda and data.x.is_cuda
    assert data.pos.dtype == torch.float64 and torch.equal(data.pos.cpu(), pos)
    assert data.x.dtype == torch.float32 and data.x.shape == x32.shape == (n, C + 1)
    assert data.y.tolist() == y.tolist() == [3] and data.name == "im"
    assert data.edge_index is None and data.edge_attr is None
    got = data.x.cpu()
    if reduce == "max" and n > 1:
        assert torch.equal(got, x32)
        return
    ref_err = (x32.double() - x64).abs()
    err = (got.double() - x64).abs()
    bound = torch.maximum(2 * ref_err, torch.full_like(ref_err, 1e-6 * x64.abs().max().item()))
    print(f"{case} {reduce}: max err {float(err.max()):.3e}, restatement's "
          f"{float(ref_err.max()):.3e}")
    assert bool((err <= bound).all()), (float(err.max()), float(ref_err.max()))


@pytest.mark.parametrize("case", ["interp", "wide", "background"])
def test_knn_graph_of_the_nodes(cuda, case):
    """configs/config.py:47 on the extractor's output."""
    logits, feats, re = _inputs(case)
    pos = _expected(case, "mean", cuda)[0]
    data = _extractor("mean", re).nodes_from_maps(logits.to(cuda), feats.to(cuda), 0)
    data = KNNGraph(k=6, loop=True)(data)
    assert torch.equal(data.edge_index.cpu(), ref.knn_graph(pos, 6, loop=True))
    assert data.edge_attr is None


def test_more_components_than_cc_pool_takes(cuda):
    cls = torch.zeros(128, 128, dtype=torch.int64)
    cls[::2, ::2] = 1  # 4096 dots
    feats = torch.zeros(1, 1, 128, 128)
    with pytest.raises(ValueError, match="4032"):
        _extractor("mean").nodes_from_maps(cases.logits_of(cls, 5, 0).to(cuda), feats.to(cuda), 0)
