"""The batch entries of the lesion-node chain (csrc/ccl_batch.hip, csrc/ccpool_resample.hip)
against the CPU restatement tests/ccl_ref.py applied per image and concatenated.

label_pool_batch, ccl_batch and ccl_stats_batch are exact. cc_pool_resample pools a bilinear
resampling it never stores; it is compared with F.interpolate + the reference's scatter in
float64, and held per node to the rule of tests/test_gpu_lesion_nodes.py:
    |got - x64| <= max(2 * max over the node's channels of |x32 - x64|, 1e-6 * max|x64|)
where x32 is the same restatement in fp32 (torch's fp32 interpolate, then the fp32 pool). Per
node, not per element: the fused path rounds in other places than the restatement, so an element
where the restatement happens to be nearly exact bounds nothing. Bit-equality with torch's
interpolate is not asked for (its own fp32 tap weights are off by up to ~18 * 2^-24 * max|f| at
non-dyadic scales), except with identity taps, where max and the counts are exact.
Measured on one MI355X (printed by the tests): see DESIGN §4.5."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle.pyg_ref as ref
from lesion_gnn_amd import ops
from lesion_gnn_amd.datasets.nodes import lesions
from tests import ccl_cases as cases
from tests import ccl_ref

pytestmark = pytest.mark.gpu


# ---- label_pool_batch --------------------------------------------------------------------------

@pytest.mark.parametrize("src,dst", [((7, 9), (3, 4)), ((3, 4), (5, 5))])
def test_label_pool_batch(cuda, src, dst):
    z = torch.randn(2, 5, *src, generator=torch.Generator().manual_seed(src[0]))
    got = ops.label_pool_batch(z.to(cuda), dst)
    assert got.dtype == torch.uint8 and got.shape == (2, *dst)
    for b in range(2):
        assert torch.equal(got[b].cpu(), ccl_ref.label_pool(z[b], dst))


# ---- ccl_batch, ccl_stats_batch ------------------------------------------------------------------

H9, W67 = 9, 67  # rows wider than a wave; 603 pixels: a flat 1024-pixel block straddles images


@functools.lru_cache(maxsize=None)
def _ccl_images():
    """An all-foreground image between one whose last row and one whose first row are foreground
    (a union across an image border would join them), an all-background one, a blob map."""
    imgs = np.zeros((5, H9, W67), dtype=np.uint8)
    imgs[0, -1] = 1
    imgs[0, 2, 3:40] = 2
    imgs[1] = 1
    imgs[2, 0] = 3
    imgs[2, 4:6, 60:] = 1
    imgs[4] = cases.blob_classes(H9, W67, 14, seed=5).numpy().astype(np.uint8)
    imgs[4, 0, ::2] = 1  # isolated pixels in its first row
    return imgs


@functools.lru_cache(maxsize=None)
def _ccl_expected(connectivity):
    """Per image (nlabel, labels, stats, centroids) of the restatement."""
    return [ccl_ref.connected_components_with_stats(im, connectivity) for im in _ccl_images()]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_ccl_batch(cuda, connectivity):
    imgs = torch.from_numpy(_ccl_images()).to(cuda)
    want = _ccl_expected(connectivity)
    labels, num, ptr = ops.ccl_batch(imgs, connectivity)
    assert labels.dtype == torch.int64 and labels.shape == imgs.shape
    assert num.dtype == torch.int32 and ptr.dtype == torch.int64
    nl = [w[0] for w in want]
    assert nl[3] == 1 and nl[1] == 2
    assert num.tolist() == nl
    assert ptr.tolist() == [0] + np.cumsum(nl).tolist()
    for b, w in enumerate(want):
        assert torch.equal(labels[b].cpu(), torch.from_numpy(w[1])), b
        one, n1, p1 = ops.ccl_batch(imgs[b:b + 1], connectivity)
        single, ns = ops.ccl(imgs[b], connectivity)
        assert torch.equal(one[0], single) and n1.tolist() == ns.tolist() == [w[0]]
        assert p1.tolist() == [0, w[0]]
    again = ops.ccl_batch(imgs, connectivity)
    assert all(torch.equal(a, b) for a, b in zip((labels, num, ptr), again))


@functools.lru_cache(maxsize=None)
def _tiny_images():
    """2049 seeded 8 x 8 images (one root-count block each), a third of the pixels foreground,
    every 7th image empty, and their component counts by the restatement (8-connectivity)."""
    rng = np.random.default_rng(11)
    imgs = (rng.random((2049, 8, 8)) < 0.33).astype(np.uint8) * rng.integers(1, 4, (2049, 8, 8),
                                                                               dtype=np.uint8)
    imgs[::7] = 0
    return imgs, [ccl_ref.connected_components_with_stats(im, 8)[:2] for im in imgs]


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_ccl_batch_scan_lengths(cuda, B):
    """k_ccl_scan over B block counts, at the wave edge, the tile edge (1024) and with a carry
    over two tiles: num_labels, node_ptr and the labels of the first B tiny images."""
    imgs, want = _tiny_images()
    labels, num, ptr = ops.ccl_batch(torch.from_numpy(imgs[:B]).to(cuda), 8)
    nl = [w[0] for w in want[:B]]
    assert len(set(nl)) > 1 or B == 1
    assert num.tolist() == nl
    assert ptr.tolist() == [0] + np.cumsum(nl).tolist()
    assert torch.equal(labels.cpu(), torch.from_numpy(np.stack([w[1] for w in want[:B]])))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_ccl_stats_batch(cuda, connectivity):
    imgs = torch.from_numpy(_ccl_images()).to(cuda)
    want = _ccl_expected(connectivity)
    labels, _, ptr = ops.ccl_batch(imgs, connectivity)
    total = sum(w[0] for w in want)
    stats, cent = ops.ccl_stats_batch(labels, ptr, total)
    assert stats.dtype == torch.int32 and cent.dtype == torch.float64
    assert torch.equal(stats.cpu(), torch.from_numpy(np.concatenate([w[2] for w in want])))
    assert torch.equal(cent.cpu(), torch.from_numpy(np.concatenate([w[3] for w in want])))


def test_ccl_stats_batch_counts_labels_outside_their_image(cuda):
    labels = torch.zeros(2, 4, 4, dtype=torch.int64, device=cuda)
    labels[0, 0, 0] = 1
    labels[1, 1, 1] = 2  # image 1 owns one row
    ptr = torch.tensor([0, 2, 3], device=cuda)
    with pytest.raises(IndexError, match="1 labels"):
        ops.ccl_stats_batch(labels, ptr, 3)
    stats, _ = ops.ccl_stats_batch(labels, ptr, 3, validate=False)
    assert stats[:, 4].tolist() == [15, 1, 15]


# ---- cc_pool_resample ---------------------------------------------------------------------------

# (h, w) -> (H, W), C
RESAMPLE = {
    "dyadic": ((24, 24), (48, 48), 16),
    "nondyadic": ((10, 12), (48, 40), 5),
    "down": ((24, 24), (16, 18), 16),
    "identity": ((16, 16), (16, 16), 8),
    "wide": ((16, 16), (32, 32), 1024),
}


@functools.lru_cache(maxsize=None)
def _components(size, seeds):
    """Per image (nlabel, labels) of a blob map, and the node offsets."""
    out = [ccl_ref.label(cases.blob_classes(*size, 12, seed=s).numpy(), 8) for s in seeds]
    return out, [0] + np.cumsum([n for n, _ in out]).tolist()


def _pool_ref(feats, comps, reduce):
    """F.interpolate'd feats (B, C, H, W) pooled per image by the reference's scatter (nlabel
    passed as 2: the scatter, never the one-node shortcut)."""
    return torch.cat([ref.extract_features_by_cc(torch.from_numpy(lab), feats[b:b + 1], 2, reduce)
                      for b, (_, lab) in enumerate(comps)])


@functools.lru_cache(maxsize=None)
def _resample_case(case, reduce):
    src, dst, C = RESAMPLE[case]
    comps, ptr = _components(dst, (21, 22))
    feats = torch.randn(2, C, *src, generator=torch.Generator().manual_seed(C + src[0]))
    kw = dict(size=dst, mode="bilinear", align_corners=False)
    x32 = _pool_ref(F.interpolate(feats, **kw), comps, reduce)
    x64 = _pool_ref(F.interpolate(feats.double(), **kw), comps, reduce)
    return feats, comps, ptr, x32, x64


def _assert_rule(got, x32, x64, what):
    ref_err = (x32.double() - x64).abs()
    err = (got.double() - x64).abs()
    bound = torch.clamp(2 * ref_err.amax(1, keepdim=True), min=1e-6 * float(x64.abs().max()))
    print(f"{what}: max err {float(err.max()):.3e}, restatement's {float(ref_err.max()):.3e}, "
          f"largest err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (float(err.max()), float(ref_err.max()))


def _device_inputs(cuda, feats, comps, ptr):
    labels = torch.from_numpy(np.stack([lab for _, lab in comps])).to(cuda)
    return feats.to(cuda), labels, torch.tensor(ptr, dtype=torch.int64, device=cuda)


@pytest.mark.parametrize("tight", [False, True], ids=["bins4032", "tight"])
@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("case", list(RESAMPLE))
def test_cc_pool_resample(cuda, case, reduce, tight):
    """tight: max_nodes as small as the batch allows (four channels per workgroup where there
    are four); else the default 4032 bins (one channel per workgroup, more than 64 KB of LDS)."""
    feats, comps, ptr, x32, x64 = _resample_case(case, reduce)
    f, labels, node_ptr = _device_inputs(cuda, feats, comps, ptr)
    nmax = max(n for n, _ in comps) if tight else None
    run = lambda: ops.cc_pool_resample(f, labels, node_ptr, ptr[-1], reduce == "max",  # noqa: E731
                                       max_nodes=nmax, return_counts=True)
    got, counts = run()
    assert got.dtype == torch.float32 and got.shape == x32.shape
    want_counts = np.concatenate([np.bincount(lab.reshape(-1), minlength=n) for n, lab in comps])
    assert counts.tolist() == want_counts.tolist()
    if case == "identity" and reduce == "max":
        assert torch.equal(got.cpu(), x32)
    _assert_rule(got.cpu(), x32, x64, f"{case} {reduce} {'tight' if tight else '4032'}")
    again, _ = run()
    assert torch.equal(got, again)


@functools.lru_cache(maxsize=None)
def _dotted():
    """64 x 64: image 0 is a grid of 1024 isolated dots (1025 nodes: past 1024 LDS bins), image
    1 a blob map."""
    dots = cases.images(64, 64)["dots"]
    comps = [ccl_ref.label(dots, 8), ccl_ref.label(cases.blob_classes(64, 64, 12, 31).numpy(), 8)]
    assert comps[0][0] == 1025
    feats = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(64))
    return feats, comps, [0, 1025, 1025 + comps[1][0]]


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_cc_pool_resample_1025_nodes(cuda, reduce):
    feats, comps, ptr = _dotted()
    x32 = _pool_ref(feats, comps, reduce)
    x64 = _pool_ref(feats.double(), comps, reduce)
    f, labels, node_ptr = _device_inputs(cuda, feats, comps, ptr)
    for nmax in (None, 1025):
        got, counts = ops.cc_pool_resample(f, labels, node_ptr, ptr[-1], reduce == "max",
                                           max_nodes=nmax, return_counts=True)
        want = np.concatenate([np.bincount(lab.reshape(-1), minlength=n) for n, lab in comps])
        assert counts.tolist() == want.tolist()
        if reduce == "max":
            assert torch.equal(got.cpu(), x32)
        _assert_rule(got.cpu(), x32, x64, f"dotted {reduce} max_nodes={nmax}")
        assert torch.equal(got, ops.cc_pool_resample(f, labels, node_ptr, ptr[-1],
                                                     reduce == "max", max_nodes=nmax))


def test_cc_pool_resample_refuses_and_counts(cuda):
    feats, comps, ptr = _dotted()
    f, labels, node_ptr = _device_inputs(cuda, feats, comps, ptr)
    with pytest.raises(ValueError, match="4032"):
        ops.cc_pool_resample(f, labels, node_ptr, ptr[-1], False, max_nodes=4033)
    with pytest.raises(ValueError, match="65536"):  # a 129 x 128 source map to stage
        ops.cc_pool_resample(torch.zeros(2, 1, 129, 128, device=cuda), labels, node_ptr, ptr[-1],
                             False)
    with pytest.raises(IndexError, match="labels outside"):  # bins for fewer nodes than there are
        ops.cc_pool_resample(f, labels, node_ptr, ptr[-1], False, max_nodes=1000)


def test_more_components_than_cc_pool_resample_takes(cuda):
    cls = torch.zeros(2, 128, 128, dtype=torch.int64)
    cls[1, ::2, ::2] = 1  # 4096 dots in image 1
    logits = torch.cat([cases.logits_of(c, 5, 0) for c in cls]).to(cuda)
    ex = lesions.LesionsExtractor(lesions.LesionsNodesConfig(
        feature_source=lesions.SegmentationEncoderFeatures(layer=4)))
    with pytest.raises(ValueError, match="image 1: 4097 .*4032"):
        ex.nodes_from_batch(logits, torch.zeros(2, 1, 128, 128, device=cuda), [0, 0])
