"""Connected-component labelling, component statistics and the class-map pooling on the GPU
(csrc/ccl.hip) against the CPU restatement tests/ccl_ref.py: labels, nlabel and stats equal,
centroids bit-equal, for connectivity 4 and 8, on images that put components across every border
and corner of whatever tiling the kernels use."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lesion_gnn_amd import ops
from lesion_gnn_amd.datasets.nodes.lesions import connected_components_with_stats
from tests import ccl_cases as cases
from tests import ccl_ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _images(size):
    return cases.images(*size)


@functools.lru_cache(maxsize=None)
def _expected(size, name, connectivity):
    """Computed once per module and shared (read-only) by the tests that need it."""
    return ccl_ref.connected_components_with_stats(_images(size)[name], connectivity)


def _run(img, connectivity, cuda):
    n, cc, stats, centroids = connected_components_with_stats(torch.from_numpy(img).to(cuda),
                                                              connectivity)
    return n, cc.cpu(), stats.cpu(), centroids.cpu()


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ccl_matches_the_restatement(cuda, size, connectivity):
    for name, img in _images(size).items():
        n, cc, stats, centroids = _run(img, connectivity, cuda)
        wn, wcc, wstats, wcent = _expected(size, name, connectivity)
        assert n == wn, (name, n, wn)
        assert cc.dtype == torch.int64 and cc.shape == img.shape
        assert torch.equal(cc, torch.from_numpy(wcc)), name
        assert stats.dtype == torch.int32 and torch.equal(stats, torch.from_numpy(wstats)), name
        assert centroids.dtype == torch.float64
        assert torch.equal(centroids, torch.from_numpy(wcent)), name


@pytest.mark.parametrize("connectivity", [4, 8])
def test_runs_of_hundreds_of_segments(cuda, connectivity):
    """Rows far wider than the 64 pixels one wave labels at once: a run's segments are linked one
    by one in any order."""
    size = (3, 20001)
    for name in ("ones", "rows", "serpentine", "noise0.9"):
        n, cc, stats, centroids = _run(_images(size)[name], connectivity, cuda)
        wn, wcc, wstats, wcent = _expected(size, name, connectivity)
        assert n == wn and torch.equal(cc, torch.from_numpy(wcc)), name
        assert torch.equal(stats, torch.from_numpy(wstats)), name
        assert torch.equal(centroids, torch.from_numpy(wcent)), name


def test_component_counts_of_the_regular_images(cuda):
    """The counts the images were chosen for, stated without the restatement."""
    H, W = 65, 63
    im = _images((H, W))
    for name, connectivity, want in [
            ("zeros", 8, 1), ("ones", 4, 2), ("checkerboard", 8, 2),
            ("checkerboard", 4, (H * W + 1) // 2 + 1), ("dots", 8, 33 * 32 + 1),
            ("rows", 8, 33 + 1), ("columns", 4, 32 + 1), ("serpentine", 4, 2), ("spiral", 4, 2),
            ("combs", 8, 3), ("rings", 8, 16 + 1)]:
        labels, num = ops.ccl(torch.from_numpy(im[name]).to(cuda), connectivity)
        assert int(num) == want, (name, connectivity)
        assert int(labels.max()) == want - 1


@pytest.mark.parametrize("connectivity", [4, 8])
def test_two_calls_give_equal_outputs(cuda, connectivity):
    for name in ("noise0.41", "spiral", "dots"):
        img = _images((512, 512))[name]
        a, b = _run(img, connectivity, cuda), _run(img, connectivity, cuda)
        assert a[0] == b[0] == _expected((512, 512), name, connectivity)[0]
        assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])), name


def test_input_dtypes_are_cast_like_byte(cuda):
    img = _images((37, 53))["classes"]
    want = _expected((37, 53), "classes", 8)
    for t in (torch.from_numpy(img), torch.from_numpy(img != 0), torch.from_numpy(img).long(),
              torch.from_numpy(img).float() + 0.0):
        n, cc, _, _ = connected_components_with_stats(t.to(cuda))
        assert n == want[0] and torch.equal(cc.cpu(), torch.from_numpy(want[1]))
    # .byte() truncates: 0.5 is background
    n, _, _, _ = connected_components_with_stats(torch.full((4, 4), 0.5, device=cuda))
    assert n == 1


def test_stats_count_out_of_range_labels(cuda):
    lab = torch.tensor([[0, 1, 7], [-2, 1, 0]], device=cuda)
    with pytest.raises(IndexError, match="2 labels outside"):
        ops.ccl_stats(lab, 2)
    stats, centroids = ops.ccl_stats(lab, 2, validate=False)  # the others are still counted
    assert stats.cpu().tolist() == [[0, 0, 3, 2, 2], [1, 0, 1, 2, 2]]
    assert centroids.cpu().tolist() == [[1.0, 0.5], [1.0, 0.5]]


def test_stats_of_a_label_without_pixels_are_zero(cuda):
    lab = torch.tensor([[0, 2, 2]], device=cuda)
    stats, centroids = ops.ccl_stats(lab, 4)
    assert stats.cpu().tolist() == [[0, 0, 1, 1, 1], [0, 0, 0, 0, 0], [1, 0, 2, 1, 2],
                                    [0, 0, 0, 0, 0]]
    assert centroids.cpu().tolist() == [[0.0, 0.0], [0.0, 0.0], [1.5, 0.0], [0.0, 0.0]]


def test_stats_of_labels_past_the_shared_memory_bins(cuda):
    """More labels than a workgroup keeps bins for (the dots image at 130 x 257: 8386), each
    component one pixel: stats straight from the image."""
    size = (130, 257)
    n, cc, stats, centroids = _run(_images(size)["dots"], 8, cuda)
    assert n == 65 * 129 + 1
    ys, xs = np.nonzero(_images(size)["dots"])
    assert torch.equal(stats[1:, 0], torch.from_numpy(xs).int())
    assert torch.equal(stats[1:, 1], torch.from_numpy(ys).int())
    assert bool((stats[1:, 2:] == 1).all())
    assert torch.equal(centroids[1:], torch.from_numpy(np.stack([xs, ys], 1)).double())


@pytest.mark.parametrize("src,dst", [((37, 53), (8, 8)), ((37, 53), (16, 11)),
                                     ((37, 53), (37, 53)), ((64, 64), (64, 64)),
                                     ((8, 8), (16, 16)), ((1024, 1024), (512, 512))])
def test_label_pool_equals_torch(cuda, src, dst):
    z = torch.randn(5, *src, generator=torch.Generator().manual_seed(src[0] + dst[1]))
    want = F.adaptive_max_pool2d(z.argmax(0, keepdim=True)[None].float(), dst)[0, 0].byte()
    got = ops.label_pool(z.to(cuda), dst)
    assert got.dtype == torch.uint8 and got.shape == dst
    assert torch.equal(got.cpu(), want)
    assert torch.equal(want, ccl_ref.label_pool(z, dst))


def test_label_pool_takes_the_first_of_equal_maxima(cuda):
    z = torch.randint(0, 3, (5, 37, 53), generator=torch.Generator().manual_seed(3)).float()
    assert int((z == z.max(0).values).sum(0).max()) > 1  # ties exist
    for dst in ((37, 53), (16, 11)):
        want = F.adaptive_max_pool2d(z.argmax(0, keepdim=True)[None].float(), dst)[0, 0].byte()
        assert torch.equal(ops.label_pool(z.to(cuda), dst).cpu(), want)
