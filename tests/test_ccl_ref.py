"""tests/ccl_ref.py (the CPU restatement the GPU connected-component tests compare against) pinned
by hand-written answers and against scipy.ndimage.label."""
import numpy as np
import pytest
import torch

from tests import ccl_cases as cases
from tests import ccl_ref


def _check(img, connectivity, nlabel, labels, stats, centroids):
    n, lab, st, ce = ccl_ref.connected_components_with_stats(np.array(img, dtype=np.uint8),
                                                              connectivity)
    assert n == nlabel
    assert lab.dtype == np.int64 and lab.tolist() == labels
    assert st.dtype == np.int32 and st.tolist() == stats
    assert ce.dtype == np.float64 and ce.tolist() == centroids


DIAG = [[1, 0, 0],
        [0, 1, 0],
        [0, 0, 0]]


def test_diagonal_touch_is_one_component_at_8():
    _check(DIAG, 8, 2, [[1, 0, 0], [0, 1, 0], [0, 0, 0]],
           [[0, 0, 3, 3, 7], [0, 0, 2, 2, 2]], [[8 / 7, 8 / 7], [0.5, 0.5]])


def test_diagonal_touch_is_two_components_at_4():
    _check(DIAG, 4, 3, [[1, 0, 0], [0, 2, 0], [0, 0, 0]],
           [[0, 0, 3, 3, 7], [0, 0, 1, 1, 1], [1, 1, 1, 1, 1]],
           [[8 / 7, 8 / 7], [0.0, 0.0], [1.0, 1.0]])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_u_is_numbered_by_its_first_pixel(connectivity):
    """The arms meet only in the last row, after the dot between them has been seen: the right
    arm still belongs to component 1 and the dot is component 2."""
    img = [[1, 0, 0, 0, 1],
           [1, 0, 1, 0, 1],
           [1, 0, 0, 0, 1],
           [1, 1, 1, 1, 1]]
    _check(img, connectivity, 3,
           [[1, 0, 0, 0, 1], [1, 0, 2, 0, 1], [1, 0, 0, 0, 1], [1, 1, 1, 1, 1]],
           [[1, 0, 3, 3, 8], [0, 0, 5, 4, 11], [2, 1, 1, 1, 1]],
           [[2.0, 1.0], [2.0, 21 / 11], [2.0, 1.0]])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_touching_classes_are_one_component(connectivity):
    _check([[1, 2, 0], [0, 0, 0], [0, 3, 3]], connectivity, 3,
           [[1, 1, 0], [0, 0, 0], [0, 2, 2]],
           [[0, 0, 3, 3, 5], [0, 0, 2, 1, 2], [1, 2, 2, 1, 2]],
           [[1.0, 1.0], [0.5, 0.0], [1.5, 2.0]])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_all_zero_and_all_one(connectivity):
    _check([[0, 0, 0], [0, 0, 0]], connectivity, 1, [[0, 0, 0], [0, 0, 0]],
           [[0, 0, 3, 2, 6]], [[1.0, 0.5]])
    # the background keeps label 0 when no pixel carries it: a row of zeros
    _check([[1, 1, 1], [1, 1, 1]], connectivity, 2, [[1, 1, 1], [1, 1, 1]],
           [[0, 0, 0, 0, 0], [0, 0, 3, 2, 6]], [[0.0, 0.0], [1.0, 0.5]])


def test_wide_image_known_answer():
    """6 x 7, 8-connectivity: a component found late in the raster (its first pixel in row 1)
    that swallows pixels seen before it would be under a two-pass scheme."""
    img = [[0, 0, 0, 1, 0, 0, 4],
           [1, 0, 1, 0, 0, 0, 4],
           [0, 1, 0, 0, 0, 0, 0],
           [0, 0, 0, 0, 2, 2, 0],
           [3, 0, 0, 0, 2, 0, 0],
           [3, 3, 0, 0, 0, 0, 1]]
    _check(img, 8, 6,
           [[0, 0, 0, 1, 0, 0, 2],
            [1, 0, 1, 0, 0, 0, 2],
            [0, 1, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 3, 3, 0],
            [4, 0, 0, 0, 3, 0, 0],
            [4, 4, 0, 0, 0, 0, 5]],
           [[0, 0, 7, 6, 29], [0, 0, 4, 3, 4], [6, 0, 1, 2, 2], [4, 3, 2, 2, 3], [0, 4, 2, 2, 3],
            [6, 5, 1, 1, 1]],
           [[88 / 29, 71 / 29], [1.5, 1.0], [6.0, 0.5], [13 / 3, 10 / 3], [1 / 3, 14 / 3],
            [6.0, 5.0]])


@pytest.mark.parametrize("size", [(1, 1), (1, 70), (70, 1), (33, 31), (65, 63), (130, 257)])
def test_against_scipy(size):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, img in cases.images(*size).items():
        for connectivity, rank in ((4, 1), (8, 2)):
            want, m = ndimage.label(img, ndimage.generate_binary_structure(2, rank))
            n, got = ccl_ref.label(img, connectivity)
            assert n == m + 1 and np.array_equal(got, want), (name, connectivity)


def test_case_images_are_what_they_claim():
    im = cases.images(37, 53)
    assert ccl_ref.label(im["checkerboard"], 8)[0] == 2
    assert ccl_ref.label(im["checkerboard"], 4)[0] == (37 * 53 + 1) // 2 + 1
    assert ccl_ref.label(im["dots"], 8)[0] == 19 * 27 + 1
    assert ccl_ref.label(im["serpentine"], 4)[0] == 2
    assert ccl_ref.label(im["spiral"], 8)[0] == 2 and im["spiral"].sum() > 37 * 53 // 3
    assert ccl_ref.label(im["combs"], 8)[0] == 3
    assert ccl_ref.label(im["rings"], 8)[0] == 10 + 1  # rings at depths 0, 2, ..., 18
    assert int(im["classes"].max()) == 4


def test_label_pool_windows_match_torch_on_upsampling():
    """adaptive_max_pool2d's windows, [floor(i Hin / H), ceil((i + 1) Hin / H)), restated."""
    z = torch.rand(5, 8, 8, generator=torch.Generator().manual_seed(0))
    am = z.argmax(0)
    got = ccl_ref.label_pool(z, (16, 11))
    for i in range(16):
        for j in range(11):
            win = am[i * 8 // 16:-(-(i + 1) * 8 // 16), j * 8 // 11:-(-(j + 1) * 8 // 11)]
            assert int(got[i, j]) == int(win.max())


def test_lesion_nodes_ref_single_node():
    z = cases.logits_of(torch.zeros(8, 8, dtype=torch.int64), 5, 0)
    f = torch.rand(1, 3, 4, 4, generator=torch.Generator().manual_seed(1))
    pos, x, y = ccl_ref.lesion_nodes_ref(z, f, 2, "max")
    assert pos.tolist() == [[3.0, 3.0]]  # (1.5, 1.5) * 8 / 4
    torch.testing.assert_close(x, torch.cat([f.mean((2, 3)), torch.zeros(1, 1)], 1))
    assert y.tolist() == [2]
