"""The float64 restatement tests/sift_ref.py itself: known answers (a constant image, two Gaussian
blobs), the committed fixture tests/golden/sift_48x64.npz, and the conditions the cases of
tests/sift_cases.py must meet so that the GPU tests can ask for equality."""
import os

import numpy as np
import pytest

from tests import sift_cases as cases
from tests import sift_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_48x64.npz")
TEXTURES = [f"texture{H}x{W}" for H, W in cases.TEXTURE_SIZES]


def test_constant_image_has_no_keypoints():
    out = sift_ref.extract(cases.constant(), 16, 1.6)
    # a plateau passes the 26-neighbour test wherever rounding left the DoG nonzero; the
    # refinement rejects every such candidate (det = 0)
    assert out["x"].shape == (0, 128) and out["pos"].shape == (0, 2) and out["score"].shape == (0,)


@pytest.mark.parametrize("s,cx,cy", cases.BLOBS)
def test_blob(s, cx, cy):
    """The strongest keypoint sits on the blob: within 0.1 px of its centre + 0.25 (the shift of
    the bilinear doubling, which OpenCV has too), its size within a factor 2^(1/3) of 2 s."""
    out = sift_ref.extract(cases.blob(s, cx, cy), 10000, 1.6)
    x, y, size = out["kf"][0, :3]
    print(f"blob s = {s} at ({cx}, {cy}): keypoint ({x:.3f}, {y:.3f}) size {size:.3f}")
    assert abs(x - (cx + 0.25)) < 0.1 and abs(y - (cy + 0.25)) < 0.1
    assert 2 * s / 2 ** (1 / 3) < size < 2 * s * 2 ** (1 / 3)
    assert out["score"][0] == out["score"].max()


def test_gray_weights():
    rgb = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 100]]], dtype=np.uint8)
    # the reference's RGB array read as BGR: red gets 0.114, blue 0.299
    assert sift_ref.gray(rgb).tolist() == [[29, 150, 76, 148]]
    g = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(sift_ref.gray(g), g)


def test_octaves_and_kernels():
    assert sift_ref.octave_dims(48, 64) == [(96, 128), (48, 64), (24, 32), (12, 16)]
    assert sift_ref.octave_dims(44, 52)[-1] == (11, 13)  # one interior row, repeated reflection
    assert sift_ref.octave_dims(37, 41) == [(74, 82), (37, 41), (18, 20)]
    assert len(sift_ref.octave_dims(96, 128)) == 5
    assert sift_ref.kernel_size(sift_ref.base_sigma(0.8)) == 3  # the 0.01 floor
    assert sift_ref.kernel_size(sift_ref.level_sigmas(1.6)[-1]) == 27
    assert sift_ref.reflect101(np.array([-14, -1, 0, 10, 11, 24]), 11).tolist() == [6, 1, 0, 10, 9, 4]
    w = sift_ref.gaussian_kernel(1.6)
    assert abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1])
    gb, db = sift_ref.level_bounds(48, 64, 1.6)
    assert 2e-3 < gb[0][5] < 4e-3 and db[0][0] == gb[0][0] + gb[0][1]


def test_select_keeps_ties_and_orders():
    kf = np.array([[1, 1, 2, 10, 0.5], [2, 2, 2, 10, 0.9], [1, 1, 2, 10, 0.5], [3, 3, 2, 10, 0.5],
                   [4, 4, 2, 10, 0.1]], dtype=np.float32)
    ki = np.zeros((5, 2), dtype=np.int32)
    out, _, order = sift_ref.select(kf, ki, 2)
    assert order.tolist() == [1, 0, 3]  # row 2 duplicates row 0; rows 0 and 3 tie at the cut
    assert out[:, 0].tolist() == [1.0, 0.5, 1.5]  # halved
    assert sift_ref.select(kf, ki, 10)[2].tolist() == [1, 0, 3, 4]


def test_solve3():
    A = [[2.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 4.0]]
    x = sift_ref.solve3(A, [1.0, 2.0, 3.0])
    assert np.allclose(np.array(A) @ np.array(x), [1.0, 2.0, 3.0], rtol=0, atol=1e-14)
    assert sift_ref.solve3([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]], [1, 1, 1]) == [0, 0, 0]


def test_gradient_bin_ties():
    dx = np.array([1.0, -1.0, -1.0, 1.0, 1.0, 0.0, 0.0])
    dy = np.array([1.0, 1.0, -1.0, -1.0, 0.0, 1.0, 0.0])
    assert sift_ref.gradient_bin(dx, dy).tolist() == [4, 13, 22, 31, 0, 9, 0]


def test_golden_is_reproduced():
    z = np.load(GOLDEN)
    assert np.array_equal(z["image"], cases.texture(48, 64))  # the case is what the fixture holds
    out = sift_ref.extract(z["image"], int(z["num_keypoints"]), float(z["sigma"]))
    assert np.array_equal(out["kf"].view(np.uint32), z["kf"].view(np.uint32))
    assert np.array_equal(out["ki"], z["ki"])
    assert np.array_equal(out["x"], z["x"].astype(np.float32))
    assert len(z["kf"]) > 16  # the cut falls on a tie, which is kept


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_case_conditions(name):
    """Conditions on the inputs, not measurements: fix the inputs if one fails."""
    out = cases.oracle(name)
    print(f"{name}: {out['candidates']} candidates, survivors per octave "
          f"{out['survivors'].tolist()}, {len(out['kf'])} keypoints, margin {out['margin']:.2e} "
          f"({out['margin_where']})")
    if name in TEXTURES:
        assert (out["survivors"] >= 5).sum() >= 2
    assert out["two_peaks"]
    assert out["margin"] > 1e-9
    assert len(out["kf"]) > 16  # num_keypoints = 16 cuts


def test_selection_cuts():
    all_ = cases.oracle("texture48x64")
    cut = cases.oracle("texture48x64", 16)
    n = len(cut["kf"])
    assert 16 <= n < len(all_["kf"])
    assert np.array_equal(cut["kf"], all_["kf"][:n]) and np.array_equal(cut["x"], all_["x"][:n])
    assert (np.diff(all_["score"]) <= 0).all()
