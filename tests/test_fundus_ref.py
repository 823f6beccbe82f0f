"""Known answers for the fundus preprocessing oracle itself (tests/fundus_ref.py): no GPU, no
library. Each value below was worked out by hand or follows from a property of the arithmetic."""
import numpy as np
import pytest

from tests import fundus_ref as ref


def _random(h, w, c=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


@pytest.mark.parametrize("h,w", [(2, 2), (5, 7), (16, 16), (33, 70)])
def test_identity_at_equal_size(h, w):
    img = _random(h, w)
    assert np.array_equal(ref.resize_linear(img, h, w), img)
    lab = _random(h, w, 1)[:, :, 0] % 5
    assert np.array_equal(ref.resize_nearest(lab, h, w), lab)


def test_exact_halving_is_the_rounded_mean_of_four():
    img = _random(12, 18, seed=1)
    a = img.astype(np.int64)
    want = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    assert np.array_equal(ref.resize_linear(img, 6, 9), want.astype(np.uint8))


@pytest.mark.parametrize("value", [0, 255])
@pytest.mark.parametrize("new", [(3, 5), (7, 7), (29, 40), (64, 11)])
def test_a_constant_image_stays_constant(value, new):
    img = np.full((13, 17, 3), value, np.uint8)
    assert np.array_equal(ref.resize_linear(img, *new), np.full(new + (3,), value, np.uint8))


def test_two_by_two_to_four_by_four_by_hand():
    """sc = 0.5 on both axes. Taps: d = 0 -> f = -0.25 -> clamped to (0; 2048, 0); d = 1 -> f =
    0.25 -> (0; 1536, 512); d = 2 -> f = 0.75 -> (0; 512, 1536); d = 3 -> f = 1.25 -> s = 1 =
    src - 1 -> (1; 2048, 0). Rows after the horizontal pass, >> 4: [0, 3200, 9600, 12800] and
    [25600, 20480, 10240, 5120]; e.g. out[1][1] = ((1536 * 3200 >> 16) + (512 * 20480 >> 16) + 2)
    >> 2 = (75 + 160 + 2) >> 2 = 59."""
    s, a0, a1 = ref.linear_taps(4, 2)
    assert s.tolist() == [0, 0, 0, 1]
    assert a0.tolist() == [2048, 1536, 512, 2048] and a1.tolist() == [0, 512, 1536, 0]
    img = np.array([[0, 100], [200, 40]], np.uint8)[:, :, None]
    want = [[0, 25, 75, 100], [50, 59, 76, 85], [150, 126, 79, 55], [200, 160, 80, 40]]
    assert ref.resize_linear(img, 4, 4)[:, :, 0].tolist() == want


def test_nearest_indices():
    assert ref.nearest_index(4, 2).tolist() == [0, 0, 1, 1]
    assert ref.nearest_index(2, 5).tolist() == [0, 2]
    assert ref.nearest_index(3, 3).tolist() == [0, 1, 2]
    assert ref.nearest_index(7, 3).max() == 2


@pytest.mark.parametrize("h,w,S,want", [(37, 23, 16, (16, 10)), (2848, 4288, 512, (340, 512)),
                                        (33, 2, 17, (17, 1)), (1, 40, 16, (1, 16))])
def test_size_rule(h, w, S, want):
    assert ref.new_size(h, w, S) == want  # (1, 40, 16): rint(0.4) = 0 is clamped to 1


def test_size_rule_rounds_half_to_even():
    assert ref.new_size(5, 20, 10) == (2, 10)   # 2.5 -> 2
    assert ref.new_size(7, 20, 10) == (4, 10)   # 3.5 -> 4
    assert ref.new_size(20, 3, 10) == (10, 2)   # 1.5 -> 2


def test_pad_split_for_odd_remainders():
    assert ref.pad_offsets(10, 17, 17) == (3, 0)   # 7 rows: 3 above, 4 below
    assert ref.pad_offsets(16, 11, 16) == (0, 2)   # 5 columns: 2 left, 3 right
    assert ref.pad_offsets(12, 16, 16) == (2, 0)
    img = np.full((10, 17, 3), 9, np.uint8)
    out = ref.pad(img, 17)
    assert out.shape == (17, 17, 3)
    assert (out[:3] == 0).all() and (out[3:13] == 9).all() and (out[13:] == 0).all()


def test_box_rule():
    H, W = 9, 12
    img = np.zeros((H, W, 3), np.uint8)
    img[:, :, 1:] = 255                       # green and blue do not count
    assert ref.box(img) == (0, W, 0, H)       # empty
    img[4, 5, 0] = 200
    assert ref.box(img) == (0, W, 0, H)       # a single pixel
    img[4, 9, 0] = 200
    assert ref.box(img) == (0, W, 0, H)       # one row
    img[4, 9, 0] = 0
    img[7, 5, 0] = 200
    assert ref.box(img) == (0, W, 0, H)       # one column
    img[7, 9, 0] = 26
    assert ref.box(img) == (5, 9, 4, 7)
    assert ref.crop(img, ref.box(img)).shape == (3, 4, 3)  # the last lit row and column drop out
    img[2, 3, 0] = 25                         # strict: 25 is not above 25.0
    assert ref.box(img) == (5, 9, 4, 7)
    assert ref.box(img, 24.5) == (3, 9, 2, 7)
    assert ref.box(img, 26.0) == (0, W, 0, H)  # 26 is not above 26.0: only column 5 is left


def test_normalize_and_the_whole_chain():
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    m, r = ref.norm_constants(mean, std)
    assert m[0] == float(np.float32(0.485 * 255.0)) and r[2] == float(np.float32(1 / (0.225 * 255.0)))
    img = np.zeros((40, 30, 3), np.uint8)
    img[5:36, 4:27] = _random(31, 23, seed=2) | 32     # lit: red >= 32
    lab = (_random(40, 30, 1, seed=3)[:, :, 0] % 5).astype(np.uint8)
    out = ref.preprocess(img, 16, mean, std, mask=lab)
    assert out["box"].tolist() == [4, 26, 5, 35]
    assert out["geom"].tolist() == [4, 5, 22, 30, 12, 16, 2, 0]
    assert out["uint8"].shape == (16, 16, 3) and out["image"].shape == (3, 16, 16)
    assert (out["uint8"][:, :2] == 0).all() and (out["uint8"][:, 14:] == 0).all()
    assert np.array_equal(out["image"][1, :, 0], np.full(16, -m[1] * r[1]))
    assert out["mask"].shape == (16, 16) and out["mask"].max() <= 4 and (out["mask"][:, :2] == 0).all()
