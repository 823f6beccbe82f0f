"""GPU: the fundus preprocessing (lesion_gnn_amd/datasets/fundus.py, csrc/fundus.hip) against the
numpy oracle tests/fundus_ref.py. Every integer output (boxes, geom, uint8, mask) is compared with
torch.equal: the pixel path is integer arithmetic, so there is no tolerance. The normalised output
is held to the float64 oracle within 4 * 2**-24 / min(std): the inputs are integers <= 255, m_c and
r_c are one fp32 rounding each, the subtraction and the product one each, so the absolute error is
below 4 * 2**-24 * 255 / (255 * std)."""
import functools
import warnings

import numpy as np
import pytest
import torch

from lesion_gnn_amd import _lib
from lesion_gnn_amd.datasets.fundus import (IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD,
                                            FundusAutocrop, FundusPreprocess)
from lesion_gnn_amd.datasets.nodes.sift import SiftExtractor
from tests import fundus_ref as ref

pytestmark = pytest.mark.gpu

MEAN, STD = IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD
ATOL = 4 * 2.0 ** -24 / min(STD)


def dark(h, w, seed=0):
    """(h, w, 3) uint8: red in 0..25 (not lit at threshold 25), green and blue anything."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[:, :, 0] = rng.integers(0, 26, (h, w))
    return img


def framed(H, W, y0, x0, ch, cw, seed=0):
    """A dark H x W image whose lit pixels fill rows y0..y0 + ch and columns x0..x0 + cw, so the
    box is (x0, x0 + cw, y0, y0 + ch) and the crop ch x cw."""
    rng = np.random.default_rng(seed + 1000)
    img = dark(H, W, seed)
    img[y0:y0 + ch + 1, x0:x0 + cw + 1, 0] = rng.integers(26, 256, (ch + 1, cw + 1))
    return img


def labels(h, w, seed=0):
    return np.random.default_rng(seed + 2000).integers(0, 5, (h, w), dtype=np.uint8)


def gpu(a, dev):
    return torch.from_numpy(a.copy()).to(dev)  # a copy: the shared cases are read-only


def boxes_of(images, dev, threshold=25.0):
    return FundusAutocrop(threshold).boxes([gpu(i, dev) for i in images]).cpu()


def want_boxes(images, threshold=25.0):
    return torch.tensor([ref.box(i, threshold) for i in images], dtype=torch.int32)


# ----------------------------------------------------------------------------------------------
# the box
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("H,W", [(5, 7), (33, 70), (64, 67)])  # W * 3 is no multiple of 16
def test_box_of_a_lit_rectangle(cuda, H, W):
    images = [framed(H, W, 1, 2, H - 3, W - 4, seed=1), framed(H, W, 0, 0, H - 1, W - 1, seed=2),
              framed(H, W, H - 3, W - 3, 2, 2, seed=3), framed(H, W, 0, 1, 1, 1, seed=4)]
    got = boxes_of(images, cuda)
    assert torch.equal(got, want_boxes(images))
    assert got[0].tolist() == [2, W - 2, 1, H - 2] and got[1].tolist() == [0, W - 1, 0, H - 1]


# the bytes in front of the first aligned one are 15, 14, 13, 11, 9, 3, 1, 0: their remainders
# mod 3 put the first red byte of a 48-byte group at byte 0, 1 and 2 (all three phases)
@pytest.mark.parametrize("offset", [1, 2, 3, 5, 7, 13, 15, 16])
def test_box_of_a_view_at_an_odd_byte_offset(cuda, offset):
    H, W = 33, 70
    img = framed(H, W, 0, 0, H - 1, W - 1, seed=5)  # lit up to the first and last byte's pixel
    inner = framed(H, W, 3, 5, 20, 50, seed=6)
    for a in (img, inner):
        buf = torch.zeros(offset + a.size + 64, dtype=torch.uint8, device=cuda)
        buf[offset + a.size:] = 255            # lit bytes right behind the image: never read
        buf[:offset] = 255                     # and right in front of it
        view = buf[offset:offset + a.size].view(H, W, 3)
        view.copy_(gpu(a, cuda))
        assert view.data_ptr() % 16 == offset % 16 and view.is_contiguous()
        got = FundusAutocrop().boxes([view]).cpu()
        assert torch.equal(got, want_boxes([a]))


def test_box_fallbacks(cuda):
    H, W = 33, 70
    empty = dark(H, W, 7)
    single = empty.copy()
    single[12, 40, 0] = 200
    row = empty.copy()
    row[12, 3:60, 0] = 200
    column = empty.copy()
    column[2:30, 40, 0] = 200
    last = empty.copy()
    last[H - 1, W - 1, 0] = 255           # only the last pixel of the last row
    first = empty.copy()
    first[0, 0, 0] = 255
    images = [empty, single, row, column, last, first]
    got = boxes_of(images, cuda)
    assert torch.equal(got, want_boxes(images))
    assert got.tolist() == [[0, W, 0, H]] * 6


def test_box_of_the_four_corners_and_of_the_two_ends(cuda):
    H, W = 64, 67
    corners = dark(H, W, 8)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        corners[y, x, 0] = 26
    ends = dark(H, W, 9)
    ends[0, 0, 0] = ends[H - 1, W - 1, 0] = 255
    got = boxes_of([corners, ends], cuda)
    assert torch.equal(got, want_boxes([corners, ends]))
    assert got.tolist() == [[0, W - 1, 0, H - 1]] * 2


def test_box_threshold_is_strict_and_a_float(cuda):
    H, W = 33, 70
    img = np.zeros((H, W, 3), np.uint8)
    img[2, 3, 0] = img[30, 65, 0] = 25     # the outer pair: exactly 25
    img[5, 8, 0] = img[20, 50, 0] = 26     # the inner pair: 26
    for thr, want in ((25.0, [8, 50, 5, 20]), (25.5, [8, 50, 5, 20]), (24.5, [3, 65, 2, 30]),
                      (24.0, [3, 65, 2, 30]), (26.0, [0, W, 0, H]), (-1.0, [0, W - 1, 0, H - 1]),
                      (255.0, [0, W, 0, H])):
        got = boxes_of([img], cuda, thr)
        assert torch.equal(got, want_boxes([img], thr)), thr
        assert got[0].tolist() == want, thr


def test_box_reads_red_only(cuda):
    H, W = 33, 70
    img = np.zeros((H, W, 3), np.uint8)
    img[:, :, 1:] = 255
    assert boxes_of([img], cuda).tolist() == [[0, W, 0, H]]
    img[4:9, 6:30, 0] = 26
    assert boxes_of([img], cuda).tolist() == [[6, 29, 4, 8]]


def test_box_of_an_image_that_several_workgroups_share(cuda):
    """150 x 250 pixels are 2344 groups of 16 pixels; a workgroup's share is 782 of them
    (lgnn_fundus_bbox_share), so three workgroups read the image: groups [0, 782), [782, 1564)
    and [1564, 2344), counted from the first 16-byte-aligned byte (the allocation is aligned:
    group g holds pixels 16 g .. 16 g + 15). The only lit pixels are pixel 2 * 250 + 10 = 510
    (group 31, the first workgroup) and pixel 149 * 250 + 200 = 37450 (group 2340, the last)."""
    H, W = 150, 250
    assert _lib.load().lgnn_fundus_bbox_share(H, W) == 782
    img = dark(H, W, 10)
    img[2, 10, 0] = img[149, 200, 0] = 255
    t = gpu(img, cuda)
    assert t.data_ptr() % 16 == 0
    got = FundusAutocrop().boxes([t]).cpu()
    assert torch.equal(got, want_boxes([img])) and got.tolist() == [[10, 200, 2, 149]]
    middle = dark(H, W, 11)
    middle[70, 100, 0] = middle[80, 120, 0] = 255  # pixels 17600 and 20120: the second workgroup
    assert boxes_of([middle], cuda).tolist() == [[100, 120, 70, 80]]


# ----------------------------------------------------------------------------------------------
# the whole chain
# ----------------------------------------------------------------------------------------------

# name -> (H, W, y0, x0, crop h, crop w): the crop that is resized
CASES = {
    "upscale_5x3": (12, 9, 4, 2, 5, 3),
    "reduce_37x23": (45, 31, 3, 5, 37, 23),
    "halve_32x32": (40, 36, 2, 3, 32, 32),
    "identity_16x11": (20, 19, 1, 6, 16, 11),
    "identity_17x9": (20, 19, 1, 6, 17, 9),
    "height_2": (9, 40, 3, 4, 2, 30),
    "height_1": (9, 50, 5, 4, 1, 40),   # two lit rows; new_h = rint(0.4) = 0 is clamped to 1
    "width_1": (50, 9, 4, 5, 40, 1),
}


@functools.lru_cache(maxsize=None)
def case(name, S):
    """(image, mask, oracle) of one case: computed once, shared, never written to."""
    if name == "random_200x150":
        img = np.random.default_rng(12).integers(0, 256, (200, 150, 3), dtype=np.uint8)
    else:
        img = framed(*CASES[name], seed=len(name))
    lab = labels(*img.shape[:2], seed=len(name))
    for a in (img, lab):
        a.setflags(write=False)
    return img, lab, ref.preprocess(img, S, MEAN, STD, mask=lab)


def check(pre, b, want, with_mask=True):
    assert torch.equal(pre.boxes[b].cpu(), torch.from_numpy(want["box"]))
    assert torch.equal(pre.geom[b].cpu(), torch.from_numpy(want["geom"]))
    assert torch.equal(pre.uint8[b].cpu(), torch.from_numpy(want["uint8"]))
    if with_mask:
        assert torch.equal(pre.mask[b].cpu(), torch.from_numpy(want["mask"]))
    got = pre.image[b].cpu().double()
    err = (got - torch.from_numpy(want["image"])).abs().max().item()
    assert err <= ATOL, (err, ATOL)
    # padding: v = 0 gives float32(-m_c * r_c) exactly
    x_min, y_min, w, h, new_w, new_h, left, top = want["geom"].tolist()
    S = got.shape[-1]
    padding = torch.ones(S, S, dtype=torch.bool)
    padding[top:top + new_h, left:left + new_w] = False
    m, r = ref.norm_constants(MEAN, STD)
    for c in range(3):
        value = np.float32(-np.float32(m[c])) * np.float32(r[c])
        assert (pre.image[b, c].cpu()[padding] == float(value)).all()


@pytest.mark.parametrize("S", [16, 17])  # both parities of the padding remainder
@pytest.mark.parametrize("name", list(CASES))
def test_chain_matches_the_oracle(cuda, name, S):
    img, lab, want = case(name, S)
    H, W, y0, x0, ch, cw = CASES[name]
    assert want["box"].tolist() == [x0, x0 + cw, y0, y0 + ch]
    pre = FundusPreprocess(S)([gpu(img, cuda)], masks=[gpu(lab, cuda)], return_uint8=True)
    assert pre.image.shape == (1, 3, S, S) and pre.image.dtype == torch.float32
    assert pre.uint8.shape == (1, S, S, 3) and pre.mask.shape == (1, S, S)
    check(pre, 0, want)


def test_chain_on_a_random_image(cuda):
    img, lab, want = case("random_200x150", 64)
    pre = FundusPreprocess(64)(gpu(img, cuda)[None], masks=gpu(lab, cuda)[None],
                               return_uint8=True)
    check(pre, 0, want)
    alone = FundusPreprocess(64)(gpu(img, cuda)[None])  # the float output alone
    assert alone.uint8 is None and alone.mask is None
    assert torch.equal(alone.image, pre.image)


def test_other_normalisation_constants_and_threshold(cuda):
    mean, std, thr = (0.5, 0.25, 0.0), (0.5, 1.0, 0.125), 100.0
    img = np.random.default_rng(13).integers(0, 256, (33, 70, 3), dtype=np.uint8)
    want = ref.preprocess(img, 17, mean, std, threshold=thr)
    pre = FundusPreprocess(17, mean, std, threshold=thr)([gpu(img, cuda)], return_uint8=True)
    assert torch.equal(pre.boxes[0].cpu(), torch.from_numpy(want["box"]))
    assert torch.equal(pre.uint8[0].cpu(), torch.from_numpy(want["uint8"]))
    err = (pre.image[0].cpu().double() - torch.from_numpy(want["image"])).abs().max().item()
    assert err <= 4 * 2.0 ** -24 / min(std)


def test_a_list_of_three_sizes_equals_three_calls(cuda):
    names = ["reduce_37x23", "upscale_5x3", "height_1"]
    S = 16
    imgs = [gpu(case(n, S)[0], cuda) for n in names]
    labs = [gpu(case(n, S)[1], cuda) for n in names]
    fp = FundusPreprocess(S)
    pre = fp(imgs, masks=labs, return_uint8=True)
    for b, n in enumerate(names):
        check(pre, b, case(n, S)[2])
        one = fp([imgs[b]], masks=[labs[b]], return_uint8=True)
        for field in ("image", "uint8", "mask", "boxes", "geom"):
            assert torch.equal(getattr(pre, field)[b], getattr(one, field)[0]), (n, field)


def test_a_batch_tensor_equals_the_list_of_its_slices(cuda):
    rng = np.random.default_rng(14)
    stack = np.stack([framed(33, 70, 2 + b, 3 * b, 25, 40 + b, seed=20 + b) for b in range(3)])
    labs = rng.integers(0, 5, (3, 33, 70), dtype=np.uint8)
    t, m = gpu(stack, cuda), gpu(labs, cuda)
    fp = FundusPreprocess(17)
    whole = fp(t, masks=m, return_uint8=True)
    parts = fp([t[b] for b in range(3)], masks=[m[b] for b in range(3)], return_uint8=True)
    for field in ("image", "uint8", "mask", "boxes", "geom"):
        assert torch.equal(getattr(whole, field), getattr(parts, field)), field
    for b in range(3):
        check(whole, b, ref.preprocess(stack[b], 17, MEAN, STD, mask=labs[b]))


def test_more_images_than_one_launch_takes(cuda):
    B = _lib.LGNN_FUNDUS_MAX_IMAGES + 3
    images = [framed(12 + b, 9 + (b % 4), 1, 1, 6 + b % 3, 4 + b % 2, seed=40 + b)
              for b in range(B)]
    pre = FundusPreprocess(16)([gpu(i, cuda) for i in images], return_uint8=True)
    for b in range(B):
        check(pre, b, ref.preprocess(images[b], 16, MEAN, STD), with_mask=False)


def test_to_original_carries_the_lit_corners_back(cuda):
    """The destination pixel nearest to where a lit corner pixel's centre lands maps back to
    within half a destination pixel, in source pixels (w / new_w, h / new_h), of the corner."""
    H, W = 40, 30
    img = dark(H, W, 15)
    corners = [(6, 4), (6, 25), (37, 4), (37, 25)]  # (y, x)
    for y, x in corners:
        img[y, x, 0] = 255
    pre = FundusPreprocess(32)([gpu(img, cuda)])
    x_min, y_min, w, h, new_w, new_h, left, top = pre.geom[0].tolist()
    assert (x_min, y_min, w, h) == (4, 6, 21, 31)
    step = np.array([w / new_w, h / new_h])
    bound = 0.5 * step
    assert (bound <= 1.0).all()  # within one source pixel here
    src = np.array([[x, y] for y, x in corners], np.float64)
    landed = (src - [x_min, y_min] + 0.5) / step - 0.5 + [left, top]
    pos = torch.from_numpy(np.rint(landed)).to(cuda)
    back = pre.to_original(pos, 0).cpu().numpy()
    assert (np.abs(back - src) <= bound + 1e-9).all(), (back, src, bound)
    same = pre.to_original(pos, torch.zeros(4, dtype=torch.int64, device=cuda)).cpu().numpy()
    assert np.array_equal(same, back)


# ----------------------------------------------------------------------------------------------
# determinism, capture, and the extractor behind it
# ----------------------------------------------------------------------------------------------


def pair(seed):
    return np.stack([framed(33, 70, 2, 3 + seed, 25, 40, seed=30 + seed),
                     framed(33, 70, 5, 1, 20 + seed, 60, seed=31 + seed)])


def test_two_calls_give_equal_bits(cuda):
    t = gpu(pair(0), cuda)
    fp = FundusPreprocess(16)
    a, b = fp(t, return_uint8=True), fp(t, return_uint8=True)
    for field in ("image", "uint8", "boxes", "geom"):
        assert torch.equal(getattr(a, field), getattr(b, field)), field


def test_capture_and_replay_on_a_refilled_buffer(cuda):
    """A straight-line graph (no parallel branches): the two entries on one stream."""
    fp = FundusPreprocess(16)
    first, second = gpu(pair(0), cuda), gpu(pair(1), cuda)
    buf = first.clone()
    want_first, want_second = fp(first, return_uint8=True), fp(second, return_uint8=True)
    assert not torch.equal(want_first.uint8, want_second.uint8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fp(buf, return_uint8=True)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = fp(buf, return_uint8=True)
    graph.replay()
    torch.cuda.synchronize()
    for field in ("image", "uint8", "boxes", "geom"):
        assert torch.equal(getattr(got, field), getattr(want_first, field)), field
    buf.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    for field in ("image", "uint8", "boxes", "geom"):
        assert torch.equal(getattr(got, field), getattr(want_second, field)), field


def test_preprocessed_images_feed_the_sift_extractor(cuda):
    """Two photographs of different sizes become one batch for SiftExtractor.nodes_from_batch."""
    gen = torch.Generator().manual_seed(16)

    def photograph(H, W):
        coarse = torch.rand(1, 3, H // 8, W // 8, generator=gen)
        img = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bicubic")
        img = (img.clamp(0, 1) * 200 + 40).to(torch.uint8)[0].permute(1, 2, 0).contiguous()
        img[:6] = 0
        img[:, -9:] = 0
        return img.to(cuda)

    pre = FundusPreprocess(64)([photograph(96, 128), photograph(136, 104)], return_uint8=True)
    assert pre.uint8.shape == (2, 64, 64, 3)
    ex = SiftExtractor(8, 1.6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nodes = ex.nodes_from_batch(pre.uint8, [3, 1])
        alone = [ex.nodes_from_image(pre.uint8[b], y) for b, y in enumerate([3, 1])]
    assert len(nodes) == 2 and int(nodes.ptr_host[-1]) > 0
    for b in range(2):
        assert torch.equal(nodes[b].x, alone[b].x)
        assert torch.equal(nodes[b].pos, alone[b].pos)
        assert torch.equal(nodes[b].score, alone[b].score)
        assert nodes[b].y.tolist() == alone[b].y.tolist()
