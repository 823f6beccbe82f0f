"""The SIFT kernels (csrc/sift.hip) stage by stage against the float64 restatement
tests/sift_ref.py. Each stage starts from the oracle's inputs, or from the previous stage's device
output handed to the oracle, so an error cannot pass from one stage into the next unseen.

Pyramid: gray exactly; the Gaussian and DoG levels within a derived absolute bound
(sift_ref.level_bounds): every level is a convex combination of values in [0, 255], one separable
blur of ksize taps adds at most 2 * (ksize + 1) * 2^-24 * 255, carried from level to level and
across octaves; a DoG level's bound is the sum of its two levels'. About 3e-3 in octave 0 at sigma
1.6, where a wrong tap or border index gives errors above 0.1 on these textures.
Candidates: the oracle's fp32 DoG -> the same list in the same order, exactly.
Keypoints: the device's own pyramid handed to the oracle -> the same keypoints in the same order,
pt, size, angle and response bit-equal as fp32.
Descriptors: the oracle's keypoints on the device's pyramid -> every element within 1 unit and at
most 1 element in 10^4 different at all (the final rounding; the oracle's margin condition keeps
the decisions before it clear of float64 rounding).
Measured on one MI355X (printed by the tests): see DESIGN §4.11."""
import functools

import numpy as np
import pytest
import torch

from lesion_gnn_amd import ops
from tests import sift_cases as cases
from tests import sift_ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def oracle_pyramid(name):
    """(gray, gauss64, dog64) of a case, computed once; do not modify."""
    _, image, sigma = cases.case(name)
    g = sift_ref.gray(image)
    return (g,) + sift_ref.pyramid(g, sigma)


def device_pyramid(cuda, name):
    _, image, sigma = cases.case(name)
    return ops.sift_pyramid(torch.from_numpy(image.copy())[None].to(cuda), sigma)


def host_levels(levels):
    """Per-octave (1, L, h, w) device tensors -> per-octave (L, h, w) numpy arrays."""
    return [t[0].cpu().numpy() for t in levels]


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_pyramid(cuda, name):
    _, image, sigma = cases.case(name)
    g, gauss, dog = oracle_pyramid(name)
    got = device_pyramid(cuda, name)
    assert torch.equal(got.gray[0].cpu(), torch.from_numpy(g))
    gb, db = sift_ref.level_bounds(*g.shape, sigma)
    assert [tuple(t.shape[2:]) for t in got.gauss] == [a.shape[1:] for a in gauss]
    worst = 0.0
    for o, (dg, dd) in enumerate(zip(host_levels(got.gauss), host_levels(got.dog))):
        for i in range(6):
            err = np.abs(dg[i].astype(np.float64) - gauss[o][i]).max()
            worst = max(worst, err / gb[o][i])
            print(f"{name} octave {o} gauss {i}: max|err| {err:.3e} bound {gb[o][i]:.3e}")
            assert err <= gb[o][i]
        for i in range(5):
            err = np.abs(dd[i].astype(np.float64) - dog[o][i]).max()
            print(f"{name} octave {o} dog {i}: max|err| {err:.3e} bound {db[o][i]:.3e}")
            assert err <= db[o][i]
    print(f"{name}: largest error / bound {worst:.3f}")


def test_pyramid_batch_equals_single(cuda):
    imgs = torch.from_numpy(cases.batch3()).to(cuda)
    whole = ops.sift_pyramid(imgs, 1.6)
    for b in range(3):
        one = ops.sift_pyramid(imgs[b:b + 1], 1.6)
        assert torch.equal(one.gray[0], whole.gray[b])
        for a, w in zip(one.gauss + one.dog, whole.gauss + whole.dog):
            assert torch.equal(a[0], w[b])


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_candidates(cuda, name):
    _, _, dog64 = oracle_pyramid(name)
    dog = sift_ref.to_f32(dog64)
    want = sift_ref.candidates(dog)
    pyr = ops.SiftPyramid.from_levels(None, [torch.from_numpy(d)[None].to(cuda) for d in dog])
    got = ops.sift_candidates(pyr).cpu().numpy()
    print(f"{name}: {len(want)} candidates")
    assert len(want) > 0
    assert (got[:, 0] == 0).all()
    assert np.array_equal(got[:, 1:], want)


def test_candidates_batch_order(cuda):
    """Two images in one call: image 0's list, then image 1's, each as alone."""
    dogs = [sift_ref.to_f32(oracle_pyramid(n)[2]) for n in ("texture48x64", "texture48x64_sigma1.2")]
    levels = [torch.from_numpy(np.stack([a, b])).to(cuda) for a, b in zip(*dogs)]
    got = ops.sift_candidates(ops.SiftPyramid.from_levels(None, levels)).cpu().numpy()
    want = [sift_ref.candidates(d) for d in dogs]
    n0 = len(want[0])
    assert (got[:n0, 0] == 0).all() and (got[n0:, 0] == 1).all()
    assert np.array_equal(got[:n0, 1:], want[0]) and np.array_equal(got[n0:, 1:], want[1])


@pytest.mark.parametrize("num_keypoints", cases.NUM_KEYPOINTS)
@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_keypoints(cuda, name, num_keypoints):
    _, _, sigma = cases.case(name)
    pyr = device_pyramid(cuda, name)
    cand = ops.sift_candidates(pyr)
    kf, ki, ptr, ptr_host = ops.sift_keypoints(pyr, cand, sigma, num_keypoints)
    gauss, dog = host_levels(pyr.gauss), host_levels(pyr.dog)
    # the candidates are exact on any fp32 DoG, so the oracle's own list must be the device's
    want_cand = sift_ref.candidates(dog)
    assert np.array_equal(cand.cpu().numpy()[:, 1:], want_cand)
    want_kf, want_ki = sift_ref.keypoints(gauss, dog, sigma, num_keypoints, cand=want_cand)
    print(f"{name} num_keypoints {num_keypoints}: {len(want_kf)} keypoints")
    assert len(want_kf) >= min(num_keypoints, 16)
    assert ptr_host.tolist() == [0, len(want_kf)] and torch.equal(ptr.cpu(), ptr_host)
    got_kf, got_ki = kf.cpu().numpy(), ki.cpu().numpy()
    assert (got_ki[:, 0] == 0).all() and np.array_equal(got_ki[:, 1:], want_ki)
    names = ("x", "y", "size", "angle", "response")
    for k, field in enumerate(names):
        same = got_kf[:, k].view(np.uint32) == want_kf[:, k].view(np.uint32)
        assert same.all(), (field, np.nonzero(~same)[0][:5], got_kf[~same][:3], want_kf[~same][:3])


def _check_noise_batch(cuda, batch, H, W, num_keypoints, sigma=0.8):
    """A seeded-noise batch through count, candidates and keypoints: row_ptr, the candidate list,
    the keypoints and node_ptr against the oracle run image by image on the device's pyramid.
    Returns (scan rows, candidates)."""
    from lesion_gnn_amd import _lib

    imgs = np.random.default_rng(17 * batch + H).integers(0, 256, (batch, H, W, 3), dtype=np.uint8)
    pyr = ops.sift_pyramid(torch.from_numpy(imgs).to(cuda), sigma)
    dims = sift_ref.octave_dims(H, W)
    per_image = 3 * sum(h for h, _ in dims)
    rows = _lib.load().lgnn_sift_rows(batch, H, W)
    assert rows == batch * per_image
    counts = torch.empty(rows, dtype=torch.int32, device=cuda)
    row_ptr = torch.empty(rows + 1, dtype=torch.int32, device=cuda)
    _lib.call("lgnn_sift_count", pyr.dog_flat, batch, H, W, counts, row_ptr, _lib.stream(cuda))
    gauss = [t.cpu().numpy() for t in pyr.gauss]
    dog = [t.cpu().numpy() for t in pyr.dog]
    want_cand = [sift_ref.candidates([d[b] for d in dog]) for b in range(batch)]
    # a candidate's scan row: image, octave, layer 1..3, row
    base = np.concatenate([[0], np.cumsum([3 * h for h, _ in dims])])
    heights = np.array([h for h, _ in dims])
    per_row = np.zeros(rows, dtype=np.int64)
    for b, c in enumerate(want_cand):
        np.add.at(per_row, b * per_image + base[c[:, 0]] + (c[:, 1] - 1) * heights[c[:, 0]] + c[:, 2],
                  1)
    assert np.array_equal(row_ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(per_row)]))
    cand = ops.sift_candidates(pyr)
    got = cand.cpu().numpy()
    assert np.array_equal(got[:, 0], np.repeat(np.arange(batch), [len(c) for c in want_cand]))
    assert np.array_equal(got[:, 1:], np.concatenate(want_cand))
    kf, ki, ptr, ptr_host = ops.sift_keypoints(pyr, cand, sigma, num_keypoints)
    want = [sift_ref.keypoints([g[b] for g in gauss], [d[b] for d in dog], sigma, num_keypoints,
                               cand=want_cand[b]) for b in range(batch)]
    sizes = [len(w[0]) for w in want]
    assert ptr_host.tolist() == [0] + np.cumsum(sizes).tolist() and torch.equal(ptr.cpu(), ptr_host)
    got_ki = ki.cpu().numpy()
    assert np.array_equal(got_ki[:, 0], np.repeat(np.arange(batch), sizes))
    assert np.array_equal(got_ki[:, 1:], np.concatenate([w[1] for w in want]))
    assert np.array_equal(kf.cpu().numpy().view(np.uint32),
                          np.concatenate([w[0] for w in want]).view(np.uint32))
    return rows, len(got)


def test_scans_past_one_tile(cuda):
    """More than 1024 scan rows (row_ptr) and more than 1024 candidates (the peak offsets behind
    the keypoints): both one-workgroup scans carry across a tile."""
    rows, ncand = _check_noise_batch(cuda, 3, 48, 64, 10000)
    print(f"{rows} scan rows, {ncand} candidates")
    assert rows > 1024 and ncand > 1024


def test_node_ptr_of_65_images(cuda):
    """node_ptr past one wave of images, with the response cut at 8 keypoints an image."""
    _check_noise_batch(cuda, 65, 16, 16, 8)


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_descriptors(cuda, name):
    _, _, sigma = cases.case(name)
    pyr = device_pyramid(cuda, name)
    gauss, dog = host_levels(pyr.gauss), host_levels(pyr.dog)
    kf, ki = sift_ref.keypoints(gauss, dog, sigma, 10000)
    want = sift_ref.descriptors(gauss, kf, ki)
    ki3 = np.concatenate([np.zeros((len(ki), 1), np.int32), ki], axis=1)
    got = ops.sift_descriptors(pyr, torch.from_numpy(kf).to(cuda),
                               torch.from_numpy(ki3).to(cuda)).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert (got == np.rint(got)).all() and got.min() >= 0 and got.max() <= 255
    diff = np.abs(got - want)
    print(f"{name}: {len(kf)} descriptors, max|diff| {diff.max():.0f}, "
          f"{int((diff > 0).sum())} of {diff.size} elements differ")
    assert want.max() > 50  # descriptors, not zeros
    assert diff.max() <= 1
    assert (diff > 0).sum() <= diff.size * 1e-4


def test_refused_arguments(cuda):
    img = torch.zeros(1, 48, 64, dtype=torch.uint8, device=cuda)
    from lesion_gnn_amd._lib import LgnnError

    with pytest.raises(LgnnError):
        ops.sift_pyramid(img, 0.0)
    with pytest.raises(LgnnError):
        ops.sift_pyramid(img, 4.0)  # a blur radius beyond LGNN_SIFT_MAX_RADIUS
    with pytest.raises(ValueError):
        ops.sift_pyramid(img.float(), 1.6)
    pyr = ops.sift_pyramid(img, 1.6)
    with pytest.raises(ValueError):
        ops.sift_keypoints(pyr, torch.zeros(0, 5, dtype=torch.int32, device=cuda), 1.6, 0)
    # candidates outside the pyramid are skipped, not read
    bad = torch.tensor([[0, 9, 1, 7, 7], [0, 0, 1, 2, 7], [0, 0, 4, 7, 7], [0, 0, 1, 7, 200]],
                       dtype=torch.int32, device=cuda)
    kf, ki, ptr, ptr_host = ops.sift_keypoints(pyr, bad, 1.6, 16)
    assert ptr_host.tolist() == [0, 0] and kf.shape == (0, 5)
