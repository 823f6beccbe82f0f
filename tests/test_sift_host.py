"""Host-side surface of the SIFT-node entries (no GPU): the extractor's constructor and repr, the
header declarations and their binding, the argument checks that run before any launch, the sizes
the entries report against the oracle's, and what raises in Python."""
import builtins

import pytest
import torch

from lesion_gnn_amd import _lib, ops
from lesion_gnn_amd.datasets.nodes import sift
from tests import sift_ref

ENTRIES = ("lgnn_sift_num_octaves", "lgnn_sift_pyramid_floats", "lgnn_sift_pyramid",
           "lgnn_sift_rows", "lgnn_sift_count", "lgnn_sift_candidates",
           "lgnn_sift_keypoints_workspace_bytes", "lgnn_sift_keypoints", "lgnn_sift_gather",
           "lgnn_sift_descriptors")


def test_constructor_and_repr():
    ex = sift.SiftExtractor(num_keypoints=300, sigma=1.6)
    assert ex.num_keypoints == 300 and ex.sigma == 1.6
    assert repr(ex) == "SiftExtractor(num_keypoints=300, sigma=1.6)"
    cfg = sift.SiftNodesConfig(num_keypoints=50, sigma=1.2)
    assert repr(sift.SiftExtractor(cfg.num_keypoints, cfg.sigma)) == \
        "SiftExtractor(num_keypoints=50, sigma=1.2)"


def test_header_entries_are_exported_and_bound():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 40  # additions only
    assert _lib.LGNN_SIFT_MAX_RADIUS == 16 and _lib.LGNN_SIFT_MAX_PEAKS == 18
    assert [n for _, n in _lib.PARAMS["lgnn_sift_pyramid"]] == [
        "image", "batch", "height", "width", "channels", "sigma", "gray", "gauss", "gauss_floats",
        "dog", "dog_floats", "stream"]
    assert dict((n, c) for c, n in _lib.PARAMS["lgnn_sift_keypoints"])["sigma"] == "double"


@pytest.mark.parametrize("H,W", [(48, 64), (44, 52), (37, 41), (96, 128), (512, 512), (5, 300),
                                 (2, 2)])
def test_sizes_match_the_oracle(H, W):
    lib = _lib.load()
    dims = sift_ref.octave_dims(H, W)
    assert lib.lgnn_sift_num_octaves(H, W) == len(dims)
    assert ops.sift_octave_dims(H, W) == dims
    assert lib.lgnn_sift_pyramid_floats(3, H, W) == 3 * 6 * sum(h * w for h, w in dims)
    assert lib.lgnn_sift_rows(3, H, W) == 3 * 3 * sum(h for h, _ in dims)


def test_bad_arguments_return_einval_before_any_launch():
    lib = _lib.load()
    E = _lib.LGNN_EINVAL
    b = torch.zeros(1 << 16, dtype=torch.uint8)  # host memory: never dereferenced
    p, n = b.data_ptr(), b.numel()
    big = 1 << 40

    def pyramid(img=p, B=2, H=48, W=64, C=3, sigma=1.6, gray=p, g=p, ng=big, d=p, nd=big):
        return lib.lgnn_sift_pyramid(img, B, H, W, C, sigma, gray, g, ng, d, nd, None)

    for bad in (dict(H=1), dict(W=1), dict(B=0), dict(B=1 << 16), dict(C=2), dict(C=4),
                dict(sigma=0.0), dict(sigma=-1.6), dict(sigma=float("nan")),
                dict(sigma=float("inf")), dict(sigma=2.5),  # a blur radius beyond the LDS tile's
                dict(img=None), dict(gray=None), dict(g=None), dict(d=None),
                dict(ng=100), dict(nd=100),                 # capacities that do not fit
                dict(B=64, H=1 << 11, W=1 << 11)):          # B * 24 * H * W >= 2^31
        assert pyramid(**bad) == E, bad
    assert lib.lgnn_sift_num_octaves(1, 64) == 0 and lib.lgnn_sift_num_octaves(64, 1) == 0
    assert lib.lgnn_sift_pyramid_floats(0, 48, 64) == 0 and lib.lgnn_sift_rows(2, 1, 64) == 0
    # lgnn_sift_count(dog, B, H, W, counts, row_ptr, stream)
    assert lib.lgnn_sift_count(p, 2, 1, 64, p, p, None) == E
    assert lib.lgnn_sift_count(None, 2, 48, 64, p, p, None) == E
    assert lib.lgnn_sift_count(p, 2, 48, 64, None, p, None) == E
    assert lib.lgnn_sift_count(p, 2, 48, 64, p, None, None) == E
    # lgnn_sift_candidates(dog, B, H, W, row_ptr, cand, capacity, stream)
    assert lib.lgnn_sift_candidates(p, 2, 48, 1, p, p, 10, None) == E
    assert lib.lgnn_sift_candidates(p, 2, 48, 64, None, p, 10, None) == E
    assert lib.lgnn_sift_candidates(p, 2, 48, 64, p, None, 10, None) == E
    assert lib.lgnn_sift_candidates(p, 2, 48, 64, p, p, -1, None) == E
    assert lib.lgnn_sift_candidates(None, 2, 48, 64, p, p, 10, None) == E

    # lgnn_sift_keypoints(gauss, dog, B, H, W, sigma, cand, n, num_keypoints, node_ptr, ws, bytes,
    #                     stream)
    def keypoints(g=p, d=p, B=2, H=48, W=64, sigma=1.6, cand=p, nc=10, nk=16, ptr=p, ws=p,
                  nb=big):
        return lib.lgnn_sift_keypoints(g, d, B, H, W, sigma, cand, nc, nk, ptr, ws, nb, None)

    for bad in (dict(H=1), dict(B=0), dict(sigma=0.0), dict(nc=-1), dict(nc=1 << 30), dict(nk=0),
                dict(g=None), dict(d=None), dict(cand=None), dict(ptr=None), dict(ws=None),
                dict(nb=64)):
        assert keypoints(**bad) == E, bad
    # lgnn_sift_gather(B, n, node_ptr, total, kf, ki, ws, bytes, stream)
    assert lib.lgnn_sift_gather(0, 10, p, 5, p, p, p, big, None) == E
    assert lib.lgnn_sift_gather(2, -1, p, 5, p, p, p, big, None) == E
    assert lib.lgnn_sift_gather(2, 10, None, 5, p, p, p, big, None) == E
    assert lib.lgnn_sift_gather(2, 10, p, -1, p, p, p, big, None) == E
    assert lib.lgnn_sift_gather(2, 10, p, 5, None, p, p, big, None) == E
    assert lib.lgnn_sift_gather(2, 10, p, 5, p, None, p, big, None) == E
    assert lib.lgnn_sift_gather(2, 10, p, 5, p, p, None, big, None) == E
    assert lib.lgnn_sift_gather(2, 10, p, 5, p, p, p, 64, None) == E
    # lgnn_sift_descriptors(gauss, B, H, W, kf, ki, n, x, stream)
    assert lib.lgnn_sift_descriptors(p, 2, 1, 64, p, p, 5, p, None) == E
    assert lib.lgnn_sift_descriptors(p, 2, 48, 64, p, p, -1, p, None) == E
    assert lib.lgnn_sift_descriptors(None, 2, 48, 64, p, p, 5, p, None) == E
    assert lib.lgnn_sift_descriptors(p, 2, 48, 64, None, p, 5, p, None) == E
    assert lib.lgnn_sift_descriptors(p, 2, 48, 64, p, None, 5, p, None) == E
    assert lib.lgnn_sift_descriptors(p, 2, 48, 64, p, p, 5, None, None) == E


def test_workspace_bytes():
    lib = _lib.load()
    ws = lib.lgnn_sift_keypoints_workspace_bytes
    assert ws(2, 100) >= 100 * 18 * (32 + 4 + 4 + 4) + 100 * 36
    assert ws(2, 0) > 0 and ws(0, 10) == 0 and ws(2, -1) == 0 and ws(2, 1 << 30) == 0


def test_cpu_tensors_raise():
    img = torch.zeros(2, 48, 64, 3, dtype=torch.uint8)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.sift_pyramid(img, 1.6)
    flat = torch.zeros(2 * 6 * 4)
    pyr = ops.SiftPyramid(None, flat, flat, (2, 48, 64))
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.sift_candidates(pyr)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.sift_keypoints(pyr, torch.zeros(3, 5, dtype=torch.int32), 1.6, 16)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.sift_descriptors(pyr, torch.zeros(3, 5), torch.zeros(3, 3, dtype=torch.int32))
    ex = sift.SiftExtractor(16, 1.6)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ex.nodes_from_image(img[0], 1)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ex.nodes_from_image(img[0, :, :, 0], 1)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ex.nodes_from_batch(img, [0, 1])


def test_wrong_dtype_or_shape_raises(monkeypatch):
    ex = sift.SiftExtractor(16, 1.6)
    with pytest.raises(ValueError, match="uint8"):
        ex.nodes_from_image(torch.zeros(48, 64, 3), 1)
    with pytest.raises(ValueError, match=r"\(H, W, 3\) or \(H, W\)"):
        ex.nodes_from_image(torch.zeros(2, 48, 64, 3, dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match=r"\(B, H, W, 3\) or \(B, H, W\)"):
        ex.nodes_from_batch(torch.zeros(2, 48, 64, 4, dtype=torch.uint8), [0, 1])
    with pytest.raises(ValueError, match=r"\(B, H, W, 3\) or \(B, H, W\)"):
        ex.nodes_from_batch(torch.zeros(48, 64, dtype=torch.uint8), [0, 1])
    with pytest.raises(ValueError):
        ops.sift_pyramid(torch.zeros(2, 48, 64, 3), 1.6)
    # past the device check
    monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    img = torch.zeros(2, 48, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="3 labels for 2 images"):
        ex.nodes_from_batch(img, [0, 1, 2])
    with pytest.raises(ValueError, match="1 names for 2 images"):
        ex.nodes_from_batch(img, [0, 1], ["a"])
    with pytest.raises(ValueError, match="at least 2 x 2"):
        ex.nodes_from_batch(img[:, :1], [0, 1])
    with pytest.raises(ValueError, match="sigma must be positive"):
        sift.SiftExtractor(16, 0.0).nodes_from_batch(img, [0, 1])
    with pytest.raises(ValueError, match="num_keypoints must be at least 1"):
        sift.SiftExtractor(0, 1.6).nodes_from_batch(img, [0, 1])
    with pytest.raises(ValueError, match=r"cand must be a \(n, 5\) int32"):
        ops.sift_keypoints(ops.SiftPyramid(None, img, img, (2, 48, 64)), torch.zeros(3, 4), 1.6, 16)


def test_call_without_pil_names_the_alternative(monkeypatch):
    real = builtins.__import__

    def no_pil(name, *a, **kw):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **kw)

    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(ImportError, match="nodes_from_image"):
        sift.SiftExtractor(16, 1.6)("missing.png", 0)


def test_call_on_a_missing_file():
    pytest.importorskip("PIL.Image")
    with pytest.raises(RuntimeError, match="Could not read image"):
        sift.SiftExtractor(16, 1.6)("no_such_file.png", 0)


def test_sift_nodes_batch_indexing():
    ptr = torch.tensor([0, 2, 2, 5])
    batch = sift.SiftNodesBatch(
        x=torch.arange(640.).view(5, 128), pos=torch.zeros(5, 2, dtype=torch.float64),
        score=torch.arange(5, dtype=torch.float64), y=torch.tensor([4, 0, 1]), ptr=ptr,
        names=["a", "b", "c"])
    assert len(batch) == 3 and batch.ptr_host.tolist() == [0, 2, 2, 5]
    assert batch[0].x.shape == (2, 128) and batch[0].name == "a" and batch[0].edge_index is None
    assert batch[1].x.shape == (0, 128) and batch[1].y.tolist() == [0]
    assert batch[-1].score.tolist() == [2.0, 3.0, 4.0] and batch[-1].name == "c"
    assert batch[2].x.data_ptr() == batch.x[2:].data_ptr()
    with pytest.raises(IndexError):
        batch[3]
