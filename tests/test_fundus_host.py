"""Host-side surface of the fundus preprocessing (no GPU): the header declarations and their
binding, the argument checks that run before any launch, and what raises in Python."""
import builtins

import pytest
import torch

from lesion_gnn_amd import _lib, datasets, ops
from lesion_gnn_amd.datasets import fundus

ENTRIES = ("lgnn_fundus_bbox", "lgnn_fundus_preprocess")


def test_header_entries_are_exported_and_bound():
    lib = _lib.load()
    for name in ENTRIES + ("lgnn_fundus_bbox_share",):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 40  # additions only
    assert _lib.LGNN_FUNDUS_MAX_SIDE == 16384 and _lib.LGNN_FUNDUS_MAX_IMAGES == 16
    assert [n for _, n in _lib.PARAMS["lgnn_fundus_bbox"]] == [
        "batch", "images", "heights", "widths", "threshold", "boxes", "stream"]
    p = dict((n, c) for c, n in _lib.PARAMS["lgnn_fundus_preprocess"])
    assert p["images"] == p["masks"] == "const uint8_t* const*"
    assert p["heights"] == "const int*" and p["mean0"] == p["std2"] == "double"
    assert datasets.FundusPreprocess is fundus.FundusPreprocess
    assert datasets.FundusAutocrop is fundus.FundusAutocrop


def test_share_of_a_workgroup():
    share = _lib.load().lgnn_fundus_bbox_share
    assert share(5, 7) == 3 and share(64, 67) == 268          # one workgroup: every group
    assert share(128, 128) == 1024 and share(128, 129) == 516  # a second workgroup past 1024
    assert share(150, 250) == 782                              # 2344 groups over 3 workgroups
    assert share(2848, 4288) == (2848 * 4288 // 16 + 255) // 256
    assert share(1, 7) == 0 and share(5, 1 << 15) == 0


def test_bad_arguments_return_einval_before_any_launch():
    lib = _lib.load()
    E = _lib.LGNN_EINVAL
    b = torch.zeros(1 << 12, dtype=torch.uint8)  # host memory: never dereferenced
    p = b.data_ptr()
    import ctypes

    def table(*v, t=ctypes.c_void_p):
        return (t * len(v))(*v)

    def ints(*v):
        return table(*v, t=ctypes.c_int)

    def bbox(B=2, img=table(p, p), H=ints(9, 12), W=ints(7, 5), thr=25.0, boxes=p):
        return lib.lgnn_fundus_bbox(B, img, H, W, thr, boxes, None)

    for bad in (dict(img=None), dict(H=None), dict(W=None), dict(boxes=None), dict(B=0),
                dict(B=-1), dict(img=table(p, None)), dict(H=ints(9, 1)), dict(W=ints(1, 5)),
                dict(H=ints(9, _lib.LGNN_FUNDUS_MAX_SIDE + 1))):
        assert bbox(**bad) == E, bad

    def pre(B=2, img=table(p, p), masks=None, H=ints(9, 12), W=ints(7, 5), boxes=p, S=16,
            mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), out=p, u8=None, om=None,
            geom=None):
        return lib.lgnn_fundus_preprocess(B, img, masks, H, W, boxes, S, *mean, *std, out, u8, om,
                                          geom, None)

    for bad in (dict(img=None), dict(H=None), dict(W=None), dict(boxes=None), dict(B=0),
                dict(img=table(None, p)), dict(H=ints(1, 12)), dict(W=ints(7, 1)),
                dict(W=ints(7, _lib.LGNN_FUNDUS_MAX_SIDE + 1)), dict(S=1), dict(S=0),
                dict(S=_lib.LGNN_FUNDUS_MAX_SIDE + 1), dict(std=(0.229, 0.0, 0.225)),
                dict(std=(-0.229, 0.224, 0.225)), dict(std=(0.229, 0.224, float("nan"))),
                dict(mean=(float("inf"), 0.456, 0.406)),
                dict(out=None, u8=None),                      # both outputs NULL
                dict(om=p),                                   # out_mask without masks
                dict(om=p, masks=table(p, None))):            # a NULL mask among them
        assert pre(**bad) == E, bad


def test_cpu_tensors_raise():
    img = torch.zeros(2, 9, 7, 3, dtype=torch.uint8)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.fundus_bbox(img)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.fundus_bbox([img[0], img[1, :5]])
    boxes = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        ops.fundus_preprocess(img, boxes, 16, fundus.IMAGENET_DEFAULT_MEAN,
                              fundus.IMAGENET_DEFAULT_STD)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        fundus.FundusAutocrop().boxes(img)
    with pytest.raises(_lib.LgnnError, match="GPU only"):
        fundus.FundusPreprocess(16)(img)


def test_wrong_dtype_shape_or_size_raises(monkeypatch):
    with pytest.raises(ValueError, match="uint8"):
        ops.fundus_bbox(torch.zeros(2, 9, 7, 3))
    with pytest.raises(ValueError, match="uint8"):
        fundus.FundusPreprocess(16)([torch.zeros(9, 7, 3, dtype=torch.int32)])
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        ops.fundus_bbox(torch.zeros(2, 9, 7, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="non-empty list"):
        ops.fundus_bbox([])
    with pytest.raises(ValueError, match="square"):
        fundus.FundusPreprocess((16, 24))
    with pytest.raises(ValueError, match="at least 2"):
        fundus.FundusPreprocess(1)
    with pytest.raises(ValueError, match="std positive"):
        fundus.FundusPreprocess(16, normalization_std=(0.2, 0.0, 0.2))
    assert fundus.FundusPreprocess((16, 16)).img_size == 16
    assert fundus.FundusPreprocess([32, 32]).img_size == 32
    assert fundus.IMAGENET_DEFAULT_MEAN == (0.485, 0.456, 0.406)
    assert fundus.IMAGENET_DEFAULT_STD == (0.229, 0.224, 0.225)
    assert repr(fundus.FundusAutocrop(30)) == "FundusAutocrop(threshold=30.0)"
    # past the device check
    monkeypatch.setattr(_lib, "require_gpu", lambda *t: None)
    img = torch.zeros(2, 9, 7, 3, dtype=torch.uint8)
    boxes = torch.zeros(2, 4, dtype=torch.int32)
    mean, std = fundus.IMAGENET_DEFAULT_MEAN, fundus.IMAGENET_DEFAULT_STD
    with pytest.raises(ValueError, match=r"sides in \[2, 16384\]"):
        ops.fundus_bbox(img[:, :1])
    with pytest.raises(ValueError, match="size must be in"):
        ops.fundus_preprocess(img, boxes, 1, mean, std)
    with pytest.raises(ValueError, match="at least one of"):
        ops.fundus_preprocess(img, boxes, 16, mean, std, want_float=False)
    with pytest.raises(ValueError, match=r"boxes must be \(2, 4\) int32"):
        ops.fundus_preprocess(img, boxes[:1], 16, mean, std)
    with pytest.raises(ValueError, match="masks must match"):
        ops.fundus_preprocess(img, boxes, 16, mean, std, masks=img[:, :, :6, 0])
    with pytest.raises(ValueError, match="masks must be uint8"):
        ops.fundus_preprocess(img, boxes, 16, mean, std, masks=img[..., 0].long())


def test_from_paths_without_pil_names_the_alternative(monkeypatch):
    real = builtins.__import__

    def no_pil(name, *a, **kw):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **kw)

    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(ImportError, match="__call__"):
        fundus.FundusPreprocess(16).from_paths(["missing.png"])


def test_from_paths_on_a_missing_file():
    pytest.importorskip("PIL.Image")
    with pytest.raises(RuntimeError, match="Could not read image"):
        fundus.FundusPreprocess(16).from_paths(["no_such_file.png"])


def test_to_original_is_the_inverse_of_the_resize_mapping():
    geom = torch.tensor([[4, 5, 22, 30, 12, 16, 2, 0], [0, 0, 8, 8, 16, 16, 0, 0]],
                        dtype=torch.int32)
    batch = fundus.FundusBatch(image=None, uint8=None, mask=None, boxes=None, geom=geom)
    pos = torch.tensor([[2.0, 0.0], [13.0, 15.0]])
    got = batch.to_original(pos, 0)
    want = [[4 + 0.5 * 22 / 12 - 0.5, 5 + 0.5 * 30 / 16 - 0.5],
            [4 + 11.5 * 22 / 12 - 0.5, 5 + 15.5 * 30 / 16 - 0.5]]
    assert got.dtype == torch.float64
    torch.testing.assert_close(got, torch.tensor(want, dtype=torch.float64), rtol=0, atol=1e-12)
    two = batch.to_original(pos, torch.tensor([1, 0]))
    torch.testing.assert_close(two[0], torch.tensor([0.75, -0.25], dtype=torch.float64),
                               rtol=0, atol=1e-12)
    torch.testing.assert_close(two[1], got[1], rtol=0, atol=0)
