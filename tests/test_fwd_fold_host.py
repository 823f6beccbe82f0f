"""Host side of the folded fused GCN forward (no GPU): the new constants, the entries' argument
checks, and an fp32 emulation of the folded order of products.

Direct order (has_in_proj = 1): H_0 = X W_0^T + b_0 in fp32, then P = H_0 W_1^T. Folded order
(LGNN_S3_FWD_FOLD): W_10 = W_1 W_0 and b_10 = W_1 b_0 in fp32 (fmaf, j ascending), then
P = X W_10^T + 1 b_10^T. Both are compared with float64; the ratio of their errors is printed and
must stay below 3 (the factor of the GPU test's bar).
"""
import ctypes

import pytest
import torch

from lesion_gnn_amd import _lib


def test_constants_parse_from_header():
    assert _lib.ABI_VERSION == 40
    assert _lib.LGNN_S3_FWD_FOLD == 2 and _lib.LGNN_S3_FWD_FOLD_H0 == 3
    assert _lib.LGNN_PLANE_JOB_MAX == 8
    # the flag is a bit above every layer count
    assert _lib.LGNN_PLANE_JOB_FOLD > _lib.LGNN_PLANE_JOB_MAX
    assert _lib.LGNN_PLANE_JOB_FOLD & (_lib.LGNN_PLANE_JOB_FOLD - 1) == 0
    # lgnn_plane_job's layout is unchanged
    assert [f[0] for f in _lib.PlaneJob._fields_] == ["nl", "widths", "W", "planes", "planes_t"]


def test_plane_bytes_with_the_fold_slot():
    lib, F = _lib.load(), _lib.LGNN_PLANE_JOB_FOLD
    plane = 3 * 128 * 128 * 2
    for nl in (2, 3, 7):
        assert lib.lgnn_weight_planes_bytes(nl) == nl * plane
        assert lib.lgnn_weight_planes_bytes(nl | F) == (nl + 1) * plane + 128 * 4
    assert lib.lgnn_weight_planes_bytes(8) == 8 * plane
    assert lib.lgnn_weight_planes_bytes(1 | F) == 0  # no conv to fold into
    assert lib.lgnn_weight_planes_bytes(8 | F) == 0  # no room for b_0 behind the weights


def test_stack_fwd_refuses_unknown_modes():
    lib, E = _lib.load(), _lib.LGNN_EINVAL
    p = 4096  # any non-null address: the checks come before every use
    arr = ctypes.c_void_p * 3
    b, H = arr(p, p, p), arr(p, p, p)
    widths = (ctypes.c_int * 3)(128, 128, 128)
    for bad in (-1, 4, 5, 256):
        assert lib.lgnn_gcn_stack_fwd_s3(p, 64, 128, bad, p, p, p, 2, p, b, widths, H, p, None,
                                         None) == E
        assert lib.lgnn_gcn_stack_fwd_s3_all(p, 64, 128, bad, p, p, p, 2, p, arr(p, p, p), b,
                                             widths, H, arr(p, p), p, None, None) == E
    # folded: the fold slot needs a plane job of at most LGNN_PLANE_JOB_MAX - 1 layers
    L = 7
    a8 = ctypes.c_void_p * (L + 1)
    w8 = (ctypes.c_int * (L + 1))(*[128] * (L + 1))
    full = a8(*[p] * (L + 1))
    for mode in (_lib.LGNN_S3_FWD_FOLD, _lib.LGNN_S3_FWD_FOLD_H0):
        assert lib.lgnn_gcn_stack_fwd_s3(p, 64, 128, mode, p, p, p, L, p, full, w8, full, p, None,
                                         None) == E
    # M = 0 with a valid mode returns before any launch
    for mode in (0, 1, 2, 3):
        assert lib.lgnn_gcn_stack_fwd_s3(None, 0, 128, mode, p, p, p, 2, p, b, widths, H, p, None,
                                         None) == _lib.LGNN_OK


def test_flagged_plane_job_refuses_bad_arguments():
    lib, E, F = _lib.load(), _lib.LGNN_EINVAL, _lib.LGNN_PLANE_JOB_FOLD
    p = 4096
    widths = (ctypes.c_int * 9)(*[128] * 9)

    def planes(nl, ws):
        return lib.lgnn_weight_planes(nl, (ctypes.c_void_p * len(ws))(*ws), widths, p, None, None)

    assert planes(3 | F, [p, p, p, None]) == E       # b_0 missing
    assert planes(8 | F, [p] * 9) == E               # more than the maximum minus one
    assert planes(1 | F, [p, p]) == E                # no conv
    assert planes(9, [p] * 9) == E                   # (unflagged: as before)

    def build(nl, ws):
        job = _lib.PlaneJob()
        job.nl = nl
        for i in range(9):
            job.widths[i] = 128
        for i, w in enumerate(ws):
            job.W[i] = w
        job.planes = p
        return lib.lgnn_graph_build_planes(p, 8, 64, 0, 1, p, p, p, None, None, None, None, None,
                                           None, 0, None, None, p, 1 << 20, 0,
                                           ctypes.byref(job), None)

    assert build(3 | F, [p, p, p, None]) == E
    assert build(8 | F, [p] * 8) == E
    assert build(1 | F, [p, p]) == E
    assert build(0, []) == E


# (M, d_in, w1, w2)
SHAPES = [(4096, 128, 128, 128), (2560, 36, 64, 32), (2560, 128, 16, 128), (273, 128, 128, 128),
          (392, 20, 32, 96), (64, 128, 128, 128)]


def fold_fp32(W1: torch.Tensor, W0: torch.Tensor, b0: torch.Tensor):
    """The plane job's fold item: fp32 fmaf sums over j ascending (a product and an add rounded
    once, taken in float64 — exact for fp32 operands up to the final rounding — then to fp32)."""
    acc = torch.zeros(W1.size(0), W0.size(1), dtype=torch.float32)
    bacc = torch.zeros(W1.size(0), dtype=torch.float32)
    for j in range(W0.size(0)):
        c = W1[:, j].double()
        acc = (c[:, None] * W0[j].double()[None, :] + acc.double()).float()
        bacc = (c * b0[j].double() + bacc.double()).float()
    return acc, bacc


@pytest.mark.parametrize("shape", SHAPES)
def test_folded_order_error_vs_direct(shape):
    M, d_in, w1, w2 = shape
    gen = torch.Generator().manual_seed(M + d_in + w1 + w2)
    torch.manual_seed(M + 7 * d_in + w1 + w2)
    X = torch.randn(M, d_in, generator=gen)
    l0, l1 = torch.nn.Linear(d_in, w1), torch.nn.Linear(w1, w2)
    W0, W1 = l0.weight.detach(), l1.weight.detach()
    b0 = l0.bias.detach() + torch.randn(w1, generator=gen)
    want = (X.double() @ W0.double().t() + b0.double()) @ W1.double().t()
    direct = (X @ W0.t() + b0) @ W1.t()
    W10, b10 = fold_fp32(W1, W0, b0)
    folded = X @ W10.t() + b10
    e_dir = (direct.double() - want).abs()
    e_fold = (folded.double() - want).abs()
    ratio = e_fold.max().item() / e_dir.max().item()
    rms = (e_fold.pow(2).mean().sqrt() / e_dir.pow(2).mean().sqrt()).item()
    print(f"{shape}: direct {e_dir.max().item():.3e} folded {e_fold.max().item():.3e} "
          f"max ratio {ratio:.2f} rms ratio {rms:.2f}")
    assert ratio < 3
