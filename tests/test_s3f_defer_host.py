"""Host side of the deferred in_proj fold (no GPU): the new entries' declarations, the fold
entry's argument checks, and an fp32 emulation of the deferred summation order.

Deferred order: T = sum over tiles of G_t^T X_t and g = sum of colsum G_t in fp32, then
dW_1 = T W_0^T + g b_0^T once. Direct order (the legacy mode of the kernel): H_0 = X W_0^T + b_0 in
fp32, then dW_1 = sum over tiles of G_t^T H_{0,t}. Both are compared with float64; the ratio of
their errors is printed and must stay below 3 (the factor of the GPU test's bar).
"""
import pytest
import torch

from lesion_gnn_amd import _lib

TM = 64


def test_entries_parse_from_header():
    fold = _lib.PARAMS["lgnn_gcn_fold_wgrad"]
    assert [n for _, n in fold] == ["T", "g", "W0", "b0", "W1", "d_in", "w1", "w2", "dW0_open",
                                    "db0_open", "dW1_open", "live", "dW0", "db0", "dW1",
                                    "stream"]
    assert fold[0] == ("const float*", "T") and fold[12] == ("float*", "dW0")
    assert fold[11] == ("const int32_t*", "live")
    live = _lib.PARAMS["lgnn_reduce_jobs_live"]
    assert [n for _, n in live] == [n for _, n in _lib.PARAMS["lgnn_reduce_jobs_ce"]][:-1] + \
        ["live", "stream"]
    assert live[-2] == ("const int32_t* const*", "live")
    assert _lib.ABI_VERSION == 40


def test_fold_entry_refuses_bad_arguments():
    lib, E = _lib.load(), _lib.LGNN_EINVAL
    p = 4096  # any non-null address: the checks come before every use

    def fold(T, d_in, w1, w2):
        return lib.lgnn_gcn_fold_wgrad(T, p, p, p, p, d_in, w1, w2, None, None, None, None, p, p,
                                       p, None)

    assert fold(None, 128, 128, 128) == E
    for bad in (132, 256, 126, 30, 0, -4):
        assert fold(p, bad, 128, 128) == E
        assert fold(p, 128, bad, 128) == E
        assert fold(p, 128, 128, bad) == E
    assert lib.lgnn_gcn_fold_wgrad(p, None, p, p, p, 128, 128, 128, None, None, None, None, p, p,
                                   p, None) == E
    assert lib.lgnn_gcn_fold_wgrad(p, p, p, p, p, 128, 128, 128, None, None, None, None, p, p,
                                   None, None) == E
    assert lib.lgnn_reduce_jobs_live(1, None, None, None, None, None, None, None, None, 0, None,
                                     None) == E


# (M, d_in, w1, w2): the GPU test's shapes (rows = 64 x graphs, or the sizes' sums)
SHAPES = [(300 * 64, 128, 128, 128), (40 * 64, 36, 64, 32), (40 * 64, 128, 16, 128),
          (273, 128, 128, 128), (392, 128, 128, 128)]


@pytest.mark.parametrize("shape", SHAPES)
def test_deferred_order_error_vs_direct(shape):
    M, d_in, w1, w2 = shape
    gen = torch.Generator().manual_seed(M + d_in + w1 + w2)
    X = torch.randn(M, d_in, generator=gen)
    G = torch.randn(M, w2, generator=gen)
    lin = torch.nn.Linear(d_in, w1)
    W0 = lin.weight.detach()
    b0 = lin.bias.detach() + torch.randn(w1, generator=gen)
    want = G.double().t() @ (X.double() @ W0.double().t() + b0.double())
    H0 = X @ W0.t() + b0
    direct = torch.zeros(w2, w1)
    T = torch.zeros(w2, d_in)
    g = torch.zeros(w2)
    for r in range(0, M, TM):
        Gt = G[r:r + TM]
        direct += Gt.t() @ H0[r:r + TM]
        T += Gt.t() @ X[r:r + TM]
        g += Gt.sum(0)
    deferred = T @ W0.t() + torch.outer(g, b0)
    e_dir = (direct.double() - want).abs().max().item()
    e_def = (deferred.double() - want).abs().max().item()
    print(f"{shape}: direct {e_dir:.3e} deferred {e_def:.3e} ratio {e_def / e_dir:.2f}")
    assert e_def < 3 * e_dir
