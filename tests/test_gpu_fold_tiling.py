"""GPU: the two in_proj fold products, bit for bit against an exact fp32-fma oracle on the CPU.

  * the fold slot of the plane job (s3_util.h wplanes_fold_item; 2 rows of W_10 per workgroup, one
    (n, k) per thread): W_10[n][k] is the fp32 fmaf chain over j ascending from +0, b_10[n] the
    same chain with b_0; W_10 is split into three RNE bf16 planes stored in fragment order, with
    zeros past the widths. Run from lgnn_weight_planes (k_wplanes), from k_prep and from
    k_prep_sorted; the layers' slots are those of the job without the fold.
  * the fold launch lgnn_gcn_fold_wgrad (foldgrad.hip; 2 output rows per workgroup, one element
    per thread): dW_0[i][k] the chain over n ascending, dW_1[n][i] the chain over k ascending, then
    fmaf(g[n], b_0[i], .), then the open total; db_0[i] four interleaved double chains (n mod 4)
    combined as (s0 + s1) + (s2 + s3), plus the open total in double, cast once. With live = null,
    1 and 0, and the open totals absent, separate and aliased to the outputs.

The oracle's fmaf is a float64 product (exact: 24 + 24 bits) plus the addend with the sum's error
recovered by TwoSum and folded in as a sticky bit (round to odd), then one rounding to float32;
`test_oracle_methods_agree` (no GPU) checks it against libm's fmaf term by term on every chain of
these inputs.

The widths [d_in, w1, w2] have rows and columns that are no multiple of the 2 (or the earlier 8)
rows per workgroup, one 16-byte piece per row, chains shorter than 64 terms and chains that are
not, and sizes past which only padding is left.
"""
import ctypes
import ctypes.util
import functools

import numpy as np
import pytest
import torch

from lesion_gnn_amd import _lib, ops, synth
from lesion_gnn_amd.graph import Graph

WIDTHS = [[4, 4, 4], [36, 64, 32], [128, 16, 128], [20, 8, 12], [12, 128, 100]]
_ids = ["-".join(map(str, w)) for w in WIDTHS]
f32 = np.float32


# ----------------------------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """Correctly rounded float32 a * b + c, elementwise (float32 arrays in, float32 out)."""
    p = a.astype(np.float64) * b.astype(np.float64)  # exact
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c = s + err exactly
    # round to odd: where s is inexact and its last bit even, the neighbour on err's side
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return odd.astype(np.float32)


def chain32(A, B):
    """[n][k] = the fmaf chain over j ascending of A[n][j] B[j][k], from +0."""
    acc = np.zeros((A.shape[0], B.shape[1]), f32)
    for j in range(A.shape[1]):
        acc = fma32(A[:, j:j + 1], B[j:j + 1, :], acc)
    return acc


@functools.lru_cache(maxsize=None)
def _scalar_fmaf():
    """libm's fmaf (math.fma is the float64 one: rounding its result to float32 rounds twice)."""
    fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").fmaf
    fn.restype = ctypes.c_float
    fn.argtypes = [ctypes.c_float] * 3
    return fn


def chain32_scalar(A, B):
    fmaf = _scalar_fmaf()
    out = np.zeros((A.shape[0], B.shape[1]), f32)
    Al, Bl = A.tolist(), B.tolist()
    for n in range(A.shape[0]):
        for k in range(B.shape[1]):
            acc = 0.0
            for j in range(A.shape[1]):
                acc = fmaf(Al[n][j], Bl[j][k], acc)
            out[n, k] = acc
    return out


def bf16_rne(v):
    """float32 -> (bf16 bits as uint16, the bf16 value as float32), round to nearest even."""
    u = v.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16))
    r = r.astype(np.uint32)
    return r.astype(np.uint16), (r << np.uint32(16)).view(np.float32)


def split3(v):
    """The three planes of v = hi + mid + lo, [3][...] uint16."""
    out = []
    for i in range(3):
        bits, back = bf16_rne(np.ascontiguousarray(v))
        out.append(bits)
        if i < 2:
            v = v - back
    return np.stack(out)


def _perm16(k):
    return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1)


def decode_slot(raw_slot):
    """49152 uint16 of one slot in fragment order -> [plane][row][k] uint16."""
    s = raw_slot.reshape(3, 4, 8, 2, 32, 8).transpose(0, 1, 4, 2, 3, 5).reshape(3, 128, 128)
    return s[:, :, _perm16(np.arange(128))]


@functools.lru_cache(maxsize=None)
def _slot_inputs(i):
    d_in, w1, w2 = WIDTHS[i]
    gen = torch.Generator().manual_seed(31 + i)
    W0 = torch.randn(w1, d_in, generator=gen) / d_in ** 0.5
    W1 = torch.randn(w2, w1, generator=gen) / w1 ** 0.5
    b0 = torch.randn(w1, generator=gen)
    return W0, W1, b0


@functools.lru_cache(maxsize=None)
def _slot_oracle(i):
    """(planes [3][128][128] uint16, b_10 [128] float32) of the fold slot, zero padded."""
    d_in, w1, w2 = WIDTHS[i]
    W0, W1, b0 = (t.numpy() for t in _slot_inputs(i))
    W10 = np.zeros((128, 128), f32)
    W10[:w2, :d_in] = chain32(W1, W0)
    b10 = np.zeros(128, f32)
    b10[:w2] = chain32(W1, b0[:, None])[:, 0]
    return split3(W10), b10


@functools.lru_cache(maxsize=None)
def _fold_inputs(i):
    d_in, w1, w2 = WIDTHS[i]
    gen = torch.Generator().manual_seed(57 + i)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float32)

    return dict(T=rnd(w2, d_in), g=rnd(w2), W0=rnd(w1, d_in), b0=rnd(w1), W1=rnd(w2, w1),
                o0=rnd(w1, d_in), ob=rnd(w1), o1=rnd(w2, w1))


@functools.lru_cache(maxsize=None)
def _fold_oracle(i):
    """The closed sums (dW_0, db_0 in double, dW_1) before the open totals."""
    p = {k: v.numpy() for k, v in _fold_inputs(i).items()}
    dW0 = chain32(np.ascontiguousarray(p["W1"].T), p["T"])
    dW1 = fma32(p["g"][:, None], p["b0"][None, :], chain32(p["T"], np.ascontiguousarray(p["W0"].T)))
    W1d, gd = p["W1"].astype(np.float64), p["g"].astype(np.float64)
    s4 = np.zeros((4, W1d.shape[1]))
    for n in range(W1d.shape[0]):
        s4[n % 4] = W1d[n] * gd[n] + s4[n % 4]  # (the product of two float32 is exact in double)
    db0 = (s4[0] + s4[1]) + (s4[2] + s4[3])
    return dW0, db0, dW1


def _fold_want(i, live, opens):
    """Outputs of the fold launch: `opens` None or the three open totals (numpy)."""
    dW0, db0, dW1 = _fold_oracle(i)
    if not live:
        dW0, db0, dW1 = np.zeros_like(dW0), np.zeros_like(db0), np.zeros_like(dW1)
    if opens is None:
        return dW0, db0.astype(f32), dW1
    return dW0 + opens[0], (db0 + opens[1].astype(np.float64)).astype(f32), dW1 + opens[2]


# ----------------------------------------------------------------------------------------------
# no GPU: the oracle against libm's fmaf on these inputs
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(WIDTHS)), ids=_ids)
def test_oracle_methods_agree(i):
    W0, W1, b0 = (t.numpy() for t in _slot_inputs(i))
    p = {k: v.numpy() for k, v in _fold_inputs(i).items()}
    for A, B in ((W1, W0), (W1, b0[:, None]), (np.ascontiguousarray(p["W1"].T), p["T"]),
                 (p["T"], np.ascontiguousarray(p["W0"].T))):
        a, b = chain32(A, B), chain32_scalar(A, B)
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_fma32_double_rounding_midpoint():
    """a b exactly on a float32 midpoint, c far below float64's last bit: the float64 sum is the
    midpoint itself and only the sticky bit says which side the exact value lies on."""
    a, b = f32(3), f32(1 + 2.0 ** -23)  # a b = 3 + 2^-22 + 2^-23; float32 spacing there: 2^-22
    for c, want in ((f32(-2.0 ** -80), f32(3 + 2.0 ** -22)), (f32(2.0 ** -80), f32(3 + 2.0 ** -21))):
        got = fma32(np.array([a]), np.array([b]), np.array([c]))[0]
        assert got == want == f32(_scalar_fmaf()(float(a), float(b), float(c)))
    assert f32(float(a) * float(b) + -2.0 ** -80) == f32(3 + 2.0 ** -21)  # (rounding twice fails)


# ----------------------------------------------------------------------------------------------
# the fold slot
# ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(WIDTHS)), ids=_ids)
def test_fold_slot_bits(cuda, i):
    widths = WIDTHS[i]
    nl = 2
    W0, W1, b0 = (t.to(cuda) for t in _slot_inputs(i))
    Ws = [W0, W1]
    want_planes, want_b10 = _slot_oracle(i)
    b = synth.make_batch(3, n=64, k=4, d_in=4, seed=2)
    ei = b.edge_index.to(cuda)
    gen = torch.Generator().manual_seed(9)
    shuffled = ei[:, torch.randperm(ei.size(1), generator=gen).to(cuda)].contiguous()
    got = {}

    def job():
        planes, _ = ops.plane_buffers(Ws, fold=True)
        planes.fill_(0x7A7A)
        return planes, ops.plane_job(Ws, widths[0], planes, None, b0)

    planes, j = job()
    ops.run_plane_job(j, cuda)
    got["lgnn_weight_planes"] = planes
    for name, edges, kind, sorted_on in (("k_prep_sorted", ei, "gcn_lazy", 1),
                                         ("k_prep_sorted, unsorted edges", shuffled, "gcn_lazy", 1),
                                         ("k_prep", ei, "gcn", 1),
                                         ("k_prep lazy", shuffled, "gcn_lazy", 0)):
        planes, j = job()
        with _lib.path_option(_lib.LGNN_OPT_GRAPH_SORTED, sorted_on):
            _, done = Graph(edges, b.num_nodes).csr_planes(kind, j)
        assert done, name
        got[name] = planes
    torch.cuda.synchronize()
    plain, _ = ops.weight_planes(Ws, widths[0])
    plain = plain.cpu().flatten()
    for name, p in got.items():
        p = p.cpu()
        assert torch.equal(p[:nl * 49152], plain), f"{name}: the layers' slots differ"
        raw = p.numpy().view(np.uint16)
        slot = decode_slot(raw[nl * 49152:(nl + 1) * 49152])
        assert np.array_equal(slot, want_planes), \
            f"{name}: {int((slot != want_planes).sum())} plane elements differ"
        b10 = raw[(nl + 1) * 49152:].view(np.float32)
        assert b10.shape == (128,)
        assert np.array_equal(b10.view(np.int32), want_b10.view(np.int32)), f"{name}: b_10"
    # the padding of the oracle itself is zero, so the slots' is
    d_in, w1, w2 = widths
    assert not want_planes[:, w2:].any() and not want_planes[:, :, d_in:].any()
    assert not want_b10[w2:].any()


# ----------------------------------------------------------------------------------------------
# the fold launch
# ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("open_mode", ["absent", "separate", "aliased"])
@pytest.mark.parametrize("live", [None, 1, 0])
@pytest.mark.parametrize("i", range(len(WIDTHS)), ids=_ids)
def test_fold_launch_bits(cuda, i, live, open_mode):
    d_in, w1, w2 = WIDTHS[i]
    p = _fold_inputs(i)
    alive = live is None or live == 1
    T, g = p["T"].to(cuda), p["g"].to(cuda)
    if not alive:  # unread
        T, g = torch.full_like(T, float("nan")), torch.full_like(g, float("nan"))
    W0, b0, W1 = p["W0"].to(cuda), p["b0"].to(cuda), p["W1"].to(cuda)
    word = None if live is None else torch.full((1,), live, dtype=torch.int32, device=cuda)
    totals = [p["o0"], p["ob"], p["o1"]]
    if open_mode == "absent":
        opens = [None, None, None]
        outs = [torch.full(sh, float("nan"), device=cuda) for sh in ((w1, d_in), (w1,), (w2, w1))]
    elif open_mode == "separate":
        opens = [t.to(cuda) for t in totals]
        outs = [torch.full_like(t, float("nan")) for t in opens]
    else:
        outs = [t.to(cuda) for t in totals]
        opens = outs
    _lib.call("lgnn_gcn_fold_wgrad", T, g, W0, b0, W1, d_in, w1, w2, *opens, word, *outs,
              _lib.stream(cuda))
    torch.cuda.synchronize()
    want = _fold_want(i, alive, None if open_mode == "absent" else [t.numpy() for t in totals])
    for name, got, w in zip(("dW0", "db0", "dW1"), outs, want):
        got = got.cpu().numpy()
        assert got.shape == w.shape and got.dtype == w.dtype == np.float32, name
        assert np.array_equal(got.view(np.int32), w.view(np.int32)), \
            f"{name}: {int((got.view(np.int32) != w.view(np.int32)).sum())} elements differ"
    if not alive and open_mode == "aliased":  # the totals, untouched
        for got, t in zip(outs, totals):
            assert torch.equal(got.cpu().view(torch.int32), t.view(torch.int32))
    if open_mode == "separate":  # and the totals given apart are only read
        for t, o in zip(opens, totals):
            assert torch.equal(t.cpu(), o)
