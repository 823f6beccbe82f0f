"""A restatement, kernel by kernel, of the formulas csrc/gat.hip documents (plain torch on the CPU).

Test-only; next to tests/trajectory_ref.py. Every function is dtype-parametric: it computes in the
dtype of the floating tensors it is given, so the same code is ref64 (the reference) and ref32 (the
scale of the bar, tests/gat_cases.py). Each function takes what its kernel takes, so a test hands
it the device's own float32 a_s, a_d, alpha, Y, dZ, da_e and da_d, widened: every kernel is then
compared on its own, and no logit changes sign between the two sides (the float32 sum of two
float32 numbers has the sign of the exact sum).

  att       lgnn_gat_att        a_s[j,h] = <xp_j[h], att_src[h]>, a_d[i,h] = <xp_i[h], att_dst[h]>
  fwd       lgnn_gat_fwd        e_ij = leaky(a_s[j] + a_d[i]); alpha = exp(e - max_i e) /
                                (sum_i exp(.) + 1e-16); Y_i = act(sum_j alpha_ij mask_ij xp_j + bias)
  bwd_edge  lgnn_gat_bwd_edge   the comment above k_gat_bwd_edge
  pool_dY   the dY lgnn_gat_bwd_edge_pool forms from the readout's gradient
  bwd_node  lgnn_gat_bwd_node + lgnn_reduce_partials   the comment above k_gat_bwd_node

tests/test_gat_ref.py pins the chain att -> fwd -> bwd_edge -> bwd_node to the float64 autograd of
oracle.pyg_ref.GATConv.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

import oracle.pyg_ref as ref

ACT_NONE, ACT_ELU = "none", "elu"


class Csr(NamedTuple):
    """The "gat" CSR of Graph.csr("gat"): entries grouped by target, edge order inside a row, the
    re-added self loop last."""
    n: int
    rowptr: torch.Tensor  # int64 [n + 1]
    col: torch.Tensor     # int64 [nnz] source of each entry
    dst: torch.Tensor     # int64 [nnz] target (row) of each entry


class TCsr(NamedTuple):
    """Its transpose: entries grouped by source."""
    n: int
    tptr: torch.Tensor  # int64 [n + 1]
    tidx: torch.Tensor  # int64 [nnz] target of each transposed entry
    tmap: torch.Tensor  # int64 [nnz] target-CSR position of each transposed entry
    src: torch.Tensor   # int64 [nnz] source (row) of each transposed entry


def _ptr(index: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n + 1, dtype=torch.int64)
    out[1:] = torch.bincount(index, minlength=n).cumsum(0)
    return out


def gat_csr(edge_index: torch.Tensor, n: int) -> tuple[Csr, TCsr]:
    """edge_index [2, E] (source, target) -> (Csr, TCsr) over remove_self_loops + add_self_loops,
    stably sorted by target (by source for the transpose)."""
    ei = ref.add_self_loops(ref.remove_self_loops(edge_index), n)
    perm = torch.sort(ei[1], stable=True).indices
    col, dst = ei[0][perm], ei[1][perm]
    tperm = torch.sort(col, stable=True).indices
    return (Csr(n, _ptr(dst, n), col, dst),
            TCsr(n, _ptr(col, n), dst[tperm], tperm, col[tperm]))


def _heads(t: torch.Tensor, H: int) -> torch.Tensor:
    return t.reshape(t.size(0), H, -1)


def leaky(v: torch.Tensor, slope: float) -> torch.Tensor:
    return torch.where(v > 0, v, v * slope)


def att(XP, att_src, att_dst, H: int):
    """XP [M, H*C], att_src / att_dst [H*C] -> a_s, a_d [M, H]."""
    xs = _heads(XP, H)
    return ((xs * att_src.reshape(1, H, -1)).sum(-1), (xs * att_dst.reshape(1, H, -1)).sum(-1))


def logits(a_s, a_d, csr: Csr, slope: float):
    """e [nnz, H] in CSR order."""
    return leaky(a_s[csr.col] + a_d[csr.dst], slope)


def fwd(XP, a_s, a_d, csr: Csr, slope: float, mask, bias, act: str):
    """-> alpha [nnz, H] (the unmasked softmax), Y [M, H*C]. mask [nnz, H] or None multiplies the
    message only."""
    H = a_s.size(1)
    e = logits(a_s, a_d, csr, slope)
    m = ref.scatter_max(e, csr.dst, csr.n)
    ex = (e - m[csr.dst]).exp()
    alpha = ex / (ref.scatter_sum(ex, csr.dst, csr.n) + 1e-16)[csr.dst]
    w = alpha if mask is None else alpha * mask
    out = ref.scatter_sum(w.unsqueeze(-1) * _heads(XP, H)[csr.col], csr.dst, csr.n)
    Y = out.reshape(csr.n, -1)
    if bias is not None:
        Y = Y + bias
    if act == ACT_ELU:
        Y = torch.nn.functional.elu(Y)
    return alpha, Y


def bwd_edge(XP, a_s, a_d, alpha, mask, dY, Y, act: str, slope: float, csr: Csr):
    """-> dZ [M, H*C], da_e [nnz, H], da_d [M, H].
        dZ_i = dY_i act'(Y_i)  (ELU' from the saved output: h > 0 ? 1 : h + 1)
        dal_ij = <dZ_i[h], xp_j[h]> mask_ij;  s_i = sum_j alpha_ij dal_ij
        da_ij = alpha_ij (dal_ij - s_i) leaky'(a_s[j] + a_d[i])  (the slope at 0, as torch)
        da_d[i] = sum_j da_ij"""
    H = a_s.size(1)
    dZ = dY * torch.where(Y > 0, torch.ones_like(Y), Y + 1) if act == ACT_ELU else dY.clone()
    dal = (_heads(dZ, H)[csr.dst] * _heads(XP, H)[csr.col]).sum(-1)
    if mask is not None:
        dal = dal * mask
    s = ref.scatter_sum(alpha * dal, csr.dst, csr.n)
    pre = a_s[csr.col] + a_d[csr.dst]
    da_e = alpha * (dal - s[csr.dst]) * torch.where(pre > 0, torch.ones_like(pre),
                                                    torch.full_like(pre, slope))
    return dZ, da_e, ref.scatter_sum(da_e, csr.dst, csr.n)


def pool_dY(dlogits, Wout, batch, gptr, mean: bool):
    """dY[i] = (dlogits[g] Wout) (/ |g| with mean pooling), g = batch[i]: the output gradient
    lgnn_gat_bwd_edge_pool forms (global pool + out_proj backward)."""
    dpooled = dlogits @ Wout
    if mean:
        cnt = (gptr[1:] - gptr[:-1]).clamp(min=1).to(dpooled.dtype)
        dpooled = dpooled / cnt.unsqueeze(-1)
    return dpooled[batch]


def bwd_node(alpha, mask, da_e, da_d, dZ, XP, att_src, att_dst, tcsr: TCsr):
    """-> dXP [M, H*C], d att_src, d att_dst, d bias [H*C].
        dXP_j[h] = sum_{j->i} alpha_ij mask_ij dZ_i[h] + (sum_i da_ij) att_src[h] + da_d[j] att_dst[h]"""
    H = alpha.size(1)
    n = tcsr.n
    w = alpha if mask is None else alpha * mask
    msg = ref.scatter_sum(w[tcsr.tmap].unsqueeze(-1) * _heads(dZ, H)[tcsr.tidx], tcsr.src, n)
    sda = ref.scatter_sum(da_e[tcsr.tmap], tcsr.src, n)
    xs = _heads(XP, H)
    dXP = msg + sda.unsqueeze(-1) * att_src.reshape(1, H, -1) + \
        da_d.unsqueeze(-1) * att_dst.reshape(1, H, -1)
    d_src = (sda.unsqueeze(-1) * xs).sum(0).reshape(-1)
    d_dst = (da_d.unsqueeze(-1) * xs).sum(0).reshape(-1)
    return dXP.reshape(n, -1), d_src, d_dst, dZ.sum(0)


def chain(x, W, att_src, att_dst, bias, csr: Csr, tcsr: TCsr, H: int, slope: float, mask,
          act: str, dY) -> dict:
    """The whole conv in the dtype of x: lin, att, fwd, bwd_edge, bwd_node and lin's backward."""
    XP = x @ W.T
    a_s, a_d = att(XP, att_src, att_dst, H)
    alpha, Y = fwd(XP, a_s, a_d, csr, slope, mask, bias, act)
    dZ, da_e, da_d = bwd_edge(XP, a_s, a_d, alpha, mask, dY, Y, act, slope, csr)
    dXP, d_src, d_dst, d_bias = bwd_node(alpha, mask, da_e, da_d, dZ, XP, att_src, att_dst, tcsr)
    return {"Y": Y, "dx": dXP @ W, "dW": dXP.T @ x, "datt_src": d_src, "datt_dst": d_dst,
            "dbias": d_bias}
