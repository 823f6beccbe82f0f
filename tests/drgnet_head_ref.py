"""Plain-torch restatement of the DRGNet head (helper of the head tests; holds no tests).

Written from the formulas of the head kernels' contract (include/lgnn.h, "DRGNet head"), on CPU
tensors of whatever float dtype the caller passes (float64 for the tests' reference):

  z1[b, r, :] = W1 x_row(b, r) + b1                       x [B, k * D], W1 [c0, 1, D]
  a1[b, q, :] = max(ELU(z1[b, 2q, :]), ELU(z1[b, 2q + 1, :]))   q < K2 = k // 2; a tie: the first
  a2[b, c, p] = ELU(b2[c] + sum_{i, t} W2[c, i, t] a1[b, p + t, i])   p < P = K2 - 4
  h = ELU(L0 flat(a2) + b0) * mask,  flat index c * P + p
  logits = L1 h + bL1

The max pool is spelled with torch.where on a strict comparison, so that the gradient of a tied
pair lands on its first row by construction (as torch's max_pool1d routes it).
"""
import torch
import torch.nn.functional as F

PARAM_NAMES = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "lins.0.weight",
               "lins.0.bias", "lins.1.weight", "lins.1.bias")


def z_rows(x, k, w1, b1):
    """z1 [B, k, c0]."""
    B, D = x.size(0), x.size(1) // k
    # products summed row by row (no GEMM blocking): equal rows give bitwise equal results, so a
    # duplicated row is an exact tie here as it is in the kernel
    return (x.view(B, k, 1, D) * w1.view(1, 1, w1.size(0), D)).sum(-1) + b1


def elu_rows(x, k, w1, b1):
    """ELU(z1) [B, k, c0]."""
    return F.elu(z_rows(x, k, w1, b1))


def head(x, k, w1, b1, w2, b2, l0w, l0b, l1w, l1b, mask=None):
    B = x.size(0)
    K2 = k // 2
    z = z_rows(x, k, w1, b1)[:, :2 * K2]              # an odd k drops its last row
    first, second = z[:, 0::2], z[:, 1::2]            # [B, K2, c0]
    # max(ELU(a), ELU(b)) = ELU(max(a, b)), ELU being monotone: the choice is made on z, where two
    # equal rows (every pair of padding rows) tie exactly. Made on ELU's outputs it would hang on
    # the CPU's vectorised expm1, whose vector body and scalar tail may round one input two ways.
    a1 = F.elu(torch.where(second > first, second, first))
    P = K2 - 4
    c1 = w2.size(0)
    z2 = b2.view(1, c1, 1).expand(B, c1, P)
    for t in range(5):                                # a2[b, c, p] += W2[c, :, t] . a1[b, p + t, :]
        z2 = z2 + torch.einsum("ci,bpi->bcp", w2[:, :, t], a1[:, t:t + P])
    a2 = F.elu(z2).reshape(B, c1 * P)
    h = F.elu(a2 @ l0w.t() + l0b)
    if mask is not None:
        h = h * mask
    return h @ l1w.t() + l1b


def pair_gaps(x, k, w1, b1, real_rows):
    """Smallest |ELU(z1[2q]) - ELU(z1[2q + 1])| over the pooled pairs that are not two padding
    rows (real_rows [B]: the number of real rows per graph)."""
    e = elu_rows(x, k, w1, b1)
    K2 = k // 2
    gap = (e[:, 0:2 * K2:2] - e[:, 1:2 * K2:2]).abs()  # [B, K2, c0]
    q = torch.arange(K2).view(1, K2, 1)
    real = (2 * q < real_rows.view(-1, 1, 1)).expand_as(gap)  # the pair's first row is real
    return float(gap[real].min()) if bool(real.any()) else float("inf")
