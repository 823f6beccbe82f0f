"""Reference statements of the set-attention path (test infrastructure, plain torch, any dtype).

Two builds of PyG 2.5.1 torch_geometric/nn/aggr/utils.py + set_transformer.py and of the
reference model src/lesion_gnn/models/set_transformer.py:16-66, over one state_dict layout:

* the restatement (`mab`, `sab`, `isab`, `pma`, `aggregation`, `model`): per set, no padding,
  hand-written softmax attention and LayerNorm, so it can take the attention-dropout masks the
  device drew (oracle.pyg_ref.DropoutMasks) where torch's MultiheadAttention draws its own;
* the padded build (`Padded*` modules): torch.nn.MultiheadAttention / LayerNorm / Linear on
  to_dense_batch-padded sets with key-padding masks, as PyG composes them. Its modules carry
  PyG's parameter names, so its state_dict is the reference's.

tests/test_set_transformer_ref.py pins the first against the second in float64; the GPU tests
compare the kernels with the first.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn


# ----------------------------------------------------------------------------------------------
# the restatement: lists of per-set row tensors
# ----------------------------------------------------------------------------------------------


def split_sets(x: torch.Tensor, sizes: list) -> list:
    return list(torch.split(x, list(sizes)))


def layer_norm(u, g, b, eps=1e-5):
    mu = u.mean(-1, keepdim=True)
    var = ((u - mu) ** 2).mean(-1, keepdim=True)  # biased
    return (u - mu) / torch.sqrt(var + eps) * g + b


class MaskFeed:
    """The flat attention-dropout masks of one forward, one per site in execution order; each
    site's mask is laid out [set][head][query][key]."""

    def __init__(self, masks: list | None):
        self.masks = list(masks) if masks is not None else None
        self.site = 0

    def next(self):
        if self.masks is None:
            return None
        m = self.masks[self.site]
        self.site += 1
        return m


def attention(q, k, v, heads, mask=None):
    """softmax(q_h k_h^T / sqrt(D)) [* mask] v_h of one set; mask flat [head][query][key]. No
    key: zero rows."""
    nq, nk, C = q.shape[0], k.shape[0], q.shape[1]
    D = C // heads
    if nk == 0:
        return q.new_zeros(nq, C) + 0.0 * q.sum() + 0.0 * (k.sum() + v.sum())
    qh = q.view(nq, heads, D).transpose(0, 1)
    kh = k.view(nk, heads, D).transpose(0, 1)
    vh = v.view(nk, heads, D).transpose(0, 1)
    s = qh @ kh.transpose(1, 2) / math.sqrt(D)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    P = e / e.sum(-1, keepdim=True)
    if mask is not None:
        P = P * mask.view(heads, nq, nk).to(P.dtype)
    return (P @ vh).transpose(0, 1).reshape(nq, C)


def mab(sd, pre, xs, ys, heads, feed: MaskFeed | None = None):
    """MultiheadAttentionBlock(x, y) per set. xs / ys: per-set query / key rows."""
    W, b = sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"]
    Wo, bo = sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"]
    Wl, bl = sd[pre + "lin.weight"], sd[pre + "lin.bias"]
    ln = (pre + "layer_norm1.weight") in sd
    C = W.shape[1]
    mask = feed.next() if feed is not None else None
    off = 0
    out = []
    for x, y in zip(xs, ys):
        nq, nk = x.shape[0], y.shape[0]
        q = x @ W[:C].T + b[:C]
        k = y @ W[C:2 * C].T + b[C:2 * C]
        v = y @ W[2 * C:].T + b[2 * C:]
        n = heads * nq * nk
        o = attention(q, k, v, heads, mask[off:off + n] if mask is not None else None)
        off += n
        u = o @ Wo.T + bo + x
        if ln:
            u = layer_norm(u, sd[pre + "layer_norm1.weight"], sd[pre + "layer_norm1.bias"])
        u = u + torch.relu(u @ Wl.T + bl)
        if ln:
            u = layer_norm(u, sd[pre + "layer_norm2.weight"], sd[pre + "layer_norm2.bias"])
        out.append(u)
    if mask is not None:
        assert off == mask.numel(), (off, mask.numel())
    return out


def sab(sd, pre, xs, heads, feed=None):
    return mab(sd, pre + "mab.", xs, xs, heads, feed)


def isab(sd, pre, xs, heads, feed=None):
    ind = sd[pre + "ind"][0]
    h = mab(sd, pre + "mab1.", [ind] * len(xs), xs, heads, feed)
    return mab(sd, pre + "mab2.", xs, h, heads, feed)


def pma(sd, pre, xs, heads, feed=None):
    W, b = sd[pre + "lin.weight"], sd[pre + "lin.bias"]
    ys = [torch.relu(x @ W.T + b) for x in xs]
    return mab(sd, pre + "mab.", [sd[pre + "seed"][0]] * len(xs), ys, heads, feed)


def _count(sd, pre):
    n = 0
    while any(k.startswith(f"{pre}{n}.") for k in sd):
        n += 1
    return n


def aggregation(sd, xs, heads, concat, masks=None):
    """SetTransformerAggregation over per-set rows xs: [B, S * C] or [B, C]."""
    feed = MaskFeed(masks)
    hs = xs
    for i in range(_count(sd, "encoders.")):
        hs = sab(sd, f"encoders.{i}.", hs, heads, feed)
    hs = pma(sd, "pma.", hs, heads, feed)
    for i in range(_count(sd, "decoders.")):
        hs = sab(sd, f"decoders.{i}.", hs, heads, feed)
    rows = []
    for x, h in zip(xs, hs):
        r = h.flatten() if concat else h.mean(0)
        rows.append(r if x.shape[0] > 0 else torch.zeros_like(r))  # nan_to_num of an empty set
    return torch.stack(rows)


def model(sd, xs, heads, concat=True, masks=None):
    """The reference SetTransformer over per-set input rows xs: logits [B, num_classes]."""
    feed = MaskFeed(masks)
    hs = [x @ sd["in_proj.weight"].T + sd["in_proj.bias"] for x in xs]
    for i in range(_count(sd, "encoders.")):
        hs = isab(sd, f"encoders.{i}.", hs, heads, feed)
    hs = pma(sd, "pma.", hs, heads, feed)
    for i in range(_count(sd, "decoders.")):
        hs = sab(sd, f"decoders.{i}.", hs, heads, feed)
    z = torch.stack([h.flatten() if concat else h.mean(0) for h in hs])
    return z @ sd["out_proj.weight"].T + sd["out_proj.bias"]


def site_numels(kind: str, sizes: list, heads: int, E: int, Dd: int, S: int, m: int = 0) -> list:
    """Mask sizes of one forward's attention sites in execution order (kind "aggregation" or
    "model")."""
    M, B = sum(sizes), len(sizes)
    if kind == "aggregation":
        enc = [heads * sum(n * n for n in sizes)] * E
    else:
        enc = [heads * m * M, heads * M * m] * E
    return enc + [heads * S * M] + [B * heads * S * S] * Dd


# ----------------------------------------------------------------------------------------------
# the padded build: PyG's composition of torch modules
# ----------------------------------------------------------------------------------------------


def to_dense_batch(x: torch.Tensor, batch: torch.Tensor, B: int):
    n = torch.bincount(batch, minlength=B)
    pos = torch.arange(x.shape[0]) - torch.repeat_interleave(torch.cumsum(n, 0) - n, n)
    dense = x.new_zeros(B, int(n.max()), x.shape[1])
    mask = torch.zeros(B, int(n.max()), dtype=torch.bool)
    dense[batch, pos] = x
    mask[batch, pos] = True
    return dense, mask


class PaddedMAB(nn.Module):
    def __init__(self, channels, heads=1, layer_norm=True, dropout=0.0):
        super().__init__()
        self.attn = nn.MultiheadAttention(channels, heads, batch_first=True, dropout=dropout)
        self.lin = nn.Linear(channels, channels)
        self.layer_norm1 = nn.LayerNorm(channels) if layer_norm else None
        self.layer_norm2 = nn.LayerNorm(channels) if layer_norm else None

    def forward(self, x, y, x_mask=None, y_mask=None):
        if y_mask is not None:
            y_mask = ~y_mask
        out, _ = self.attn(x, y, y, y_mask, need_weights=False)
        if x_mask is not None:
            out = out.masked_fill(~x_mask.unsqueeze(-1), 0.0)
        out = out + x
        if self.layer_norm1 is not None:
            out = self.layer_norm1(out)
        out = out + self.lin(out).relu()
        if self.layer_norm2 is not None:
            out = self.layer_norm2(out)
        return out


class PaddedSAB(nn.Module):
    def __init__(self, channels, heads=1, layer_norm=True, dropout=0.0):
        super().__init__()
        self.mab = PaddedMAB(channels, heads, layer_norm, dropout)

    def forward(self, x, mask=None):
        return self.mab(x, x, mask, mask)


class PaddedISAB(nn.Module):
    def __init__(self, channels, num_induced_points, heads=1, layer_norm=True, dropout=0.0):
        super().__init__()
        self.ind = nn.Parameter(torch.randn(1, num_induced_points, channels) * 0.3)
        self.mab1 = PaddedMAB(channels, heads, layer_norm, dropout)
        self.mab2 = PaddedMAB(channels, heads, layer_norm, dropout)

    def forward(self, x, mask=None):
        h = self.mab1(self.ind.expand(x.size(0), -1, -1), x, y_mask=mask)
        return self.mab2(x, h, x_mask=mask)


class PaddedPMA(nn.Module):
    def __init__(self, channels, num_seed_points=1, heads=1, layer_norm=True, dropout=0.0):
        super().__init__()
        self.lin = nn.Linear(channels, channels)
        self.seed = nn.Parameter(torch.randn(1, num_seed_points, channels) * 0.3)
        self.mab = PaddedMAB(channels, heads, layer_norm, dropout)

    def forward(self, x, mask=None):
        x = self.lin(x).relu()
        return self.mab(self.seed.expand(x.size(0), -1, -1), x, y_mask=mask)


class PaddedAggregation(nn.Module):
    def __init__(self, channels, num_seed_points=1, num_encoder_blocks=1, num_decoder_blocks=1,
                 heads=1, concat=True, layer_norm=False, dropout=0.0):
        super().__init__()
        self.concat = concat
        self.encoders = nn.ModuleList([PaddedSAB(channels, heads, layer_norm, dropout)
                                       for _ in range(num_encoder_blocks)])
        self.pma = PaddedPMA(channels, num_seed_points, heads, layer_norm, dropout)
        self.decoders = nn.ModuleList([PaddedSAB(channels, heads, layer_norm, dropout)
                                       for _ in range(num_decoder_blocks)])

    def forward(self, x, batch, B):
        x, mask = to_dense_batch(x, batch, B)
        for e in self.encoders:
            x = e(x, mask)
        x = self.pma(x, mask)
        for d in self.decoders:
            x = d(x)
        x = x.nan_to_num()
        return x.flatten(1, 2) if self.concat else x.mean(dim=1)


class PaddedSetTransformer(nn.Module):
    """The reference model file's module tree (set_transformer.py:16-66)."""

    def __init__(self, input_features, inner_dim, num_classes, num_inducing_points=1,
                 num_seed_points=1, num_encoder_blocks=1, num_decoder_blocks=1, heads=1,
                 concat=True, layer_norm=False, dropout=0.0):
        super().__init__()
        self.concat = concat
        self.in_proj = nn.Linear(input_features, inner_dim)
        self.encoders = nn.ModuleList(
            [PaddedISAB(inner_dim, num_inducing_points, heads, layer_norm, dropout)
             for _ in range(num_encoder_blocks)])
        self.pma = PaddedPMA(inner_dim, num_seed_points, heads, layer_norm, dropout)
        self.decoders = nn.ModuleList([PaddedSAB(inner_dim, heads, layer_norm, dropout)
                                       for _ in range(num_decoder_blocks)])
        self.out_proj = nn.Linear(inner_dim, num_classes)

    def forward(self, x, batch, B):
        x = self.in_proj(x)
        x, mask = to_dense_batch(x, batch, B)
        for e in self.encoders:
            x = e(x, mask)
        x = self.pma(x, mask)
        for d in self.decoders:
            x = d(x)
        x = x.flatten(1, 2) if self.concat else x.mean(dim=1)
        return self.out_proj(x)


def randomize_(module: nn.Module, seed: int = 0, scale: float = 0.3) -> None:
    """Non-trivial values for every parameter (biases and LayerNorm affine included: their
    default init, zeros and ones, would hide a swapped or dropped term)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64).to(p.dtype) * scale)
            if name.endswith(("layer_norm1.weight", "layer_norm2.weight")):
                p.add_(1.0)
