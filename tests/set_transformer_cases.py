"""Shared inputs and bars of the set-attention tests (CPU reference test and GPU tests).

Bars: outputs within 1e-4 absolute at unit-scale inputs; each gradient within
1e-4 x max|grad| of its tensor, with the 5e-6 absolute floor."""
from __future__ import annotations

import torch

from lesion_gnn_amd import _lib, synth

QB = _lib.LGNN_SET_ATTN_QROWS
KB = _lib.LGNN_SET_ATTN_KROWS

OUT_ATOL = 1e-4
GRAD_RTOL = 1e-4
GRAD_FLOOR = 5e-6

# set sizes of the kernel tests: the empty set in the middle, both block edges
KERNEL_SIZES = [1, 0, 7, KB - 1, KB, KB + 1, 2 * KB + 3, QB + 1]
HEAD_SHAPES = [(1, 1), (3, 1), (2, 4), (2, 20), (2, 64), (1, 128), (8, 16)]

AGG_VARIANTS = {
    "ln_mean": dict(channels=32, num_seed_points=16, num_encoder_blocks=2, num_decoder_blocks=2,
                    heads=2, layer_norm=True, concat=False),
    "concat": dict(channels=32, num_seed_points=1, num_encoder_blocks=1, num_decoder_blocks=1,
                   heads=2, layer_norm=False, concat=True),
}
MODEL_KW = dict(input_features=37, inner_dim=64, num_classes=5, num_inducing_points=3,
                num_seed_points=1, num_encoder_blocks=1, num_decoder_blocks=1, heads=4,
                layer_norm=True, dropout=0.0)


def module_batch(d_in: int, empty: bool = True):
    """(synth batch, sizes): 12 log-normal sets, one above KB rows and (empty) one without rows."""
    sizes = synth.graph_sizes(12, "lognormal", torch.Generator().manual_seed(5))
    sizes = [min(s, KB - 2) for s in sizes]
    sizes[7] = KB + 9
    if empty:
        sizes[3] = 0
    return synth.make_batch(12, k=2, d_in=d_in, seed=3, sizes=sizes), sizes


def assert_output(got: torch.Tensor, want: torch.Tensor, what: str = "output") -> float:
    err = (got.double().cpu() - want.double()).abs().max().item() if want.numel() else 0.0
    print(f"{what}: max|err| {err:.3e}")
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert err <= OUT_ATOL, f"{what}: {err:.3e} > {OUT_ATOL}"
    return err


def assert_grad(got: torch.Tensor, want: torch.Tensor, what: str) -> float:
    scale = want.abs().max().item() if want.numel() else 0.0
    err = (got.double().cpu() - want.double()).abs().max().item() if want.numel() else 0.0
    tol = max(GRAD_RTOL * scale, GRAD_FLOOR)
    print(f"{what}: max|err| {err:.3e} (max|grad| {scale:.3e}, bar {tol:.3e})")
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    return err
