"""CPU: the cases and the bar of tests/tile_width_cases.py are what the GPU tests of
tests/test_gpu_tile_widths.py take them for.

- every size case has the tile structure it is named for (open flags, node count, a 1-node graph
  and a graph smaller than k where stated);
- every width case is eligible for the tile fast path at every layer and plans the fused GCN
  forward and backward (a later change in eligibility would otherwise let the GPU tests pass on
  some other kernel);
- the bar is not degenerate: the float64 and float32 oracle steps are finite and differ, and the
  float32 oracle at one CPU thread passes the bar against the default thread count with the C the
  GPU tests use (measured on an 8-thread CPU: gcn 0.97 x at the most; gin 7.1 x on w_b
  tail_open, grad/convs.0.nn.lins.1.bias, a column sum that cancels, 4.6 x the next: the scale is
  one float32 run, so a ratio is only as steady as that run). GIN's vanishing gradients are
  printed there, not held to the device's 5e-6 floor: that floor is absolute while their rounding
  noise grows with the gradients' scale, and plain torch float32 at one thread sits at 5.3e-6 on
  w_c / tail_open / add (largest gradient 19), where the device measures 9.6e-7 at the most.
"""
import pytest
import torch

from lesion_gnn_amd import ops
from tests import tile_width_cases as tw
from tests import trajectory_ref as tr

MODEL_CASES = [("gcn", w, s) for w in tw.WIDTH_CASES for s in tw.SIZE_CASES] + \
              [("gin", w, s) for w in tw.GIN_WIDTH_CASES for s in tw.GIN_SIZE_CASES]


@pytest.mark.parametrize("scase", list(tw.SIZE_CASES))
def test_size_case_tile_structure(scase):
    sizes = tw.SIZE_CASES[scase]
    assert sum(sizes) == tw.NODES[scase] <= 444
    for wcase in tw.WIDTH_CASES:
        b = tw.batch(wcase, scase)
        assert b.num_nodes == tw.NODES[scase] and b.num_graphs == len(sizes)
        assert tw.open_flags(b.edge_index, b.num_nodes) == tw.FLAGS[scase], wcase
        assert int(b.y.max()) < tw.WIDTH_CASES[wcase][2]
        # every tile far below the 2048 CSR entries a closed tile may hold (64 x (k + 1))
        assert b.edge_index.size(1) <= tw.K_NN * b.num_nodes


def test_size_cases_cover_the_edges():
    mixed = tw.SIZE_CASES["mixed"]
    assert 1 in mixed and any(1 < n < tw.K_NN for n in mixed)
    f = tw.FLAGS["mixed"]
    assert f[0] == 0 and f[1] == 0       # a full closed tile, a closed tile of two graphs
    assert mixed[:3] == [64, 30, 34]
    assert f[4] == 0 and 1 in f[:4]      # a closed tile after open ones
    assert f[-1] == 1 and tw.NODES["mixed"] % 64  # the partial last tile is open
    assert tw.NODES["tail_open"] % 64 == 1 and tw.FLAGS["tail_open"][-1] == 1
    assert tw.NODES["tail_closed"] % 64 == 37 and not any(tw.FLAGS["tail_closed"])
    assert tw.NODES["m65"] % 64 == 1 and tw.FLAGS["m65"] == [1, 1]
    assert tw.NODES["m63"] == 63 and tw.NODES["one"] == 1


def test_width_cases_cover_the_edges():
    widths = set()
    for d_in, hidden, _ in tw.WIDTH_CASES.values():
        widths |= {d_in, *hidden}
    assert min(widths) == 4 and max(widths) == 128
    assert any(4 < w < 16 for w in widths)
    assert 36 in widths and 68 in widths and 124 in widths
    steps = [b - a for _, h, _ in tw.WIDTH_CASES.values() for a, b in zip(h, h[1:])]
    assert min(steps) < 0 < max(steps)   # widths change in both directions between layers
    assert [4, 68, 128] == tw.WIDTH_CASES["w_b"][1]  # 128 next to narrow widths
    assert {c for _, _, c in tw.WIDTH_CASES.values()} == {3, 5, 8}
    assert all(w % 32 for w in widths - {128})  # none a multiple of 32 but 128 itself


@pytest.mark.parametrize("wcase", list(tw.WIDTH_CASES))
def test_width_case_is_on_the_tile_kernels(wcase):
    d_in, hidden, classes = tw.WIDTH_CASES[wcase]
    shapes = tw.layer_shapes(wcase)
    assert all(ops.fast_shape(K, N) for N, K in shapes)
    L = len(hidden) - 1
    plan = ops.gcn_plan(shapes, L, lazy_ok=True)
    assert plan.fused and plan.fused_bwd and plan.keeps_planes and all(plan.saved_s)
    assert plan.kind == "gcn_lazy"
    assert classes <= 8  # the head fold of the single-launch backward takes every case
    if wcase in tw.GIN_WIDTH_CASES:
        assert ops.fast_shape(d_in, hidden[0])
        for a, b in zip(hidden, hidden[1:]):
            assert ops.gin_bn_fused(a, b, b) and ops.gin_plan(a, b, b).bn_fused
    for K, N in tw.LINEAR_KN:
        assert ops.fast_shape(K, N)


@pytest.mark.parametrize("family,wcase,scase", MODEL_CASES)
def test_oracles_are_finite_and_differ(family, wcase, scase):
    pools = ("mean", "add") if family == "gin" else (tw.POOL[wcase],)
    for pool in pools:
        r64, r32 = tw.oracle_pair(family, wcase, scase, pool)
        assert r64.keys() == r32.keys()
        differ = 0
        for k, v in r64.items():
            assert torch.isfinite(v.double()).all() and torch.isfinite(r32[k].double()).all(), k
            if v.is_floating_point() and not torch.equal(v, r32[k]):
                differ += 1
            if v.is_floating_point() and k not in tw.zero_grad_keys(family, r64):
                rel = (r32[k] - v).abs().max().item() / max(v.abs().max().item(), 1e-30)
                assert rel <= 1e-5, f"{k}: float32 oracle off by {rel:.3g} x max|t|"
        assert differ >= len(r64) // 2, (differ, len(r64))
        # the float32 oracle passes its own bar at C = 1
        tw.check(r32, r64, r32, 1.0, family, tr.GIN_EXCLUDED if family == "gin" else None)


@pytest.mark.parametrize("family,wcase,scase", MODEL_CASES)
def test_float32_oracle_at_one_thread_passes_the_bar(family, wcase, scase):
    pool = "add" if family == "gin" else tw.POOL[wcase]
    r64, r32 = tw.oracle_pair(family, wcase, scase, pool)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        one = tw.step(tw.build(family, wcase, pool, oracle=True), tw.batch(wcase, scase),
                      torch.float32, eval_after=family == "gin")
    finally:
        torch.set_num_threads(threads)
    r = tw.ratios(one, r64, r32, family, tr.GIN_EXCLUDED if family == "gin" else None)
    print(f"{family} {wcase} {scase}: one thread at {tw.worst(r)[0]:.3g} x ({tw.worst(r)[1]})")
    bad = {k: v for k, v in r.items() if not v <= tw.C}
    assert not bad, bad
    z = tw.zero_grad_errors(one, r64, family)
    print(f"{family} {wcase} {scase}: vanishing gradients off by {z}")
    assert all(v < float("inf") for v in z.values())


def test_check_refuses_other_exclusions():
    t = {"grad/w": torch.ones(2, dtype=torch.float64)}
    with pytest.raises(ValueError):
        tw.check(t, t, t, 1.0, "gcn", exclude=("in_proj.bias",))
    with pytest.raises(ValueError):
        tw.check(t, t, t, 1.0, "gin", exclude=("out_proj.bias",))
    tw.check(t, t, t, 1.0, "gin", exclude=tr.GIN_EXCLUDED)
    # a vanishing gradient is held to the absolute floor, not dropped
    z = {"grad/in_proj.bias": torch.zeros(2, dtype=torch.float64)}
    off = {"grad/in_proj.bias": torch.full((2,), 1e-5, dtype=torch.float64)}
    nan = {"grad/in_proj.bias": torch.full((2,), float("nan"), dtype=torch.float64)}
    tw.check(z, z, z, 1.0, "gin", exclude=tr.GIN_EXCLUDED)
    for bad in (off, nan):
        with pytest.raises(AssertionError):
            tw.check(bad, z, z, float("inf"), "gin", exclude=tr.GIN_EXCLUDED)
    # the BatchNorm statistics are under the ratio bar here, every one
    s = {"state/convs.0.nn.norms.0.module.running_mean": torch.ones(2, dtype=torch.float64)}
    s_off = {k: v + 1e-3 for k, v in s.items()}
    with pytest.raises(AssertionError):
        tw.check(s_off, s, s, 16.0, "gin", exclude=tr.GIN_EXCLUDED)
