"""CPU: the trajectory bar of tests/trajectory_ref.py tests what it claims to (it tests the test,
so the GPU bar of tests/test_gpu_trajectory.py cannot hide a failure).

Conditioning: per family the float32 oracle's trajectory (the six-step schedule and the
captured-replay schedule) stays within 1e-4 x max|p| of the float64 oracle's on every compared
tensor, so the bar C x (that error) is tight. Measured, six steps: 1.5e-6 (gcn), 1.4e-5 on the
state and 6.0e-5 on the eval logits (gin), 1.1e-5 (gat, dropout masks on); captured schedule:
2.0e-6, 1.7e-5, 1.3e-6.

Detection: the mutant is the float32 oracle with ONE weight seen one step stale by ONE step's
forward and backward (step 3 of 6: what a kernel reading last step's copy of a weight would
compute). check(C = 16) must flag every tensor of the final state, the eval logits and every loss
from step 3 on; the smallest mutant ratio must be at least 30 x the bar (measured: 2514 gcn
loss/3, 686 gin eval logits, 5734 gat out_proj.bias; the largest 8e4 to 4e5), and the losses
before the mutation equal the oracle's. On the captured-replay schedule (lr 1e-3) the same mutant,
placed at the first replay, must fail the bar on most tensors."""
import pytest
import torch

from tests import trajectory_ref as tr

C_MAX = 16  # the largest C tests/test_gpu_trajectory.py may use
STALE = {"gcn": "convs.1.lin.weight", "gin": "convs.1.nn.lins.1.weight",
         "gat": "convs.2.lin.weight"}
MUTANT_STEP = 3


@pytest.fixture(scope="module")
def oracles():
    cache = {}

    def get(family, dtype, stale=None, captured=False):
        key = (family, dtype, stale, captured)
        if key not in cache:
            masks = tr.cpu_masks if family == "gat" else None
            kw = dict(batches=tr.capture_batches(family), eval_after=None, adam=tr.CAPTURE_ADAM,
                      scheduler=False) if captured else {}
            cache[key] = tr.run_oracle(family, dtype, masks, stale=stale, **kw)
        return cache[key]
    return get


@pytest.mark.parametrize("captured", [False, True], ids=["six_steps", "captured_schedule"])
@pytest.mark.parametrize("family", ["gcn", "gin", "gat"])
def test_float32_oracle_is_well_conditioned(oracles, family, captured):
    r64 = oracles(family, torch.float64, captured=captured).named()
    r32 = oracles(family, torch.float32, captured=captured).named()
    assert r64.keys() == r32.keys()
    worst = 0.0
    for k, v in r64.items():
        if not v.is_floating_point():
            assert torch.equal(v, r32[k]), k
            continue
        if tr.excluded(family, k):
            continue
        assert torch.isfinite(v).all() and torch.isfinite(r32[k]).all(), k
        rel = (r32[k] - v).abs().max().item() / max(v.abs().max().item(), 1e-30)
        print(f"{family} {k}: float32 oracle off by {rel:.3g} x max|p|")
        worst = max(worst, rel)
        assert rel <= 1e-4, f"{family} {k}: {rel:.3g}"
    print(f"{family}: worst {worst:.3g}")


@pytest.mark.parametrize("captured", [False, True], ids=["six_steps", "captured_schedule"])
@pytest.mark.parametrize("family", ["gcn", "gin", "gat"])
def test_one_stale_weight_for_one_step_is_caught(oracles, family, captured):
    r64 = oracles(family, torch.float64, captured=captured).named()
    r32 = oracles(family, torch.float32, captured=captured).named()
    mutant = oracles(family, torch.float32, (MUTANT_STEP, STALE[family]), captured).named()
    # the unmutated float32 oracle passes its own bar at C = 1, the mutant's early losses too
    tr.check(r32, r64, r32, 1.0, family)
    ratios = tr.ratios(mutant, r64, r32, family)
    for t in range(MUTANT_STEP):
        assert torch.equal(mutant[f"loss/{t}"], r32[f"loss/{t}"])
    # what the mutation can reach: everything but the earlier losses and the buffers no step
    # writes (GINConv.eps, train_eps=False), which stay at their initial value
    init = tr.initial_state(family)
    fixed = {f"state/{k}" for k, v in init.items() if torch.equal(r64[f"state/{k}"], tr.to64(v))}
    assert all(k.endswith(".eps") for k in fixed)
    hit = {k: v for k, v in ratios.items() if k not in fixed
           and not (k.startswith("loss/") and int(k[5:]) < MUTANT_STEP)}
    assert any(k.startswith("state/") for k in hit) and ("eval_logits" in hit or captured)
    k_min = min(hit, key=hit.get)
    print(f"{family}: smallest mutant ratio {hit[k_min]:.4g} ({k_min}), "
          f"largest {max(hit.values()):.4g}")
    with pytest.raises(AssertionError) as e:
        tr.check(mutant, r64, r32, C_MAX, family)
    if captured:
        # at lr = 1e-3 one step moves a weight a tenth as far: the bar still flags most tensors,
        # the clearest by more than 30 x the bar (measured: 2.2e4 to 9e4; the faintest, a loss one
        # step later, 14 for gcn)
        flagged = [k for k, v in hit.items() if v > C_MAX]
        assert 2 * len(flagged) > len(hit) and max(hit.values()) >= 30 * C_MAX
        assert all(k in str(e.value) for k in flagged)
        return
    assert hit[k_min] >= 30 * C_MAX, f"{family} {k_min}: {hit[k_min]:.4g}"
    assert all(k in str(e.value) for k in hit)  # every one reported, at once


def test_check_refuses_other_exclusions():
    t = {"state/w": torch.ones(2, dtype=torch.float64)}
    with pytest.raises(ValueError):
        tr.check(t, t, t, 1.0, "gcn", exclude=("in_proj.bias",))
    with pytest.raises(ValueError):
        tr.check(t, t, t, 1.0, "gin", exclude=("out_proj.bias",))
    tr.check(t, t, t, 1.0, "gin", exclude=tr.GIN_EXCLUDED)
    assert not tr.excluded("gcn", "state/in_proj.bias")
    assert tr.excluded("gin", "state/convs.2.nn.lins.0.bias")
    assert not tr.excluded("gin", "state/convs.1.nn.norms.0.module.running_mean")
    # integer buffers must be equal, whatever C
    n = {"state/n": torch.tensor(6)}
    with pytest.raises(AssertionError):
        tr.check({"state/n": torch.tensor(7)}, n, n, float("inf"), "gin")
