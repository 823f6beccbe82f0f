"""The condition of the fit fixture (tests/fit_ref.py), on the CPU: at the seeds of fit_ref.SEEDS
the float32 and the float64 oracle make the same decisions (which validations save, where the run
stops) and have equal confusion matrices at every validation and at the test, and the smallest
top-2 logit margin of the float64 run is at least 100 times the largest logit difference between
the two runs. Only then may tests/test_gpu_fit.py assert the device's counts and decisions equal
to the float64 oracle's: a float32 implementation of the same arithmetic cannot flip an argmax.

Measured here (margin / largest difference), chosen as the widest of seeds 0..19:
  gcn  batch 20: seed 7,  1.34e-2 / 6.5e-6 (2050 x)   batch 10000: seed 19, 9.66e-3 / 1.4e-6 (6845 x)
  gin  batch 20: seed 17, 3.75e-3 / 7.9e-6 (478 x)    batch 10000: seed 10, 5.52e-3 / 1.8e-5 (302 x)
  gat  batch 20: seed 7,  1.06e-2 / 4.7e-6 (2256 x)   batch 10000: seed 4,  6.28e-3 / 1.4e-6 (4387 x)
GIN runs at lr 1e-4: at 1e-3 none of the seeds 0..19 met the condition (ratios 2 to 43)."""
import pytest
import torch

from tests import fit_ref as fr


@pytest.mark.parametrize("batch_size", fr.BATCH_SIZES)
@pytest.mark.parametrize("family", fr.FAMILIES)
def test_fixture_condition(family, batch_size):
    r64 = fr.fit_oracle(family, batch_size, torch.float64)
    r32 = fr.fit_oracle(family, batch_size, torch.float32)
    holds, margin, diff = fr.fixture_condition(r64, r32)
    print(f"{family} batch {batch_size} seed {fr.SEEDS[family, batch_size]}: margin {margin:.3g}, "
          f"float32 - float64 {diff:.3g}, decisions {r64.decisions()}")
    assert holds, (margin, diff, r64.decisions(), r32.decisions())
    # the run is a whole one: three validations, a test on both datasets, every key of train()
    assert len(r64.validations) == 3 and len(r64.train_losses) == fr.MAX_EPOCHS
    assert sorted(r64.test) == sorted(f"test_{d}_{m}" for d in ("testA", "testB")
                                      for m in fr.METRIC_NAMES)
    assert fr.MONITOR in r64.validations[0] and "val_valB_loss" in r64.validations[0]


def test_collate_edges_ref_against_a_hand_made_case():
    # two graphs of 2 and 3 rows; edges (source, target) inside each
    ptr = torch.tensor([0, 2, 5])
    ei = torch.tensor([[0, 1, 1, 2, 3, 4, 4], [0, 0, 1, 2, 2, 3, 4]])
    w = torch.arange(7, dtype=torch.float32)
    eptr = torch.tensor([0, 3, 7])
    out, ow, optr = fr.collate_edges_ref(ei, w, eptr, ptr, [1, 0, 1])
    assert out.tolist() == [[0, 1, 2, 2, 3, 4, 4, 5, 6, 7, 7], [0, 0, 1, 2, 3, 3, 4, 5, 5, 6, 7]]
    assert ow.tolist() == [3, 4, 5, 6, 0, 1, 2, 3, 4, 5, 6] and optr.tolist() == [0, 4, 7, 11]
    out, ow, optr = fr.collate_edges_ref(ei, None, eptr, ptr, [])
    assert out.shape == (2, 0) and ow is None and optr.tolist() == [0]
