"""GPU: `lesion_gnn_amd.training.train` on the fixture of tests/fit_ref.py, against the CPU
oracle of the same run in float64 (fit_ref.fit_oracle).

a. test_fit_vs_float64_oracle (gcn, gin, gat; three steps per epoch and one): the train-loss
   sequence, every validation loss, the final state_dict and the state_dict inside the best
   checkpoint file are held to the bar of tests/trajectory_ref.py,
       max|got - ref64| <= C x max(max|ref32 - ref64|, 1e-6 max|ref64|),
   with the C of tests/test_gpu_trajectory.py (16) and its GIN exclusions, no others. Given the
   fixture condition (tests/test_fit_ref.py), the confusion matrices of every validation and of
   the test, the validations that saved, the last epoch run and the test dict's keys equal the
   float64 oracle's, exactly. The metrics derived from those counts (kappa, accuracy, F1,
   precision, recall), and auroc and auprc, are compared at 1e-12 relative, the tolerance
   tests/test_gpu_metrics.py holds the same quantities to: the device and numpy evaluate the
   same ratios of equal integers, in another order of float64 operations.
b. test_resume: fit 20 epochs, then resume to 30 from last.ckpt, and from the best checkpoint
   file, which was written at a validation in the middle of the run. Two identical uninterrupted
   30-epoch runs are compared first; where they are bitwise equal, each resumed run must be bitwise
   the uninterrupted one in state_dict and in the loss sequence, otherwise it is held to bar a.
c. test_script_main: scripts.train.main on saved stores and a config file returns train()'s dict.

Every test prints its largest ratios before it asserts."""
import math
import os

import numpy as np
import pytest
import torch

from lesion_gnn_amd import training
from lesion_gnn_amd.datasets import GraphStore
from tests import fit_ref as fr
from tests import trajectory_ref as tr
from tests.test_gpu_trajectory import C

pytestmark = pytest.mark.gpu

CASES = [(f, b) for f in fr.FAMILIES for b in fr.BATCH_SIZES]


@pytest.fixture(scope="module")
def stores(cuda):
    return {name: GraphStore(x.to(cuda), pos.to(cuda), y, ptr)
            for name, (x, pos, y, ptr) in fr.fixture_tensors().items()}


@pytest.fixture(scope="module")
def device_runs(stores, tmp_path_factory):
    """(family, batch_size) -> (test dict, trainer, run_dir) of training.run, each run once."""
    cache = {}

    def get(family, batch_size):
        key = (family, batch_size)
        if key not in cache:
            run_dir = tmp_path_factory.mktemp(f"{family}-{batch_size}")
            out, trainer, _ = training.run(fr.make_config(family, batch_size), stores, run_dir)
            cache[key] = (out, trainer, run_dir)
        return cache[key]
    return get


def named(trainer) -> dict:
    """The device run's compared tensors under fit_ref.FitResult.named()'s keys."""
    out = {f"train_loss/{e}": torch.tensor(v, dtype=torch.float64)
           for e, v in enumerate(trainer.train_losses)}
    for i, metrics in enumerate(trainer.validations):
        for name in ("valA", "valB"):
            out[f"val_loss/{i}/{name}"] = torch.tensor(metrics[f"val_{name}_loss"],
                                                       dtype=torch.float64)
    cb = trainer.checkpoint_callback
    for tag, path in (("final", cb.last_model_path), ("best", cb.best_model_path)):
        state = torch.load(path, map_location="cpu", weights_only=True)["state_dict"]
        out.update({f"{tag}/{k}": v for k, v in fr.strip_state(state).items()})
    return out


def report(what, ratios):
    for k, v in sorted(ratios.items(), key=lambda kv: -kv[1])[:8]:
        print(f"{what} {k}: {v:.3g}")


def same(got: float, want: float, rel: float = 1e-12) -> bool:
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("family,batch_size", CASES)
def test_fit_vs_float64_oracle(cuda, device_runs, family, batch_size):
    r64 = fr.fit_oracle(family, batch_size, torch.float64)
    r32 = fr.fit_oracle(family, batch_size, torch.float32)
    assert fr.fixture_condition(r64, r32)[0]
    out, trainer, run_dir = device_runs(family, batch_size)
    cb = trainer.checkpoint_callback

    # decisions and counts: equal to the float64 oracle's
    assert (tuple(cb.saved), trainer.current_epoch) == r64.decisions()
    assert len(trainer.validations) == len(r64.validations) == 3
    for got, want in zip(trainer.val_confusion_matrices + [trainer.confusion_matrices],
                         r64.val_confusions + [r64.test_confusions], strict=True):
        assert sorted(got) == sorted(want)
        for name in want:
            assert np.array_equal(got[name].numpy(), want[name]), name
    assert sorted(out) == sorted(r64.test)
    for key, want in r64.test.items():
        assert same(out[key], want), (key, out[key], want)
    for got, want in zip(trainer.validations, r64.validations, strict=True):
        assert sorted(got) == sorted(want)
        for key in want:
            if not key.endswith("_loss"):
                assert same(got[key], want[key]), (key, got[key], want[key])

    # the files: one best checkpoint named after its epoch and step, last.ckpt, the log
    steps = len(range(0, 48, batch_size))
    best_epoch = 10 * cb.saved[-1] + 9
    assert sorted(os.listdir(run_dir)) == sorted(
        [f"epoch={best_epoch}-step={steps * (best_epoch + 1)}.ckpt", "last.ckpt", "metrics.jsonl"])
    last = torch.load(cb.last_model_path, map_location="cpu", weights_only=True)
    assert last["epoch"] == 29 and last["global_step"] == 30 * steps
    assert all(k.startswith(("model.", "criterion.")) for k in last["state_dict"])
    assert len(last["optimizer_states"]) == 1 and last["lr_schedulers"] == []
    assert last["monitor"] == fr.MONITOR and same(last["best_score"], cb.best_score)

    # the numbers: the float64 oracle's, within C times the float32 oracle's own distance
    got = named(trainer)
    detail = {}
    ratios = tr.ratios(got, r64.named(), r32.named(), family, detail)
    report(f"fit {family} batch {batch_size}", ratios)
    worst = max(ratios, key=ratios.get)
    print(f"fit {family} batch {batch_size}: max ratio {ratios[worst]:.4g} ({worst}) over "
          f"{len(ratios)} tensors")
    tr.check(got, r64.named(), r32.named(), C, family,
             exclude=tr.GIN_EXCLUDED if family == "gin" else None)


def _losses_and_state(trainer):
    state = torch.load(trainer.checkpoint_callback.last_model_path, map_location="cpu",
                       weights_only=True)["state_dict"]
    return list(trainer.train_losses), state


def _bitwise(a, b) -> bool:
    return a[0] == b[0] and a[1].keys() == b[1].keys() and \
        all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_resume(cuda, stores, device_runs, tmp_path):
    family, batch_size = "gcn", 20
    first = _losses_and_state(device_runs(family, batch_size)[1])
    _, again, _ = training.run(fr.make_config(family, batch_size), stores, tmp_path / "again")
    deterministic = _bitwise(first, _losses_and_state(again))
    print(f"two uninterrupted runs bitwise equal: {deterministic}")

    part = tmp_path / "part"
    _, short, _ = training.run(fr.make_config(family, batch_size, max_epochs=20), stores, part)
    assert short.current_epoch == 19 and len(short.train_losses) == 20
    _, resumed, _ = training.run(fr.make_config(family, batch_size), stores, part,
                                 ckpt_path=part / "last.ckpt")
    assert resumed.current_epoch == 29 and len(resumed.validations) == 1  # epoch 29's only
    assert resumed.checkpoint_callback.saved == again.checkpoint_callback.saved
    got = _losses_and_state(resumed)
    # from the middle of a run: the best file of a 20-epoch fit, written at a validation
    mid = tmp_path / "mid"
    _, short2, _ = training.run(fr.make_config(family, batch_size, max_epochs=20), stores, mid)
    best = short2.checkpoint_callback.best_model_path
    at = torch.load(best, map_location="cpu", weights_only=True)
    assert at["callbacks"][0]["best_model_path"] == best and at["epoch"] in (9, 19)
    _, resumed2, _ = training.run(fr.make_config(family, batch_size), stores, mid, ckpt_path=best)
    assert len(resumed2.validations) == (29 - at["epoch"]) // 10
    assert resumed2.checkpoint_callback.saved == again.checkpoint_callback.saved
    assert os.path.exists(resumed2.checkpoint_callback.best_model_path)
    got2 = _losses_and_state(resumed2)
    if deterministic:
        for g in (got, got2):
            assert g[0] == first[0]
            for k, v in first[1].items():
                assert torch.equal(g[1][k], v), k
        return
    # not reproducible bit for bit on this device: the resumed run is held to the oracle bar
    r64 = fr.fit_oracle(family, batch_size, torch.float64)
    r32 = fr.fit_oracle(family, batch_size, torch.float32)

    def pick(d):
        return {k: v for k, v in d.items() if k.startswith(("train_loss/", "final/"))}

    for g in (got, got2):
        named_got = {f"train_loss/{e}": torch.tensor(v, dtype=torch.float64)
                     for e, v in enumerate(g[0])}
        named_got.update({f"final/{k}": v for k, v in fr.strip_state(g[1]).items()})
        tr.check(named_got, pick(r64.named()), pick(r32.named()), C, family)


def test_script_main(cuda, stores, device_runs, tmp_path, capsys):
    from lesion_gnn_amd.scripts import train as script

    family, batch_size = "gcn", 10000
    want = device_runs(family, batch_size)[0]
    store_dir = tmp_path / "stores"
    store_dir.mkdir()
    for name, store in stores.items():
        store.save(store_dir / f"{name}.pt")
    config = tmp_path / "config.py"
    config.write_text("from tests.fit_ref import make_config\n"
                      f"cfg = make_config({family!r}, {batch_size})\n")
    got = script.main(["--config", str(config), "--stores", str(store_dir),
                       "--run-dir", str(tmp_path / "run")])
    assert sorted(got) == sorted(want)
    for key in want:
        assert same(got[key], want[key], 0.0), (key, got[key], want[key])
    import json
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(printed) == sorted(want)
    assert os.path.exists(tmp_path / "run" / "last.ckpt")
