"""Host side of lesion_gnn_amd.training (no GPU): ModelCheckpoint and EarlyStopping on scripted
metric sequences, the split of the transform chain into hoisted and per-batch parts, the
validation schedule and the scheduler check, and `Trainer.fit` itself over a small module and
datamodule on the host: the schedule of the loop, the state inside the checkpoints written at a
validation, and a resume from such a checkpoint."""
import json
import math
import os

import pytest
import torch

from lesion_gnn_amd.datasets import DataConfig, hoisted_transforms
from lesion_gnn_amd.datasets.datamodule import ToSparseTensor
from lesion_gnn_amd.knn import KNNGraph, RadiusGraph
from lesion_gnn_amd.training import EarlyStopping, ModelCheckpoint, Trainer
from lesion_gnn_amd.transforms import GaussianDistance, TransformConfig

KEY = "val_DDR_kappa"


def run_checkpoint(tmp_path, mode, values):
    """Feed one value per validation (epochs 9, 19, ...; 3 steps per epoch): (callback, the
    directory's files after each validation)."""
    cb = ModelCheckpoint(tmp_path, KEY, mode)
    listing = []
    for i, v in enumerate(values):
        epoch = 10 * i + 9
        cb.on_validation_end({KEY: v, "other": 1.0}, epoch, 3 * (epoch + 1),
                             lambda e=epoch: {"epoch": e, "state_dict": {"w": torch.ones(1) * e}})
        listing.append(sorted(os.listdir(tmp_path)))
    return cb, listing


def test_checkpoint_max_improvement_tie_and_file_names(tmp_path):
    cb, listing = run_checkpoint(tmp_path, "max", [0.5, 0.5, 0.7, 0.6])
    # the first validation saves; the tie keeps the old file; 0.7 replaces it; 0.6 does not
    assert listing == [["epoch=9-step=30.ckpt", "last.ckpt"]] * 2 + \
        [["epoch=29-step=90.ckpt", "last.ckpt"]] * 2
    assert cb.saved == [0, 2] and cb.best_score == 0.7
    assert cb.best_model_path == os.path.join(str(tmp_path), "epoch=29-step=90.ckpt")
    best = torch.load(cb.best_model_path, weights_only=True)
    last = torch.load(cb.last_model_path, weights_only=True)
    assert best["epoch"] == 29 and best["monitor"] == KEY and best["best_score"] == 0.7
    assert last["epoch"] == 39 and last["best_score"] == 0.7  # last.ckpt follows every validation
    assert float(best["state_dict"]["w"]) == 29.0


def test_checkpoint_min_mode(tmp_path):
    cb, listing = run_checkpoint(tmp_path, "min", [1.0, 1.5, 0.9, 0.9])
    assert cb.saved == [0, 2] and cb.best_score == 0.9
    assert listing[-1] == ["epoch=29-step=90.ckpt", "last.ckpt"]


def test_checkpoint_first_validation_always_saves_and_nan_never_improves(tmp_path):
    cb, listing = run_checkpoint(tmp_path, "max", [math.nan, 0.1, math.nan])
    assert cb.saved == [0, 1] and cb.best_score == 0.1
    assert listing[0] == ["epoch=9-step=30.ckpt", "last.ckpt"]
    assert listing[-1] == ["epoch=19-step=60.ckpt", "last.ckpt"]


def test_checkpoint_last_at_end_of_fit_and_missing_key(tmp_path):
    cb = ModelCheckpoint(tmp_path, KEY, "max")
    cb.save_last_checkpoint({"epoch": 4})
    assert os.listdir(tmp_path) == ["last.ckpt"] and cb.best_model_path is None
    with pytest.raises(KeyError, match="val_APTOS_kappa"):  # the logged keys are listed
        cb.on_validation_end({"val_APTOS_kappa": 0.3}, 9, 30, dict)
    with pytest.raises(ValueError):
        ModelCheckpoint(tmp_path, KEY, "best")


def stops_at(mode, patience, values):
    """The index of the validation at which EarlyStopping asks to stop (None: never)."""
    cb = EarlyStopping(KEY, mode, patience)
    for i, v in enumerate(values):
        if cb.on_validation_end({KEY: v}):
            return i
    return None


@pytest.mark.parametrize("mode,sign", [("max", 1.0), ("min", -1.0)])
def test_early_stopping_patience(mode, sign):
    up = [sign * v for v in (0.1, 0.2, 0.3, 0.4)]
    for patience in (0, 1, 3):
        assert stops_at(mode, patience, up) is None  # strict improvements never stop
    flat = [sign * v for v in (0.1, 0.2, 0.2, 0.15, 0.1, 0.0, 0.0)]
    assert stops_at(mode, 0, flat) == 2   # the tie is no improvement
    assert stops_at(mode, 1, flat) == 2
    assert stops_at(mode, 3, flat) == 4
    # an improvement resets the wait
    again = [sign * v for v in (0.1, 0.0, 0.0, 0.3, 0.2, 0.2, 0.2)]
    assert stops_at(mode, 3, again) == 6
    assert stops_at(mode, 1, [sign * 0.5]) is None  # the first validation improves on nothing


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
@pytest.mark.parametrize("mode", ["max", "min"])
def test_early_stopping_not_finite_stops_at_once(mode, bad):
    assert stops_at(mode, 3, [0.1, bad, 0.5]) == 1
    assert stops_at(mode, 3, [bad]) == 0


def test_early_stopping_missing_key():
    with pytest.raises(KeyError, match="val_APTOS_kappa"):
        EarlyStopping(KEY, "max", 1).on_validation_end({"val_APTOS_kappa": 0.3})


def chain(*transforms):
    return DataConfig(train_datasets=[], val_datasets=[], test_datasets=[],
                      transforms=list(transforms), batch_size=4, num_workers=0)


KNN = TransformConfig(name="KNNGraph", kwargs=dict(k=6, loop=True))
RADIUS = TransformConfig(name="RadiusGraph", kwargs=dict(r=0.1))
WEIGHT = TransformConfig(name="GaussianDistance", kwargs=dict(sigma=0.3))
ATTR = TransformConfig(name="GaussianDistance", kwargs=dict(sigma=0.3, save_as="edge_attr_cat"))
SPARSE = TransformConfig(name="ToSparseTensor")


def kinds(ts):
    return [type(t) for t in ts]


def test_hoisted_transforms_split():
    assert [kinds(p) for p in hoisted_transforms(chain(KNN))] == [[KNNGraph], []]
    assert [kinds(p) for p in hoisted_transforms(chain(KNN, WEIGHT))] == \
        [[KNNGraph, GaussianDistance], []]
    assert [kinds(p) for p in hoisted_transforms(chain(ATTR))] == [[], [GaussianDistance]]
    assert [kinds(p) for p in hoisted_transforms(chain(RADIUS, SPARSE))] == \
        [[RadiusGraph], [ToSparseTensor]]
    assert hoisted_transforms(chain()) == ([], [])
    # an edge_attr mode ends the run; weights without a graph to weigh are not hoisted
    assert [kinds(p) for p in hoisted_transforms(chain(KNN, ATTR, WEIGHT))] == \
        [[KNNGraph], [GaussianDistance, GaussianDistance]]
    assert [kinds(p) for p in hoisted_transforms(chain(WEIGHT, KNN))] == \
        [[], [GaussianDistance, KNNGraph]]


def test_validation_schedule():
    t = Trainer(max_epochs=25)
    assert [e for e in range(t.max_epochs) if t.validates_after(e)] == [9, 19]
    t = Trainer(max_epochs=7, check_val_every_n_epoch=3)
    assert [e for e in range(t.max_epochs) if t.validates_after(e)] == [2, 5]


class Batch:
    def __init__(self, x, y):
        self.x, self.y, self.num_graphs = x, y, x.size(0)


class Evaluator:
    device = torch.device("cpu")

    def confusion_matrix(self):
        return torch.zeros(2, 2, dtype=torch.int64)


class Module(torch.nn.Module):
    """A linear model with Trainer's module interface; the monitored value of validation i is
    SCORES[i], counted in a buffer so that a checkpoint carries the count."""

    SCORES = [0.1, 0.5, 0.3, 0.3, 0.2]

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.model = torch.nn.Linear(4, 1)
        self.register_buffer("validations", torch.zeros((), dtype=torch.int64))

    def training_step(self, batch, i=0):
        return ((self.model(batch.x).squeeze(1) - batch.y) ** 2).mean()

    def validation_step(self, batch, i=0, idx=0, dataset_name=None):
        pass

    test_step = validation_step

    def evaluator(self, stage, name):
        return Evaluator()

    def reset_metrics(self, stage):
        pass

    def epoch_metrics(self, stage):
        if stage == "test":
            return {"test_DDR_kappa": float(self.model.weight.sum())}
        self.validations += 1
        return {KEY: self.SCORES[int(self.validations) - 1], "val_DDR_loss": 1.0}

    def configure_optimizers(self):
        return torch.optim.SGD(self.parameters(), lr=0.05, momentum=0.9)


class Data:
    """Two training batches of 3 and 1 graphs per epoch, one validation batch."""

    def __init__(self):
        gen = torch.Generator().manual_seed(1)
        self.batches = [Batch(torch.randn(n, 4, generator=gen), torch.randn(n, generator=gen))
                        for n in (3, 1)]

    def train_dataloader(self):
        return self.batches

    def val_dataloader(self):
        return {"DDR": self.batches[:1]}

    test_dataloader = val_dataloader


def fit(run_dir, max_epochs, ckpt_path=None, patience=2):
    callbacks = [ModelCheckpoint(run_dir, KEY, "max"), EarlyStopping(KEY, "max", patience)]
    trainer = Trainer(max_epochs, callbacks=callbacks, run_dir=run_dir)
    module = Module()
    steps = []  # (epoch, global step) of every validation
    hook = callbacks[0].on_validation_end

    def recorded(metrics, epoch, global_step, make_checkpoint):
        steps.append((epoch, global_step))
        return hook(metrics, epoch, global_step, make_checkpoint)

    callbacks[0].on_validation_end = recorded
    trainer.fit(module, Data(), ckpt_path=ckpt_path)
    return trainer, module, steps


def test_fit_validates_every_tenth_epoch_and_writes_last_at_the_end(tmp_path):
    trainer, module, steps = fit(tmp_path, 25)
    assert steps == [(9, 20), (19, 40)]  # after epochs 9 and 19 only, two steps per epoch
    assert trainer.current_epoch == 24 and trainer.global_step == 50
    assert len(trainer.validations) == 2 and len(trainer.train_losses) == 25
    assert sorted(os.listdir(tmp_path)) == ["epoch=19-step=40.ckpt", "last.ckpt", "metrics.jsonl"]
    last = torch.load(tmp_path / "last.ckpt", weights_only=True)
    assert last["epoch"] == 24 and last["global_step"] == 50  # rewritten at the end of fit
    for k, v in module.state_dict().items():
        assert torch.equal(last["state_dict"][k], v)
    # train_loss: the mean weighted by the batches' graphs (3 and 1)
    rows = [json.loads(line) for line in (tmp_path / "metrics.jsonl").read_text().splitlines()]
    assert [(r["epoch"], r["global_step"]) for r in rows] == [(9, 20), (19, 40), (24, 50)]
    assert rows[0][KEY] == 0.1 and rows[0]["train_loss"] == trainer.train_losses[9]
    assert trainer.test(module, Data(), ckpt="best") == {
        "test_DDR_kappa": float(torch.load(tmp_path / "epoch=19-step=40.ckpt", weights_only=True)
                                ["state_dict"]["model.weight"].sum())}


def test_checkpoints_written_at_a_validation_hold_the_state_after_it(tmp_path):
    trainer, _, _ = fit(tmp_path, 20)  # ends right after the second validation
    ckpt, stop = trainer.callbacks
    assert (ckpt.best_score, ckpt.saved, stop.best_score, stop.wait) == (0.5, [0, 1], 0.5, 0)
    best = torch.load(ckpt.best_model_path, weights_only=True)  # written at the validation only
    assert os.path.basename(ckpt.best_model_path) == "epoch=19-step=40.ckpt"
    assert best["callbacks"] == [ckpt.state_dict(), stop.state_dict()]
    assert best["best_score"] == 0.5 and best["best_model_path"] == ckpt.best_model_path
    assert os.path.exists(best["callbacks"][0]["best_model_path"])
    assert int(best["state_dict"]["validations"]) == 2
    # the last.ckpt of a validation as well: stop a run there by its patience
    trainer, _, steps = fit(tmp_path / "stopped", 50, patience=1)
    ckpt, stop = trainer.callbacks
    assert steps == [(9, 20), (19, 40), (29, 60)] and stop.stopped and trainer.current_epoch == 29
    last = torch.load(ckpt.last_model_path, weights_only=True)
    assert last["callbacks"] == [ckpt.state_dict(), stop.state_dict()]
    assert last["callbacks"][1] == {"best_score": 0.5, "wait": 1, "stopped": True}
    assert os.path.exists(last["callbacks"][0]["best_model_path"])


def test_resume_from_a_checkpoint_written_at_a_validation(tmp_path):
    whole, module, _ = fit(tmp_path / "whole", 50, patience=3)
    part, _, _ = fit(tmp_path / "part", 20, patience=3)
    best = part.callbacks[0].best_model_path  # epoch 19's, written at the second validation
    resumed, again, steps = fit(tmp_path / "part", 50, ckpt_path=best, patience=3)
    # scores 0.1, 0.5, 0.3, 0.3, 0.2: three validations without an improvement stop at epoch 49
    assert steps == [(29, 60), (39, 80), (49, 100)]
    assert resumed.train_losses == whole.train_losses and resumed.global_step == 100
    for k, v in module.state_dict().items():
        assert torch.equal(again.state_dict()[k], v), k
    for a, b in zip(resumed.callbacks, whole.callbacks):
        sa, sb = a.state_dict(), b.state_dict()
        sa.pop("best_model_path", None), sb.pop("best_model_path", None)
        assert sa == sb
    ckpt = resumed.callbacks[0]
    assert ckpt.saved == [0, 1] and ckpt.best_model_path == best and os.path.exists(best)
    assert resumed.callbacks[1].stopped and resumed.callbacks[1].wait == 3
    assert sorted(os.listdir(tmp_path / "part")) == \
        ["epoch=19-step=40.ckpt", "last.ckpt", "metrics.jsonl"]
    resumed.test(again, Data(), ckpt="best")  # the best file is there to be opened


def test_reduce_lr_on_plateau_is_refused_by_name():
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.SGD([p], lr=0.1)
    plateau = torch.optim.lr_scheduler.ReduceLROnPlateau(opt)
    with pytest.raises(NotImplementedError, match="ReduceLROnPlateau"):
        Trainer(max_epochs=1, optimizers={"optimizer": opt, "lr_scheduler": {
            "scheduler": plateau, "monitor": "val_loss", "interval": "epoch", "frequency": 1}})
    step = torch.optim.lr_scheduler.StepLR(opt, 1)
    t = Trainer(max_epochs=1, optimizers={"optimizer": opt, "lr_scheduler": {
        "scheduler": step, "interval": "step", "frequency": 2}})
    assert t._configured == (opt, step, "step", 2)
