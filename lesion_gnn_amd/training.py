"""Training from a config: reference src/lesion_gnn/training.py:14-77 (`train(config)`) without
Lightning and W&B. `Trainer` is the part of lightning.Trainer the reference uses — the epoch
loop over `training_step`, validation every `check_val_every_n_epoch` epochs, `test` at the best
weights — driving the step methods of models/base.py; `ModelCheckpoint` and `EarlyStopping` are
the two Lightning callbacks of training.py:44-62, restated as plain host classes over the metrics
dict of a validation.

A training epoch without validation reads nothing back from the device: the loader sizes its
batches on the host (with hoisted edges, DataModule(hoist=True), it makes no device read at
all), the loss is accumulated on the device and read when a validation reads metrics anyway.
"""
from __future__ import annotations

import json
import math
import os
import random

import torch

from .datasets.datamodule import DataModule
from .models import get_model

VALIDATION_INTERVAL = 10  # reference training.py:15


def _monitored(metrics: dict, monitor: str) -> float:
    if monitor not in metrics:
        raise KeyError(f"monitored metric {monitor!r} was not logged; logged: {sorted(metrics)}")
    return float(metrics[monitor])


def _improves(mode: str, value: float, best: float | None) -> bool:
    """A strict improvement on `best` (None: nothing seen yet). NaN never improves."""
    if math.isnan(value):
        return False
    if best is None or math.isnan(best):
        return True
    return value < best if mode == "min" else value > best


def _check_mode(mode: str) -> str:
    if mode not in ("min", "max"):
        raise ValueError(f"mode must be 'min' or 'max', got {mode!r}")
    return mode


class ModelCheckpoint:
    """lightning's ModelCheckpoint(dirpath, monitor, mode, save_last=True, save_top_k=1) as the
    reference builds it: `epoch={e}-step={s}.ckpt` when the monitored value strictly improves (the
    first validation always saves, a tie keeps the old file, the previous best is deleted) and
    `last.ckpt` at every validation and at the end of fit. `saved` lists the validations (0, 1,
    ...) that wrote a best file."""

    def __init__(self, dirpath, monitor: str, mode: str = "min", save_last: bool = True,
                 save_top_k: int = 1):
        if save_top_k != 1:
            raise NotImplementedError("ModelCheckpoint: save_top_k must be 1 (the reference's)")
        self.dirpath, self.monitor, self.mode = str(dirpath), monitor, _check_mode(mode)
        self.save_last = bool(save_last)
        self.best_score: float | None = None
        self.best_model_path: str | None = None
        self.last_model_path: str | None = None
        self.saved: list[int] = []
        self._validations = 0

    def _write(self, name: str, checkpoint: dict) -> str:
        os.makedirs(self.dirpath, exist_ok=True)
        path = os.path.join(self.dirpath, name)
        checkpoint = dict(checkpoint, monitor=self.monitor, best_score=self.best_score,
                          best_model_path=self.best_model_path)
        torch.save(checkpoint, path)
        return path

    def on_validation_end(self, metrics: dict, epoch: int, global_step: int, make_checkpoint
                          ) -> bool:
        """One validation's metrics; make_checkpoint() -> the checkpoint dict. True when a new
        best file was written."""
        value = _monitored(metrics, self.monitor)
        index, better = self._validations, _improves(self.mode, value, self.best_score)
        # the first validation saves whatever its value is (a NaN too, as top-k of nothing)
        better = better or self.best_model_path is None
        # the bookkeeping first: the checkpoint holds the callbacks' state after this validation,
        # so that a run resumed from it knows the best score and the file that holds it
        self._validations += 1
        old = self.best_model_path
        if better:
            name = f"epoch={epoch}-step={global_step}.ckpt"
            self.best_score, self.best_model_path = value, os.path.join(self.dirpath, name)
            self.saved.append(index)
        checkpoint = make_checkpoint()
        if better:
            self._write(name, checkpoint)
            if old is not None and old != self.best_model_path and os.path.exists(old):
                os.remove(old)
        self.save_last_checkpoint(checkpoint)
        return better

    def save_last_checkpoint(self, checkpoint: dict) -> None:
        if self.save_last:
            self.last_model_path = self._write("last.ckpt", checkpoint)

    def state_dict(self) -> dict:
        return {"best_score": self.best_score, "best_model_path": self.best_model_path,
                "saved": list(self.saved), "validations": self._validations}

    def load_state_dict(self, state: dict) -> None:
        self.best_score, self.best_model_path = state["best_score"], state["best_model_path"]
        self.saved, self._validations = list(state["saved"]), state["validations"]


class EarlyStopping:
    """lightning's EarlyStopping(monitor, mode, patience), counted in validations: a strict
    improvement resets the wait, anything else increments it and stops at wait >= patience; a
    monitored value that is not finite stops at once."""

    def __init__(self, monitor: str, mode: str = "min", patience: int = 3):
        if patience < 0:
            raise ValueError("patience must be >= 0")
        self.monitor, self.mode, self.patience = monitor, _check_mode(mode), int(patience)
        self.best_score: float | None = None
        self.wait = 0
        self.stopped = False

    def on_validation_end(self, metrics: dict) -> bool:
        """One validation's metrics; True when training should stop."""
        value = _monitored(metrics, self.monitor)
        if not math.isfinite(value):
            self.stopped = True
        elif _improves(self.mode, value, self.best_score):
            self.best_score, self.wait = value, 0
        else:
            self.wait += 1
            self.stopped = self.stopped or self.wait >= self.patience
        return self.stopped

    def state_dict(self) -> dict:
        return {"best_score": self.best_score, "wait": self.wait, "stopped": self.stopped}

    def load_state_dict(self, state: dict) -> None:
        self.best_score, self.wait, self.stopped = state["best_score"], state["wait"], \
            state["stopped"]


def unpack_optimizers(configured) -> tuple:
    """(optimizer, scheduler or None, interval, frequency) of what configure_optimizers returned
    (an optimizer, or Lightning's {"optimizer", "lr_scheduler": {...}} dict). A scheduler whose
    step takes a metric has nothing to be driven by here."""
    if not isinstance(configured, dict):
        return configured, None, "epoch", 1
    sc = configured.get("lr_scheduler")
    if sc is None:
        return configured["optimizer"], None, "epoch", 1
    sc = sc if isinstance(sc, dict) else {"scheduler": sc}
    scheduler = sc["scheduler"]
    if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
        raise NotImplementedError("ReduceLROnPlateau steps on a monitored metric, which this "
                                  "Trainer does not feed to schedulers")
    interval, frequency = sc.get("interval", "epoch"), int(sc.get("frequency", 1))
    if interval not in ("epoch", "step") or frequency < 1:
        raise ValueError("lr_scheduler: interval is 'epoch' or 'step', frequency >= 1")
    return configured["optimizer"], scheduler, interval, frequency


def _host(obj):
    """A checkpoint-ready copy: every tensor inside on the host."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_host(v) for v in obj)
    return obj


class Trainer:
    """The epoch loop. `optimizers`: what module.configure_optimizers() returned (default: fit
    calls it). After fit: `train_losses` (one per epoch run, the batch-size weighted mean of the
    steps' losses), `validations` (the metrics dict of each), `current_epoch` (the last epoch
    run), `global_step`, `should_stop`."""

    def __init__(self, max_epochs: int, check_val_every_n_epoch: int = VALIDATION_INTERVAL,
                 callbacks=(), run_dir=None, optimizers=None):
        if max_epochs < 0 or check_val_every_n_epoch < 1:
            raise ValueError("max_epochs >= 0 and check_val_every_n_epoch >= 1")
        self.max_epochs = int(max_epochs)
        self.check_val_every_n_epoch = int(check_val_every_n_epoch)
        self.callbacks = list(callbacks)
        self.run_dir = None if run_dir is None else str(run_dir)
        self._configured = None if optimizers is None else unpack_optimizers(optimizers)
        self.current_epoch, self.global_step, self.should_stop = -1, 0, False
        self.train_losses: list[float] = []
        self.validations: list[dict] = []
        self.confusion_matrices: dict[str, torch.Tensor] = {}
        self.val_confusion_matrices: list[dict[str, torch.Tensor]] = []
        self._loss_acc = None
        self._train_loader = None

    # -- helpers ---------------------------------------------------------------------------------

    def validates_after(self, epoch: int) -> bool:
        return (epoch + 1) % self.check_val_every_n_epoch == 0

    @property
    def checkpoint_callback(self) -> ModelCheckpoint | None:
        return next((c for c in self.callbacks if isinstance(c, ModelCheckpoint)), None)

    def _log(self, metrics: dict) -> None:
        if self.run_dir is None:
            return
        os.makedirs(self.run_dir, exist_ok=True)
        row = dict(metrics, epoch=self.current_epoch, global_step=self.global_step)
        with open(os.path.join(self.run_dir, "metrics.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")

    def _read_train_losses(self) -> None:
        """One host read of the loss sums of every epoch run so far."""
        n = self.current_epoch + 1
        if self._loss_acc is None or n <= len(self.train_losses):
            return
        acc = self._loss_acc[:n].cpu()
        self.train_losses = [float(acc[e, 0] / acc[e, 1]) if float(acc[e, 1]) else math.nan
                             for e in range(n)]

    def checkpoint(self, module) -> dict:
        """The checkpoint dict: tensors, numbers, strings, lists and dicts only, so
        torch.load(weights_only=True) reads it. It holds the state of the train loader's
        generator and of the model's own dropout generator (`model._dropout_rng`), not torch's
        global generators: a model that draws from those (torch's own dropout) resumes on another
        random stream than an uninterrupted run."""
        optimizer, scheduler = self._configured[:2]
        generator = getattr(self._train_loader, "generator", None)
        rng = getattr(getattr(module, "model", None), "_dropout_rng", None)
        return {
            "epoch": self.current_epoch, "global_step": self.global_step,
            "state_dict": _host(module.state_dict()),
            "optimizer_states": [_host(optimizer.state_dict())],
            "lr_schedulers": [] if scheduler is None else [_host(scheduler.state_dict())],
            "callbacks": [c.state_dict() for c in self.callbacks],
            "loader_generator": None if generator is None else generator.get_state(),
            "dropout_rng": None if rng is None else _host(rng),
            "loss_acc": None if self._loss_acc is None else _host(self._loss_acc),
        }

    def _restore(self, module, ckpt_path) -> None:
        ck = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        optimizer, scheduler = self._configured[:2]
        module.load_state_dict(ck["state_dict"])
        optimizer.load_state_dict(ck["optimizer_states"][0])
        for p, st in optimizer.state.items():  # torch leaves a loaded "step" where it was saved
            for k, v in st.items():
                if isinstance(v, torch.Tensor) and v.device != p.device:
                    st[k] = v.to(p.device)
        if scheduler is not None:
            scheduler.load_state_dict(ck["lr_schedulers"][0])
        for c, state in zip(self.callbacks, ck["callbacks"]):
            c.load_state_dict(state)
        generator = getattr(self._train_loader, "generator", None)
        if generator is not None and ck["loader_generator"] is not None:
            generator.set_state(ck["loader_generator"])
        rng = getattr(getattr(module, "model", None), "_dropout_rng", None)
        if rng is not None and ck["dropout_rng"] is not None:
            rng.copy_(ck["dropout_rng"])
        if ck["loss_acc"] is not None:
            n = min(ck["loss_acc"].size(0), self._loss_acc.size(0))
            self._loss_acc[:n].copy_(ck["loss_acc"][:n])
        self.current_epoch, self.global_step = ck["epoch"], ck["global_step"]

    def _evaluate(self, module, loaders: dict, stage: str) -> dict:
        step = module.validation_step if stage == "val" else module.test_step
        module.eval()
        module.reset_metrics(stage)
        for idx, (name, loader) in enumerate(loaders.items()):
            for i, batch in enumerate(loader):
                step(batch, i, idx, dataset_name=name)
        metrics = module.epoch_metrics(stage)
        cms = {name: module.evaluator(stage, name).confusion_matrix().cpu() for name in loaders
               if module.evaluator(stage, name).device is not None}
        if stage == "val":
            self.val_confusion_matrices.append(cms)
        else:
            self.confusion_matrices = cms
        return metrics

    # -- the loops -------------------------------------------------------------------------------

    def prepare(self, module, max_epochs: int | None = None) -> None:
        """The optimizers (module.configure_optimizers() unless given at construction) and the
        device-side loss sums, one [sum of loss x graphs, graphs] row per epoch."""
        if self._configured is None:
            self._configured = unpack_optimizers(module.configure_optimizers())
        device = next(module.parameters()).device
        rows = max(self.max_epochs if max_epochs is None else max_epochs, 1)
        self._loss_acc = torch.zeros(rows, 2, dtype=torch.float64, device=device)

    def train_epoch(self, module, loader, epoch: int) -> None:
        """One training epoch over `loader`: no device read."""
        optimizer, scheduler, interval, frequency = self._configured
        self.current_epoch = epoch
        module.train()
        acc = self._loss_acc[epoch]
        for i, batch in enumerate(loader):
            optimizer.zero_grad(set_to_none=True)
            loss = module.training_step(batch, i)
            loss.backward()
            optimizer.step()
            self.global_step += 1
            # Lightning's on_epoch mean, weighted by the batch size; two in-place ops, no read
            acc[0].add_(loss.detach(), alpha=batch.num_graphs)
            acc[1].add_(batch.num_graphs)
            if scheduler is not None and interval == "step" and \
                    self.global_step % frequency == 0:
                scheduler.step()
        if scheduler is not None and interval == "epoch" and (epoch + 1) % frequency == 0:
            scheduler.step()

    def fit(self, module, datamodule, ckpt_path=None) -> None:
        self.prepare(module)
        self._train_loader = loader = datamodule.train_dataloader()
        val_loaders = datamodule.val_dataloader()
        if ckpt_path is not None:
            self._restore(module, ckpt_path)
            self.should_stop = any(c.stopped for c in self.callbacks
                                   if isinstance(c, EarlyStopping))
        for epoch in range(self.current_epoch + 1, self.max_epochs):
            if self.should_stop:
                break
            self.train_epoch(module, loader, epoch)
            if self.validates_after(epoch) and val_loaders:
                self._validate(module, val_loaders)
        self._read_train_losses()
        ckpt = self.checkpoint_callback
        if ckpt is not None:
            ckpt.save_last_checkpoint(self.checkpoint(module))
        self._log({"train_loss": self.train_losses[-1]} if self.train_losses else {})

    def _validate(self, module, val_loaders: dict) -> None:
        with torch.no_grad():
            metrics = self._evaluate(module, val_loaders, "val")
        self._read_train_losses()
        metrics = dict(metrics, train_loss=self.train_losses[-1])
        self.validations.append(metrics)
        self._log(metrics)
        # EarlyStopping before ModelCheckpoint, whatever their order in `callbacks`: the files
        # written at this validation hold every callback's state after it
        for c in self.callbacks:
            if isinstance(c, EarlyStopping):
                self.should_stop = c.on_validation_end(metrics) or self.should_stop
        for c in self.callbacks:
            if isinstance(c, ModelCheckpoint):
                c.on_validation_end(metrics, self.current_epoch, self.global_step,
                                    lambda: self.checkpoint(module))

    def test(self, module, datamodule, ckpt: str | None = "best") -> dict:
        """The test loaders through test_step at the "best" or "last" checkpoint's weights (None:
        the module's current ones): the flat metrics dict; the confusion matrices are kept as
        `confusion_matrices[dataset]` ([target][pred], host)."""
        if ckpt is not None:
            cb = self.checkpoint_callback
            path = None if cb is None else \
                {"best": cb.best_model_path, "last": cb.last_model_path}[ckpt]
            if path is None:
                raise ValueError(f"test(ckpt={ckpt!r}): no such checkpoint was written")
            module.load_state_dict(torch.load(path, map_location="cpu",
                                              weights_only=True)["state_dict"])
        with torch.no_grad():
            metrics = self._evaluate(module, datamodule.test_dataloader(), "test")
        self._log(metrics)
        return metrics


def run(config, stores: dict, run_dir=None, device=None, ckpt_path=None) -> tuple:
    """`train`, returning (test metrics, trainer, module): the trainer keeps the loss sequence,
    every validation's metrics and confusion matrices and the callbacks' decisions. ckpt_path: a
    checkpoint of an earlier run of the same config to resume the fit from."""
    torch.manual_seed(config.seed)  # L.seed_everything
    random.seed(config.seed)
    try:
        import numpy
        numpy.random.seed(config.seed)
    except ImportError:
        pass
    if device is None:
        device = next(iter(stores.values())).x.device
    if run_dir is None:
        run_dir = os.path.join("checkpoints", f"{config.project_name}-seed{config.seed}")

    datamodule = DataModule(config.dataset, compile=config.model.compile, stores=stores,
                            hoist=True)
    datamodule.generator = torch.Generator().manual_seed(config.seed)
    datamodule.setup("fit")  # train (and val) datasets before the placeholders

    config.model.optimizer.class_weights.value = datamodule.get_class_weights(
        mode=config.model.optimizer.class_weights_mode)
    config.model.num_classes.value = datamodule.num_classes
    config.model.input_features.value = datamodule.num_features

    model = get_model(config.model).to(device)
    optimizers = model.configure_optimizers()

    callbacks = [ModelCheckpoint(dirpath=run_dir, monitor=config.monitored_metric,
                                 mode=config.monitor_mode, save_last=True, save_top_k=1)]
    if config.early_stopping_patience is not None:
        callbacks.append(EarlyStopping(
            monitor=config.monitored_metric, mode=config.monitor_mode,
            patience=config.early_stopping_patience // VALIDATION_INTERVAL))
    trainer = Trainer(max_epochs=config.max_epochs, check_val_every_n_epoch=VALIDATION_INTERVAL,
                      callbacks=callbacks, run_dir=run_dir, optimizers=optimizers)
    trainer.fit(model, datamodule, ckpt_path=ckpt_path)

    datamodule.setup("test")
    return trainer.test(model, datamodule, ckpt="best"), trainer, model


def train(config, stores: dict, run_dir=None, device=None) -> dict[str, float]:
    """Reference training.py:14-77 over GPU-resident `stores` (dataset name -> GraphStore): seed,
    DataModule(hoist=True), placeholders, model, fit with ModelCheckpoint (and EarlyStopping when
    the config sets a patience), then the test metrics at the best checkpoint's weights, as the
    flat {"test_<dataset>_<metric>": value} dict. run_dir (checkpoints and metrics.jsonl)
    defaults to checkpoints/<project_name>-seed<seed>/."""
    return run(config, stores, run_dir, device)[0]
