"""Grading metrics accumulated on the device (csrc/metrics.hip; state and definitions:
include/lgnn.h, "Evaluation").

Replaces what the reference evaluates a model with — the torchmetrics collections of
BaseLightningModule.setup_metrics (src/lesion_gnn/models/base.py:120-145) and the referable-DR
metrics of src/lesion_gnn/metrics.py — without torchmetrics: `update` is one launch per batch and
never synchronises (it can be captured in a graph), `compute` is one launch sequence and one host
read per epoch. The metrics are those of the accumulated state, not the reference's batch-size
weighted mean of per-batch values (equal when a loader yields one batch).
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import LgnnError

_NAMES = ("micro_acc", "kappa", "macro_f1", "macro_precision", "macro_recall", "acc", "f1",
          "precision", "recall", "auroc", "auprc", "loss")
_LOSS_KINDS = {"CE": (False, 0), "MSE": (True, 0), "SmoothL1": (True, 1)}


class GradingMetrics:
    """One evaluator: confusion matrix, referable counts, loss sums and (probabilistic mode) up
    to `capacity` referable scores, held on the device of the first `update`.

    num_classes: C; regression: `update` takes the model's raw regression output [B] or [B, 1]
    (clamped and rounded in the kernel) instead of logits [B, C]; loss_kind: "CE" (probabilistic)
    or "MSE" / "SmoothL1" (regression); class_weight: the CE class weights [C] or None."""

    def __init__(self, num_classes: int, regression: bool, loss_kind: str,
                 class_weight: torch.Tensor | None = None, capacity: int = 65536):
        loss_kind = getattr(loss_kind, "value", loss_kind)
        if loss_kind not in _LOSS_KINDS or _LOSS_KINDS[loss_kind][0] != bool(regression):
            raise ValueError(f"loss kind {loss_kind!r} does not go with regression={regression}")
        if not 1 <= num_classes <= _lib.LGNN_EVAL_MAX_CLASSES:
            raise ValueError(f"num_classes must be in [1, {_lib.LGNN_EVAL_MAX_CLASSES}]")
        if not 0 <= capacity < 2 ** 31:
            raise ValueError("capacity must be in [0, 2^31)")
        if class_weight is not None and class_weight.numel() != num_classes:
            raise ValueError("class_weight must have one value per class")
        self.num_classes = int(num_classes)
        self.regression = bool(regression)
        self.loss_kind = loss_kind
        self.capacity = int(capacity)
        self.overflow = False  # set by compute()
        self._class_weight = class_weight
        self._weight = None    # the weights on the state's device
        self._counts = None    # allocated by the first update (or merge)

    # ------------------------------------------------------------------------------------------

    def _allocate(self, dev: torch.device) -> None:
        C = self.num_classes
        self._counts = torch.zeros(C * C + _lib.LGNN_EVAL_EXTRA, dtype=torch.int64, device=dev)
        self._loss_acc = torch.zeros(2, dtype=torch.float64, device=dev)
        self._result = torch.zeros(_lib.LGNN_EVAL_RESULTS, dtype=torch.float64, device=dev)
        self._scores = self._positive = self._workspace = None
        if not self.regression:
            n = max(self.capacity, 1)
            self._scores = torch.zeros(n, dtype=torch.float32, device=dev)
            self._positive = torch.zeros(n, dtype=torch.int32, device=dev)
            nbytes = _lib.query("lgnn_eval_workspace_bytes", self.capacity)
            self._workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            if self._class_weight is not None:
                self._weight = self._class_weight.detach().to(dev, torch.float32).contiguous()

    def _state(self, what: str):
        if self._counts is None:
            raise LgnnError(f"GradingMetrics.{what}: no batch has been given to update() yet")
        return self._counts

    @property
    def device(self) -> torch.device | None:
        return None if self._counts is None else self._counts.device

    def update(self, logits: torch.Tensor, y: torch.Tensor) -> None:
        """Add one batch: logits [B, C] (or the regression output [B] / [B, 1]) float32 and the
        int64 grades y [B]. One launch, no host synchronisation."""
        _lib.require_gpu(logits, y)
        if logits.dtype != torch.float32 or y.dtype != torch.int64:
            raise TypeError(f"update takes float32 outputs and int64 targets, got {logits.dtype} "
                            f"and {y.dtype}")
        if self.regression:
            if logits.dim() == 2 and logits.size(1) != 1 or logits.dim() not in (1, 2):
                raise ValueError("a regression output must be [B] or [B, 1]")
        elif logits.dim() != 2 or logits.size(1) != self.num_classes:
            raise ValueError(f"logits must be [B, {self.num_classes}]")
        B = logits.size(0)
        if y.dim() != 1 or y.numel() != B:
            raise ValueError("targets must be [B]")
        if B == 0:
            return
        dev = logits.device
        if self._counts is None:
            self._allocate(dev)
        elif dev != self._counts.device:
            raise LgnnError(f"this evaluator's state is on {self._counts.device}, got {dev}")
        smooth = _LOSS_KINDS[self.loss_kind][1]
        _lib.call("lgnn_eval_update", logits.detach().contiguous(), y.contiguous(), self._weight,
                  B, self.num_classes, int(self.regression), smooth, self._counts,
                  self._loss_acc, self._scores, self._positive, self.capacity, _lib.stream(dev))

    def _launch_compute(self) -> torch.Tensor:
        """Enqueue lgnn_eval_compute; the device result vector (LGNN_EVAL_R_* indices)."""
        counts = self._state("compute")
        _lib.call("lgnn_eval_compute", counts, self._loss_acc, self._scores, self._positive,
                  self.capacity, self.num_classes, int(self.regression), self._result,
                  self._workspace, 0 if self._workspace is None else self._workspace.numel(),
                  _lib.stream(counts.device))
        return self._result

    def compute(self) -> dict[str, float]:
        """The metrics of everything added since the last reset (one host read). Raises LgnnError
        when a target was outside [0, C). `overflow` is set, and auroc / auprc are NaN, when more
        than `capacity` rows were added; regression evaluators have no auroc / auprc."""
        r = self._launch_compute().tolist()
        n_bad = int(r[_lib.LGNN_EVAL_R_NBAD])
        if n_bad > 0:
            raise LgnnError(f"GradingMetrics: {n_bad} target(s) outside [0, {self.num_classes})")
        self.overflow = r[_lib.LGNN_EVAL_R_OVERFLOW] != 0.0
        out = {name: r[getattr(_lib, "LGNN_EVAL_R_" + name.upper())] for name in _NAMES}
        if self.regression:
            del out["auroc"], out["auprc"]
        return out

    def state(self) -> dict[str, torch.Tensor | None]:
        """The device tensors of include/lgnn.h's layout (not copies): counts, loss_acc, scores,
        positive (the last two None for regression). What a multi-rank sync would exchange."""
        self._state("state")
        return {"counts": self._counts, "loss_acc": self._loss_acc, "scores": self._scores,
                "positive": self._positive}

    def confusion_matrix(self) -> torch.Tensor:
        """[C, C] int64 on the device, [target][pred] (a copy)."""
        C = self.num_classes
        return self._state("confusion_matrix")[:C * C].view(C, C).clone()

    def reset(self) -> None:
        """Forget every batch (no host synchronisation; the stored scores need no clearing)."""
        if self._counts is not None:
            self._counts.zero_()
            self._loss_acc.zero_()
        self.overflow = False

    def merge(self, other: "GradingMetrics") -> None:
        """Add `other`'s batches to this evaluator: the counters and loss sums are summed and its
        stored scores appended, as if this evaluator had been given both streams (the loss sums to
        double rounding). One launch; `other` is left as it is."""
        same = ("num_classes", "regression", "loss_kind", "capacity")
        if other is self or any(getattr(self, k) != getattr(other, k) for k in same):
            raise ValueError("merge takes another evaluator of the same configuration")
        if other._counts is None:
            return
        dev = other._counts.device
        if self._counts is None:
            self._allocate(dev)
        elif dev != self._counts.device:
            raise LgnnError(f"this evaluator's state is on {self._counts.device}, the other's on "
                            f"{dev}")
        _lib.call("lgnn_eval_merge", self.num_classes, self._counts, self._loss_acc,
                  self._scores, self._positive, other._counts, other._loss_acc, other._scores,
                  other._positive, self.capacity, _lib.stream(dev))
