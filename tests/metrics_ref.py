"""Float64 numpy restatement of the grading metrics (lesion_gnn_amd.metrics / csrc/metrics.hip),
written from the definitions: the checker of tests/test_gpu_metrics.py, itself pinned against
scikit-learn by tests/test_metrics_ref.py.

AUROC and average precision are integrated over the distinct thresholds of the sorted scores (the
curves torchmetrics builds with thresholds=None), not counted pair by pair as the kernel does.
"""
from __future__ import annotations

import math

import numpy as np

NAN = float("nan")


def _div0(a, b) -> float:
    """a / b with a zero denominator giving 0 (torchmetrics' _safe_divide, sklearn's
    zero_division=0)."""
    return float(a) / float(b) if b != 0 else 0.0


def predicted_class(logits: np.ndarray) -> np.ndarray:
    """The lowest index among each row's maxima (torch.argmax / np.argmax)."""
    return np.argmax(np.asarray(logits, dtype=np.float64), axis=1).astype(np.int64)


def referable_score(logits: np.ndarray) -> np.ndarray:
    """softmax(z)[2:].sum() per row in float64 (reference metrics.py:24-25)."""
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True))[:, 2:].sum(axis=1)


def regression_pred(z: np.ndarray, num_classes: int) -> tuple[np.ndarray, np.ndarray]:
    """(clamped output p, round(p) half to even as torch.round) of a regression output."""
    p = np.clip(np.asarray(z, dtype=np.float64).reshape(-1), 0.0, float(num_classes - 1))
    return p, np.rint(p).astype(np.int64)


def confusion_matrix(pred, target, num_classes: int) -> np.ndarray:
    """[target][pred] int64."""
    conf = np.zeros((num_classes, num_classes), dtype=np.int64)
    np.add.at(conf, (np.asarray(target, dtype=np.int64), np.asarray(pred, dtype=np.int64)), 1)
    return conf


def referable_counts(rpred, rtarget) -> tuple[int, int, int, int]:
    """(tn, fp, fn, tp) of boolean predictions against boolean targets."""
    rpred, rtarget = np.asarray(rpred, dtype=bool), np.asarray(rtarget, dtype=bool)
    return (int((~rpred & ~rtarget).sum()), int((rpred & ~rtarget).sum()),
            int((~rpred & rtarget).sum()), int((rpred & rtarget).sum()))


def multiclass_metrics(conf: np.ndarray) -> dict[str, float]:
    """micro accuracy, quadratic kappa and macro F1 / precision / recall of a confusion matrix.
    kappa = 1 - sum w O / sum w E with w = (i - j)^2 and E = rows x cols / n, evaluated as
    1 - n sum w O / sum w rows x cols (both sums exact integers); 0 / 0 gives NaN. A class in
    neither the predictions nor the targets is left out of the macro means (torchmetrics 1.3.1,
    and sklearn's default labels)."""
    conf = np.asarray(conf, dtype=np.int64)
    C = conf.shape[0]
    n = int(conf.sum())
    rows, cols = conf.sum(axis=1), conf.sum(axis=0)
    idx = np.arange(C)
    w = (idx[:, None] - idx[None, :]) ** 2
    wo = int((w * conf).sum())
    we = int((w * np.outer(rows, cols)).sum())
    kappa = 1.0 - float(n * wo) / float(we) if we != 0 else NAN
    f1, prec, rec = [], [], []
    for k in range(C):
        tp = int(conf[k, k])
        fp, fn = int(cols[k]) - tp, int(rows[k]) - tp
        if tp + fp + fn == 0:
            continue
        f1.append(_div0(2 * tp, 2 * tp + fp + fn))
        prec.append(_div0(tp, tp + fp))
        rec.append(_div0(tp, tp + fn))
    return {"micro_acc": _div0(int(np.trace(conf)), n), "kappa": kappa,
            "macro_f1": _div0(math.fsum(f1), len(f1)),
            "macro_precision": _div0(math.fsum(prec), len(prec)),
            "macro_recall": _div0(math.fsum(rec), len(rec))}


def referable_metrics(tn: int, fp: int, fn: int, tp: int) -> dict[str, float]:
    return {"acc": _div0(tp + tn, tn + fp + fn + tp), "f1": _div0(2 * tp, 2 * tp + fp + fn),
            "precision": _div0(tp, tp + fp), "recall": _div0(tp, tp + fn)}


def _curve(scores, positive):
    """Cumulative (tp, fp) at each distinct threshold, thresholds descending."""
    s = np.asarray(scores, dtype=np.float64)
    pos = np.asarray(positive, dtype=bool)
    order = np.argsort(-s, kind="stable")
    s, pos = s[order], pos[order]
    last = np.r_[np.nonzero(np.diff(s))[0], s.size - 1]  # the last sample of each tie group
    return np.cumsum(pos)[last].astype(np.int64), np.cumsum(~pos)[last].astype(np.int64)


def auroc(scores, positive) -> float:
    """The trapezoid integral of the ROC curve over the distinct thresholds; NaN without a
    positive or without a negative."""
    pos = np.asarray(positive, dtype=bool)
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if n_pos == 0 or n_neg == 0:
        return NAN
    tp, fp = _curve(scores, pos)
    tp0, fp0 = np.r_[0, tp[:-1]], np.r_[0, fp[:-1]]
    twice_area = int(((fp - fp0) * (tp + tp0)).sum())
    return twice_area / (2.0 * n_pos * n_neg)


def auprc(scores, positive) -> float:
    """Average precision: the step integral sum_k (R_k - R_{k-1}) P_k over the distinct
    thresholds; NaN without a positive."""
    pos = np.asarray(positive, dtype=bool)
    n_pos = int(pos.sum())
    if n_pos == 0:
        return NAN
    tp, fp = _curve(scores, pos)
    tp0 = np.r_[0, tp[:-1]]
    return math.fsum((int(a) - int(a0)) * (int(a) / (int(a) + int(b)))
                     for a, a0, b in zip(tp, tp0, fp)) / n_pos


def evaluate(outputs, target, num_classes: int, regression: bool) -> dict:
    """Everything the evaluator holds and reports for model outputs (logits [B, C], or the raw
    regression output [B]) and grades: {"confusion", "referable" (tn, fp, fn, tp), "scores"
    (float64; None for regression), "positive", "metrics"}. The loss is not restated here."""
    target = np.asarray(target, dtype=np.int64)
    positive = target >= 2
    if regression:
        _, pred = regression_pred(outputs, num_classes)
        scores, rpred = None, pred >= 2
    else:
        pred = predicted_class(outputs)
        scores = referable_score(outputs)
        rpred = scores > 0.5
    conf = confusion_matrix(pred, target, num_classes)
    ref = referable_counts(rpred, positive)
    metrics = {**multiclass_metrics(conf), **referable_metrics(*ref)}
    if not regression:
        metrics["auroc"] = auroc(scores, positive)
        metrics["auprc"] = auprc(scores, positive)
    return {"confusion": conf, "referable": ref, "scores": scores, "positive": positive,
            "metrics": metrics}
