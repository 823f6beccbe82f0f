"""CPU checks of the evaluation surface: tests/metrics_ref.py (the float64 restatement the GPU
tests compare the kernels with) against scikit-learn and hand-computed cases; the header's new
entries; BaseModule's evaluation methods; evaluators stay out of state_dict(). No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    """name -> (logits [B, C] float64, targets [B]): random data, a class in neither predictions
    nor targets, tie-heavy scores, and rows whose referable probability is exactly 0.5."""
    rng = np.random.default_rng(7)
    out = {"random": (rng.normal(size=(500, 5)) * 2, rng.integers(0, 5, 500))}
    z = rng.normal(size=(300, 5))
    z[:, 3] = -50.0  # class 3 is never predicted ...
    y = rng.integers(0, 3, 300)  # ... and never a target
    out["absent_class"] = (z, np.where(y == 2, 4, y))
    out["ties"] = (rng.integers(-1, 2, size=(400, 5)) * 0.5, rng.integers(0, 5, 400))
    z = rng.integers(-2, 3, size=(64, 4)) * 0.5
    z[::4] = 0.0  # four equal logits: softmax 1/4 each, the referable score exactly 0.5
    out["half"] = (z, rng.integers(0, 4, 64))
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_sklearn(name):
    pytest.importorskip("sklearn")
    from sklearn import metrics as sk

    z, y = CASES[name]
    C = z.shape[1]
    ev = mr.evaluate(z, y, C, regression=False)
    pred, m = mr.predicted_class(z), ev["metrics"]
    assert int(ev["confusion"].sum()) == len(y) and sum(ev["referable"]) == len(y)
    assert np.array_equal(ev["confusion"], sk.confusion_matrix(y, pred, labels=np.arange(C)))
    close = dict(rel=1e-12, abs=1e-12)
    assert m["micro_acc"] == pytest.approx(sk.accuracy_score(y, pred), **close)
    # labels given: the weights are distances between grades, not between the positions of the
    # grades that happen to occur (sklearn's default would renumber 0 1 2 4 as 0 1 2 3)
    assert m["kappa"] == pytest.approx(
        sk.cohen_kappa_score(y, pred, weights="quadratic", labels=np.arange(C)), **close)
    for key, fn in (("macro_f1", sk.f1_score), ("macro_precision", sk.precision_score),
                    ("macro_recall", sk.recall_score)):
        assert m[key] == pytest.approx(fn(y, pred, average="macro", zero_division=0), **close)
    rt, rp = y >= 2, ev["scores"] > 0.5
    assert m["acc"] == pytest.approx(sk.accuracy_score(rt, rp), **close)
    assert m["f1"] == pytest.approx(sk.f1_score(rt, rp, zero_division=0), **close)
    assert m["precision"] == pytest.approx(sk.precision_score(rt, rp, zero_division=0), **close)
    assert m["recall"] == pytest.approx(sk.recall_score(rt, rp, zero_division=0), **close)
    assert m["auroc"] == pytest.approx(sk.roc_auc_score(rt, ev["scores"]), **close)
    assert m["auprc"] == pytest.approx(sk.average_precision_score(rt, ev["scores"]), **close)


def test_cases_hold_what_they_are_for():
    z, y = CASES["absent_class"]
    conf = mr.evaluate(z, y, 5, False)["confusion"]
    assert conf[3].sum() == 0 and conf[:, 3].sum() == 0
    z, y = CASES["ties"]
    assert len(np.unique(mr.referable_score(z))) < len(y) // 4
    z, y = CASES["half"]
    s = mr.referable_score(z)
    assert (s[::4] == 0.5).all() and not (s[::4] > 0.5).any()  # 0.5 is not referable (strict >)


def test_pairwise_definition_of_auroc_and_auprc():
    """The kernel's pairwise sums (include/lgnn.h) equal the restatement's threshold integrals."""
    rng = np.random.default_rng(3)
    s = rng.integers(0, 6, 200) / 8.0
    pos = rng.random(200) < 0.3
    neg_s, pos_s = s[~pos], s[pos]
    gt = np.array([(neg_s < v).sum() for v in pos_s])
    eq = np.array([(neg_s == v).sum() for v in pos_s])
    tp = np.array([(pos_s >= v).sum() for v in pos_s])
    fp = np.array([(neg_s >= v).sum() for v in pos_s])
    assert mr.auroc(s, pos) == pytest.approx((gt + eq / 2).sum() / (pos.sum() * (~pos).sum()),
                                             rel=1e-14)
    assert mr.auprc(s, pos) == pytest.approx((tp / (tp + fp)).sum() / pos.sum(), rel=1e-14)


def test_hand_computed_cases():
    y = np.array([0, 1, 2, 3, 4, 2, 1])
    perfect = mr.multiclass_metrics(mr.confusion_matrix(y, y, 5))
    assert perfect["kappa"] == 1.0 and perfect["micro_acc"] == 1.0 and perfect["macro_f1"] == 1.0
    constant = mr.multiclass_metrics(mr.confusion_matrix(np.full_like(y, 2), y, 5))
    assert constant["kappa"] == 0.0
    assert constant["macro_recall"] == pytest.approx(1 / 5)  # classes 0..4 all among the targets
    # one class only, predicted and true: no expected disagreement to compare with
    assert math.isnan(mr.multiclass_metrics(mr.confusion_matrix([1, 1], [1, 1], 3))["kappa"])
    # [[2, 1], [0, 1]]: n wO = 4, w rows x cols = 2 * 3 + 2 * 1 -> kappa = 1 - 4 / 8
    assert mr.multiclass_metrics(np.array([[2, 1], [0, 1]]))["kappa"] == 0.5
    # half to even, after the clamp to [0, C - 1]
    p, r = mr.regression_pred(np.array([0.5, 1.5, 2.5, 3.5, -3.0, 9.0, 2.4999]), 5)
    assert r.tolist() == [0, 2, 2, 4, 0, 4, 2] and p.tolist()[4:6] == [0.0, 4.0]
    assert torch.round(torch.tensor([0.5, 1.5, 2.5, 3.5])).tolist() == [0.0, 2.0, 2.0, 4.0]
    ev = mr.evaluate(np.array([0.5, 1.5, 2.5]), np.array([0, 2, 3]), 5, regression=True)
    assert ev["referable"] == (1, 0, 0, 2) and "auroc" not in ev["metrics"]
    # scores 0.9+ 0.8- 0.8+ 0.1-: 3.5 of 4 pairs ordered; AP = (1/2)(1) + (1/2)(2/3)
    s, pos = np.array([0.9, 0.8, 0.8, 0.1]), np.array([True, False, True, False])
    assert mr.auroc(s, pos) == 3.5 / 4 and mr.auprc(s, pos) == pytest.approx(5 / 6, rel=1e-15)
    assert math.isnan(mr.auroc(s, np.ones(4, bool))) and mr.auprc(s, np.ones(4, bool)) == 1.0
    assert math.isnan(mr.auroc(s, np.zeros(4, bool))) and math.isnan(mr.auprc(s, np.zeros(4, bool)))
    assert mr.referable_metrics(0, 0, 0, 0) == {"acc": 0.0, "f1": 0.0, "precision": 0.0,
                                                "recall": 0.0}


def test_header_declares_the_evaluation_entries():
    from lesion_gnn_amd import _lib

    text = open(os.path.join(ROOT, "include", "lgnn.h")).read()
    assert re.search(r"^#define LGNN_ABI_VERSION 40$", text, flags=re.M)
    assert _lib.ABI_VERSION == 40
    for name in ("lgnn_eval_update", "lgnn_eval_compute", "lgnn_eval_workspace_bytes",
                 "lgnn_eval_merge"):
        assert name in _lib.SIGNATURES, name
    assert [p[1] for p in _lib.PARAMS["lgnn_eval_update"]] == [
        "z", "target", "weight", "B", "C", "regression", "smooth_l1", "counts", "loss_acc",
        "scores", "positive", "capacity", "stream"]
    assert _lib.PARAMS["lgnn_eval_compute"][7] == ("double*", "result")
    assert _lib.LGNN_EVAL_RANK_CHUNK >= 64 and _lib.LGNN_EVAL_RESULTS == 16
    assert _lib.LGNN_EVAL_EXTRA == 6
    # every entry cites the reference lines it replaces
    block = text[text.index("Evaluation: grading metrics"):]
    assert "models/base.py:190-233" in block and "metrics.py" in block


def test_library_validates_evaluation_arguments_without_gpu():
    from lesion_gnn_amd import _lib

    lib = _lib.load()
    assert lib.lgnn_abi_version() == 40
    assert lib.lgnn_eval_update(None, None, None, 4, 5, 0, 0, None, None, None, None, 16,
                                None) == _lib.LGNN_EINVAL
    assert lib.lgnn_eval_update(1, 1, None, 4, _lib.LGNN_EVAL_MAX_CLASSES + 1, 0, 0, 1, 1, 1, 1,
                                16, None) == _lib.LGNN_EINVAL
    assert lib.lgnn_eval_update(1, 1, None, 4, 5, 0, 0, 1, 1, None, None, 16,
                                None) == _lib.LGNN_EINVAL  # probabilistic needs the score buffer
    assert lib.lgnn_eval_compute(1, 1, 1, 1, 16, 5, 0, 1, 1, 8, None) == _lib.LGNN_ENOSPC
    assert lib.lgnn_eval_workspace_bytes(100) == 1600
    assert lib.lgnn_eval_merge(5, 1, 1, None, None, 1, 1, None, None, 0, None) == _lib.LGNN_EINVAL


def _gcn_module(loss_type="CE"):
    from lesion_gnn_amd.models import GCNConfig, OptimizerConfig, get_model

    cfg = GCNConfig(optimizer=OptimizerConfig(loss_type=loss_type), hidden_channels=[16, 16],
                    dropout=0.0, compile=False)
    cfg.num_classes.value, cfg.input_features.value = 5, 8
    cfg.optimizer.class_weights.value = torch.ones(5)
    return get_model(cfg)


def _gin_module():
    from lesion_gnn_amd.models import GINConfig, OptimizerConfig, get_model

    cfg = GINConfig(optimizer=OptimizerConfig(), hidden_channels=[16, 16], dropout=0.0,
                    compile=False, pool="add")
    cfg.num_classes.value, cfg.input_features.value = 5, 8
    cfg.optimizer.class_weights.value = torch.ones(5)
    return get_model(cfg)


def test_base_module_has_the_evaluation_methods():
    from lesion_gnn_amd.models import BaseModule

    for name in ("logits_to_preds", "validation_step", "test_step", "epoch_metrics",
                 "reset_metrics"):
        assert callable(getattr(BaseModule, name)), name
    m = _gcn_module()
    z = torch.tensor([[0.2, 0.7], [1.5, 2.5]])
    assert m.logits_to_preds(z) is z  # reference base.py:191-192
    reg = _gcn_module("MSE")
    assert reg.logits_to_preds(torch.tensor([0.5, 1.5, 2.5, 3.2])).tolist() == [0, 2, 2, 3]
    assert m.epoch_metrics("val") == {}
    m.reset_metrics("val")


@pytest.mark.parametrize("make", [_gcn_module, _gin_module])
def test_evaluators_stay_out_of_the_module_state(make):
    from lesion_gnn_amd.metrics import GradingMetrics

    m = make()
    keys, nparams = list(m.state_dict()), len(list(m.parameters()))
    children, buffers = list(m.named_modules()), [k for k, _ in m.named_buffers()]
    ev = m.evaluator("val", "DDR")
    assert isinstance(ev, GradingMetrics) and m.evaluator("val", "DDR") is ev
    assert m.evaluator("test", "DDR") is not ev
    assert (ev.num_classes, ev.regression, ev.loss_kind) == (5, False, "CE")
    assert list(m.state_dict()) == keys and len(list(m.parameters())) == nparams
    assert list(m.named_modules()) == children and [k for k, _ in m.named_buffers()] == buffers
    m.to(torch.float32)
    assert list(m.state_dict()) == keys


def test_grading_metrics_refuses_cpu_tensors_and_bad_configurations():
    from lesion_gnn_amd._lib import LgnnError
    from lesion_gnn_amd.metrics import GradingMetrics

    ev = GradingMetrics(5, False, "CE")
    with pytest.raises(LgnnError):
        ev.update(torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(LgnnError):
        ev.compute()
    with pytest.raises(ValueError):
        GradingMetrics(5, True, "CE")
    with pytest.raises(ValueError):
        GradingMetrics(5, False, "MSE")
    with pytest.raises(ValueError):
        ev.merge(GradingMetrics(4, False, "CE"))
    ev.reset()
    assert ev.overflow is False and ev.device is None
