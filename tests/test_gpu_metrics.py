"""GPU checks of the evaluation path (csrc/metrics.hip, lesion_gnn_amd.metrics, BaseModule's
validation_step / test_step / epoch_metrics) against tests/metrics_ref.py, the float64 restatement
that tests/test_metrics_ref.py pins to scikit-learn.

Bounds: every counter bit-exact; the scalar metrics derived from counters within 1e-12 relative
(both sides are a handful of double operations on the same integers); stored scores within 1e-6
absolute of a float64 softmax (fp32 epsilon times a few operations on values <= 1); AUROC / AUPRC
within 1e-12 relative of the restatement applied to the scores the kernel stored (so a last-ulp
difference in a score cannot move a pair from one side to the other); the loss within 1e-6
relative of torch's CPU criterion."""
import copy
import math

import numpy as np
import pytest
import torch

from lesion_gnn_amd import _lib, synth
from lesion_gnn_amd._lib import LgnnError
from lesion_gnn_amd.metrics import GradingMetrics
from tests import metrics_ref as mr

pytestmark = pytest.mark.gpu

T = _lib.LGNN_EVAL_RANK_CHUNK
COUNTER_KEYS = ("micro_acc", "kappa", "macro_f1", "macro_precision", "macro_recall", "acc", "f1",
                "precision", "recall")


# ----------------------------------------------------------------------------------------------
# inputs and comparisons
# ----------------------------------------------------------------------------------------------

def grid_logits(B, C, seed):
    """Logits on a coarse grid (multiples of 0.5 in [-2, 2]): argmax ties and duplicate rows."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (B, C), generator=g).float() * 0.5, \
        torch.randint(0, C, (B,), generator=g)


def grid_regression(B, C, seed):
    """Regression outputs [B, 1] on multiples of 0.5 in [-1, C]: both clamp bounds and every
    half-way case of the rounding."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 2 * C + 1, (B, 1), generator=g).float() * 0.5, \
        torch.randint(0, C, (B,), generator=g)


def rank_inputs(N, pattern, seed):
    """C = 3 logits (0, 0, v) with v from 8 values: 8 distinct referable scores e^v / (2 + e^v);
    targets 2 (referable) or 0 by `pattern`."""
    g = torch.Generator().manual_seed(seed)
    z = torch.zeros(N, 3)
    z[:, 2] = torch.randint(-4, 4, (N,), generator=g).float() * 0.5
    if pattern == "mixed":
        y = torch.randint(0, 2, (N,), generator=g) * 2
    elif pattern == "all_positive":
        y = torch.full((N,), 2)
    elif pattern == "all_negative":
        y = torch.zeros(N, dtype=torch.int64)
    else:  # one positive, in the last chunk
        y = torch.zeros(N, dtype=torch.int64)
        y[N - 1 - (N // 3)] = 2
    return z, y


def same(got: float, want: float, rel: float) -> bool:
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    return abs(got - want) <= rel * abs(want)


def snapshot(ev: GradingMetrics) -> dict:
    """The evaluator's state on the host: counters split up, the stored rows only."""
    st = ev.state()
    C = ev.num_classes
    counts = st["counts"].cpu().numpy()
    n = int(counts[C * C + _lib.LGNN_EVAL_NSEEN])
    out = {"confusion": counts[:C * C].reshape(C, C).copy(),
           "referable": tuple(int(v) for v in counts[C * C:C * C + 4]), "n_seen": n,
           "n_bad": int(counts[C * C + _lib.LGNN_EVAL_NBAD]),
           "loss_acc": st["loss_acc"].cpu().numpy().copy()}
    if st["scores"] is not None:
        stored = min(n, ev.capacity)
        out["scores"] = st["scores"][:stored].cpu().numpy().copy()
        out["positive"] = st["positive"][:stored].cpu().numpy().astype(bool)
    return out


def assert_states_equal(a: dict, b: dict, loss_bitwise: bool = True):
    assert np.array_equal(a["confusion"], b["confusion"])
    assert (a["referable"], a["n_seen"], a["n_bad"]) == (b["referable"], b["n_seen"], b["n_bad"])
    if "scores" in a:
        assert a["scores"].tobytes() == b["scores"].tobytes()
        assert np.array_equal(a["positive"], b["positive"])
    if loss_bitwise:
        assert a["loss_acc"].tobytes() == b["loss_acc"].tobytes()
    else:  # the same terms summed in another grouping: double rounding
        np.testing.assert_allclose(a["loss_acc"], b["loss_acc"], rtol=1e-12)


def torch_loss(kind, out, y, C, weight=None):
    """torch's CPU criterion as the reference applies it (models/base.py:88-96, :204-206)."""
    F = torch.nn.functional
    if kind == "CE":
        return F.cross_entropy(out, y, weight=weight).item()
    p = torch.clamp(out.reshape(-1), 0, C - 1)
    return (F.mse_loss if kind == "MSE" else F.smooth_l1_loss)(p, y.float()).item()


def check_against_restatement(ev, got, out, y, kind, weight=None):
    """Every bound of the module docstring, for evaluator `ev` (metrics `got`) fed (out, y)."""
    C, regression = ev.num_classes, ev.regression
    want = mr.evaluate(out.numpy(), y.numpy(), C, regression)
    if not regression:  # the test's own inputs: no float64 score within fp32 rounding of 0.5
        assert (np.abs(want["scores"] - 0.5) > 1e-6).all()
    st = snapshot(ev)
    assert np.array_equal(st["confusion"], want["confusion"])
    assert st["referable"] == want["referable"]
    assert (st["n_seen"], st["n_bad"]) == (len(y), 0)
    assert np.array_equal(ev.confusion_matrix().cpu().numpy(), want["confusion"])
    for key in COUNTER_KEYS:
        assert same(got[key], want["metrics"][key], 1e-12), (key, got[key], want["metrics"][key])
    if regression:
        assert "auroc" not in got and "auprc" not in got
    else:
        assert np.abs(st["scores"].astype(np.float64) - want["scores"]).max() <= 1e-6
        assert np.array_equal(st["positive"], want["positive"])
        stored = st["scores"].astype(np.float64)
        for key, fn in (("auroc", mr.auroc), ("auprc", mr.auprc)):
            ref = fn(stored, st["positive"])
            assert same(got[key], ref, 1e-12), (key, got[key], ref)
    assert same(got["loss"], torch_loss(kind, out, y, C, weight), 1e-6)
    assert ev.overflow is False


# ----------------------------------------------------------------------------------------------
# the kernels
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["CE", "CE_weighted", "MSE", "SmoothL1"])
@pytest.mark.parametrize("C", [2, 5, 7])
@pytest.mark.parametrize("B", [1, 3, 1024, 5000])
def test_counters_metrics_scores_and_loss(cuda, B, C, kind):
    seed = 1000 * B + 10 * C + len(kind)
    weight = None
    if kind.startswith("CE"):
        out, y = grid_logits(B, C, seed)
        if kind == "CE_weighted":
            weight = torch.rand(C, generator=torch.Generator().manual_seed(seed)) + 0.1
        ev = GradingMetrics(C, False, "CE", class_weight=weight)
    else:
        out, y = grid_regression(B, C, seed)
        ev = GradingMetrics(C, True, kind)
    ev.update(out.to(cuda), y.to(cuda))
    check_against_restatement(ev, ev.compute(), out, y, kind.split("_")[0], weight)


@pytest.mark.parametrize("N", [1, 63, 64, 65, T - 1, T + 1, 2 * T + 17])
def test_rank_kernel_sizes(cuda, N):
    """AUROC / AUPRC at sizes around the wave, the workgroup and the LDS chunk, on at most 8
    distinct scores: mixed classes, all positive, all negative, a single positive."""
    for k, pattern in enumerate(("mixed", "all_positive", "all_negative", "one_positive")):
        z, y = rank_inputs(N, pattern, 31 * N + k)
        ev = GradingMetrics(3, False, "CE")
        ev.update(z.to(cuda), y.to(cuda))
        got = ev.compute()
        st = snapshot(ev)
        assert len(np.unique(st["scores"])) <= 8 and len(st["scores"]) == N
        assert np.array_equal(st["positive"], (y >= 2).numpy())
        stored = st["scores"].astype(np.float64)
        want_roc, want_prc = mr.auroc(stored, st["positive"]), mr.auprc(stored, st["positive"])
        assert same(got["auroc"], want_roc, 1e-12), (pattern, got["auroc"], want_roc)
        assert same(got["auprc"], want_prc, 1e-12), (pattern, got["auprc"], want_prc)
        if pattern == "all_positive":
            assert math.isnan(got["auroc"]) and got["auprc"] == 1.0
        elif pattern == "all_negative":
            assert math.isnan(got["auroc"]) and math.isnan(got["auprc"])
        elif N > 1:
            assert 0.0 <= got["auroc"] <= 1.0 and 0.0 < got["auprc"] <= 1.0


def test_updates_append_across_batches(cuda):
    """Updates of 5, 64, 1 and 130 rows hold what one update of the 200 rows holds."""
    z, y = grid_logits(200, 5, 11)
    whole, parts = GradingMetrics(5, False, "CE"), GradingMetrics(5, False, "CE")
    whole.update(z.to(cuda), y.to(cuda))
    lo = 0
    for size in (5, 64, 1, 130):
        parts.update(z[lo:lo + size].to(cuda), y[lo:lo + size].to(cuda))
        lo += size
    assert_states_equal(snapshot(parts), snapshot(whole), loss_bitwise=False)
    a, b = parts.compute(), whole.compute()
    assert all(same(a[k], b[k], 0.0) for k in a if k != "loss") and same(a["loss"], b["loss"],
                                                                         1e-12)
    check_against_restatement(parts, a, z, y, "CE")


def test_captured_update_replays_append(cuda):
    """One captured update replayed on refilled inputs = the same updates run eagerly, bit for
    bit: the append offset is read on the device."""
    batches = [grid_logits(70, 5, 20 + k) for k in range(3)]
    eager = GradingMetrics(5, False, "CE")
    for z, y in batches:
        eager.update(z.to(cuda), y.to(cuda))
    sz, sy = batches[0][0].to(cuda), batches[0][1].to(cuda)
    ev = GradingMetrics(5, False, "CE")
    ev.update(sz, sy)  # allocates the state, loads the kernel
    ev.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(sz, sy)
    for z, y in batches:
        sz.copy_(z)
        sy.copy_(y)
        graph.replay()
    torch.cuda.synchronize()
    assert_states_equal(snapshot(ev), snapshot(eager))
    assert snapshot(ev)["n_seen"] == 210
    assert ev.compute() == eager.compute()
    check_against_restatement(ev, ev.compute(), torch.cat([b[0] for b in batches]),
                              torch.cat([b[1] for b in batches]), "CE")


def test_capacity_overflow(cuda):
    z, y = grid_logits(130, 5, 5)
    ev = GradingMetrics(5, False, "CE", capacity=100)
    ev.update(z[:64].to(cuda), y[:64].to(cuda))
    ev.update(z[64:].to(cuda), y[64:].to(cuda))
    got = ev.compute()
    want = mr.evaluate(z.numpy(), y.numpy(), 5, False)
    st = snapshot(ev)
    assert ev.overflow is True and math.isnan(got["auroc"]) and math.isnan(got["auprc"])
    assert np.array_equal(st["confusion"], want["confusion"])
    assert st["referable"] == want["referable"] and st["n_seen"] == 130
    assert len(st["scores"]) == 100
    assert np.abs(st["scores"] - want["scores"][:100]).max() <= 1e-6
    for key in COUNTER_KEYS:
        assert same(got[key], want["metrics"][key], 1e-12), key
    assert same(got["loss"], torch_loss("CE", z, y, 5), 1e-6)
    ev.reset()
    ev.update(z[:100].to(cuda), y[:100].to(cuda))  # exactly full is not an overflow
    got = ev.compute()
    assert ev.overflow is False and not math.isnan(got["auprc"])


@pytest.mark.parametrize("regression", [False, True])
def test_bad_target_raises(cuda, regression):
    C = 5
    out, y = grid_regression(9, C, 3) if regression else grid_logits(9, C, 3)
    y[4] = C
    ev = GradingMetrics(C, regression, "MSE" if regression else "CE")
    ev.update(out.to(cuda), y.to(cuda))
    st = snapshot(ev)
    assert (st["n_seen"], st["n_bad"]) == (8, 1)  # counted as bad and as nothing else
    keep = torch.arange(9) != 4
    want = mr.evaluate(out[keep].numpy(), y[keep].numpy(), C, regression)
    assert np.array_equal(st["confusion"], want["confusion"])
    if not regression:
        assert len(st["scores"]) == 8
    with pytest.raises(LgnnError, match="outside"):
        ev.compute()
    y[4] = -1
    ev.reset()
    ev.update(out.to(cuda), y.to(cuda))
    with pytest.raises(LgnnError):
        ev.compute()


@pytest.mark.parametrize("regression", [False, True])
def test_merge_equals_one_evaluator_fed_both_streams(cuda, regression):
    C = 5
    make = grid_regression if regression else grid_logits
    kind = "SmoothL1" if regression else "CE"
    (z1, y1), (z2, y2) = make(150, C, 1), make(77, C, 2)
    a, b, both = (GradingMetrics(C, regression, kind) for _ in range(3))
    a.update(z1.to(cuda), y1.to(cuda))
    b.update(z2[:40].to(cuda), y2[:40].to(cuda))
    b.update(z2[40:].to(cuda), y2[40:].to(cuda))
    for z, y in ((z1, y1), (z2, y2)):
        both.update(z.to(cuda), y.to(cuda))
    before = snapshot(b)
    a.merge(b)
    assert_states_equal(snapshot(b), before)  # the source is left as it is
    assert_states_equal(snapshot(a), snapshot(both), loss_bitwise=False)
    got, want = a.compute(), both.compute()
    assert got.keys() == want.keys()
    assert all(same(got[k], want[k], 0.0 if k != "loss" else 1e-12) for k in got)
    check_against_restatement(a, got, torch.cat([z1, z2]), torch.cat([y1, y2]), kind)
    empty = GradingMetrics(C, regression, kind)
    empty.merge(both)  # into an evaluator that has seen nothing
    assert_states_equal(snapshot(empty), snapshot(both))


def test_two_runs_are_bitwise_equal(cuda):
    z, y = grid_logits(3000, 7, 9)
    w = torch.rand(7, generator=torch.Generator().manual_seed(9)) + 0.1
    runs = []
    for _ in range(2):
        ev = GradingMetrics(7, False, "CE", class_weight=w)
        for lo in range(0, 3000, 1000):
            ev.update(z[lo:lo + 1000].to(cuda), y[lo:lo + 1000].to(cuda))
        got = ev.compute()
        runs.append((snapshot(ev), {k: np.float64(v).tobytes() for k, v in got.items()}))
    assert_states_equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]


def test_cpu_tensors_raise(cuda):
    ev = GradingMetrics(5, False, "CE")
    with pytest.raises(LgnnError):
        ev.update(torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError):
        ev.update(torch.zeros(4, 5, device=cuda), torch.zeros(4, dtype=torch.int32, device=cuda))


# ----------------------------------------------------------------------------------------------
# BaseModule
# ----------------------------------------------------------------------------------------------

def _gcn_module():
    from lesion_gnn_amd.models import GCNConfig, OptimizerConfig, get_model

    cfg = GCNConfig(optimizer=OptimizerConfig(), hidden_channels=[32, 32], dropout=0.0,
                    compile=False)
    cfg.num_classes.value, cfg.input_features.value = 5, 32
    cfg.optimizer.class_weights.value = torch.tensor([0.5, 1.0, 2.0, 1.5, 1.0])
    return get_model(cfg), "CE"


def _gat_module():
    from lesion_gnn_amd.models import get_model
    from tests.test_config import reference_model_section

    cfg = reference_model_section()  # GAT, MSE
    cfg.hiddden_channels = [32] * 3
    cfg.dropout, cfg.compile = 0.0, False
    cfg.num_classes.value, cfg.input_features.value = 5, 32
    cfg.optimizer.class_weights.value = torch.ones(5)
    return get_model(cfg), "MSE"


@pytest.mark.parametrize("make", [_gcn_module, _gat_module])
def test_module_validation_and_test_steps(cuda, make):
    torch.manual_seed(0)
    module, kind = make()
    module = module.to(cuda).eval()
    untouched = copy.deepcopy(module)
    keys = list(module.state_dict())
    batches = [synth.make_batch(8, n=64, k=6, d_in=32, seed=40 + i).to(cuda) for i in range(2)]
    # scale the head so that the 16 outputs spread over the grades
    for m in (module, untouched):
        with torch.no_grad():
            m.model.out_proj.weight.mul_(20.0)
    for i, b in enumerate(batches):
        assert module.validation_step(b, i, dataset_name="DDR") is None
    got = module.epoch_metrics("val")
    with torch.no_grad():
        outs = [module(b).cpu() for b in batches]  # regression: clamped, as the reference's
    out, y = torch.cat(outs), torch.cat([b.y.cpu() for b in batches])
    names = list(COUNTER_KEYS) + ["loss"] + ([] if module.is_regression else ["auroc", "auprc"])
    assert sorted(got) == sorted(f"val_DDR_{n}" for n in names) and "val_DDR_kappa" in got
    ev = module.evaluator("val", "DDR")
    want = mr.evaluate(out.numpy(), y.numpy(), 5, module.is_regression)
    st = snapshot(ev)
    assert np.array_equal(st["confusion"], want["confusion"]) and st["n_seen"] == 16
    assert st["referable"] == want["referable"]
    for key in COUNTER_KEYS:
        assert same(got[f"val_DDR_{key}"], want["metrics"][key], 1e-12), key
    if not module.is_regression:
        assert np.abs(st["scores"] - want["scores"]).max() <= 1e-6
        stored = st["scores"].astype(np.float64)
        assert same(got["val_DDR_auroc"], mr.auroc(stored, st["positive"]), 1e-12)
        assert same(got["val_DDR_auprc"], mr.auprc(stored, st["positive"]), 1e-12)
    weight = getattr(module.criterion, "weight", None)
    assert same(got["val_DDR_loss"],
                torch_loss(kind, out, y, 5, None if weight is None else weight.cpu()), 1e-6)
    # test_step: the reference's pair; its metrics under the dataloader index, without a loss
    pred, yb = module.test_step(batches[0], 0, dataloader_idx=1)
    assert pred.dtype == torch.int64 and torch.equal(yb, batches[0].y)
    if module.is_regression:
        assert torch.equal(pred.cpu(), torch.round(outs[0]).long())
    else:
        assert torch.equal(pred.cpu(), torch.argmax(outs[0], dim=1))
    tested = module.epoch_metrics("test")
    assert "test_1_kappa" in tested and "test_1_loss" not in tested
    assert module.epoch_metrics("val") == got  # reading does not reset
    module.reset_metrics("val")
    assert snapshot(ev)["n_seen"] == 0 and module.epoch_metrics("test") == tested
    # nothing else changed: the module's state, and the training step's loss
    assert list(module.state_dict()) == keys
    assert torch.equal(module.train().training_step(batches[0]).detach(),
                       untouched.train().training_step(batches[0]).detach())
