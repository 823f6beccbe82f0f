"""CPU references of the edge collation and of `lesion_gnn_amd.training.train`. Test-only; next to
tests/loader_ref.py and tests/trajectory_ref.py.

`collate_edges_ref` is PyG's Collater for edge_index (and an edge attribute) after the per-graph
transforms: the selected graphs' edge slices, each moved from its graph's rows in the store to its
rows in the batch, concatenated. Copies and integer adds are exact: every comparison is
`torch.equal`.

`fit_oracle(family, batch_size, dtype)` is the whole of `train()` in plain CPU torch on the
oracle's models (oracle/pyg_ref.py), in float32 or float64: the same seeds, the same host-drawn
`epoch_order`, `synth.knn_edges` per graph, `collate_ref` + `collate_edges_ref` per batch,
torch.optim.AdamW, `metrics_ref` for every validation and test, and the package's own callback
classes applied to the oracle's metric sequence.

The fixture: a train store of 48 graphs (sizes 1, 2, 3, 5, 70, 130, 300 and 41 lognormal ones),
two validation and two test stores of 16 graphs, 16 features, 5 grades that the features carry
(channel y of every node is shifted by 1), KNNGraph(k=6, loop=True); GCN, GIN and GAT (heads 2)
with hidden [32, 32], dropout 0, cross-entropy; 30 epochs, validation every 10, patience 2
validations, monitor val_valA_kappa (max). SEEDS holds, per (family, batch_size), a seed at which
the float32 and float64 oracles agree on every confusion matrix and decision with the margin
tests/test_fit_ref.py asserts.
"""
from __future__ import annotations

import dataclasses
import math
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

import oracle.pyg_ref as ref
from lesion_gnn_amd import synth
from lesion_gnn_amd.datasets import batch_bounds, epoch_order
from lesion_gnn_amd.datasets.base import BaseDatasetConfig
from lesion_gnn_amd.datasets.datamodule import DataConfig
from lesion_gnn_amd.models import (GATConfig, GCNConfig, GINConfig, OptimizerConfig, get_model)
from lesion_gnn_amd.training import VALIDATION_INTERVAL, EarlyStopping, ModelCheckpoint
from lesion_gnn_amd.transforms import TransformConfig
from lesion_gnn_amd.utils.config import Config
from tests import metrics_ref as mr
from tests.loader_ref import collate_ref

D_IN, CLASSES, K = 16, 5, 6
HIDDEN = [32, 32]
MAX_EPOCHS, PATIENCE = 30, 20
TRAIN_FIXED = [1, 2, 3, 5, 70, 130, 300]
FAMILIES = ("gcn", "gin", "gat")
BATCH_SIZES = (20, 10000)
MONITOR = "val_valA_kappa"
# GIN: at 1e-3 no seed in 0..19 meets the fixture condition (the float32 oracle is 2e-4 to 7e-4
# from the float64 one in the logits after 30 epochs: BatchNorm and Adam's eps = 1e-8), so its rate
# is lowered, as the condition is not to be loosened
LR = {"gcn": 1e-3, "gin": 1e-4, "gat": 1e-3}
METRIC_NAMES = ("micro_acc", "kappa", "macro_f1", "macro_precision", "macro_recall", "acc", "f1",
                "precision", "recall", "auroc", "auprc")
COUNT_METRICS = METRIC_NAMES[:9]
# per (family, batch_size), the seed in 0..19 at which the fixture condition holds by the widest
# margin over the float32 oracle's distance (tests/test_fit_ref.py asserts it and records both)
SEEDS = {("gcn", 20): 7, ("gcn", 10000): 19, ("gin", 20): 17, ("gin", 10000): 10,
         ("gat", 20): 7, ("gat", 10000): 4}


# ----------------------------------------------------------------------------------------------
# edges
# ----------------------------------------------------------------------------------------------


def store_edges(pos: torch.Tensor, ptr: torch.Tensor, k: int = K, loop: bool = True):
    """(edge_index [2, E] over the store's rows, edge_ptr [G + 1]): KNNGraph(k, loop) per graph."""
    pieces, counts = [], []
    for g in range(ptr.numel() - 1):
        a, b = int(ptr[g]), int(ptr[g + 1])
        ei = synth.knn_edges(pos[None, a:b], k, loop)[0] + a if b > a else \
            torch.empty(2, 0, dtype=torch.int64)
        pieces.append(ei)
        counts.append(ei.size(1))
    edge_ptr = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
    return torch.cat(pieces, dim=1).contiguous(), edge_ptr


def collate_edges_ref(edge_index, edge_weight, edge_ptr, ptr, ids):
    """(edge_index [2, sum m_b], edge_weight or None, edge_ptr [B + 1]) of the graphs `ids`."""
    ids = [int(i) for i in ids]
    sizes = [int(ptr[i + 1] - ptr[i]) for i in ids]
    out_ptr = [0]
    for s in sizes:
        out_ptr.append(out_ptr[-1] + s)
    cols = [slice(int(edge_ptr[i]), int(edge_ptr[i + 1])) for i in ids]
    parts = [edge_index[:, c] - int(ptr[i]) + o for c, i, o in zip(cols, ids, out_ptr)]
    out_ei = torch.cat(parts, dim=1) if ids else edge_index[:, :0]
    out_w = None
    if edge_weight is not None:
        out_w = torch.cat([edge_weight[c] for c in cols]) if ids else edge_weight[:0]
    m = torch.tensor([0] + [c.stop - c.start for c in cols], dtype=torch.int64)
    return out_ei.contiguous(), out_w, m.cumsum(0)


# ----------------------------------------------------------------------------------------------
# the fixture
# ----------------------------------------------------------------------------------------------


def make_store_tensors(sizes: list[int], seed: int):
    """(x, pos, y, ptr) on the host; the grade is carried by the features."""
    gen = torch.Generator().manual_seed(seed)
    G, ptr = len(sizes), torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
    rows = int(ptr[-1])
    y = torch.randint(0, CLASSES, (G,), generator=gen)
    x = torch.randn(rows, D_IN, generator=gen, dtype=torch.float32)
    pos = torch.rand(rows, 2, generator=gen, dtype=torch.float64)
    graph = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    x[torch.arange(rows), y[graph]] += 1.0
    return x, pos, y, ptr


def fixture_tensors() -> dict:
    """Dataset name -> (x, pos, y, ptr), host tensors."""
    gen = torch.Generator().manual_seed(4242)
    out = {"train": make_store_tensors(
        TRAIN_FIXED + synth.graph_sizes(48 - len(TRAIN_FIXED), "lognormal", gen), 100)}
    for i, name in enumerate(("valA", "valB", "testA", "testB")):
        out[name] = make_store_tensors(synth.graph_sizes(16, "lognormal", gen), 101 + i)
    return out


def _dataset(name: str) -> BaseDatasetConfig:
    return BaseDatasetConfig(name=name, root="", nodes=None)


def make_config(family: str, batch_size: int, seed: int | None = None, max_epochs: int = MAX_EPOCHS,
                lr: float | None = None) -> Config:
    # the defaults: AdamW, weight_decay 0.01, cross-entropy, uniform class weights
    opt = OptimizerConfig(lr=LR[family] if lr is None else lr)
    if family == "gcn":
        model = GCNConfig(optimizer=opt, hidden_channels=list(HIDDEN), dropout=0.0, compile=False)
    elif family == "gin":
        model = GINConfig(optimizer=opt, hidden_channels=list(HIDDEN), dropout=0.0, compile=False)
    else:
        model = GATConfig(optimizer=opt, hiddden_channels=list(HIDDEN), heads=2, dropout=0.0,
                          compile=False)
    data = DataConfig(train_datasets=[_dataset("train")],
                      val_datasets=[_dataset("valA"), _dataset("valB")],
                      test_datasets=[_dataset("testA"), _dataset("testB")],
                      transforms=[TransformConfig(name="KNNGraph", kwargs=dict(k=K, loop=True))],
                      batch_size=batch_size, num_workers=0)
    return Config(dataset=data, model=model, monitored_metric=MONITOR, monitor_mode="max",
                  early_stopping_patience=PATIENCE, max_epochs=max_epochs,
                  seed=SEEDS[family, batch_size] if seed is None else seed,
                  project_name="fit-fixture")


# ----------------------------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------------------------


@dataclasses.dataclass
class FitResult:
    train_losses: list        # one float64 0-d tensor per epoch run
    val_losses: list          # per validation: {dataset: float64 0-d tensor}
    validations: list         # per validation: the metrics dict (floats)
    val_confusions: list      # per validation: {dataset: [C, C] int64 array}
    saved: list               # the validations that wrote a best checkpoint
    last_epoch: int           # the last epoch run
    final_state: dict         # state_dict after fit, keys without "model.", float64
    best_state: dict          # state_dict of the best checkpoint, likewise
    test: dict                # the flat test metrics
    test_confusions: dict
    logits: list              # every validation and test logits tensor, float64, in order

    def named(self) -> dict:
        out = {f"train_loss/{e}": v for e, v in enumerate(self.train_losses)}
        for i, d in enumerate(self.val_losses):
            out.update({f"val_loss/{i}/{name}": v for name, v in d.items()})
        out.update({f"final/{k}": v for k, v in self.final_state.items()})
        out.update({f"best/{k}": v for k, v in self.best_state.items()})
        return out

    def decisions(self) -> tuple:
        return tuple(self.saved), self.last_epoch


def to64(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu()
    return t.double() if t.is_floating_point() else t.clone()


def strip_state(state: dict) -> dict:
    """A module state_dict with the `model.` prefix dropped and the criterion's buffer left out,
    floating tensors as float64."""
    return {k[len("model."):]: to64(v) for k, v in state.items() if k.startswith("model.")}


def _oracle_model(family: str, dtype):
    if family == "gat":
        m = ref.GAT(D_IN, list(HIDDEN), CLASSES, heads=2, dropout=0.0)
    else:
        m = getattr(ref, family.upper())(D_IN, list(HIDDEN), CLASSES, 0.0)
    return m.to(dtype)


def metrics_of(stage: str, name: str, logits: torch.Tensor, y: torch.Tensor, weight) -> tuple:
    """({f"{stage}_{name}_{metric}": value}, confusion matrix, loss tensor) of one dataset."""
    res = mr.evaluate(logits.double().numpy(), y.numpy(), CLASSES, False)
    out = {f"{stage}_{name}_{k}": float(v) for k, v in res["metrics"].items()}
    loss = F.cross_entropy(logits, y, weight=weight)
    if stage == "val":
        out[f"val_{name}_loss"] = float(loss)
    return out, res["confusion"], to64(loss)


_CACHE: dict = {}


def fit_oracle(family: str, batch_size: int, dtype: torch.dtype, seed: int | None = None,
               max_epochs: int = MAX_EPOCHS, lr: float | None = None) -> FitResult:
    key = (family, batch_size, dtype, seed, max_epochs, lr)
    if key not in _CACHE:
        _CACHE[key] = _fit_oracle(family, batch_size, dtype, seed, max_epochs, lr)
    return _CACHE[key]


def _fit_oracle(family, batch_size, dtype, seed, max_epochs, lr) -> FitResult:
    config = make_config(family, batch_size, seed, max_epochs, lr)
    data = fixture_tensors()
    edges = {name: store_edges(t[1], t[3]) for name, t in data.items()}

    def batches(name: str, order: torch.Tensor):
        x, pos, y, ptr = data[name]
        ei, eptr = edges[name]
        for a, b in batch_bounds(order.numel(), batch_size):
            ids = order[a:b]
            bx, _, by, bb, _ = collate_ref(x, pos, y, ptr, ids)
            bei, _, _ = collate_edges_ref(ei, None, eptr, ptr, ids)
            yield bx.to(dtype), bei, bb, by, ids.numel()

    # train(): seed, (data), placeholders, model, optimizer
    torch.manual_seed(config.seed)
    generator = torch.Generator().manual_seed(config.seed)
    counts = torch.unique(data["train"][2], return_counts=True)[1]
    config.model.optimizer.class_weights.value = torch.ones_like(counts).float()
    config.model.num_classes.value = int(data["train"][2].max()) + 1
    config.model.input_features.value = D_IN
    module = get_model(config.model)  # the package's initial weights, built on the host
    model = _oracle_model(family, dtype)
    model.load_state_dict({k[len("model."):]: v.detach().clone()
                           for k, v in module.state_dict().items() if k.startswith("model.")})
    weight = config.model.optimizer.class_weights.value.to(dtype)
    opt = torch.optim.AdamW(model.parameters(), lr=config.model.optimizer.lr,
                            weight_decay=config.model.optimizer.weight_decay, foreach=False)

    tmp = tempfile.TemporaryDirectory()
    ckpt = ModelCheckpoint(tmp.name, config.monitored_metric, config.monitor_mode)
    stop = EarlyStopping(config.monitored_metric, config.monitor_mode,
                         config.early_stopping_patience // VALIDATION_INTERVAL)
    res = FitResult([], [], [], [], [], -1, {}, {}, {}, {}, [])

    def evaluate(stage: str, names) -> tuple:
        model.eval()
        metrics, confusions, losses = {}, {}, {}
        with torch.no_grad():
            for name in names:
                order = epoch_order(data[name][2].numel(), False)
                outs = [(model(bx, bei, bb, n), by) for bx, bei, bb, by, n in batches(name, order)]
                logits, y = torch.cat([o for o, _ in outs]), torch.cat([t for _, t in outs])
                m, confusions[name], losses[name] = metrics_of(stage, name, logits, y, weight)
                metrics.update(m)
                res.logits.append(to64(logits))
        return metrics, confusions, losses

    G, step = data["train"][2].numel(), 0
    for epoch in range(max_epochs):
        if stop.stopped:
            break
        res.last_epoch = epoch
        model.train()
        total, seen = 0.0, 0
        for bx, bei, bb, by, n in batches("train", epoch_order(G, True, generator)):
            opt.zero_grad(set_to_none=True)
            loss = F.cross_entropy(model(bx, bei, bb, n), by, weight=weight)
            loss.backward()
            opt.step()
            step += 1
            total, seen = total + float(loss.detach().double()) * n, seen + n
        res.train_losses.append(torch.tensor(total / seen, dtype=torch.float64))
        if (epoch + 1) % VALIDATION_INTERVAL == 0:
            metrics, confusions, losses = evaluate("val", ("valA", "valB"))
            metrics["train_loss"] = float(res.train_losses[-1])
            res.validations.append(metrics)
            res.val_confusions.append(confusions)
            res.val_losses.append(losses)
            ckpt.on_validation_end(metrics, epoch, step, lambda: {
                "state_dict": {k: v.detach().clone() for k, v in model.state_dict().items()}})
            stop.on_validation_end(metrics)
    res.saved = list(ckpt.saved)
    res.final_state = {k: to64(v) for k, v in model.state_dict().items()}
    best = torch.load(ckpt.best_model_path, weights_only=True)["state_dict"]
    res.best_state = {k: to64(v) for k, v in best.items()}
    model.load_state_dict(best)
    res.test, res.test_confusions, _ = evaluate("test", ("testA", "testB"))
    tmp.cleanup()
    return res


def fixture_condition(r64: FitResult, r32: FitResult) -> tuple:
    """(holds, margin, diff): the float32 and float64 oracles agree on every confusion matrix and
    decision, and the smallest top-2 logit margin of the float64 run is at least 100 times the
    largest logit difference between the two runs."""
    same = r64.decisions() == r32.decisions() and len(r64.logits) == len(r32.logits) and all(
        np.array_equal(a[n], b[n]) for a, b in zip(r64.val_confusions + [r64.test_confusions],
                                                    r32.val_confusions + [r32.test_confusions])
        for n in a)
    if not same:
        return False, math.nan, math.nan
    margin = min(float((t.topk(2, dim=1).values[:, 0] - t.topk(2, dim=1).values[:, 1]).min())
                 for t in r64.logits)
    diff = max(float((a - b).abs().max()) for a, b in zip(r64.logits, r32.logits))
    return margin >= 100.0 * diff, margin, diff
