"""Optimizers whose step is one HIP launch (lgnn_adam_step, lgnn_adam_step_dlr, lgnn_sgd_step):
drop-ins for torch.optim.Adam / AdamW (amsgrad=False) and torch.optim.SGD as the reference's
configure_optimizers builds them (models/base.py:162-188). torch runs the same updates as
multi_tensor_apply launches plus a step-count kernel.

State per parameter mirrors torch's ('step', 'exp_avg', 'exp_avg_sq'; SGD: 'momentum_buffer',
and a 'step' of its own when momentum != 0); every parameter of a group shares one device step
tensor. Graph-capturable: the launch reads only device pointers. By default lr / betas / eps /
weight_decay are launch arguments, so fixed inside a captured graph.
No CPU path: parameters and gradients must be contiguous fp32 GPU tensors.

Training with a schedule on a captured step: build the optimizer with capturable=True (the
parameters already on the GPU). Each group's "lr" is then a 0-dim fp32 device tensor that the
launch reads on the device and that is never replaced: torch's schedulers fill_ it, so

    opt = Adam(model.parameters(), lr=1e-3, capturable=True)
    sched = LinearWarmupCosineAnnealingLR(opt, warmup_epochs=5, max_epochs=50)
    ... warm up, then capture forward + backward + opt.step() into a graph ...
    for batch in loader:
        refill the static inputs; graph.replay(); sched.step()      # between replays

changes the rate of the next replay with no host synchronisation. The rate then steps in fp32
(a scheduler's recursive form adds and scales the fp32 tensor; within 1e-5 of the base rate of
the float schedule over 500 epochs, tests/test_sched_tensor_lr.py). load_state_dict and
add_param_group keep the tensors too (values are copied in): a captured graph keeps its pointer.
"""
from __future__ import annotations

import math
import warnings

import torch

from . import _lib

MAX_TENSORS = 16  # LGNN_MAX_ADAM


class _DeviceLrOptimizer(torch.optim.Optimizer):
    """What Adam and SGD share: the per-group step ticket, and capturable=True's learning rate,
    one fp32 device tensor per group that lives as long as the optimizer."""

    def __init__(self, params, defaults, capturable: bool):
        lr = defaults["lr"]
        if isinstance(lr, torch.Tensor) and not capturable:
            raise ValueError("lgnn optim: a tensor lr needs capturable=True")
        self._capturable = bool(capturable)
        self._tickets: dict[int, torch.Tensor] = {}
        super().__init__(params, defaults)

    def _ticket(self, gi: int, dev) -> torch.Tensor:
        ticket = self._tickets.get(gi)
        if ticket is None:
            # last_workgroup's two-level ticket: 9 words, zeroed once, left zero
            ticket = self._tickets[gi] = torch.zeros(9, dtype=torch.int32, device=dev)
        return ticket

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if not self._capturable:
            return
        group = self.param_groups[-1]
        ps = group["params"]
        if not ps or any(not p.is_cuda or p.device != ps[0].device for p in ps):
            raise ValueError("lgnn optim: capturable=True places lr beside the parameters, which "
                             "must be on one GPU when the optimizer is built")
        lr = group["lr"]
        if isinstance(lr, torch.Tensor):  # the caller's own device rate, taken as it is
            if lr.numel() != 1 or lr.dtype != torch.float32 or lr.device != ps[0].device:
                raise ValueError("lgnn optim: a tensor lr is one fp32 element on the "
                                 "parameters' device")
        else:
            group["lr"] = torch.full((), float(lr), dtype=torch.float32, device=ps[0].device)

    def load_state_dict(self, state_dict):
        held = [g["lr"] for g in self.param_groups]
        super().load_state_dict(state_dict)  # replaces every group's values by the loaded ones
        for group, mine in zip(self.param_groups, held):
            lr = group["lr"]
            if not self._capturable:
                if isinstance(lr, torch.Tensor):  # saved by a capturable optimizer
                    group["lr"] = float(lr)
                continue
            if isinstance(lr, torch.Tensor):
                mine.copy_(lr.detach().to(mine.device, torch.float32).reshape(mine.shape))
            else:
                mine.fill_(float(lr))
            group["lr"] = mine  # the tensor a captured graph reads


class Adam(_DeviceLrOptimizer):
    def __init__(self, params, lr: float | torch.Tensor = 1e-3, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0, maximize: bool = False,
                 amsgrad: bool = False, decoupled: bool = False, capturable: bool = False):
        if amsgrad:
            raise NotImplementedError("lgnn Adam: amsgrad")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("lgnn Adam: lr, eps and weight_decay must be >= 0")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        maximize=maximize)
        super().__init__(params, defaults, capturable)
        self._decoupled = decoupled

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            _lib.require_gpu(*ps)
            dev = ps[0].device
            step_t = None
            for p in ps:
                if p.dtype != torch.float32 or not p.is_contiguous() or \
                        p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    raise _lib.LgnnError("lgnn Adam: contiguous fp32 parameters and gradients")
                st = self.state[p]
                if not st:
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                step_t = st.get("step", step_t)
            if step_t is None:
                step_t = torch.zeros((), dtype=torch.float32, device=dev)
            for p in ps:
                self.state[p]["step"] = step_t
            ticket = self._ticket(gi, dev)
            b1, b2 = group["betas"]
            # capturable: the group's device tensor, read by the launch (lgnn_adam_step_dlr)
            entry, lr = ("lgnn_adam_step_dlr", group["lr"]) if self._capturable else \
                ("lgnn_adam_step", float(group["lr"]))

            for c in range(0, len(ps), MAX_TENSORS):
                chunk = ps[c:c + MAX_TENSORS]
                _lib.call(entry, len(chunk), chunk, [p.grad for p in chunk],
                          [self.state[p]["exp_avg"] for p in chunk],
                          [self.state[p]["exp_avg_sq"] for p in chunk],
                          [p.numel() for p in chunk], step_t, ticket, lr,
                          float(b1), float(b2), float(group["eps"]),
                          float(group["weight_decay"]), int(self._decoupled),
                          int(group["maximize"]), int(c + MAX_TENSORS >= len(ps)),
                          _lib.stream(dev))
        return loss


class AdamW(Adam):
    def __init__(self, params, lr: float | torch.Tensor = 1e-3, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 1e-2, maximize: bool = False,
                 amsgrad: bool = False, capturable: bool = False):
        super().__init__(params, lr, betas, eps, weight_decay, maximize, amsgrad, decoupled=True,
                         capturable=capturable)


class SGD(_DeviceLrOptimizer):
    """torch.optim.SGD in one launch per 16 tensors (lgnn_sgd_step). With momentum the group's
    parameters share a device step count, which keeps torch's first-step rule (buf = g) under
    graph replay; a state loaded from torch.optim.SGD has buffers and no step, and continues
    from those buffers."""

    def __init__(self, params, lr: float | torch.Tensor = 1e-3, momentum: float = 0.0,
                 dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                 maximize: bool = False, capturable: bool = False):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening,
                        weight_decay=weight_decay, nesterov=nesterov, maximize=maximize)
        super().__init__(params, defaults, capturable)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            _lib.require_gpu(*ps)
            dev = ps[0].device
            for p in ps:
                if p.dtype != torch.float32 or not p.is_contiguous() or \
                        p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    raise _lib.LgnnError("lgnn SGD: contiguous fp32 parameters and gradients")
            momentum = float(group["momentum"])
            if momentum == 0.0:
                runs = [(ps, None, None, False)]  # no buffer, no first-step rule: no step is kept
            else:
                new = [p for p in ps if self.state[p].get("momentum_buffer") is None]
                old = [p for p in ps if self.state[p].get("momentum_buffer") is not None]
                step_t = next((self.state[p]["step"] for p in old if "step" in self.state[p]),
                              None)
                if step_t is None:  # buffers without a step: a state loaded from torch
                    step_t = torch.full((), 1.0 if old else 0.0, dtype=torch.float32, device=dev)
                elif step_t.device != dev or step_t.dtype != torch.float32:
                    step_t = step_t.to(dev, torch.float32)
                for p in new:
                    self.state[p]["momentum_buffer"] = torch.zeros_like(p)
                for p in ps:
                    self.state[p]["step"] = step_t
                ticket = self._ticket(gi, dev)
                if old and new:  # late joiners take their first step (buf = g) on a count of 0
                    runs = [(new, torch.zeros_like(step_t), ticket, False),
                            (old, step_t, ticket, True)]
                else:
                    runs = [(ps, step_t, ticket, True)]
            lr = group["lr"]
            lr, lr_dev = (0.0, lr) if isinstance(lr, torch.Tensor) else (float(lr), None)
            for run, step_t, ticket, advance in runs:
                for c in range(0, len(run), MAX_TENSORS):
                    chunk = run[c:c + MAX_TENSORS]
                    bufs = None if step_t is None else \
                        [self.state[p]["momentum_buffer"] for p in chunk]
                    _lib.call("lgnn_sgd_step", len(chunk), chunk, [p.grad for p in chunk], bufs,
                              [p.numel() for p in chunk], step_t, ticket, lr, lr_dev, momentum,
                              float(group["dampening"]), float(group["weight_decay"]),
                              int(group["nesterov"]), int(group["maximize"]),
                              int(advance and c + MAX_TENSORS >= len(run)),
                              _lib.stream(dev))
        return loss


class LinearWarmupCosineAnnealingLR(torch.optim.lr_scheduler.LRScheduler):
    """pl_bolts.optimizers.lr_scheduler.LinearWarmupCosineAnnealingLR (pl_bolts 0.7.0), the
    scheduler the reference's configure_optimizers builds by name (models/base.py:174-175; pl_bolts
    is not installed here). A closed-form schedule per base lr b, epoch e (= last_epoch), warmup
    w, max m, start s, minimum eta, as pl_bolts' _get_closed_form_lr():
      e < w:  s + e (b - s) / max(1, w - 1)          (linear warmup from s to b)
      e >= w: eta + (b - eta) (1 + cos(pi (e - w) / (m - w))) / 2   (cosine to eta at e = m)
    get_lr() is pl_bolts' recursive form (each step from the group's current lr), restated case
    for case, so the schedule equals pl_bolts' for every warmup including w = 0 (where pl_bolts
    starts at warmup_start_lr and decays from there, unlike the closed form)."""

    def __init__(self, optimizer, warmup_epochs: int, max_epochs: int,
                 warmup_start_lr: float = 0.0, eta_min: float = 0.0, last_epoch: int = -1):
        self.warmup_epochs = int(warmup_epochs)
        self.max_epochs = int(max_epochs)
        self.warmup_start_lr = float(warmup_start_lr)
        self.eta_min = float(eta_min)
        super().__init__(optimizer, last_epoch)

    def _closed_form(self, base_lr: float) -> float:
        e, w, m = self.last_epoch, self.warmup_epochs, self.max_epochs
        if e < w:
            return self.warmup_start_lr + e * (base_lr - self.warmup_start_lr) / max(1, w - 1)
        span = max(1, m - w)
        return self.eta_min + 0.5 * (base_lr - self.eta_min) * (1 + math.cos(math.pi * (e - w)
                                                                               / span))

    def _get_closed_form_lr(self):
        return [self._closed_form(b) for b in self.base_lrs]

    def get_lr(self):
        if not getattr(self, "_get_lr_called_within_step", True):
            warnings.warn("To get the last learning rate computed by the scheduler, please use "
                          "`get_last_lr()`.", UserWarning)
        e, w, m, s, eta = (self.last_epoch, self.warmup_epochs, self.max_epochs,
                           self.warmup_start_lr, self.eta_min)
        span = max(1, m - w)
        groups = self.optimizer.param_groups
        if e == 0:
            return [s] * len(self.base_lrs)
        if e < w:
            return [g["lr"] + (b - s) / max(1, w - 1) for b, g in zip(self.base_lrs, groups)]
        if e == w:
            return list(self.base_lrs)
        if (e - 1 - m) % (2 * span) == 0:
            return [g["lr"] + (b - eta) * (1 - math.cos(math.pi / span)) / 2
                    for b, g in zip(self.base_lrs, groups)]
        return [(1 + math.cos(math.pi * (e - w) / span)) / (1 + math.cos(math.pi * (e - w - 1) / span))
                * (g["lr"] - eta) + eta for g in groups]

