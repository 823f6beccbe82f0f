"""CPU: the host side of the SGD and device-rate optimizer entries: the header's declarations,
the argument checks that run before any launch, and the constructors' refusals."""
import ctypes

import pytest
import torch

from lesion_gnn_amd import _lib, optim


def test_entries_are_declared_exported_and_typed():
    lib = _lib.load()
    P, I32, F32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["lgnn_adam_step_dlr"] == (
        I32, [I32, P, P, P, P, P, P, P, P, F32, F32, F32, F32, I32, I32, I32, P])
    assert _lib.SIGNATURES["lgnn_sgd_step"] == (
        I32, [I32, P, P, P, P, P, P, F32, P, F32, F32, F32, I32, I32, I32, P])
    for name in ("lgnn_adam_step_dlr", "lgnn_sgd_step"):
        assert hasattr(lib, name), name
    # lgnn_adam_step with `const float* lr` in place of `float lr`, nothing else
    a, d = _lib.PARAMS["lgnn_adam_step"], _lib.PARAMS["lgnn_adam_step_dlr"]
    assert a[8] == ("float", "lr") and d[8] == ("const float*", "lr")
    assert a[:8] + a[9:] == d[:8] + d[9:]
    assert [n for _, n in _lib.PARAMS["lgnn_sgd_step"]] == [
        "n", "params", "grads", "momentum_buf", "numels", "step", "ticket", "lr", "lr_dev",
        "momentum", "dampening", "weight_decay", "nesterov", "maximize", "advance", "stream"]


def test_entries_validate_before_launching():
    lib, E = _lib.load(), _lib.LGNN_EINVAL
    # Adam on a device rate: a null lr, and lgnn_adam_step's own checks
    assert lib.lgnn_adam_step_dlr(0, None, None, None, None, None, 1, 1, None, 0.9, 0.999, 1e-8,
                                  0.0, 0, 0, 1, None) == E
    assert lib.lgnn_adam_step_dlr(0, None, None, None, None, None, None, 1, 1, 0.9, 0.999, 1e-8,
                                  0.0, 0, 0, 1, None) == E
    assert lib.lgnn_adam_step_dlr(optim.MAX_TENSORS + 1, 1, 1, 1, 1, 1, 1, 1, 1, 0.9, 0.999, 1e-8,
                                  0.0, 0, 0, 1, None) == E
    # SGD: momentum needs the buffers, the step and the ticket; nesterov as torch
    sgd = lib.lgnn_sgd_step
    assert sgd(1, 1, 1, None, 1, 1, 1, 0.1, None, 0.9, 0.0, 0.0, 0, 0, 1, None) == E
    assert sgd(0, None, None, None, None, None, 1, 0.1, None, 0.9, 0.0, 0.0, 0, 0, 1, None) == E
    assert sgd(0, None, None, None, None, 1, None, 0.1, None, 0.9, 0.0, 0.0, 0, 0, 1, None) == E
    assert sgd(0, None, None, None, None, 1, 1, 0.1, None, 0.0, 0.0, 0.0, 1, 0, 1, None) == E
    assert sgd(0, None, None, None, None, 1, 1, 0.1, None, 0.9, 0.3, 0.0, 1, 0, 1, None) == E
    assert sgd(optim.MAX_TENSORS + 1, 1, 1, 1, 1, 1, 1, 0.1, None, 0.9, 0.0, 0.0, 0, 0, 1,
               None) == E
    assert sgd(1, 1, 1, None, None, None, None, 0.1, None, 0.0, 0.0, 0.0, 0, 0, 0, None) == E


def test_sgd_constructor_checks_as_torch():
    w = [torch.nn.Parameter(torch.zeros(2))]
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1.0),
               dict(lr=0.1, nesterov=True), dict(lr=0.1, momentum=0.9, dampening=0.1,
                                                 nesterov=True)):
        with pytest.raises(ValueError):
            torch.optim.SGD(w, **kw)
        with pytest.raises(ValueError):
            optim.SGD(w, **kw)
    o = optim.SGD(w, lr=0.1, momentum=0.9, nesterov=True)
    g = o.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["nesterov"]) == (0.1, 0.9, 0.0, True)
    assert not o.state  # nothing is allocated before the first step


@pytest.mark.parametrize("cls", [optim.Adam, optim.AdamW, optim.SGD])
def test_capturable_needs_parameters_on_the_gpu(cls):
    w = [torch.nn.Parameter(torch.zeros(2))]
    with pytest.raises(ValueError, match="GPU"):
        cls(w, lr=1e-3, capturable=True)
    with pytest.raises(ValueError, match="capturable"):
        cls(w, lr=torch.tensor(1e-3))  # a tensor rate is the capturable path's
    assert isinstance(cls(w, lr=1e-3).param_groups[0]["lr"], float)  # the default: as before


def test_configure_optimizers_builds_the_package_sgd():
    from lesion_gnn_amd.models import GCNConfig, OptimizerConfig, get_model
    from lesion_gnn_amd.models.base import OptimizerAlgo

    cfg = GCNConfig(optimizer=OptimizerConfig(algo=OptimizerAlgo.SGD, loss_type="MSE"),
                    hidden_channels=[16, 16], dropout=0.0, compile=False)
    cfg.num_classes.value, cfg.input_features.value = 5, 8
    module = get_model(cfg)
    opt = module.configure_optimizers()
    assert type(opt) is optim.SGD
    assert opt.param_groups[0]["lr"] == 0.001 and opt.param_groups[0]["weight_decay"] == 0.01
    with pytest.raises(ValueError, match="GPU"):  # the keyword reaches the constructor
        module.configure_optimizers(capturable=True)
