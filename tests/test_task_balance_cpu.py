"""-m "not gpu": the host side of the task-loss balancing - header prototypes and exported symbols of the new entry
points (the pattern of tests/test_loss_ignore_cpu.py), their argument checks (made before a device is touched), the
unchanged default MTLModule, the argument errors of TaskBalancer / MTLModule, and FlatArena(extra_params=)."""
import argparse

import pytest
import torch

NEW_ENTRY_POINTS = {
    "vmtl_task_balance_state_bytes": ["T"],
    "vmtl_task_balance_fwd": ["l0", "l1", "l2", "l3", "T", "mode", "param", "state", "accumulate", "total", "weights",
                              "stream"],
    "vmtl_task_balance_bwd": ["grad_out", "weights", "l0", "l1", "l2", "l3", "param", "mode", "T", "g0", "g1", "g2", "g3",
                              "dparam", "stream"],
    "vmtl_dwa_epoch_update": ["state", "param", "T", "temperature", "stream"],
}
X = 0x1000  # a non-null, 8-byte aligned "pointer": the argument checks return before anything dereferences it


def test_new_entry_points_are_declared_and_exported():
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import HEADER, lib, parse_header

    protos = parse_header(HEADER)
    l = lib()
    for name, args in NEW_ENTRY_POINTS.items():
        assert name in protos, f"{name} is not declared in vmtl.h"
        assert protos[name][2] == args
        assert hasattr(l._dll, name), f"{name} declared in vmtl.h but not exported"
    text = HEADER.read_text()
    for k, v in ops.BALANCE_MODES.items():
        assert f"#define VMTL_BALANCE_{k.upper()} {v}" in text
    assert "lit_module.py:120-131" in text
    f = l.raw("vmtl_task_balance_state_bytes")  # host only: 3 T + 2 doubles
    assert [f(T) for T in (0, 1, 2, 3, 4, 5)] == [0, 40, 64, 88, 112, 0]
    assert ops.balance_state_doubles(2) == 8
    with pytest.raises(ValueError):
        ops.balance_state_doubles(5)


def test_entry_points_check_their_arguments_before_touching_a_device():
    from vision_mtl_amd._lib import lib

    l = lib()
    fwd, bwd, upd = l.raw("vmtl_task_balance_fwd"), l.raw("vmtl_task_balance_bwd"), l.raw("vmtl_dwa_epoch_update")
    # null pointers
    assert fwd(None, None, None, None, 2, 0, None, None, 0, None, None, None) == -1
    assert fwd(X, None, None, None, 2, 0, X, None, 0, X, X, None) == -1       # the second of T = 2 losses
    assert fwd(X, X, None, None, 2, 0, None, None, 0, X, X, None) == -1       # the log-variances
    assert fwd(X, X, None, None, 2, 1, None, None, 0, X, X, None) == -1       # the DWA weights
    assert fwd(X, X, None, None, 2, 1, X, None, 1, X, X, None) == -1          # accumulate without state
    assert fwd(X, X, None, None, 2, 1, X, X + 4, 1, X, X, None) == -1         # state not 8-byte aligned
    assert fwd(X, X, None, None, 2, 2, None, None, 0, None, X, None) == -1    # total
    assert fwd(X, X, None, None, 2, 2, None, None, 0, X, None, None) == -1    # weights
    assert bwd(None, None, None, None, None, None, None, 0, 2, None, None, None, None, None, None) == -1
    assert bwd(None, X, X, X, None, None, X, 0, 2, X, X, None, None, X, None) == -1   # grad_out
    assert bwd(X, None, X, X, None, None, X, 0, 2, X, X, None, None, X, None) == -1   # weights
    assert bwd(X, X, X, None, None, None, X, 0, 2, X, X, None, None, X, None) == -1   # a loss
    assert bwd(X, X, X, X, None, None, None, 0, 2, X, X, None, None, X, None) == -1   # the log-variances
    assert bwd(X, X, X, X, None, None, X, 0, 2, None, None, None, None, None, None) == -1  # nothing to write
    assert upd(None, None, 2, 2.0, None) == -1
    assert upd(X, None, 2, 2.0, None) == -1
    assert upd(None, X, 2, 2.0, None) == -1
    assert upd(X + 4, X, 2, 2.0, None) == -1
    # T outside 1..4, an unknown mode, a temperature that is not positive
    for T in (0, 5, -1):
        assert fwd(X, X, X, X, T, 0, X, X, 0, X, X, None) == -1
        assert bwd(X, X, X, X, X, X, X, 0, T, X, X, X, X, X, None) == -1
        assert upd(X, X, T, 2.0, None) == -1
    for mode in (-1, 3):
        assert fwd(X, X, X, X, 2, mode, X, X, 0, X, X, None) == -1
        assert bwd(X, X, X, X, X, X, X, mode, 2, X, X, X, X, X, None) == -1
    for tau in (0.0, -1.0, float("nan")):
        assert upd(X, X, 2, tau, None) == -1


def _mtan(**kw):
    from vision_mtl_amd.utils.pipeline_utils import init_model

    return init_model(argparse.Namespace(model_name="mtan", **kw), argparse.Namespace(num_classes=5))


def test_default_module_is_unchanged():
    plain = _mtan()
    assert not hasattr(plain, "task_balancer")
    assert "loss_balancing" not in plain.hparams
    assert list(plain.state_dict()) == ["model." + k for k in plain.model.state_dict()]
    assert [id(p) for p in plain.parameters()] == [id(p) for p in plain.model.parameters()]


def test_module_with_a_balancer():
    from vision_mtl_amd.balancing import TaskBalancer
    from vision_mtl_amd.lit_module import MTLModule

    plain = _mtan()
    keys = list(plain.state_dict())
    unc = _mtan(loss_balancing="uncertainty")
    assert isinstance(unc.task_balancer, TaskBalancer) and unc.task_balancer.method == "uncertainty"
    assert list(unc.state_dict()) == keys + ["task_balancer.log_vars"]
    ps = list(unc.parameters())
    assert [id(p) for p in ps[:-1]] == [id(p) for p in unc.model.parameters()] and ps[-1] is unc.task_balancer.log_vars
    assert unc.task_balancer.log_vars.tolist() == [0.0, 0.0]
    dwa = _mtan(loss_balancing="dwa", dwa_temperature=0.5)
    assert dwa.task_balancer.temperature == 0.5 and dwa.hparams["loss_balancing"] == "dwa"
    assert list(dwa.state_dict()) == keys + ["task_balancer.dwa_weights", "task_balancer.dwa_state"]
    assert dwa.task_balancer.dwa_state.dtype == torch.float64 and dwa.task_balancer.dwa_state.numel() == 8
    assert len(list(dwa.parameters())) == len(list(plain.parameters()))
    geo = _mtan(loss_balancing="geometric")
    assert list(geo.state_dict()) == keys and len(list(geo.parameters())) == len(list(plain.parameters()))
    own = TaskBalancer("uncertainty", init_log_vars=(0.5, -0.5))
    m = MTLModule(torch.nn.Linear(1, 1), num_classes=5, loss_balancing=own)
    assert m.task_balancer is own and own.log_vars.tolist() == [0.5, -0.5]
    unc.load_state_dict(unc.state_dict())  # strict
    with pytest.raises(RuntimeError):  # a checkpoint of another scheme is not silently accepted
        plain.load_state_dict(unc.state_dict())


def test_argument_errors():
    from vision_mtl_amd.balancing import TaskBalancer
    from vision_mtl_amd.lit_module import MTLModule

    with pytest.raises(ValueError, match="method"):
        TaskBalancer("gradnorm")
    for tau in (0.0, -2.0):
        with pytest.raises(ValueError, match="temperature"):
            TaskBalancer("dwa", temperature=tau)
    with pytest.raises(ValueError, match="init_log_vars"):
        TaskBalancer("uncertainty", init_log_vars=(0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match="init_log_vars"):
        TaskBalancer("dwa", init_log_vars=(0.1, 0.2))
    with pytest.raises(ValueError, match="tasks"):
        TaskBalancer("geometric", tasks=("a", "b", "c", "d", "e"))
    one = torch.ones(())
    for method in ("uncertainty", "dwa", "geometric"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            TaskBalancer(method)([one, one])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TaskBalancer("dwa").on_train_epoch_end()
    with pytest.raises(ValueError, match="expected 2 losses"):
        TaskBalancer("geometric")([one])
    lin = torch.nn.Linear(1, 1)
    for kw in (dict(loss_segm_weight=0.5), dict(loss_depth_weight=2.0)):
        with pytest.raises(ValueError, match="static loss weights"):
            MTLModule(lin, num_classes=5, loss_balancing="uncertainty", **kw)
    with pytest.raises(ValueError, match="method"):
        MTLModule(lin, num_classes=5, loss_balancing="pcgrad")
    with pytest.raises(ValueError, match="loss_balancing"):
        MTLModule(lin, num_classes=5, loss_balancing=3)
    with pytest.raises(ValueError, match="tasks"):
        MTLModule(lin, num_classes=5, loss_balancing=TaskBalancer("geometric", tasks=("depth", "segm")))
    with pytest.raises(ValueError, match="temperature"):
        MTLModule(lin, num_classes=5, loss_balancing="dwa", dwa_temperature=0.0)


def _small():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))


def test_flat_arena_extra_params_keep_the_model_offsets():
    from vision_mtl_amd import dp

    base = dp.FlatArena(_small())
    model, p = _small(), torch.nn.Parameter(torch.tensor([0.8, -0.2]))
    arena = dp.FlatArena(model, extra_params=[p])
    assert arena.offsets[:-1] == base.offsets and arena.offsets[-1] == base.numel
    assert arena.numel == base.numel + 2 and arena.params[-1] is p
    assert torch.equal(arena.flat_param[:base.numel], base.flat_param)
    assert arena.flat_param[-2:].tolist() == pytest.approx([0.8, -0.2])
    assert p.data_ptr() == arena.flat_param.data_ptr() + 4 * base.numel  # re-homed: the fused update reaches it
    assert p.grad.data_ptr() == arena.flat_grad.data_ptr() + 4 * base.numel and p._vmtl_arena is arena
    assert dp.FlatArena(_small(), extra_params=None).numel == dp.FlatArena(_small(), extra_params=[]).numel == base.numel
    with pytest.raises(ValueError, match="extra_params"):
        dp.FlatArena(_small(), extra_params=[torch.zeros(2)])
    with pytest.raises(ValueError, match="already"):
        m = _small()
        dp.FlatArena(m, extra_params=[next(m.parameters())])


def test_arena_adam_state_dict_covers_the_extra_parameter():
    from vision_mtl_amd import dp

    model, p = _small(), torch.nn.Parameter(torch.zeros(2))
    n = len(list(model.parameters()))
    arena = dp.FlatArena(model, extra_params=[p])
    sd = dp.ArenaAdam(arena, lr=1e-3).state_dict()
    ref = torch.optim.Adam(list(model.parameters()) + [p], lr=1e-3).state_dict()
    assert sd["param_groups"][0]["params"] == ref["param_groups"][0]["params"] == list(range(n + 1))
