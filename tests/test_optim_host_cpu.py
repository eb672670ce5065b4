"""-m "not gpu": the host side of dp.ArenaAdam's new options - AdamW's flag in the torch.optim state-dict wire format, the
capturable tensor learning rate, argument validation - and the C ABI surface of csrc/optim.hip."""
import pytest
import torch


def _model():
    from vision_mtl_amd.models.mtan_model import MTANMiniUnet

    torch.manual_seed(1)
    return MTANMiniUnet(3, {"depth": 1, "segm": 3}, 8, 4, 2)


def _stepped(cls, model, **kw):
    opt = cls(model.parameters(), **kw)
    g = torch.Generator().manual_seed(2)
    for _ in range(2):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def test_optim_entry_points_declared_and_exported():
    from vision_mtl_amd._lib import lib

    l = lib()
    for name in ("vmtl_grad_sumsq_workspace_bytes", "vmtl_grad_sumsq", "vmtl_optim_control", "vmtl_adam_step_ex",
                 "vmtl_grad_clip_"):
        assert name in l.protos and l.raw(name) is not None
    ws = l.raw("vmtl_grad_sumsq_workspace_bytes")
    assert ws(1) == 8 and ws(1024) == 8 and ws(1025) == 16 and ws(1 << 40) == 1024 * 8
    assert [n for n in l.protos["vmtl_adam_step_ex"][2]][-1] == "stream"


def test_adamw_state_dict_round_trips_with_torch():
    from vision_mtl_amd import dp

    model = _model()
    sd = _stepped(torch.optim.AdamW, model, lr=5e-4, weight_decay=0.05).state_dict()
    assert sd["param_groups"][0]["decoupled_weight_decay"] is True
    arena = dp.FlatArena(model)
    opt = dp.ArenaAdamW(arena, lr=123.0)
    assert opt.param_groups[0]["decoupled_weight_decay"] is True and opt.param_groups[0]["weight_decay"] == 1e-2
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g["lr"] == 5e-4 and g["weight_decay"] == 0.05 and g["decoupled_weight_decay"] is True
    assert float(arena._adam["step"]) == 2.0
    out = opt.state_dict()
    assert out["param_groups"][0]["decoupled_weight_decay"] is True
    assert "max_grad_norm" not in out["param_groups"][0] and "skip_nonfinite" not in out["param_groups"][0]
    again = torch.optim.AdamW(model.parameters(), lr=1.0)
    again.load_state_dict(out)
    assert again.param_groups[0]["decoupled_weight_decay"] is True and again.param_groups[0]["weight_decay"] == 0.05
    assert torch.equal(again.state[arena.params[5]]["exp_avg_sq"], sd["state"][5]["exp_avg_sq"])
    # the flag travels with the checkpoint: an AdamW session loaded into a default ArenaAdam decays the AdamW way,
    # and torch.optim.Adam accepts what that optimizer writes
    plain = dp.ArenaAdam(arena, lr=1.0)
    assert plain.param_groups[0]["decoupled_weight_decay"] is False
    plain.load_state_dict(sd)
    assert plain.param_groups[0]["decoupled_weight_decay"] is True
    torch.optim.Adam(model.parameters(), lr=1.0).load_state_dict(plain.state_dict())


def test_adam_state_dict_still_loads_into_default_arena_adam():
    from vision_mtl_amd import dp

    model = _model()
    sd = _stepped(torch.optim.Adam, model, lr=5e-4).state_dict()
    arena = dp.FlatArena(model)
    opt = dp.ArenaAdam(arena, lr=123.0)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g["lr"] == 5e-4 and g["decoupled_weight_decay"] is False and float(arena._adam["step"]) == 2.0
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and opt.capturable is False
    assert opt.grad_norm is None and opt.skipped_steps is None  # the default path has no control block
    flat_m = torch.cat([sd["state"][i]["exp_avg"].reshape(-1) for i in range(len(arena.params))])
    assert torch.equal(arena._adam["m"], flat_m)


def test_capturable_lr_is_a_tensor_inside_and_a_float_outside():
    from vision_mtl_amd import dp

    model = _model()
    arena = dp.FlatArena(model)
    opt = dp.ArenaAdam(arena, lr=5e-4, capturable=True)
    lr_t = opt.param_groups[0]["lr"]
    assert isinstance(lr_t, torch.Tensor) and lr_t.dim() == 0 and lr_t.dtype == torch.float32
    assert arena._adam is not None and arena._optim is not None  # allocated at construction, not inside a capture
    out = opt.state_dict()
    assert isinstance(out["param_groups"][0]["lr"], float) and out["param_groups"][0]["lr"] == pytest.approx(5e-4)
    # torch's scheduler lowers a tensor lr in place: the address a captured launch reads stays valid
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=0, factor=0.5)
    sched.step(1.0)
    sched.step(2.0)
    assert opt.param_groups[0]["lr"] is lr_t and float(lr_t) == pytest.approx(2.5e-4)
    # and so does a checkpoint restore
    sd = _stepped(torch.optim.Adam, _model(), lr=7e-4).state_dict()
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] is lr_t and float(lr_t) == pytest.approx(7e-4)


def test_argument_validation():
    from vision_mtl_amd import dp

    arena = dp.FlatArena(_model())
    with pytest.raises(ValueError, match="max_grad_norm"):
        dp.ArenaAdam(arena, lr=1e-3, max_grad_norm=-1.0)
    with pytest.raises(ValueError, match="capturable"):
        dp.ArenaAdam(arena, lr=torch.tensor(1e-3))
    with pytest.raises(ValueError):
        arena.clip_grad_norm_(-1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        arena.grad_norm()  # a CPU arena: the kernels refuse, nothing falls back to torch
    dp.ArenaAdam(arena, lr=torch.tensor(1e-3), capturable=True)
    dp.ArenaAdamW(arena, max_grad_norm=0.0, skip_nonfinite=True)
