"""-m "not gpu": the host side of the averaged weights - the C ABI surface of csrc/weight_avg.hip and its argument checks
(no device is touched), tests/weight_avg_oracle.py against torch.optim.swa_utils.AveragedModel, dp.ArenaAverage over a CPU
FlatArena (validation, the AveragedModel checkpoint wire format) and the launches of an ArenaAdam without an average."""
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from tests import weight_avg_oracle as O

ERR_ARG = -1
LAUNCHING = ("vmtl_wavg_control", "vmtl_wavg_update", "vmtl_adam_step_wavg", "vmtl_wavg_buffers", "vmtl_swap_table_",
             "vmtl_swap_")


def _model():
    from vision_mtl_amd.models.mtan_model import MTANMiniUnet

    torch.manual_seed(1)
    return MTANMiniUnet(3, {"depth": 1, "segm": 3}, 8, 4, 2)


def _L():
    from vision_mtl_amd._lib import lib

    return lib()


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_declared_and_exported():
    L = _L()
    for name in LAUNCHING:
        assert name in L.protos and L.raw(name) is not None
        assert L.protos[name][2][-1] == "stream", name
    assert "vmtl_wavg_desc_bytes" in L.protos and L.raw("vmtl_wavg_desc_bytes")() == 24
    from vision_mtl_amd import ops

    for fn in ("wavg_state", "wavg_control", "wavg_update", "adam_step_wavg", "wavg_buffers", "swap_"):
        assert callable(getattr(ops, fn))


# fake, never dereferenced addresses: every call below must return before it touches a device
P, G, M, V, E, CTL, ST, D = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000


def test_control_argument_errors():
    f = _L().raw("vmtl_wavg_control")
    assert f(None, None, 0, 0.9, 0.0, 0, None) == ERR_ARG          # null state
    assert f(ST + 4, None, 0, 0.9, 0.0, 0, None) == ERR_ARG        # the 64-bit counter needs 8-byte alignment
    assert f(ST, CTL + 2, 0, 0.9, 0.0, 0, None) == ERR_ARG         # misaligned control block
    for mode in (-1, 2, 7):
        assert f(ST, None, mode, 0.9, 0.0, 0, None) == ERR_ARG     # bad mode
    for decay in (-0.5, 1.5, float("nan")):
        assert f(ST, None, 0, decay, 0.0, 0, None) == ERR_ARG      # an EMA decay outside [0, 1]


def test_update_argument_errors():
    f = _L().raw("vmtl_wavg_update")
    assert f(None, P, ST, 8, None) == ERR_ARG
    assert f(E, None, ST, 8, None) == ERR_ARG
    assert f(E, P, None, 8, None) == ERR_ARG
    assert f(E, P, ST, 0, None) == ERR_ARG
    assert f(E, P, ST, -3, None) == ERR_ARG
    assert f(E + 2, P, ST, 8, None) == ERR_ARG
    assert f(E, P + 1, ST, 8, None) == ERR_ARG
    assert f(E, P, ST + 4, 8, None) == ERR_ARG


def test_fused_step_argument_errors():
    f = _L().raw("vmtl_adam_step_wavg")
    good = [P, G, M, V, E, CTL, ST]
    tail = (1e-3, None, 1e-8, 0.0, 0, 1.0)
    for i in range(len(good)):
        args = list(good)
        args[i] = None
        assert f(*args, *tail, 8, None) == ERR_ARG, f"null pointer {i}"
    for i in range(5):
        args = list(good)
        args[i] += 2
        assert f(*args, *tail, 8, None) == ERR_ARG, f"misaligned pointer {i}"
    args = list(good)
    args[6] += 4
    assert f(*args, *tail, 8, None) == ERR_ARG
    assert f(*good, *tail, 0, None) == ERR_ARG
    assert f(*good, *tail, -1, None) == ERR_ARG


def test_table_argument_errors():
    L = _L()
    f, s = L.raw("vmtl_wavg_buffers"), L.raw("vmtl_swap_table_")
    assert f(None, 1, 8, ST, None) == ERR_ARG and s(None, 1, 8, None) == ERR_ARG
    assert f(D, 0, 8, ST, None) == ERR_ARG and s(D, 0, 8, None) == ERR_ARG
    assert f(D, 65536, 8, ST, None) == ERR_ARG and s(D, 65536, 8, None) == ERR_ARG
    assert f(D, 1, 0, ST, None) == ERR_ARG and s(D, 1, 0, None) == ERR_ARG
    assert f(D + 4, 1, 8, ST, None) == ERR_ARG and s(D + 4, 1, 8, None) == ERR_ARG
    assert f(D, 1, 8, None, None) == ERR_ARG
    assert f(D, 1, 8, ST + 4, None) == ERR_ARG


def test_swap_argument_errors():
    f = _L().raw("vmtl_swap_")
    assert f(None, P, 8, None) == ERR_ARG and f(P, None, 8, None) == ERR_ARG
    assert f(P, G, 0, None) == ERR_ARG and f(P, G, -1, None) == ERR_ARG
    assert f(P + 1, G, 8, None) == ERR_ARG and f(P, G + 2, 8, None) == ERR_ARG
    assert f(P, P, 8, None) == ERR_ARG              # the same buffer
    assert f(P, P + 16, 8, None) == ERR_ARG         # b starts inside a
    assert f(P + 28, P, 8, None) == ERR_ARG         # a starts inside b (one element shared)


# ----------------------------------------------------------------------------- the oracle against torch
def test_oracle_weights():
    assert O.weight(0, "ema", 0.9) == (1.0, True) and O.weight(0, "swa") == (1.0, True)
    assert O.weight(3, "swa") == (0.25, False)
    assert O.weight(5, "ema", 0.75) == (0.25, False)
    assert O.weight(1, "ema", 0.999, warmup=True)[0] == pytest.approx(1 - 2 / 11)      # timm: (1 + n) / (10 + n)
    assert O.weight(10 ** 6, "ema", 0.999, warmup=True)[0] == pytest.approx(1 - 0.999)  # the cap
    o = O.AverageOracle(torch.zeros(2), "ema", 0.5)
    o.update(torch.tensor([2.0, 4.0]))                       # copy
    o.update(torch.tensor([9.0, 9.0]), skipped=True)         # nothing
    assert o.n == 1 and torch.equal(o.e, torch.tensor([2.0, 4.0], dtype=torch.float64))
    o.update(torch.tensor([4.0, 0.0]))
    assert o.n == 2 and torch.equal(o.e, torch.tensor([3.0, 2.0], dtype=torch.float64))


@pytest.mark.parametrize("mode", ["ema", "swa"])
def test_oracle_matches_torch_averaged_model(mode):
    """four updates of a small CPU model; torch computes in fp32, so the oracle's accumulated fp32 allowance applies"""
    decay = 0.9
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay)) if mode == "ema" else AveragedModel(model)
    flat = lambda m: torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    o = O.AverageOracle(flat(model), mode, decay, warmup=False)
    g = torch.Generator().manual_seed(4)
    for k in range(4):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.3)
        avg.update_parameters(model)
        o.update(flat(model))
        assert int(avg.n_averaged) == o.n == k + 1
        if k == 0:
            assert torch.equal(flat(avg.module).double(), o.e), "the first update is a copy"
        O.assert_within(flat(avg.module), o, what=f"{mode} update {k} against AveragedModel")
    assert float(o.bound.max()) > 0.0


# ----------------------------------------------------------------------------- dp.ArenaAverage on the CPU
def test_argument_validation():
    from vision_mtl_amd import dp

    model = _model()
    arena = dp.FlatArena(model)
    with pytest.raises(ValueError, match="FlatArena"):
        dp.ArenaAverage(model)
    with pytest.raises(ValueError, match="mode"):
        dp.ArenaAverage(arena, mode="mean")
    for decay in (-0.1, 1.5, float("nan"), "0.9", True):
        with pytest.raises(ValueError, match="decay"):
            dp.ArenaAverage(arena, decay=decay)
    with pytest.raises(ValueError, match="warmup"):
        dp.ArenaAverage(arena, mode="swa", warmup=True)
    avg = dp.ArenaAverage(arena)
    assert (avg.decay, avg.mode, avg.warmup, avg.use_buffers) == (0.999, "ema", False, False)
    assert torch.equal(avg.flat_avg, arena.flat_param) and avg.flat_avg.data_ptr() != arena.flat_param.data_ptr()
    n = avg.n_averaged
    assert n.dim() == 0 and n.dtype == torch.int64 and int(n) == 0
    other = dp.FlatArena(_model())
    with pytest.raises(ValueError, match="same arena"):
        dp.ArenaAdam(other, average=avg)
    with pytest.raises(ValueError, match="same arena"):
        avg.update(dp.ArenaAdam(other))
    opt = dp.ArenaAdam(arena, average=avg)
    assert opt.average is avg and "average" not in opt.state_dict()["param_groups"][0]
    with pytest.raises(ValueError, match="twice"):
        avg.update(opt)


def test_update_and_swap_have_no_cpu_fallback():
    from vision_mtl_amd import dp

    arena = dp.FlatArena(_model())
    for use_buffers in (False, True):
        avg = dp.ArenaAverage(arena, use_buffers=use_buffers)
        before = avg.flat_avg.clone()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            avg.update()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            avg.swap()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            with avg.applied():
                pass
        assert arena._applied_average is None and torch.equal(avg.flat_avg, before) and int(avg.n_averaged) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dp.ArenaAdam(arena, average=avg).step()


def _torch_averaged(model, use_buffers, updates=3):
    t = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.9), use_buffers=use_buffers)
    g = torch.Generator().manual_seed(5)
    for _ in range(updates):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
            for b in model.buffers():
                if b.is_floating_point():
                    b.add_(torch.rand(b.shape, generator=g) * 0.1)
        t.update_parameters(model)
    return t


@pytest.mark.parametrize("use_buffers", [False, True])
def test_state_dict_round_trips_with_torch(use_buffers):
    from vision_mtl_amd import dp

    model = _model()
    t = _torch_averaged(model, use_buffers)
    sd = t.state_dict()
    arena = dp.FlatArena(model)
    avg = dp.ArenaAverage(arena, decay=0.9, use_buffers=use_buffers)
    avg.load_state_dict(sd)
    assert int(avg.n_averaged) == 3
    out = avg.state_dict()
    assert list(out.keys()) == list(sd.keys())
    for k in sd:
        assert out[k].shape == sd[k].shape and out[k].dtype == sd[k].dtype, k
        if use_buffers and k.endswith("num_batches_tracked"):
            continue  # torch averages this integer; here it stays the live model's (documented)
        assert torch.equal(out[k], sd[k]), k
    # the average really differs from the live parameters, and lives in the flat buffer in arena order
    assert not torch.equal(avg.flat_avg, arena.flat_param)
    flat = torch.cat([sd["module." + k].reshape(-1) for k, p in model.named_parameters() if p.requires_grad])
    assert torch.equal(avg.flat_avg, flat)
    # and back: torch loads what this object writes (strict), values bit-equal
    back = AveragedModel(model, use_buffers=use_buffers)
    back.load_state_dict(out)
    for k, v in back.state_dict().items():
        assert torch.equal(v, out[k]), k
    # averaged_state_dict: exactly module.state_dict()'s keys, the averaged values
    from vision_mtl_amd.lit_module import MTLModule

    module = MTLModule(model, num_classes=3, device="cpu")
    asd = avg.averaged_state_dict(module)
    msd = module.state_dict()
    assert list(asd.keys()) == list(msd.keys())
    for k in msd:
        assert asd[k].shape == msd[k].shape and asd[k].data_ptr() != msd[k].data_ptr()
        if k.endswith("num_batches_tracked"):
            assert torch.equal(asd[k], msd[k])
        else:
            assert torch.equal(asd[k], sd["module." + k[len("model."):]]), k
    assert list(avg.averaged_state_dict(model).keys()) == list(model.state_dict().keys())


def test_mismatched_checkpoints_raise():
    from vision_mtl_amd import dp

    model = _model()
    arena = dp.FlatArena(model)
    avg = dp.ArenaAverage(arena)
    good = avg.state_dict()
    before = avg.flat_avg.clone()
    key = next(k for k in good if k.startswith("module.") and good[k].dim() == 4)
    for bad in (
        {k: v for k, v in good.items() if k != key},                       # a missing parameter
        {**good, "module.not_there": torch.zeros(1)},                      # an unknown key
        {k: v for k, v in good.items() if k != "n_averaged"},              # no counter
        {**good, key: good[key][:, :, :1]},                                # a wrong shape
        {**good, "n_averaged": torch.tensor(1.5)},                         # not an integer
        model.state_dict(),                                                # a plain model checkpoint
        None,
    ):
        with pytest.raises(ValueError):
            avg.load_state_dict(bad)
    assert torch.equal(avg.flat_avg, before) and int(avg.n_averaged) == 0, "a refused checkpoint writes nothing"
    avg.load_state_dict({**good, "n_averaged": torch.tensor(7)})
    assert int(avg.n_averaged) == 7


def test_extra_params_travel_under_documented_keys():
    from vision_mtl_amd import dp
    from vision_mtl_amd.lit_module import MTLModule

    model = _model()
    module = MTLModule(model, num_classes=3, device="cpu", loss_balancing="uncertainty")
    extras = list(module.task_balancer.parameters())
    arena = dp.FlatArena(model, extra_params=extras)
    avg = dp.ArenaAverage(arena)
    avg.flat_avg.add_(1.0)
    sd = avg.state_dict()
    keys = [k for k in sd if k.startswith(dp.ArenaAverage.EXTRA_KEY)]
    assert keys == [f"arena_extra.{i}" for i in range(len(extras))] and len(keys) >= 1
    assert torch.equal(sd[keys[0]], extras[0].detach() + 1.0)
    # without the extra keys the rest is torch's format; with them missing this object refuses
    AveragedModel(model).load_state_dict({k: v for k, v in sd.items() if k not in keys})
    with pytest.raises(ValueError, match="arena_extra"):
        avg.load_state_dict({k: v for k, v in sd.items() if k not in keys})
    avg.load_state_dict(sd)
    asd = avg.averaged_state_dict(module)
    assert list(asd.keys()) == list(module.state_dict().keys())
    bal = [k for k in asd if k.startswith("task_balancer.")]
    assert bal and all(torch.equal(asd[k], module.state_dict()[k] + 1.0) for k in bal)


# ----------------------------------------------------------------------------- the launches of the optimizer
ADAM = ("vmtl_adam_step", sorted(["p", "g", "m", "v", "step_ptr", "lr", "b1", "b2", "eps", "weight_decay", "grad_scale", "n"]))
SUMSQ = ("vmtl_grad_sumsq", sorted(["g", "grad_scale", "workspace", "n"]))
CONTROL = ("vmtl_optim_control", sorted(["workspace", "n", "max_norm", "skip_nonfinite", "step_ptr", "b1", "b1_lo", "b2",
                                         "b2_lo", "ctl"]))
ADAM_EX = ("vmtl_adam_step_ex", sorted(["p", "g", "m", "v", "ctl", "lr", "lr_ptr", "eps", "weight_decay", "decoupled",
                                        "grad_scale", "n"]))
WAVG_CONTROL = ("vmtl_wavg_control", sorted(["state", "ctl", "mode", "decay", "decay_lo", "warmup"]))
ADAM_WAVG = ("vmtl_adam_step_wavg", sorted(ADAM_EX[1] + ["e", "state"]))
WAVG_BUFFERS = ("vmtl_wavg_buffers", sorted(["descs", "n", "max_n", "state"]))


def _recorded(monkeypatch):
    from vision_mtl_amd import ops

    calls = []
    monkeypatch.setattr(ops, "_k", lambda name, _flop=None, _xflop=None, **kw: calls.append((name, sorted(kw))))
    monkeypatch.setattr(ops, "_flat", lambda t, name: t)  # CPU tensors: nothing is launched, the calls are recorded
    return calls


def test_optimizer_without_average_issues_the_launches_it_always_issued(monkeypatch):
    from vision_mtl_amd import dp

    calls = _recorded(monkeypatch)
    arena = dp.FlatArena(_model())
    dp.ArenaAdam(arena, lr=1e-3).step()
    assert calls == [ADAM], "the default path is the parent's fast path: one launch"
    del calls[:]
    dp.ArenaAdam(arena, lr=1e-3, max_grad_norm=1.0).step()
    assert calls == [SUMSQ, CONTROL, ADAM_EX]
    del calls[:]
    dp.ArenaAdamW(arena, lr=1e-3).step()
    assert calls == [CONTROL, ADAM_EX]
    del calls[:]
    # an ArenaAverage that merely exists changes nothing
    avg = dp.ArenaAverage(arena)
    dp.ArenaAdam(arena, lr=1e-3).step()
    assert calls == [ADAM]
    del calls[:]
    # with it: the extended path, one control launch more, the update launch replaced
    dp.ArenaAdam(arena, lr=1e-3, average=avg).step()
    assert calls == [CONTROL, WAVG_CONTROL, ADAM_WAVG]
    del calls[:]
    dp.ArenaAdam(arena, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, average=avg).step()
    assert calls == [SUMSQ, CONTROL, WAVG_CONTROL, ADAM_WAVG]
    del calls[:]
    # the stand-alone update: control + one pass
    avg.update()
    assert calls == [WAVG_CONTROL, ("vmtl_wavg_update", ["e", "n", "p", "state"])]


def test_module_attribute_changes_no_hparams_or_keys():
    from vision_mtl_amd import dp
    from vision_mtl_amd.lit_module import MTLModule

    model = _model()
    module = MTLModule(model, num_classes=3, device="cpu")
    assert module.weight_average is None
    hp, keys = dict(module.hparams), list(module.state_dict().keys())
    module.weight_average = dp.ArenaAverage(dp.FlatArena(model))
    assert module.hparams == hp and list(module.state_dict().keys()) == keys
    assert len(list(module.parameters())) == len(list(model.parameters()))
