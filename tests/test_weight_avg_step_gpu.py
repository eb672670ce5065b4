"""dp.ArenaAverage in the training loop and under evaluation, on the tiny MTAN model of the step tests
(MTANMiniUnet(3, {"depth": 1, "segm": 3}, 8, 4, 2), batch 2x3x32x32).

Bit equality wherever two paths run the same kernels on the same values: the live parameters with and without an average,
the fused and the two-launch form, eager and captured, and the evaluation loss under `module.weight_average` against a
second module loaded from averaged_state_dict().  The average itself is held to the accumulated bound of
tests/weight_avg_oracle.py against the oracle fed the same fp32 parameter trajectory.

The three training forms share ArenaAdam's options, skip_nonfinite=True among them: ArenaAdam(average=) always takes the
extended update (csrc/optim.hip), and the comparison is bit for bit against the same kernel; the default ArenaAdam runs
the older one-launch kernel, whose rounding differs, and is compared with the two-launch form only."""
import pytest
import torch

from tests import weight_avg_oracle as O

pytestmark = pytest.mark.gpu

LR = 2e-3
DECAY = 0.9
C, B, H, W = 3, 2, 32, 32
OPT = dict(lr=LR, skip_nonfinite=True)


def _model(dev, seed=1):
    from vision_mtl_amd.models.mtan_model import MTANMiniUnet

    torch.manual_seed(seed)
    return MTANMiniUnet(3, {"depth": 1, "segm": 3}, 8, 4, 2).to(dev).train()


def _batches(n, dev, first=500):
    from vision_mtl_amd.data import synthetic_batch

    return [{k: v.to(dev) for k, v in synthetic_batch(B, H, W, C, seed=first + i, masked=0.1).items()} for i in range(n)]


def _setup(dev, seed=1):
    from vision_mtl_amd import dp
    from vision_mtl_amd.lit_module import MTLModule

    model = _model(dev, seed)
    module = MTLModule(model, num_classes=C, device=str(dev))
    return model, module, dp.FlatArena(model)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _buffers(model):
    return [b.detach().clone() for b in model.buffers()]


def _train(dev, form, steps=4, opt_kw=OPT, mode="ema", warmup=False, use_buffers=False):
    """form: "alone" | "fused" (ArenaAdam(average=)) | "update" (ArenaAdam + avg.update(opt)).  Returns the setup, the
    average and the fp32 parameter (and buffer) trajectory."""
    from vision_mtl_amd import dp

    model, module, arena = _setup(dev)
    avg = None if form == "alone" else dp.ArenaAverage(arena, decay=DECAY, mode=mode, warmup=warmup,
                                                       use_buffers=use_buffers)
    opt = dp.ArenaAdam(arena, average=avg if form == "fused" else None, **opt_kw)
    p0 = arena.flat_param.detach().cpu().clone()
    traj, btraj = [], []
    for b in _batches(steps, dev):
        arena.rebind_grads()
        module.training_step(dict(b), 0).backward()
        opt.step()
        if form == "update":
            avg.update(opt)
        traj.append(arena.flat_param.detach().cpu().clone())
        btraj.append([x.cpu() for x in _buffers(model)])
    return dict(model=model, module=module, arena=arena, avg=avg, opt=opt, p0=p0, traj=traj, btraj=btraj)


_RUNS = {}


def _run(dev, form):
    if form not in _RUNS:
        _RUNS[form] = _train(dev, form)
    return _RUNS[form]


# ----------------------------------------------------------------------------- training
def test_average_leaves_the_live_parameters_alone_and_both_forms_agree(dev):
    alone, fused, update = (_run(dev, f) for f in ("alone", "fused", "update"))
    for k in range(4):
        assert torch.equal(_bits(alone["traj"][k]), _bits(fused["traj"][k])), f"step {k}: ArenaAdam(average=) moved p"
        assert torch.equal(_bits(alone["traj"][k]), _bits(update["traj"][k])), f"step {k}: avg.update() moved p"
    assert torch.equal(_bits(fused["avg"].flat_avg), _bits(update["avg"].flat_avg)), "fused and two-launch averages differ"
    assert int(fused["avg"].n_averaged) == int(update["avg"].n_averaged) == 4
    assert float(fused["opt"].skipped_steps) == 0.0
    o = O.AverageOracle(alone["p0"], "ema", DECAY)
    for p in alone["traj"]:
        o.update(p)
    O.assert_within(fused["avg"].flat_avg, o, what="EMA after 4 training steps")
    assert not torch.equal(fused["avg"].flat_avg.cpu(), alone["traj"][-1]), "the average is not the last parameters"


def test_default_optimizer_with_update_keeps_its_fast_path_bits(dev):
    """ArenaAdam with default options (the one-launch kernel) + avg.update(opt): the live parameters of ArenaAdam alone"""
    a = _train(dev, "alone", steps=2, opt_kw=dict(lr=LR))
    u = _train(dev, "update", steps=2, opt_kw=dict(lr=LR), mode="swa")
    assert u["arena"]._optim is None, "the default optimizer has no control block: update() passes none"
    for k in range(2):
        assert torch.equal(_bits(a["traj"][k]), _bits(u["traj"][k]))
    o = O.AverageOracle(a["p0"], "swa")
    for p in a["traj"]:
        o.update(p)
    O.assert_within(u["avg"].flat_avg, o, what="SWA after 2 steps")


def test_buffers_are_averaged_on_request(dev):
    r = _train(dev, "fused", steps=3, use_buffers=True, warmup=True)
    avg, model = r["avg"], r["model"]
    floats = [i for i, b in enumerate(model.buffers()) if b.is_floating_point()]
    assert len(avg._buf_avg) == len(floats) > 0
    for j, i in enumerate(floats):
        o = O.AverageOracle(r["btraj"][0][i].reshape(-1), "ema", DECAY, warmup=True)
        for k in range(3):
            o.update(r["btraj"][k][i].reshape(-1))
        got = avg._buf_avg[j].reshape(-1)
        assert bool((( got.double().cpu() - o.e).abs() <= o.bound).all()), f"buffer {i}"
    changed = any(not torch.equal(a.cpu(), r["btraj"][-1][i]) for a, i in zip(avg._buf_avg, floats))
    assert changed, "the averaged buffers are not the live ones"


# ----------------------------------------------------------------------------- evaluation
def _second_module(dev, state_dict):
    """A second module (its own arena: the same layout and alignment) holding `state_dict`."""
    from vision_mtl_amd import ops

    model, module, arena = _setup(dev, seed=2)
    module.load_state_dict(state_dict)
    ops.packs.invalidate()
    return module.eval(), arena


@pytest.mark.parametrize("use_buffers", [False, True])
def test_validation_under_the_average_is_the_averaged_model(dev, use_buffers):
    from vision_mtl_amd import dp, ops
    from vision_mtl_amd.graphed import GraphedEval

    r = _train(dev, "fused", steps=3, use_buffers=use_buffers)
    module, model, arena, avg = r["module"], r["model"], r["arena"], r["avg"]
    module.eval()
    batch = _batches(1, dev, first=900)[0]
    with torch.no_grad():
        live_loss = module.validation_step(dict(batch), 0).clone()
        geval = GraphedEval(module, dict(batch), stage="val")  # captured before the module knows an average
        assert torch.equal(geval(dict(batch)), live_loss)
    second, _ = _second_module(dev, avg.averaged_state_dict(module))
    with torch.no_grad():
        want = second.validation_step(dict(batch), 0).clone()
    assert not torch.equal(want, live_loss), "the averaged model should not score like the live one here"

    p_before, b_before, e_before = arena.flat_param.detach().clone(), _buffers(model), avg.flat_avg.clone()
    ptrs = [p.data_ptr() for p in model.parameters()]
    module.weight_average = avg
    with torch.no_grad():
        got = module.validation_step(dict(batch), 0).clone()
        assert torch.equal(_bits(got), _bits(want)), (float(got), float(want))
        assert torch.equal(_bits(module.test_step(dict(batch), 0)), _bits(want))
        with pytest.raises(ValueError, match="weight_average"):
            geval(dict(batch))  # the attribute changed since construction
        geval.weight_average = avg  # ... and the caller says the capture is to follow it: no recapture
        assert torch.equal(_bits(geval(dict(batch))), _bits(want))
        assert torch.equal(_bits(geval(dict(batch))), _bits(want))
        # a capture built with the average set: construction applies nothing and has no side effects
        g2 = GraphedEval(module, dict(batch), stage="val")
        assert torch.equal(_bits(arena.flat_param), _bits(p_before)) and arena._applied_average is None
        assert torch.equal(_bits(g2(dict(batch))), _bits(want))
        # predict: the averaged model's predictions
        want_pred = second.predict_step({"img": batch["img"]})
        got_pred = module.predict_step({"img": batch["img"]})
        assert torch.equal(got_pred["segm"], want_pred["segm"]) and torch.equal(got_pred["depth"], want_pred["depth"])
    assert torch.equal(_bits(arena.flat_param), _bits(p_before)), "the live parameters changed"
    assert torch.equal(_bits(avg.flat_avg), _bits(e_before)), "the average changed"
    for a, b in zip(_buffers(model), b_before):
        assert torch.equal(a, b), "a BatchNorm buffer changed"
    assert [p.data_ptr() for p in model.parameters()] == ptrs
    # training never applies it, and the next eager step sees the live weights again
    module.weight_average = None
    with torch.no_grad():
        assert torch.equal(_bits(module.validation_step(dict(batch), 0)), _bits(live_loss))
    del ops


# ----------------------------------------------------------------------------- capture
def test_captured_step_with_average_advances_by_itself(dev):
    from vision_mtl_amd import dp

    gen = torch.Generator().manual_seed(21)
    n = _setup(dev)[2].numel
    grads = [(torch.randn(n, generator=gen) * s).to(dev) for s in (1.0, 3.0, 0.5)]

    def build():
        _, _, arena = _setup(dev)
        avg = dp.ArenaAverage(arena, decay=DECAY, warmup=True)
        return arena, avg, dp.ArenaAdam(arena, lr=LR, skip_nonfinite=True, capturable=True, average=avg)

    arena_e, avg_e, opt_e = build()  # eager (also loads every kernel before the capture below)
    for g in grads:
        arena_e.flat_grad.copy_(g)
        opt_e.step()
    arena_c, avg_c, opt_c = build()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_c.step()
    assert int(avg_c.n_averaged) == 0, "capturing runs nothing"
    for g in grads:
        arena_c.flat_grad.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    from vision_mtl_amd import ops

    ops.packs.invalidate()
    assert int(avg_c.n_averaged) == 3 and int(avg_e.n_averaged) == 3
    assert torch.equal(_bits(arena_c.flat_param), _bits(arena_e.flat_param))
    assert torch.equal(_bits(avg_c.flat_avg), _bits(avg_e.flat_avg)), "the replayed average differs from the eager one"
    assert not torch.equal(_bits(avg_c.flat_avg), _bits(arena_c.flat_param))


def test_captured_update_alone(dev):
    """avg.update() captured on its own: no allocation, no host sync, the counter advances per replay"""
    from vision_mtl_amd import dp

    _, _, arena = _setup(dev)
    avg = dp.ArenaAverage(arena, mode="swa")
    ref = dp.ArenaAverage(arena, mode="swa")
    gen = torch.Generator().manual_seed(22)
    ps = [torch.randn(arena.numel, generator=gen).to(dev) for _ in range(3)]
    for p in ps:
        arena.flat_param.copy_(p)
        ref.update()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        avg.update()
    for p in ps:
        arena.flat_param.copy_(p)
        graph.replay()
    torch.cuda.synchronize()
    assert int(avg.n_averaged) == 3
    assert torch.equal(_bits(avg.flat_avg), _bits(ref.flat_avg))
    o = O.AverageOracle(ps[0].cpu(), "swa")
    for p in ps:
        o.update(p.cpu())
    O.assert_within(avg.flat_avg, o, what="captured SWA")


# ----------------------------------------------------------------------------- guards
def test_applied_refuses_updates_steps_and_nesting(dev):
    from vision_mtl_amd import dp

    _, _, arena = _setup(dev)
    avg = dp.ArenaAverage(arena, decay=DECAY)
    opt = dp.ArenaAdam(arena, lr=LR)
    fused = dp.ArenaAdam(arena, lr=LR, average=avg)
    arena.flat_grad.normal_()
    avg.flat_avg.add_(1.0)
    live, mean = arena.flat_param.detach().clone(), avg.flat_avg.clone()
    with avg.applied() as a:
        assert a is avg and avg.is_applied
        assert torch.equal(_bits(arena.flat_param), _bits(mean)) and torch.equal(_bits(avg.flat_avg), _bits(live))
        with pytest.raises(RuntimeError, match="applied"):
            avg.update()
        with pytest.raises(RuntimeError, match="applied"):
            opt.step()
        with pytest.raises(RuntimeError, match="applied"):
            fused.step()
        with pytest.raises(RuntimeError, match="nest"):
            with avg.applied():
                pass
        with pytest.raises(RuntimeError, match="applied"):
            avg.state_dict()
    assert not avg.is_applied and arena._applied_average is None
    assert torch.equal(_bits(arena.flat_param), _bits(live)) and torch.equal(_bits(avg.flat_avg), _bits(mean))
    # an exception inside the block still exchanges back
    with pytest.raises(KeyError):
        with avg.applied():
            raise KeyError("x")
    assert torch.equal(_bits(arena.flat_param), _bits(live)) and arena._applied_average is None
    opt.step()
    avg.update(opt)
    assert int(avg.n_averaged) == 1
