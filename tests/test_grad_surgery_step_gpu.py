"""-m gpu: one training step of `basic` with MTLModule(grad_surgery=...) against the existing fixed-weight step
(3 x 64 x 96, 19 classes, synthetic_batch(..., masked=0.1); the twin-module pattern of test_task_balance_step_gpu.py).

The property.  The surgery node hands the trunk alpha g_a + beta g_b, where g_a and g_b are the two heads' gradients of
the shared decoder map with the module's loss weights (w_s, w_d) already applied.  Every parameter BELOW the heads
therefore has the gradient of a fixed-weight step with loss_segm_weight = alpha w_s and loss_depth_weight = beta w_d,
alpha and beta the fp32 values read from `stats`; the four head tensors have the gradient of the (w_s, w_d) step.  The
fixed-weight steps run without surgery and with VMTL_SMALL_TAIL=0, the unfused tail the surgery step takes.

Yardstick (as in that file): the fixed-weight step run twice in the same test; per parameter the allowed difference
(2-norm) is the larger of the run-to-run difference and 1e-6 of the whole-gradient norm.

Whether the synthetic batch conflicts at weights (1, 1) is not known in advance; d changes sign with w_d, so the
"pcgrad" cases take the sign of w_d from one diagnostic "sum" step and assert d < 0 (the projection ran) or d > 0.

Measured on one MI355X (profiles/grad_surgery/step_tests.txt).  The steps are deterministic there (run-to-run 0), so the
bound is 1e-6 of the whole-gradient norm, and the worst ratio of a parameter's difference to it was: "sum" 0.910, "mgda"
0.962, "imtl_g" 0.910, "pcgrad" 0.944 (conflict) and 0.910 (agree).  With "sum", where the coefficients are exactly 1, the
two steps differ only in the association order of the heads' data-gradient sum (171 + 9 terms combined afterwards against
one 180-term sum): that alone is 0.91 of the bound after the backward pass through the trunk.  (With the combination
rounded twice in fp32, fma(alpha, a, beta * b), "imtl_g" stood at 1.018 and missed: csrc/surgery.hip now rounds once.)"""
import argparse
import gc

import pytest
import torch

from tests import surgery_oracle as O

pytestmark = pytest.mark.gpu
C, SHAPE = 19, (3, 64, 96)
HEADS = ("segm_head.", "depth_head.")


@pytest.fixture(autouse=True)
def _collect_models():
    yield
    gc.collect()
    torch.cuda.empty_cache()


_SD = {}


def _make():
    from vision_mtl_amd.utils.pipeline_utils import build_model

    torch.manual_seed(11)
    m = build_model(argparse.Namespace(model_name="basic", backbone_weights=None), argparse.Namespace(num_classes=C))
    if not _SD:
        _SD.update({k: v.clone() for k, v in m.state_dict().items()})
    m.load_state_dict(_SD)
    return m


def _batch(seed=11):
    from vision_mtl_amd.data import synthetic_batch

    return synthetic_batch(*SHAPE, C, seed=seed, masked=0.1)


def _module(dev, **kw):
    from vision_mtl_amd.lit_module import MTLModule

    return MTLModule(_make().to(dev).train(), num_classes=C, device=str(dev), **kw)


def _step(module, batch, dev):
    """one eager training step; (loss, {name: fp64 gradient})"""
    loss = module.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().double().cpu().clone() for n, p in module.model.named_parameters() if p.grad is not None}
    return float(loss.detach().double()), grads


def _norm(d):
    return float(torch.sqrt(sum((v ** 2).sum() for v in d.values())))


_SIGN = {}


def _conflicting_depth_weight(dev):
    """w_d in {+1, -1} under which the batch's two gradients conflict (d < 0), from one diagnostic "sum" step"""
    if not _SIGN:
        m = _module(dev, grad_surgery="sum")
        _step(m, _batch(), dev)
        st = [float(v) for v in m.grad_surgery.stats.cpu()]
        assert abs(st[5]) >= 1e-3, f"the batch's gradients are orthogonal to working precision: {st}"
        _SIGN["wd"] = 1.0 if st[1] < 0 else -1.0
        _SIGN["cos"] = st[5]
    return _SIGN["wd"]


def _assert_property(dev, method, wd, monkeypatch):
    """the surgery step against the fixed-weight steps; returns the stats"""
    monkeypatch.setenv("VMTL_SMALL_TAIL", "0")  # the fixed-weight steps take the unfused tail too
    batch = _batch()
    module = _module(dev, grad_surgery=method, loss_depth_weight=wd)
    loss_s, g_s = _step(module, batch, dev)
    st = [float(v) for v in module.grad_surgery.stats.cpu()]  # the fp32 values, exactly
    na, d, nb, alpha, beta, cos = st
    assert module.grad_surgery.counters.tolist() == [1, int(d < 0)]
    ra, rb = O.coefficients(method, na, d, nb)
    assert abs(alpha - ra) <= 2.0 ** -24 * abs(ra) and abs(beta - rb) <= 2.0 ** -24 * abs(rb)

    fixed = [_step(_module(dev, loss_segm_weight=alpha, loss_depth_weight=beta * wd), batch, dev) for _ in range(2)]
    (loss_f, g_f), (_, g_f2) = fixed
    if (alpha, beta) == (1.0, 1.0):
        loss_h, g_h = loss_f, g_f
    else:
        loss_h, g_h = _step(_module(dev, loss_depth_weight=wd), batch, dev)
    assert abs(loss_s - loss_h) <= 1e-6 * max(abs(loss_h), 1.0), "surgery acts on the gradient: the loss is the (w_s, w_d) step's"

    whole, whole_h, worst = _norm(g_f), _norm(g_h), 0.0
    assert set(g_s) == set(g_f) == set(g_h) and whole > 0
    assert sum(k.startswith(HEADS) for k in g_s) == 4
    for k in g_s:
        ref = g_h if k.startswith(HEADS) else g_f
        err, noise = float((g_s[k] - ref[k]).norm()), float((g_f[k] - g_f2[k]).norm())
        bound = max(noise, 1e-6 * (whole_h if k.startswith(HEADS) else whole))
        worst = max(worst, err / bound)
        assert err <= bound, f"{k}: |surgery - fixed| {err:.3e}, run to run {noise:.3e}, whole {whole:.3e}"
    trunk = {k: v for k, v in g_s.items() if not k.startswith(HEADS)}
    print(f"{method} w_d={wd:+.0f}: stats {st}, whole-gradient norm {whole:.6g}, run-to-run "
          f"{_norm({k: g_f[k] - g_f2[k] for k in g_f}):.3e}, surgery vs fixed (trunk) "
          f"{_norm({k: trunk[k] - g_f[k] for k in trunk}):.3e}, worst ratio to its bound {worst:.3f}")
    return st


@pytest.mark.parametrize("method", ["sum", "mgda", "imtl_g"])
def test_surgery_step_is_the_fixed_weight_step(dev, method, monkeypatch):
    st = _assert_property(dev, method, 1.0, monkeypatch)
    if method == "sum":
        assert st[3:5] == [1.0, 1.0]
    else:
        assert 0.0 <= st[3] <= 1.0 and abs(st[3] + st[4] - 1.0) <= 2.0 ** -23


@pytest.mark.parametrize("conflict", [True, False], ids=["conflict", "agree"])
def test_pcgrad_step_is_the_fixed_weight_step(dev, conflict, monkeypatch):
    wd = _conflicting_depth_weight(dev)
    st = _assert_property(dev, "pcgrad", wd if conflict else -wd, monkeypatch)
    if conflict:
        assert st[1] < 0 and st[3] > 1.0 and st[4] > 1.0, f"the projection branch must run: {st}"
    else:
        assert st[1] > 0 and st[3:5] == [1.0, 1.0], st


def test_graphed_step_follows_the_batch(dev):
    """a captured "pcgrad" step replayed on batch A, then B: each time the stats and the trunk gradients of the eager
    step on a twin; the coefficients differ between A and B, so the graph read them from the device"""
    from vision_mtl_amd import dp
    from vision_mtl_amd.graphed import GraphedStep

    wd = _conflicting_depth_weight(dev)  # batch A (the diagnostic's batch) conflicts under this weight
    batches = [_batch(11), _batch(12)]
    sd0 = {k: v.clone() for k, v in _make().state_dict().items()}

    def run(graphed):
        module = _module(dev, grad_surgery="pcgrad", loss_depth_weight=wd)
        arena = dp.FlatArena(module.model)
        if graphed:
            gstep = GraphedStep(module, _batch(10), arena=arena)
            assert module.grad_surgery.counters.tolist()[0] >= 3  # warm-up, rehearsal and capture ran the node
        else:
            arena.rebind_grads()
        out = []
        for b in batches:  # every step from the same weights and BatchNorm buffers: no optimizer in between
            module.model.load_state_dict(sd0)
            dp.ops.packs.invalidate()
            arena.flat_grad.zero_()
            arena.rebind_grads()
            module.grad_surgery.reset_counters()
            loss = gstep(b) if graphed else module.training_step({k: v.to(dev) for k, v in b.items()}, 0)
            loss.backward()
            torch.cuda.synchronize()
            out.append((loss.detach().clone(), arena.flat_grad.double().cpu(), module.grad_surgery.stats.clone(),
                        module.grad_surgery.counters.tolist()))
        return out

    eager, eager2, replay = run(False), run(False), run(True)
    assert not torch.equal(replay[0][2][3:5], replay[1][2][3:5]), "the coefficients of A and B must differ"
    assert float(replay[0][2][3]) > 1.0 and replay[0][3] == [1, 1], "batch A conflicts: the projection ran in the replay"
    for i, (g, e, e2) in enumerate(zip(replay, eager, eager2)):
        assert torch.isfinite(e[0]) and torch.equal(g[0].float(), e[0].float()), (i, float(g[0]), float(e[0]))
        assert g[3] == e[3], f"batch {i}: counters {g[3]} vs {e[3]}"
        for k in range(6):  # the same yardstick, entry by entry
            sg, se, se2 = float(g[2][k]), float(e[2][k]), float(e2[2][k])
            assert abs(sg - se) <= max(abs(se - se2), 1e-6 * abs(se)), f"batch {i}: stats[{k}] {sg!r} vs eager {se!r}"
        err, noise, whole = float((g[1] - e[1]).norm()), float((e[1] - e2[1]).norm()), float(e[1].norm())
        print(f"batch {i}: stats {g[2].tolist()}, |replay - eager| {err:.3e}, eager run to run {noise:.3e}, whole {whole:.6g}")
        assert err <= max(noise, 1e-6 * whole)


def test_evaluation_routes_are_untouched(dev):
    """validation under no_grad, and an eval-mode forward with gradients enabled, equal the default module's bit for bit
    and launch nothing of the feature"""
    from vision_mtl_amd import ops

    batch = {k: v.to(dev) for k, v in _batch().items()}
    plain, surg = _module(dev), _module(dev, grad_surgery="pcgrad")
    names, orig_k = [], ops._k

    def rec(name, *a, **kw):
        names.append(name)
        return orig_k(name, *a, **kw)

    ops._k = rec
    try:
        with torch.no_grad():
            lp, ls = plain.validation_step(dict(batch)), surg.validation_step(dict(batch))
        assert torch.equal(lp, ls)
        for k in plain.step_outputs["val"]:
            assert torch.equal(torch.stack(plain.step_outputs["val"][k]), torch.stack(surg.step_outputs["val"][k])), k
        plain.model.eval(), surg.model.eval()
        op, os_ = plain(batch["img"]), surg(batch["img"])
        assert torch.equal(op["segm"], os_["segm"]) and torch.equal(op["depth"], os_["depth"])
    finally:
        ops._k = orig_k
    assert not any("surgery" in n for n in names), "an evaluation route launched the surgery kernels"
    with pytest.raises(RuntimeError, match="no backward pass"):
        surg.grad_surgery.stats


def test_default_module_launches_what_it_always_launched(dev):
    """Three default modules - built without the argument, built with grad_surgery=None, and built with "pcgrad" whose
    attribute was then cleared - run one training step: the same launch sequence (entry point and scalar arguments), the
    same loss and the same gradients bit for bit (the eager step is deterministic), nothing of the feature, and the fused
    tail.  The surgery step adds exactly its three launches."""
    from vision_mtl_amd import ops

    batch = _batch()

    def record(module):
        seq, orig_k = [], ops._k

        def rec(name, *a, **kw):
            seq.append((name, tuple(sorted((k, v) for k, v in kw.items() if isinstance(v, (int, float))))))
            return orig_k(name, *a, **kw)

        ops._k = rec
        try:
            loss, grads = _step(module, batch, dev)
        finally:
            ops._k = orig_k
        return loss, seq, grads

    def fresh(make):
        """one module at a time: the packed-operand cache batches the operands of every live model into its launches, so
        a second live model would change their sizes"""
        gc.collect()
        ops.packs.invalidate()
        module = make()
        try:
            return record(module)
        finally:
            del module

    def cleared():
        module = _module(dev, grad_surgery="pcgrad")
        module.grad_surgery = None
        return module

    l0, s0, g0 = fresh(lambda: _module(dev))
    for what, make in (("grad_surgery=None", lambda: _module(dev, grad_surgery=None)), ("attribute cleared", cleared)):
        l1, s1, g1 = fresh(make)
        diff = [i for i, (x, y) in enumerate(zip(s0, s1)) if x != y]
        assert len(s0) == len(s1) and not diff, f"{what}: launch {diff[:1]} of {len(s0)} / {len(s1)} differs: " \
                                                f"{[(s0[i], s1[i]) for i in diff[:1]]}"
        assert l0 == l1, f"{what}: loss {l1!r} against {l0!r}"
        assert set(g0) == set(g1)
        for k in g0:
            assert torch.equal(g0[k], g1[k]), f"{what}: the gradient of {k} differs from the default module's"
    assert not any("surgery" in n for n, _ in s0)
    assert any(n == "vmtl_conv3x3_small" and dict(kw).get("Ca", 0) > 0 for n, kw in s0), "the default step takes the fused tail"
    _, s2, _ = fresh(lambda: _module(dev, grad_surgery="sum"))
    assert [n for n, _ in s2 if "surgery" in n] == ["vmtl_surgery_gram", "vmtl_surgery_control", "vmtl_surgery_combine"]


def test_captured_step_survives_another_shape_on_the_same_object(dev):
    """A captured step holds the raw addresses of the surgery object's state block, workspace and head operand.  The same
    object then serves an eager training step at ANOTHER batch shape (what a second GraphedStep's warm-up does): none of
    the three buffers of the first shape may move, and the first graph replays to the bits it gave before."""
    from vision_mtl_amd import dp
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep

    module = _module(dev, grad_surgery="pcgrad", loss_depth_weight=_conflicting_depth_weight(dev))
    arena = dp.FlatArena(module.model)
    gstep = GraphedStep(module, _batch(10), arena=arena)
    s = module.grad_surgery
    sd0 = {k: v.clone() for k, v in module.model.state_dict().items()}

    def replay():
        module.model.load_state_dict(sd0)
        dp.ops.packs.invalidate()
        arena.flat_grad.zero_()
        arena.rebind_grads()
        gstep(_batch(11)).backward()
        torch.cuda.synchronize()
        return arena.flat_grad.clone(), s.stats.clone()

    g_before, st_before = replay()
    ptrs = (s._state.data_ptr(), s._workspace.data_ptr(), sorted(b.data_ptr() for b in s._operands.values()))
    assert s._workspace.numel() * 8 == 1024 * 3 * 8, "the workspace is sized for the largest grid, once"

    other = synthetic_batch(2, 64, 64, C, seed=5, masked=0.1)  # 8192 pixels against 18432: another rows, another grid
    arena.rebind_grads()
    module.training_step({k: v.to(dev) for k, v in other.items()}, 0).backward()
    torch.cuda.synchronize()
    assert (s._state.data_ptr(), s._workspace.data_ptr()) == ptrs[:2], "a buffer a captured step holds was replaced"
    assert set(ptrs[2]) <= {b.data_ptr() for b in s._operands.values()}

    g_after, st_after = replay()
    assert torch.equal(st_before.view(torch.int32), st_after.view(torch.int32))
    assert torch.equal(g_before.view(torch.int32), g_after.view(torch.int32)), "the first graph no longer replays to its bits"
    assert float(st_after[3]) > 1.0 and bool(torch.isfinite(g_after).all())
