"""-m gpu: the task-balancing kernels (csrc/balance.hip) through ops.balance_losses / ops.dwa_epoch_update, on poisoned,
guard-banded buffers (tests.poison.patched("guard")), against the closed forms evaluated in fp64 on the CPU.

Bar: 1e-5 relative for total, weights, the per-loss gradients and the gradient of the log-variances.  The kernels do a
dozen fp32 roundings plus exp / log at a few ulp - about 1e-6 - and the bar leaves a tenfold margin over that.  The
inputs keep 1 - w_k L_k away from zero, so the relative bar is meaningful for it too."""
import math

import pytest
import torch

from tests import poison

pytestmark = pytest.mark.gpu
RTOL = 1e-5
LOSSES = (1.66, 9.9, 0.3)
LOG_VARS = (0.8, -0.2, 1.3)
DWA_W = (1.3, 0.7, 1.0)
GRAD_OUT = 0.37


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _closed_form(mode, L, param):
    """(total, weights, dparam) in fp64 from the fp32 values of the inputs"""
    T = len(L)
    if mode == "uncertainty":
        w = [math.exp(-s) for s in param]
        return sum(wk * lk + s for wk, lk, s in zip(w, L, param)), w, [1.0 - wk * lk for wk, lk in zip(w, L)]
    if mode == "dwa":
        return sum(wk * lk for wk, lk in zip(param, L)), list(param), None
    total = math.exp(sum(math.log(lk) for lk in L) / T)
    return total, [total / (T * lk) for lk in L], None


def _close(got, ref, what):
    got = [float(g) for g in (got.detach().cpu().double().flatten())]
    ref = [ref] if isinstance(ref, float) else list(ref)
    assert len(got) == len(ref), what
    for k, (a, b) in enumerate(zip(got, ref)):
        print(f"{what}[{k}]: {a!r} vs {b!r}")
        assert abs(a - b) <= RTOL * abs(b), f"{what}[{k}]: {a} vs closed form {b}"


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("mode", ["uncertainty", "dwa", "geometric"])
def test_forward_and_backward_match_the_closed_forms(dev, mode, T):
    from vision_mtl_amd import ops

    L = [_f32(x) for x in LOSSES[:T]]
    src = {"uncertainty": LOG_VARS, "dwa": DWA_W, "geometric": None}[mode]
    pv = None if src is None else [_f32(x) for x in src[:T]]
    total_ref, w_ref, dp_ref = _closed_form(mode, L, pv)
    go = _f32(GRAD_OUT)
    with poison.patched("guard") as p:
        losses = [torch.tensor(x, device=dev, requires_grad=True) for x in L]
        param = None if pv is None else torch.tensor(pv, device=dev, requires_grad=mode == "uncertainty")
        total, weights = ops.balance_losses(losses, mode, param)
        assert total.shape == () and weights.shape == (T,) and not weights.requires_grad
        (total * go).backward()
        assert p.count >= 2 + T  # total, weights and the T loss gradients all came from ops._empty
        _close(total, total_ref, "total")
        _close(weights, w_ref, "weights")
        for k, l in enumerate(losses):
            _close(l.grad, go * w_ref[k], f"g{k}")
        if mode == "uncertainty":
            _close(param.grad, [go * d for d in dp_ref], "dparam")
        elif param is not None:
            assert param.grad is None


def test_parameter_gradient_goes_into_the_arena_slot(dev):
    from vision_mtl_amd import dp, ops

    L = [_f32(x) for x in LOSSES[:2]]
    pv = [_f32(x) for x in LOG_VARS[:2]]
    _, _, dp_ref = _closed_form("uncertainty", L, pv)
    s = torch.nn.Parameter(torch.tensor(pv, device=dev))
    arena = dp.FlatArena(torch.nn.Linear(3, 1).to(dev), extra_params=[s])
    arena.flat_grad.fill_(float("nan"))
    seen = []
    s.register_hook(seen.append)  # autograd must be handed nothing: the kernel wrote the slot
    with poison.patched("guard"):
        total, _ = ops.balance_losses([torch.tensor(x, device=dev) for x in L], "uncertainty", s)
        total.backward()
        assert all(g is None for g in seen)
        _close(arena.flat_grad[-2:], dp_ref, "slot")
        assert s.grad.data_ptr() == arena.flat_grad.data_ptr() + 4 * arena.offsets[-1]
        assert bool(torch.isnan(arena.flat_grad[:-2]).all())  # and nothing else


def test_dwa_accumulation_skips_non_finite_steps_and_accumulate_off(dev):
    from vision_mtl_amd import ops

    T = 2
    w = torch.tensor([1.3, 0.7], device=dev)
    state = torch.zeros(ops.balance_state_doubles(T), dtype=torch.float64, device=dev)
    steps = [(1.5, 0.25, True), (float("nan"), 0.5, True), (2.5, 0.75, True), (3.0, 1.0, False), (0.5, float("inf"), True)]
    with poison.patched("guard"):
        for a, b, acc in steps:
            total, _ = ops.balance_losses([torch.tensor(a, device=dev), torch.tensor(b, device=dev)], "dwa", w, state,
                                          accumulate=acc)
            if math.isfinite(a) and math.isfinite(b):
                assert abs(float(total) - (_f32(1.3) * a + _f32(0.7) * b)) <= RTOL * float(total)
            else:
                assert not math.isfinite(float(total))
    # two of the five forwards count: exact in fp64 (the losses are exact binary fractions)
    assert state.tolist() == [1.5 + 2.5, 0.25 + 0.75, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert w.tolist() == [_f32(1.3), _f32(0.7)]


def _dwa_formula(prev, prev2, tau):
    r = [a / b for a, b in zip(prev, prev2)]
    e = [math.exp(x / tau) for x in r]
    return [len(r) * x / sum(e) for x in e]


@pytest.mark.parametrize("T", [2, 3])
def test_dwa_epoch_updates(dev, T):
    from vision_mtl_amd import ops

    tau = 0.7
    epochs = [((1.66, 9.9, 0.3), 4), ((1.2, 9.5, 0.31), 3), ((1.0, 7.0, 0.2), 5)]  # (mean losses, steps)
    w = torch.full((T,), 5.0, device=dev)
    state = torch.zeros(ops.balance_state_doubles(T), dtype=torch.float64, device=dev)

    def run_epoch(mean, n):
        for _ in range(n):
            ops.balance_losses([torch.tensor(m, device=dev) for m in mean[:T]], "dwa", w, state, accumulate=True)
        ops.dwa_epoch_update(state, w, tau)

    def check(hist, nepochs):
        st = state.tolist()
        assert st[:T + 2] == [0.0] * T + [0.0, float(nepochs)]  # sums and step count zeroed, epochs counted
        for name, got, ref in (("prev", st[T + 2:2 * T + 2], hist[-1]), ("prev2", st[2 * T + 2:], hist[-2])):
            for a, b in zip(got, ref):
                assert abs(a - b) <= RTOL * abs(b) if b else a == 0.0, (name, got, ref)

    zeros = [0.0] * T
    hist = [zeros, zeros]
    with poison.patched("guard"):
        ops.dwa_epoch_update(state, w, tau)  # an epoch without a step: nothing moves, not even the weights
        assert w.tolist() == [5.0] * T and state.tolist() == [0.0] * (3 * T + 2)
        for i, (mean, n) in enumerate(epochs):
            run_epoch(mean, n)
            hist.append([_f32(m) for m in mean[:T]])
            check(hist, i + 1)
            if i == 0:
                assert w.tolist() == [1.0] * T  # exactly 1 until there is a ratio
            else:
                _close(w, _dwa_formula(hist[-1], hist[-2], tau), f"w after epoch {i + 1}")
        assert abs(float(w.sum()) - T) <= 1e-5 * T
        before_w, before = w.clone(), state.clone()
        ops.dwa_epoch_update(state, w, tau)  # the empty epoch again, now with a history
        assert torch.equal(w, before_w) and torch.equal(state, before)
        # a ratio that is not positive: weights, history and epoch count stay; the epoch's sums are dropped
        run_epoch((-1.0, 1.0, 1.0), 2)
        assert torch.equal(w, before_w) and torch.equal(state, before)
        # ... and training goes on from the kept history
        run_epoch((0.9, 6.0, 0.25), 2)
        hist.append([_f32(m) for m in (0.9, 6.0, 0.25)[:T]])
        check(hist, 4)
        _close(w, _dwa_formula(hist[-1], hist[-2], tau), "w after the epoch that follows a dropped one")


@pytest.mark.parametrize("bad", [0.0, -0.5])
def test_geometric_with_a_non_positive_loss_is_nan(dev, bad):
    from vision_mtl_amd import ops

    with poison.patched("guard"):
        losses = [torch.tensor(1.66, device=dev, requires_grad=True), torch.tensor(bad, device=dev, requires_grad=True)]
        total, weights = ops.balance_losses(losses, "geometric")
        total.backward()
        assert math.isnan(float(total.detach())) and bool(torch.isnan(weights).all())
        assert all(math.isnan(float(l.grad)) for l in losses)
