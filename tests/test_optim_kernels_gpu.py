"""csrc/optim.hip against torch in fp64 on the CPU: the deterministic gradient norm, the clipped Adam / AdamW update, the
skipped non-finite step and the in-place clip (ops.grad_norm / adam_step_ex / scale_by_clip).

Checker: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / AdamW on double copies of the same fp32 inputs.

Sizes: a lone element, fewer than one vector, one workgroup's edge (255 / 257), a vector-width edge (1023) and
4096 * 256 + 5, which needs a second trip of the grid-stride loop (the float4 body has 1024 workgroups of 256 threads:
262145 vectors; the scalar fall-back of the update has 4096 workgroups).  Each size runs on a 16-byte-aligned buffer and
on buf[1:] (4-byte aligned only: 3 head elements are peeled); the update also runs with p, g, m and v at four different
offsets, which takes its scalar fall-back.

Every device buffer - gradient, parameters, moments, workspace, control block, step counter - is the payload of a
guard-banded, NaN-poisoned allocation of tests/poison.py; the guards and the elements in front of a misaligned payload
are checked at the end of each test.

TOL = 1e-6 (max-abs error over the reference's max magnitude, tests.util.assert_close) is the tolerance
test_layout_roundtrip_and_adam holds the parent's kernel to against fp32 torch; the norm's 1e-6 is derived: the sum is
accumulated in double, which leaves the final rounding to fp32 (6e-8)."""
import math

import pytest
import torch

from tests import poison
from tests.util import assert_close

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 255, 257, 1023, 4096 * 256 + 5]
OFFS = [0, 1]
TOL = 1e-6
LR = 5e-3


def _ops():
    from vision_mtl_amd import ops

    return ops


# ----------------------------------------------------------------------------- inputs and the fp64 checker (computed once)
_INPUTS = {}


def _inputs(n):
    """p0 and three gradients randn * (0.1, 10, 1), fp32, on the CPU; the same for every test of one size.  The seed is
    per size and fixed: for n = 1 and 3 it was chosen (on the CPU, from the checker's norms) so that max_norm = sqrt(n)
    does not clip the first gradient and clips the second by more than half."""
    if n not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + n)
        p0 = torch.randn(n, generator=g)
        grads = [torch.randn(n, generator=g) * s for s in (0.1, 10.0, 1.0)]
        _INPUTS[n] = (p0, grads)
    return _INPUTS[n]


_CHECK = {}


def _checker(n, wd=0.0, decoupled=False, max_norm=None, gscale=1.0, steps=(0, 1, 2)):
    """fp64 torch: per step a dict of p, m, v (after the step), norm (before clipping) and g (the clipped gradient)."""
    key = (n, wd, decoupled, max_norm, gscale, steps)
    if key not in _CHECK:
        p0, grads = _inputs(n)
        p = p0.double().clone().requires_grad_(True)
        cls = torch.optim.AdamW if decoupled else torch.optim.Adam
        opt = cls([p], lr=LR, weight_decay=wd)
        out = []
        for i in steps:
            p.grad = grads[i].double() * gscale
            if max_norm is not None:
                norm = torch.nn.utils.clip_grad_norm_([p], max_norm)
            else:
                norm = p.grad.norm()
            gc = p.grad.clone()
            opt.step()
            st = opt.state[p]
            out.append({"p": p.detach().clone(), "m": st["exp_avg"].clone(), "v": st["exp_avg_sq"].clone(),
                        "norm": norm.clone(), "g": gc})
        _CHECK[key] = out
    return _CHECK[key]


class _Bufs:
    """Guard-banded device buffers; close() checks the guards and the skipped elements in front of misaligned payloads."""

    def __init__(self, dev):
        self.P = poison.Poison("guard")
        self.like = torch.empty(0, device=dev)
        self.fronts = []

    def f32(self, n, off=0, src=None):
        base = self.P.empty(n + off, self.like)
        if off:
            self.fronts.append(base[:off])
        t = base[off:]
        if src is not None:
            t.copy_(src)
        return t

    def zeros(self, n, off=0):
        return self.f32(n, off, torch.zeros(n))

    def workspace(self, n):
        nbytes = _ops().lib().raw("vmtl_grad_sumsq_workspace_bytes")(n)
        assert nbytes % 8 == 0 and nbytes >= 8
        return self.P.empty(nbytes // 4, self.like).view(torch.float64)

    def ctl(self):
        return self.zeros(_ops().OPTIM_CTL_FLOATS)

    def close(self):
        for f in self.fronts:
            assert bool(poison.is_sentinel(f).all()), "an element in front of a misaligned payload was written"
        self.P.close()


def _state(B, n, offs):
    p0, _ = _inputs(n)
    return B.f32(n, offs[0], p0), B.zeros(n, offs[2]), B.zeros(n, offs[3]), B.zeros(1)


def _offs(off):
    return (0, 1, 2, 3) if off == "mixed" else (off,) * 4


# ----------------------------------------------------------------------------- norm
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_norm_matches_fp64_and_is_deterministic(dev, n, off):
    ops = _ops()
    _, grads = _inputs(n)
    B = _Bufs(dev)
    g = B.f32(n, off, grads[2])
    ws, ctl = B.workspace(n), B.ctl()
    a = ops.grad_norm(g, 1.0, ws, ctl).clone()
    b = ops.grad_norm(g, 1.0, ws, ctl).clone()
    h = ops.grad_norm(g, 0.5, ws, ctl).clone()
    assert a.dim() == 0 and a.is_cuda
    assert torch.equal(a, b), "two runs of the norm differ"
    ref = grads[2].double().norm()
    print(f"n={n} off={off}: norm rel err {abs(float(a) - float(ref)) / float(ref):.2e}")
    assert abs(float(a) - float(ref)) <= 1e-6 * float(ref)
    ref_h = (0.5 * grads[2].double()).norm()
    assert abs(float(h) - float(ref_h)) <= 1e-6 * float(ref_h)
    assert torch.equal(g.cpu(), grads[2]), "the norm must not write the gradient"
    B.close()


# ----------------------------------------------------------------------------- clipped update
@pytest.mark.parametrize("off", OFFS + ["mixed"])
@pytest.mark.parametrize("n", SIZES)
def test_clipped_update_matches_fp64(dev, n, off):
    """3 steps, max_norm = sqrt(n): no clipping on the first, strong clipping on the second (Adam's direction barely
    changes under a rescaled gradient, so m and v - v carries coef^2 - are compared, at every step)."""
    ops = _ops()
    _, grads = _inputs(n)
    max_norm = math.sqrt(n)
    ref = _checker(n, max_norm=max_norm)
    coefs = [min(1.0, max_norm / (float(r["norm"]) + 1e-6)) for r in ref]
    assert coefs[0] == 1.0 and coefs[1] < 0.5, coefs
    offs = _offs(off)
    B = _Bufs(dev)
    p, m, v, step = _state(B, n, offs)
    ws, ctl = B.workspace(n), B.ctl()
    for i in range(3):
        g = B.f32(n, offs[1], grads[i])
        ops.adam_step_ex(p, g, m, v, step, LR, max_grad_norm=max_norm, workspace=ws, ctl=ctl)
        assert torch.equal(g.cpu(), grads[i]), "the fused path must not write the gradient"
        c = ctl.cpu()
        assert abs(float(c[ops.CTL_NORM]) - float(ref[i]["norm"])) <= 1e-6 * float(ref[i]["norm"])
        assert abs(float(c[ops.CTL_COEF]) - coefs[i]) <= 1e-6 and float(step) == i + 1
        for k, t in (("m", m), ("v", v), ("p", p)):
            assert_close(t.cpu(), ref[i][k], tol=TOL, what=f"n={n} off={off} step {i} {k}")
    assert float(ctl[ops.CTL_SKIPPED]) == 0.0
    B.close()


# ----------------------------------------------------------------------------- L2 vs decoupled weight decay
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_l2_and_decoupled_decay(dev, n, off):
    ops = _ops()
    _, grads = _inputs(n)
    B = _Bufs(dev)
    got = {}
    for decoupled in (False, True):
        ref = _checker(n, wd=0.1, decoupled=decoupled)
        p, m, v, step = _state(B, n, _offs(off))
        ctl = B.ctl()
        for i in range(3):
            g = B.f32(n, off, grads[i])
            ops.adam_step_ex(p, g, m, v, step, LR, weight_decay=0.1, decoupled_weight_decay=decoupled, ctl=ctl)
        for k, t in (("m", m), ("v", v), ("p", p)):
            assert_close(t.cpu(), ref[2][k], tol=TOL, what=f"n={n} off={off} decoupled={decoupled} {k}")
        assert math.isnan(float(ctl[ops.CTL_NORM])) and float(ctl[ops.CTL_COEF]) == 1.0  # no norm was asked for
        got[decoupled] = p.cpu()
    # an ignored flag would make the two runs equal
    diff = float((got[True].double() - got[False].double()).abs().max())
    assert diff > TOL * float(got[False].abs().max()), diff
    B.close()


# ----------------------------------------------------------------------------- skip_nonfinite
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_skip_nonfinite(dev, n, off, bad):
    ops = _ops()
    _, grads = _inputs(n)
    poisoned = grads[1].clone()
    poisoned[(n // 2) if math.isinf(bad) else (n - 1)] = bad
    ref = _checker(n, steps=(0, 2))
    B = _Bufs(dev)
    p, m, v, step = _state(B, n, _offs(off))
    ws, ctl = B.workspace(n), B.ctl()
    ops.adam_step_ex(p, B.f32(n, off, grads[0]), m, v, step, LR, skip_nonfinite=True, workspace=ws, ctl=ctl)
    before = [t.clone() for t in (p, m, v, step)]
    gbad = B.f32(n, off, poisoned)
    ops.adam_step_ex(p, gbad, m, v, step, LR, skip_nonfinite=True, workspace=ws, ctl=ctl)
    for t, b in zip((p, m, v, step), before):
        assert torch.equal(t, b), "a skipped step must leave p, m, v and the step counter bit-for-bit untouched"
    assert float(ctl[ops.CTL_SKIPPED]) == 1.0 and float(ctl[ops.CTL_SKIP]) == 1.0 and float(step) == 1.0
    assert not math.isfinite(float(ctl[ops.CTL_NORM]))
    ops.adam_step_ex(p, B.f32(n, off, grads[2]), m, v, step, LR, skip_nonfinite=True, workspace=ws, ctl=ctl)
    assert float(step) == 2.0 and float(ctl[ops.CTL_SKIPPED]) == 1.0 and float(ctl[ops.CTL_SKIP]) == 0.0
    for k, t in (("m", m), ("v", v), ("p", p)):
        assert_close(t.cpu(), ref[1][k], tol=TOL, what=f"n={n} off={off} after the skipped step: {k}")
    # flag off: the step is taken and the result is non-finite, as torch's is
    p2, m2, v2, step2 = _state(B, n, _offs(off))
    ctl2 = B.ctl()
    ops.adam_step_ex(p2, gbad, m2, v2, step2, LR, max_grad_norm=math.sqrt(n), workspace=ws, ctl=ctl2)
    assert float(step2) == 1.0 and float(ctl2[ops.CTL_SKIPPED]) == 0.0 and float(ctl2[ops.CTL_NONFINITE]) == 1.0
    assert not bool(torch.isfinite(p2).all())
    tp = _inputs(n)[0].double().clone().requires_grad_(True)
    topt = torch.optim.Adam([tp], lr=LR)
    tp.grad = poisoned.double()
    torch.nn.utils.clip_grad_norm_([tp], math.sqrt(n))
    topt.step()
    assert not bool(torch.isfinite(tp).all())
    B.close()


# ----------------------------------------------------------------------------- in-place clip
@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_inplace_clip(dev, n, off, gscale):
    ops = _ops()
    _, grads = _inputs(n)
    max_norm = math.sqrt(n)
    ref = _checker(n, max_norm=max_norm, gscale=gscale)
    B = _Bufs(dev)
    ws, ctl = B.workspace(n), B.ctl()
    for i in (0, 1):  # not clipped / clipped
        g = B.f32(n, off, grads[i])
        norm = ops.scale_by_clip(g, max_norm, gscale, ws, ctl)
        assert abs(float(norm) - float(ref[i]["norm"])) <= 1e-6 * float(ref[i]["norm"]), "the pre-clip norm is returned"
        assert_close(g.cpu(), ref[i]["g"], tol=TOL, what=f"n={n} off={off} clipped gradient {i}")
        if i == 0 and gscale == 1.0:
            assert torch.equal(g.cpu(), grads[0]), "a gradient inside the bound is left as it is"
    assert float(ref[1]["g"].norm()) <= max_norm * (1 + 1e-9) < float(ref[1]["norm"])
    B.close()


def test_cpu_tensors_and_bad_bounds_raise(dev):
    ops = _ops()
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grad_norm(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scale_by_clip(x, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adam_step_ex(x, x, x, x, torch.zeros(1), 1e-3)
    with pytest.raises(ValueError):
        ops.scale_by_clip(x.to(dev), -1.0)
