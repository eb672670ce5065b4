"""ops.dual_head(..., surgery=GradSurgery(m)) at the shape of test_dual_head (2 x 33 x 12 x 20, heads 19 + 1).

Reference: CPU fp64 F.conv2d autograd gives the two per-task gradients of x separately (backward with the other head's
gradient zero), tests/surgery_oracle.py their Gram matrix and the coefficients, and the reference dx is
alpha g_a + beta g_b.  dx is compared with the tolerance test_dual_head uses for dx (tests.util.assert_close, 1e-4 of
the reference magnitude).

The incoming gradients are built so that the two maps are far from orthogonal: gb = s * conv(g_a, w_b), so that
g_b = s * W_b^T W_b g_a and <g_a, g_b> = s * |W_b g_a|^2; s = -1 conflicts, s = +1 does not.  Which branch ran is read
from the conflict counter.

stats against the fp64 Gram matrix: with every element of a map within tol * max|g| of its reference (the bound of
assert_close, tol = 1e-4), |delta g| <= sqrt(N) tol max|g| =: e, and so |delta n_a| <= 2 sqrt(n_a) e_a + e_a^2,
|delta d| <= sqrt(n_a) e_b + sqrt(n_b) e_a + e_a e_b (Cauchy-Schwarz), plus one fp32 rounding.

The heads' weight and bias gradients come from code the feature does not touch, fed the same operands: bit equality
with the plain node."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import surgery_oracle as O
from tests.util import assert_close, from_dev_nhwc, to_dev_nhwc

pytestmark = pytest.mark.gpu

B, CIN, H, W, CA, CB = 2, 33, 12, 20, 19, 1
TOL = 1e-4  # assert_close's default, what test_dual_head uses for dx


def _ops():
    from vision_mtl_amd import ops

    return ops


_REF = {}


def _reference(sign):
    """inputs, the two fp64 per-task gradients of x, their Gram matrix; computed once per sign"""
    if sign not in _REF:
        g = torch.Generator().manual_seed(43)
        x = torch.randn(B, CIN, H, W, generator=g)
        wa, wb = torch.randn(CA, CIN, 3, 3, generator=g) * 0.1, torch.randn(CB, CIN, 3, 3, generator=g) * 0.1
        ba, bb = torch.randn(CA, generator=g), torch.randn(CB, generator=g)
        ga = torch.randn(B, CA, H, W, generator=g)
        x64 = x.double().requires_grad_(True)
        ya, yb = F.conv2d(x64, wa.double(), ba.double(), padding=1), F.conv2d(x64, wb.double(), bb.double(), padding=1)
        (g_a,) = torch.autograd.grad(ya, x64, ga.double(), retain_graph=True)
        gb = F.conv2d(g_a, wb.double(), padding=1)
        gb = (sign * gb * (ga.norm() / gb.norm())).float()
        (g_b,) = torch.autograd.grad(yb, x64, gb.double())
        gram = O.gram(g_a, g_b)
        assert abs(O.cosine(*gram)) >= 0.09 and O.away_from_boundaries(*gram), gram
        assert O.conflicts(*gram) == (sign < 0)
        _REF[sign] = dict(x=x, wa=wa, wb=wb, ba=ba, bb=bb, ga=ga, gb=gb, g_a=g_a, g_b=g_b, gram=gram)
    return _REF[sign]


def _run(dev, r, surgery):
    ops = _ops()
    xd = to_dev_nhwc(r["x"], dev).requires_grad_(True)
    d = [r[k].to(dev).requires_grad_(True) for k in ("wa", "ba", "wb", "bb")]
    oa, ob = ops.dual_head(xd, d[0], d[1], d[2], d[3], pad=1, surgery=surgery)
    torch.autograd.backward([oa, ob], [r["ga"].to(dev), r["gb"].to(dev)])
    torch.cuda.synchronize()
    return oa.detach(), ob.detach(), xd.grad, [t.grad for t in d]


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("sign", [-1, 1], ids=["conflict", "agree"])
@pytest.mark.parametrize("method", O.METHODS)
def test_surgery_node_against_fp64(dev, method, sign):
    from vision_mtl_amd.surgery import GradSurgery

    r = _reference(sign)
    oa0, ob0, dx0, pg0 = _run(dev, r, None)
    s = GradSurgery(method)
    oa, ob, dx, pg = _run(dev, r, s)
    assert torch.equal(_bits(oa), _bits(oa0)) and torch.equal(_bits(ob), _bits(ob0)), "the forward is the plain node's"
    for name, x, y in zip(("wa", "ba", "wb", "bb"), pg, pg0):
        assert torch.equal(_bits(x), _bits(y)), f"d{name} differs from the plain node's"
    assert float(dx[..., CIN:].abs().max()) == 0.0, "pad channels of dx stay zero"

    na, d, nb = r["gram"]
    alpha, beta = O.coefficients(method, na, d, nb)
    ref = (alpha * r["g_a"] + beta * r["g_b"])
    print(f"{method}/{'conflict' if sign < 0 else 'agree'}: cos {O.cosine(na, d, nb):+.4f}, oracle (alpha, beta) = "
          f"({alpha:.6f}, {beta:.6f}), device stats {s.stats.tolist()}")
    assert_close(from_dev_nhwc(dx, CIN), ref, tol=TOL, what=f"surgery dx, {method}")
    if method == "sum":
        assert_close(from_dev_nhwc(dx, CIN), from_dev_nhwc(dx0, CIN), tol=TOL, what="'sum' dx against the plain node's")
        assert_close(from_dev_nhwc(dx0, CIN), r["g_a"] + r["g_b"], tol=TOL, what="plain dx")

    st = [float(v) for v in s.stats.double().cpu()]
    n = r["g_a"].numel()
    ea, eb = (math.sqrt(n) * TOL * float(g.abs().max()) for g in (r["g_a"], r["g_b"]))
    bounds = (2 * math.sqrt(na) * ea + ea * ea, math.sqrt(na) * eb + math.sqrt(nb) * ea + ea * eb,
              2 * math.sqrt(nb) * eb + eb * eb)
    for k, (got, want, bound) in enumerate(zip(st[:3], (na, d, nb), bounds)):
        assert abs(got - want) <= bound + 2.0 ** -24 * abs(want), f"stats[{k}] = {got!r}, fp64 {want!r}, bound {bound:.3e}"
    # the coefficients the node used are the oracle's on ITS Gram values
    da, db = O.coefficients(method, *st[:3])
    assert abs(st[3] - da) <= 2.0 ** -24 * abs(da) and abs(st[4] - db) <= 2.0 ** -24 * abs(db)
    assert s.counters.tolist() == [1, 1 if sign < 0 else 0], "the conflict counter tells which branch ran"
    if method == "pcgrad":
        assert (st[3] > 1.0 and st[4] > 1.0) if sign < 0 else (st[3] == 1.0 and st[4] == 1.0)
    assert float(s.conflict_rate()) == (1.0 if sign < 0 else 0.0)


def test_surgery_node_twice_gives_the_same_bits(dev):
    from vision_mtl_amd.surgery import GradSurgery

    r = _reference(-1)
    s = GradSurgery("pcgrad")
    _, _, dx1, _ = _run(dev, r, s)
    st1 = s.stats.clone()
    _, _, dx2, _ = _run(dev, r, s)
    assert torch.equal(_bits(dx1), _bits(dx2)) and torch.equal(_bits(st1), _bits(s.stats))
    assert s.counters.tolist() == [2, 2]


def test_surgery_node_under_poisoned_buffers(dev):
    """every buffer the node allocates NaN-poisoned and guard-banded: no launch reads what none wrote"""
    from tests import poison
    from vision_mtl_amd.surgery import GradSurgery

    r = _reference(-1)
    _, _, dx0, _ = _run(dev, r, GradSurgery("mgda"))
    with poison.patched("guard"):
        _, _, dx, _ = _run(dev, r, GradSurgery("mgda"))
    assert torch.equal(_bits(dx), _bits(dx0))
