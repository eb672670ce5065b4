"""-m "not gpu": the fp64 oracle of the gradient surgery (tests/surgery_oracle.py) against independent restatements of
each method, its degenerate cases, and the host side of the feature: header prototypes and exported symbols, argument
checks made before a device is touched, the errors of GradSurgery / MTLModule / init_model, the unchanged default
module and the unchanged default signature of ops.dual_head."""
import argparse
import inspect
import math

import pytest
import torch

from tests import surgery_oracle as O

NEW_ENTRY_POINTS = {
    "vmtl_surgery_workspace_bytes": ["rows", "width"],
    "vmtl_surgery_gram": ["a", "lda", "b", "ldb", "rows", "width", "workspace", "stream"],
    "vmtl_surgery_control": ["workspace", "rows", "width", "method", "state", "stream"],
    "vmtl_surgery_combine": ["a", "lda", "b", "ldb", "state", "out", "ldo", "rows", "width", "stream"],
}
X = 0x1000  # a non-null, 16-byte aligned "pointer": the argument checks return before anything dereferences it
SIZES = (1, 2, 17, 1000)


def _pairs():
    for kind in O.KINDS:
        for n in SIZES:
            yield kind, n, O.pair(kind, n)


# ----------------------------------------------------------------------------- the oracle against restatements
def test_test_pairs_are_away_from_every_branch_boundary():
    for kind, n, (a, b) in _pairs():
        na, d, nb = O.gram(a, b)
        assert O.away_from_boundaries(na, d, nb), (kind, n, na, d, nb)
        if kind == "disjoint":
            assert d == 0.0
        elif n >= 17:
            assert (O.cosine(na, d, nb) < -0.09) == (kind == "conflict")


def test_pcgrad_is_the_two_projections_summed():
    seen = set()
    for kind, n, (a, b) in _pairs():
        na, d, nb = O.gram(a, b)
        if O.passes_through(na, d, nb):
            continue
        a64, b64 = a.double(), b.double()
        pa = a64 - (d / nb) * b64 if d < 0 else a64  # Yu et al. 2020, algorithm 1 for two tasks: each gradient is
        pb = b64 - (d / na) * a64 if d < 0 else b64  # projected onto the normal plane of the ORIGINAL other one
        alpha, beta = O.coefficients("pcgrad", na, d, nb)
        ref, got = pa + pb, O.combine(a, b, alpha, beta)
        assert float((got - ref).abs().max()) <= 1e-14 * max(1.0, float(ref.abs().max())), (kind, n)
        if d < 0:
            # after the projection neither conflicts with the other's original any more
            assert abs(float(pa @ b64)) <= 1e-12 * math.sqrt(na * nb) and abs(float(pb @ a64)) <= 1e-12 * math.sqrt(na * nb)
            assert alpha > 1.0 and beta > 1.0
        else:
            assert (alpha, beta) == (1.0, 1.0)
        seen.add(d < 0)
    assert seen == {True, False}


def test_mgda_is_the_min_norm_point_of_the_segment():
    grid = torch.linspace(0.0, 1.0, 200001, dtype=torch.float64)
    clipped = set()
    for kind, n, (a, b) in _pairs():
        na, d, nb = O.gram(a, b)
        if O.passes_through(na, d, nb):
            continue
        alpha, beta = O.coefficients("mgda", na, d, nb)
        assert 0.0 <= alpha <= 1.0 and alpha + beta == pytest.approx(1.0, abs=1e-15)
        norms = grid ** 2 * na + 2.0 * grid * (1.0 - grid) * d + (1.0 - grid) ** 2 * nb  # |g a + (1 - g) b|^2
        best = float(grid[int(norms.argmin())])
        assert abs(alpha - best) <= 5.1e-6, (kind, n, alpha, best)  # half a grid step, and the rounding of the grid
        clipped.add(alpha in (0.0, 1.0))
        if kind == "short" and n > 1:
            assert (alpha, beta) == (0.0, 1.0)  # b = 0.05 a is the min-norm point itself
    assert clipped == {True, False}


def test_imtl_g_projects_equally_onto_both_unit_gradients():
    for kind, n, (a, b) in _pairs():
        na, d, nb = O.gram(a, b)
        if O.passes_through(na, d, nb):
            continue
        alpha, beta = O.coefficients("imtl_g", na, d, nb)
        assert alpha + beta == pytest.approx(1.0, abs=1e-15) and 0.0 < alpha < 1.0
        g = O.combine(a, b, alpha, beta)
        ua, ub = a.double() / math.sqrt(na), b.double() / math.sqrt(nb)
        assert float(g @ ua) == pytest.approx(float(g @ ub), abs=1e-12 * math.sqrt(max(na, nb))), (kind, n)


def test_sum_reports_and_does_nothing():
    a, b = O.pair("conflict", 1000)
    na, d, nb = O.gram(a, b)
    assert O.coefficients("sum", na, d, nb) == (1.0, 1.0)
    assert O.conflicts(na, d, nb) and -1.0 <= O.cosine(na, d, nb) < -0.09
    assert torch.equal(O.combine(a, b, 1.0, 1.0), a.double() + b.double())


def test_degenerate_cases():
    a, b = O.pair("agree", 17)
    zero = torch.zeros(17)
    for x, y in ((zero, b), (a, zero), (zero, zero)):  # a zero gradient: pass-through, cosine 0, no conflict
        g = O.gram(x, y)
        assert O.passes_through(*g) and O.cosine(*g) == 0.0 and not O.conflicts(*g)
        assert all(O.coefficients(m, *g) == (1.0, 1.0) for m in O.METHODS)
    g = O.gram(a, a)  # a == b: cosine 1, MGDA's denominator is 0
    assert g[0] == g[1] == g[2] and O.cosine(*g) == pytest.approx(1.0, abs=1e-15)
    assert O.coefficients("mgda", *g) == (0.5, 0.5) and O.coefficients("imtl_g", *g) == (0.5, 0.5)
    assert O.coefficients("pcgrad", *g) == (1.0, 1.0)
    x, y = O.pair("disjoint", 17)  # exact d == 0: no projection
    g = O.gram(x, y)
    assert g[1] == 0.0 and O.coefficients("pcgrad", *g) == (1.0, 1.0) and not O.conflicts(*g)
    bad = a.clone()
    bad[3] = float("nan")  # a NaN entry: pass-through, so the optimizer's skip_nonfinite still sees it
    g = O.gram(bad, b)
    assert math.isnan(g[0]) and O.passes_through(*g)
    assert all(O.coefficients(m, *g) == (1.0, 1.0) for m in O.METHODS)
    assert bool(torch.isnan(O.combine(bad, b, 1.0, 1.0)[3]))
    inf = a.clone()
    inf[0] = float("inf")
    assert O.passes_through(*O.gram(inf, b))
    with pytest.raises(ValueError):
        O.coefficients("gradnorm", 1.0, 0.0, 1.0)


def test_gram_bound_covers_a_naive_fp64_sum():
    a, b = O.pair("conflict", 1000)
    exact, bound = O.gram(a, b), O.gram_bound(a, b)
    s = [0.0, 0.0, 0.0]
    for x, y in zip(a.double().tolist(), b.double().tolist()):
        s[0] += x * x
        s[1] += x * y
        s[2] += y * y
    assert all(abs(u - v) <= w for u, v, w in zip(s, exact, bound))
    assert all(abs(u - v) <= w for u, v, w in zip(O.gram_fast(a, b), exact, bound))


# ----------------------------------------------------------------------------- the host side
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
    for k, v in ops.SURGERY_METHODS.items():
        assert f"#define VMTL_SURGERY_{k.upper()} {v}" in text
    assert f"#define VMTL_SURGERY_STATE_FLOATS {ops.SURGERY_STATE_FLOATS}" in text
    assert tuple(ops.SURGERY_METHODS) == O.METHODS
    ws = l.raw("vmtl_surgery_workspace_bytes")  # host only: three doubles per workgroup, 1024 floats per workgroup
    assert [ws(1, 1), ws(1, 1024), ws(1, 1025), ws(3, 16), ws(32 * 128 * 256, 16)] == [24, 24, 48, 24, 24 * 1024]
    assert ws(0, 4) == 0 and ws(4, 0) == 0 and ws(-1, 4) == 0 and ws(1 << 40, 1 << 40) == 0


def test_entry_points_check_their_arguments_before_touching_a_device():
    from vision_mtl_amd._lib import lib

    l = lib()
    gram, ctl, comb = l.raw("vmtl_surgery_gram"), l.raw("vmtl_surgery_control"), l.raw("vmtl_surgery_combine")
    assert gram(None, 4, X, 4, 1, 4, X, None) == -1 and gram(X, 4, None, 4, 1, 4, X, None) == -1
    assert gram(X, 4, X, 4, 1, 4, None, None) == -1 and gram(X, 4, X, 4, 1, 4, X + 4, None) == -1  # workspace
    assert gram(X + 2, 4, X, 4, 1, 4, X, None) == -1                                            # 4-byte alignment
    assert gram(X, 3, X, 4, 2, 4, X, None) == -1 and gram(X, 4, X, 3, 2, 4, X, None) == -1        # ld < width
    assert gram(X, 4, X, 4, 0, 4, X, None) == -1 and gram(X, 4, X, 4, 1, 0, X, None) == -1
    assert gram(X, 1 << 40, X, 1 << 40, 1 << 40, 1 << 40, X, None) == -1                          # rows * width
    for method in (-1, 4):  # an unknown method: unsupported, before anything else is looked at
        assert ctl(None, 1, 4, method, None, None) == -3
    assert ctl(None, 1, 4, 0, X, None) == -1 and ctl(X, 1, 4, 0, None, None) == -1
    assert ctl(X + 4, 1, 4, 0, X, None) == -1 and ctl(X, 1, 4, 0, X + 4, None) == -1
    assert ctl(X, 0, 4, 0, X, None) == -1 and ctl(X, 1, 0, 0, X, None) == -1
    assert comb(None, 4, X, 4, X, X, 4, 1, 4, None) == -1 and comb(X, 4, None, 4, X, X, 4, 1, 4, None) == -1
    assert comb(X, 4, X, 4, None, X, 4, 1, 4, None) == -1 and comb(X, 4, X, 4, X, None, 4, 1, 4, None) == -1
    assert comb(X, 4, X, 4, X + 4, X, 4, 1, 4, None) == -1                                     # state 8-byte aligned
    assert comb(X, 4, X, 4, X, X + 1, 4, 1, 4, None) == -1 and comb(X, 4, X, 4, X, X, 3, 2, 4, None) == -1
    # out overlapping an operand other than "out is a, same leading dimension" races between threads: refused
    S, A, B_, FAR = 0x9000, 0x1000, 0x1000 + 64, 0x5000  # state; an interleaved map of 8 rows [16 | 16] at A; elsewhere
    assert comb(A, 32, B_, 32, S, B_, 32, 8, 16, None) == -1         # out is b
    assert comb(A, 32, B_, 32, S, A, 16, 8, 16, None) == -1          # out is a, another leading dimension
    assert comb(A, 32, B_, 32, S, A + 32, 32, 8, 16, None) == -1     # out inside a's rows at another offset, meeting b's lanes
    assert comb(A, 32, FAR, 16, S, A + 4, 32, 8, 16, None) == -1     # out shifted by one float against a
    assert comb(A, 16, FAR, 16, S, FAR + 8, 16, 8, 16, None) == -1   # out inside b's dense range
    assert comb(A, 16, FAR, 16, S, A + 4 * 16, 16, 1, 32, None) == -1  # one row: out starts inside a


def test_grad_surgery_object():
    from vision_mtl_amd.surgery import METHODS, GradSurgery, resolve

    assert METHODS == O.METHODS
    for bad in ("gradnorm", "PCGrad", "", None, 1):
        with pytest.raises(ValueError, match="method"):
            GradSurgery(bad)
    s = GradSurgery("pcgrad")
    assert not isinstance(s, torch.nn.Module) and s.method == "pcgrad"
    with pytest.raises(RuntimeError, match="no backward pass"):
        s.stats
    s.reset_counters()  # nothing to clear yet: not an error
    assert resolve(None) is None and resolve(s) is s and resolve("mgda").method == "mgda"
    with pytest.raises(ValueError):
        resolve(3)
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.combine_flat(x, x.clone())


def test_ops_reject_cpu_tensors_and_bad_methods():
    from vision_mtl_amd import ops

    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.surgery_gram(x, x.clone(), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.surgery_control(torch.zeros(3, dtype=torch.float64), x, "sum", 1, 8)
    with pytest.raises(ValueError, match="method"):
        ops.surgery_method("cagrad")


def test_dual_head_default_signature_is_unchanged():
    from vision_mtl_amd import ops

    ps = list(inspect.signature(ops.dual_head).parameters.values())
    assert [p.name for p in ps] == ["x", "wa", "ba", "wb", "bb", "pad", "surgery"]
    assert ps[5].default == 1 and ps[6].default is None
    assert all(p.default is inspect.Parameter.empty for p in ps[:5])


def _init(name, **kw):
    from vision_mtl_amd.utils.pipeline_utils import init_model

    return init_model(argparse.Namespace(model_name=name, backbone_weights=None, **kw), argparse.Namespace(num_classes=5))


def test_module_surface():
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.surgery import GradSurgery

    plain = _init("basic")
    assert "grad_surgery" not in plain.hparams and plain.grad_surgery is None and plain.model.grad_surgery is None
    keys = list(plain.state_dict())
    m = _init("basic", grad_surgery="pcgrad")
    assert isinstance(m.grad_surgery, GradSurgery) and m.grad_surgery is m.model.grad_surgery
    assert m.hparams["grad_surgery"] == "pcgrad" and m.grad_surgery.method == "pcgrad"
    assert list(m.state_dict()) == keys and len(list(m.parameters())) == len(list(plain.parameters()))
    assert set(m.hparams) == set(plain.hparams) | {"grad_surgery"}
    own = GradSurgery("mgda")
    m2 = MTLModule(plain.model, num_classes=5, grad_surgery=own)
    assert m2.grad_surgery is own and plain.model.grad_surgery is own
    m2.grad_surgery = None  # an attribute, like train_augment
    assert plain.model.grad_surgery is None
    # combines with what acts on the losses
    both = _init("basic", grad_surgery="imtl_g", loss_balancing="uncertainty", segm_ohem_min_kept=100, depth_grad_weight=0.5)
    assert both.grad_surgery.method == "imtl_g" and both.task_balancer.method == "uncertainty"


def test_models_without_one_shared_representation_are_refused():
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils import pipeline_utils

    built = []
    orig = pipeline_utils.build_model
    pipeline_utils.build_model = lambda *a, **k: built.append(1) or orig(*a, **k)
    try:
        for name in ("csnet", "mtan"):
            with pytest.raises(ValueError, match="grad_surgery"):
                _init(name, grad_surgery="pcgrad")
        with pytest.raises(ValueError, match="method"):
            _init("basic", grad_surgery="gradnorm")
        assert not built, "the arguments are checked before the networks are built"
        mtan = _init("mtan")
    finally:
        pipeline_utils.build_model = orig
    assert "grad_surgery" not in mtan.hparams and mtan.grad_surgery is None
    for kw in (dict(grad_surgery="mgda"),):
        with pytest.raises(ValueError, match="grad_surgery"):
            MTLModule(mtan.model, num_classes=5, **kw)
        with pytest.raises(ValueError, match="grad_surgery"):
            MTLModule(torch.nn.Linear(1, 1), num_classes=5, **kw)
    with pytest.raises(ValueError, match="grad_surgery"):
        mtan.grad_surgery = "sum"
    with pytest.raises(ValueError, match="method"):
        MTLModule(torch.nn.Linear(1, 1), num_classes=5, grad_surgery="cagrad")
