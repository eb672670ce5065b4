"""csrc/surgery.hip (vmtl_surgery_gram / _control / _combine) against the fp64 oracle of tests/surgery_oracle.py.

Grid: one workgroup of 256 threads per 1024 floats of rows * width, at most 1024 workgroups, for the float4 body AND the
scalar fall-back (vmtl_surgery_control must know the number of partials without knowing which of the two ran).

Shapes (rows, width, lda): a lone element; the interleaved [rows][g_a | g_b] map of the training step (lda = 2 * width)
at 3 rows, on both sides of a workgroup-count edge (255 * 16 = 4080 floats, 4 workgroups; 257 * 16 = 4112, 5) and at
width 4; two separate maps with pad lanes whose width is no multiple of 4 (the scalar fall-back); a flat pair one short
of a vector multiple; and a flat pair of 4096 * 256 + 9 floats: 1024 workgroups * 256 threads * 4 floats = 4096 * 256,
so the first threads take a second float4 (the loop issues two float4 pairs per trip) and one or two floats are left
for the tail - aligned: head 0, 262146 float4, tail 1; on buf[1:]: head 3, 262145 float4, tail 2.  Every shape runs on
a 16-byte-aligned payload and on buf[1:]: dense rows are walked as one row, whose head is peeled; rows with a gap
take the scalar fall-back there.

Every device buffer - operands, outputs, workspace, state block - is the payload of a guard-banded, NaN-poisoned
allocation of tests/poison.py, and every launch runs under tests/launch_guard.py.  Pad lanes of separate maps hold the
poison: a read of one turns the Gram matrix into NaN.

Bounds (derived, not measured):
  Gram          |device - oracle| <= rows * width * 2^-53 * sum |x_i y_i| (products of fp32 values are exact in fp64; a
                sum of n terms in any order) + one fp32 rounding of the value the state block stores
  coefficients  within one fp32 rounding (2^-24 relative) of the oracle evaluated on the DEVICE's Gram values; exactly 1
                where the method returns 1
  combine       |out - exact| <= 2^-22 * (|alpha a_i| + |beta b_i|) per element, alpha and beta the fp32 values read back
                (the bound of two fp32 roundings with 2x head-room; the kernel evaluates in fp64 and rounds once)
Everything else is bit equality."""
import math

import pytest
import torch

from tests import launch_guard, poison
from tests import surgery_oracle as O

pytestmark = pytest.mark.gpu

BIG = 4096 * 256 + 9
SHAPES = [(1, 1, 1), (3, 16, 32), (255, 16, 32), (257, 16, 32), (5, 4, 8), (7, 3, 5), (1, 1023, 1023), (1, BIG, BIG)]
OFFS = [0, 1]
U32 = 2.0 ** -24


def _ops():
    from vision_mtl_amd import ops

    return ops


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


class _Bufs:
    """Guard-banded device buffers; close() checks the guards and the skipped elements in front of misaligned payloads."""

    def __init__(self, dev):
        self.P = poison.Poison("guard")
        self.like = torch.empty(0, device=dev)
        self.fronts = []

    def f32(self, n, off=0):
        base = self.P.empty(n + off, self.like)
        if off:
            self.fronts.append(base[:off])
        return base[off:]

    def state(self):
        t = self.f32(_ops().SURGERY_STATE_FLOATS)
        t.zero_()
        return t

    def workspace(self, rows, width):
        nbytes = _ops().lib().raw("vmtl_surgery_workspace_bytes")(rows, width)
        return self.P.empty(nbytes // 4, self.like).view(torch.float64)

    def close(self):
        for f in self.fronts:
            assert bool(poison.is_sentinel(f).all()), "an element in front of a misaligned payload was written"
        self.P.close()


def _operands(B, shape, off, a_cpu, b_cpu):
    """(a, b) as [rows][width] device views with row stride lda: the two halves of ONE interleaved map when
    lda == 2 * width, else two maps of their own whose pad lanes [width, lda) keep the poison."""
    rows, width, lda = shape
    if lda == 2 * width:
        m = B.f32(rows * lda, off).view(rows, lda)
        a, b = m[:, :width], m[:, width:]
    else:
        a = B.f32(rows * lda, off).view(rows, lda)[:, :width]
        b = B.f32(rows * lda, off).view(rows, lda)[:, :width]
    a.copy_(a_cpu.view(rows, width))
    b.copy_(b_cpu.view(rows, width))
    return a, b


def _kw(shape, ldo=None):
    rows, width, lda = shape
    kw = dict(rows=rows, width=width, lda=lda, ldb=lda)
    if ldo is not None:
        kw["ldo"] = ldo
    return kw


_CASES = {}


def _case(shape, kind):
    """inputs and oracle values of one (shape, kind), computed once"""
    key = (shape, kind)
    if key not in _CASES:
        rows, width, _ = shape
        n = rows * width
        a, b = O.pair(kind, n)
        gram = (O.gram if n <= 100000 else O.gram_fast)(a, b)
        assert O.away_from_boundaries(*gram), (shape, kind, gram)
        _CASES[key] = (a, b, gram, O.gram_bound(a, b))
    return _CASES[key]


def _check_coefficients(method, st, what):
    """the state block's coefficients and cosine against the oracle evaluated on the block's own Gram values"""
    na, d, nb, alpha, beta, cos = (float(x) for x in st[:6].double().cpu())
    ra, rb = O.coefficients(method, na, d, nb)
    for got, ref, name in ((alpha, ra, "alpha"), (beta, rb, "beta")):
        if ref == 1.0:
            assert got == 1.0, f"{what}: {name} = {got!r} where {method} returns exactly 1"
        else:
            assert abs(got - ref) <= U32 * abs(ref), f"{what}: {name} = {got!r}, oracle {ref!r}"
    rc = O.cosine(na, d, nb)
    assert abs(cos - rc) <= U32 * abs(rc), f"{what}: cosine {cos!r}, oracle {rc!r}"
    return alpha, beta


def _run(dev, shape, off, kinds=O.KINDS):
    """gram + (control + combine per method) per kind, everything checked against the oracle; returns the bits of every
    result for the run-to-run comparison"""
    ops = _ops()
    rows, width, lda = shape
    n = rows * width
    out_bits = []
    B = _Bufs(dev)
    with launch_guard.patched():
        for kind in kinds:
            a_cpu, b_cpu, gram, bound = _case(shape, kind)
            a, b = _operands(B, shape, off, a_cpu, b_cpu)
            ws = B.workspace(rows, width)
            ops.surgery_gram(a, b, ws, **_kw(shape))
            assert torch.equal(_bits(a), _bits(a_cpu.view(rows, width))) and torch.equal(_bits(b), _bits(b_cpu.view(rows, width)))
            out_bits.append(ws.view(torch.int32).cpu())
            part = ws.cpu().view(-1, 3)
            assert part.shape[0] == min(1024, (n + 1023) // 1024) and not bool(torch.isnan(part).any())
            for k in range(3):  # the partials, summed exactly on the host
                got = math.fsum(part[:, k].tolist())
                assert abs(got - gram[k]) <= bound[k], f"{shape} off {off} {kind}: Gram[{k}] {got!r} vs {gram[k]!r}"
            for method in O.METHODS:
                what = f"{shape} off {off} {kind} {method}"
                state = B.state()
                ops.surgery_control(ws, state, method, rows, width)
                st = state.clone()
                out_bits.append(_bits(st))
                for k in range(3):  # what the block stores: the fp64 sum rounded once
                    assert abs(float(st[k]) - gram[k]) <= bound[k] + U32 * abs(gram[k]), f"{what}: state[{k}]"
                alpha, beta = _check_coefficients(method, st, what)
                ra, rb = O.coefficients(method, *gram)  # the branch the exact Gram matrix takes is the one that ran
                assert (alpha == 1.0) == (ra == 1.0) and (alpha in (0.0, 1.0)) == (ra in (0.0, 1.0)), what
                counters = ops.surgery_counters(state).tolist()
                assert counters == [1, int(O.conflicts(*gram))], f"{what}: counters {counters}"
                # separate output, with pad lanes when the operands have them
                ldo = width if lda == 2 * width else lda
                out = B.f32(rows * ldo, off).view(rows, ldo)
                ops.surgery_combine(a, b, state, out[:, :width], **_kw(shape, ldo))
                got = out[:, :width].double().cpu().reshape(-1)
                exact = alpha * a_cpu.double() + beta * b_cpu.double()
                tol = 2.0 ** -22 * ((alpha * a_cpu.double()).abs() + (beta * b_cpu.double()).abs())
                err = (got - exact).abs()
                assert bool((err <= tol).all()), f"{what}: combine off by {float((err - tol).max()):.3e} over its bound"
                if ldo > width:
                    assert bool(poison.is_sentinel(out[:, width:]).all()), f"{what}: pad lanes of out are left alone"
                if method == "sum":
                    assert torch.equal(_bits(out[:, :width]), _bits((a_cpu + b_cpu).view(rows, width))), \
                        f"{what}: alpha = beta = 1 is the fp32 sum"
                out_bits.append(_bits(out[:, :width]))
                # aliased: out is a.  Same bits; b (the pad lanes of a's rows in the interleaved layout) keeps its own
                a2, b2 = _operands(B, shape, off, a_cpu, b_cpu)
                ops.surgery_combine(a2, b2, state, a2, **_kw(shape, lda))
                assert torch.equal(_bits(a2), _bits(out[:, :width])), f"{what}: the aliased form differs from the separate one"
                assert torch.equal(_bits(b2), _bits(b_cpu.view(rows, width))), f"{what}: the aliased form wrote b"
                assert torch.equal(_bits(state), _bits(st)), f"{what}: combine wrote the state block"
    B.close()
    return out_bits


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_oracle_and_are_deterministic(dev, shape, off):
    first = _run(dev, shape, off)
    second = _run(dev, shape, off)
    assert len(first) == len(second)
    for i, (x, y) in enumerate(zip(first, second)):
        assert torch.equal(x, y), f"two runs differ in result {i}"


def test_padded_output_of_the_interleaved_map(dev):
    """ldo > width with the interleaved operands: the float4 body with three different leading dimensions"""
    ops = _ops()
    shape = (33, 16, 32)
    a_cpu, b_cpu, gram, _ = _case(shape, "conflict")
    B = _Bufs(dev)
    with launch_guard.patched():
        a, b = _operands(B, shape, 0, a_cpu, b_cpu)
        ws, state = B.workspace(33, 16), B.state()
        ops.surgery_gram(a, b, ws, **_kw(shape))
        ops.surgery_control(ws, state, "pcgrad", 33, 16)
        dense, padded = B.f32(33 * 16).view(33, 16), B.f32(33 * 20).view(33, 20)
        ops.surgery_combine(a, b, state, dense, **_kw(shape, 16))
        ops.surgery_combine(a, b, state, padded[:, :16], **_kw(shape, 20))
    assert torch.equal(_bits(padded[:, :16]), _bits(dense)) and bool(poison.is_sentinel(padded[:, 16:]).all())
    assert float(state[3]) > 1.0 and float(state[4]) > 1.0
    B.close()


def test_counters_follow_a_known_conflict_pattern(dev):
    ops = _ops()
    shape = (3, 16, 32)
    B = _Bufs(dev)
    state = B.state()
    with launch_guard.patched():
        for i, kind in enumerate(("conflict", "agree", "conflict")):
            a_cpu, b_cpu, gram, _ = _case(shape, kind)
            a, b = _operands(B, shape, 0, a_cpu, b_cpu)
            ws = B.workspace(3, 16)
            ops.surgery_gram(a, b, ws, **_kw(shape))
            ops.surgery_control(ws, state, "pcgrad", 3, 16)
            assert (float(state[3]) > 1.0) == (kind == "conflict")
    c = ops.surgery_counters(state)
    assert c.dtype == torch.int64 and c.is_cuda and c.tolist() == [3, 2]
    assert float(state[6]) == 0.0 and float(state[7]) == 0.0
    B.close()


@pytest.mark.parametrize("method", O.METHODS)
def test_degenerate_pairs_on_the_device(dev, method):
    """zero gradient, a NaN entry, an inf entry: alpha = beta = 1, cosine 0, no conflict counted, the sum passes through;
    a == b: cosine 1 and MGDA's zero denominator; disjoint supports: d == 0 exactly and no projection"""
    ops = _ops()
    n = 1023
    a_cpu, b_cpu = O.pair("conflict", n)
    bad, inf = a_cpu.clone(), a_cpu.clone()
    bad[n // 2], inf[5] = float("nan"), float("inf")
    da, db = O.pair("disjoint", n)
    cases = [("zero a", torch.zeros(n), b_cpu), ("zero b", a_cpu, torch.zeros(n)), ("nan", bad, b_cpu), ("inf", inf, b_cpu),
             ("equal", a_cpu, a_cpu.clone()), ("disjoint", da, db)]
    B = _Bufs(dev)
    with launch_guard.patched():
        for name, x, y in cases:
            a, b = B.f32(n), B.f32(n)
            a.copy_(x)
            b.copy_(y)
            ws, state = B.workspace(1, n), B.state()
            ops.surgery_gram(a, b, ws)
            ops.surgery_control(ws, state, method, 1, n)
            out = ops.surgery_combine(a, b, state, B.f32(n))
            st = [float(v) for v in state[:6].cpu()]
            counters = ops.surgery_counters(state).tolist()
            if name in ("zero a", "zero b", "nan", "inf"):
                assert st[3:] == [1.0, 1.0, 0.0] and counters == [1, 0], (name, st, counters)
                got, ref = out.cpu(), x + y  # NaN and inf reach the trunk as they would have
                assert torch.equal(torch.isnan(got), torch.isnan(ref)), name
                assert torch.equal(_bits(torch.nan_to_num(got, nan=0.0)), _bits(torch.nan_to_num(ref, nan=0.0))), name
            elif name == "equal":
                assert st[0] == st[1] == st[2] and st[5] == 1.0 and counters == [1, 0]
                assert st[3:5] == {"sum": [1.0, 1.0], "pcgrad": [1.0, 1.0], "mgda": [0.5, 0.5], "imtl_g": [0.5, 0.5]}[method]
            else:
                assert st[1] == 0.0 and st[5] == 0.0 and counters == [1, 0]
                _check_coefficients(method, state, name)
                if method in ("sum", "pcgrad"):
                    assert st[3:5] == [1.0, 1.0]
    B.close()


def test_unknown_method_is_refused_without_a_launch(dev):
    ops = _ops()
    B = _Bufs(dev)
    ws, state = B.workspace(1, 8), B.state()
    ws.zero_()
    for method in (-1, 4):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            ops.lib().callk("vmtl_surgery_control", workspace=ws, rows=1, width=8, method=method, state=state,
                            stream=torch.cuda.current_stream().cuda_stream)
    with pytest.raises(ValueError, match="method"):
        ops.surgery_control(ws, state, "gradnorm", 1, 8)
    assert float(state.abs().sum()) == 0.0 and ops.surgery_counters(state).tolist() == [0, 0]
    B.close()


def test_grad_surgery_object_on_flat_buffers(dev):
    """GradSurgery.combine_flat: lazily allocated buffers, the views, conflict_rate() and reset_counters()"""
    from vision_mtl_amd.surgery import GradSurgery

    s = GradSurgery("pcgrad")
    for kind in ("conflict", "agree", "conflict", "conflict"):
        a_cpu, b_cpu = O.pair(kind, 1023)
        out = s.combine_flat(a_cpu.to(dev), b_cpu.to(dev))
        alpha, beta = (float(v) for v in s.coefficients.cpu())
        assert s.stats.shape == (6,) and s.stats.is_cuda and s.cosine.dim() == 0
        tol = 2.0 ** -22 * ((alpha * a_cpu.double()).abs() + (beta * b_cpu.double()).abs())
        assert bool(((out.double().cpu() - O.combine(a_cpu, b_cpu, alpha, beta)).abs() <= tol).all())
    rate = s.conflict_rate()
    assert rate.is_cuda and rate.dim() == 0 and float(rate) == 0.75 and s.counters.tolist() == [4, 3]
    s.reset_counters()
    assert s.counters.tolist() == [0, 0] and float(s.stats[3]) > 1.0  # the last coefficients stay
