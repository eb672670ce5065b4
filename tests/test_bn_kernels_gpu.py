"""Every entry point of csrc/bn.hip called DIRECTLY through the C ABI and compared, element by element, with the fp64
oracle of tests/bn_oracle.py (rounding bounds derived there, none fitted): the stand-alone statistics, statistics from
given rows, the row contract (rows wholly past M may hold anything), the eval statistics in their three forms, apply,
fused apply with 1..64 rows, the backward in one call and in its halves, the pooled node, and the column sums - at the
edges of the sweep geometry of csrc/reduce.h (GEOMETRY below; tests/test_bn_oracle_cpu.py asserts what each row reaches).

Every buffer a kernel sees - operands included - is a tests/poison.py "guard" buffer: outputs start as NaN, so an
element no kernel wrote fails its comparison (a NaN counts as an infinite ratio), and every buffer sits between two
guard bands that must be intact when the case ends.  Every launch goes through lib().callk, which raises on a status
other than 0.  Pad lanes of the operands hold finite junk: a pad channel read as data shows in a result.

No element is left out of any comparison: the inputs are nudged away from the activation kinks and the oracle asserts
the conditions that make this sound (bn_oracle.check_inputs, check_pool_gap).  Statistics use the project's bars:
mean 1e-5 * max|mean| + 1e-6 (test_conv2d_fwd_bwd), variance 1e-4 * max var; the variance recovered from save_invstd adds
2u (var + eps) for the fp32 invstd; results of an fp64 merge of GIVEN rows must be within 1 ulp (2u relative) and 4u.

Not covered: the grid cap of sweep_blocks (8192 blocks) - it needs more than 10^8 elements at every channel count.

Each check prints `bn-ratio <family> <route> <result> <worst error / bound>`; profiles/bn_kernel_tests/README.md holds the
figures of one run."""
import functools
import struct
from collections import namedtuple

import pytest
import torch

from tests import bn_oracle as O
from tests import poison
from tests.util import ceil4

pytestmark = pytest.mark.gpu

EPS = 1e-5
GEOMETRY = ((1, 3), (17, 4), (231, 33), (35, 1024), (40, 1025), (18, 1072), (16400, 20), (4099, 20))
FULL = ((231, 33), (40, 1025))                       # the shapes that run every combination
REST = tuple(g for g in GEOMETRY if g not in FULL)   # one combination each
GATES = ("none", "mul", "res", "mul+res")
NBLK = (1, 2, 16, 17, 64)
POOL_SHAPES = ((1, 2, 2, 3), (2, 6, 10, 33), (1, 4, 4, 1025))
LARGE_MEAN = (524288, 4)  # 512 rows per block, two rows per lane, 255 Chan merges per block
GIVEN_ROWS = ((7, 38), (64, 323), (1000, 5003))  # (pixels per row, M): five full rows and a ragged one
ACT_NAMES = tuple(O.ACTS)


def _lib():
    from vision_mtl_amd._lib import lib

    return lib()


def K(name, **kw):
    _lib().callk(name, stream=torch.cuda.current_stream().cuda_stream, **kw)


class Bufs:
    """guard-banded device buffers: operands (filled from CPU tensors) and poisoned outputs; close() checks the guards"""

    def __init__(self, dev):
        self.p = poison.Poison("guard")
        self.like = torch.empty(0, device=dev)

    def put(self, t):
        if t is None:
            return None
        d = self.p.empty(tuple(t.shape), self.like)
        d.copy_(t)
        return d

    def out(self, *shape):
        return self.p.empty(shape, self.like)

    def i64(self, value):
        t = self.p.empty(2, self.like).view(torch.int64)
        t.fill_(value)
        return t

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            self.p.close()
        else:
            self.p.bases = []


def check(family, route, what, got, ref, bound):
    r = O.worst_ratio(got.detach().cpu(), ref, bound)
    print(f"bn-ratio {family} {route} {what} {r:.3f}")
    assert r <= 1.0, f"{family} {route} {what}: worst error / bound = {r:.3g}"
    return r


# ------------------------------------------------------------------------------------------------ operands
Operands = namedtuple("Operands", "x dy mul res gam beta mean invstd")


@functools.lru_cache(maxsize=None)
def operands(M, C, seed=0, scale=1.5):
    """fp32 CPU operands [M][Cs] / [Cs]; the pad lanes hold finite junk; every third gamma is negative"""
    Cs = ceil4(C)
    g = torch.Generator().manual_seed(7919 * (M % 100003) + 31 * C + seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(M, Cs) * scale + 0.3
    gam = (torch.rand(Cs, generator=g) + 0.5) * torch.where(torch.arange(Cs) % 3 == 1, -1.0, 1.0)
    return Operands(x, rnd(M, Cs), rnd(M, Cs), rnd(M, Cs), gam, rnd(Cs) * 0.5, rnd(Cs) * 0.5 + 0.3,
                    torch.rand(Cs, generator=g) * 0.8 + 0.4)


def _params(T, affine, bn):
    mean, invstd = (T.mean, T.invstd) if bn else (None, None)
    gam, beta = (T.gam, T.beta) if affine and bn else (None, None)
    return mean, invstd, gam, beta


# ------------------------------------------------------------------------------------------------ statistics
def mean_bar(mean):
    return 1e-5 * float(mean.abs().max()) + 1e-6


def var_bar(var):
    return 1e-4 * float(var.max())


def recovered_var(invstd, C):
    is_ = invstd.detach().cpu().double()[:C]
    return 1.0 / (is_ * is_) - O.f32(EPS)


@functools.lru_cache(maxsize=None)
def stats_case(M, C, large_mean=False):
    Cs = ceil4(C)
    if large_mean:
        g = torch.Generator().manual_seed(M + C)
        x = 300.0 + 0.05 * torch.randn(M, Cs, generator=g)
    else:
        x = operands(M, C).x * (torch.arange(Cs) % 5 + 1).float()  # channel scales 1..5
    mean, var = O.exact_stats(x, C)
    return x, mean, var


def check_stats(family, route, mean, var, M, C, save_mean, save_invstd, rm=None, rv=None, old=None, momentum=None):
    """save_mean / the variance recovered from save_invstd / the running buffers against the project's bars"""
    Cs = mean.shape[0]
    bm, bv = mean_bar(mean), var_bar(var)
    ones = torch.ones(C, dtype=torch.float64)
    check(family, route, "save_mean", save_mean[:C], mean[:C], bm * ones)
    check(family, route, "var-from-invstd", recovered_var(save_invstd, C), var[:C], bv + 2 * O.U * (var[:C] + O.f32(EPS)))
    if Cs > C:
        assert float(save_mean[C:].abs().max()) == 0.0 and float(save_invstd[C:].abs().max()) == 0.0, "pad statistics"
    if rm is not None:
        rm_ref, rv_ref = O.running(old[0], old[1], mean, var, M, momentum)
        mom = O.f32(momentum)
        check(family, route, "running_mean", rm, rm_ref, mom * bm + O.U * rm_ref.abs())
        check(family, route, "running_var", rv, rv_ref, mom * bv * (M / (M - 1) if M > 1 else 1.0) + O.U * rv_ref.abs())


def check_coefs(family, route, mean, var, C, gam, beta, save_mean, save_invstd, coef_a, coef_c):
    """coef_a / coef_c: their rounding bound from the kernel's OWN save_mean / save_invstd (tight), and against the
    exact statistics with the statistics bars carried through"""
    sc, cc, ba, bc = O.coefficients(save_mean.cpu(), save_invstd.cpu(), gam, beta, C)
    check(family, route, "coef_a|own-stats", coef_a, sc, ba)
    check(family, route, "coef_c|own-stats", coef_c, cc, bc)
    Cs = mean.shape[0]
    is_ = O.invstd_of(var, EPS, C)
    sc, cc, ba, bc = O.coefficients(mean, is_, gam, beta, C)
    g = O._vec(gam, Cs, 1).abs() * O.lanes(C, Cs)
    # (var + eps)^(-1/2) is convex and decreasing: a variance off by the bar moves it most on the low side; + its rounding
    low = (var + O.f32(EPS) - var_bar(var)).clamp_min(1e-300)
    d_is = (1.0 / low.sqrt() - 1.0 / (var + O.f32(EPS)).sqrt()) * O.lanes(C, Cs) + O.U * is_
    d_sc = g * d_is
    check(family, route, "coef_a", coef_a, sc, ba + d_sc)
    check(family, route, "coef_c", coef_c, cc, bc + mean_bar(mean) * (sc.abs() + d_sc) + mean.abs() * d_sc)


@pytest.mark.parametrize("M,C", GEOMETRY + (LARGE_MEAN,))
def test_standalone_statistics(dev, M, C):
    """vmtl_bn_stats and vmtl_bn_stats_coef sweeping x themselves: momentum 0.1 and 1.0, null running buffers, a null
    num_batches_tracked, null gamma / beta.  The last case: values near 300 with a standard deviation of 0.05."""
    large = (M, C) == LARGE_MEAN
    x, mean, var = stats_case(M, C, large)
    Cs = ceil4(C)
    T = operands(min(M, 64), C)
    if large:
        assert 299.9 < float(mean[:C].min()) and float(var.max()) < 3e-3  # what this case is about
    rows = _lib().raw("vmtl_reduce_rows")(M)
    assert rows == O.red_blocks(M)
    old = (T.mean[:C].clone(), T.invstd[:C].clone())
    with Bufs(dev) as B:
        xd = B.put(x)
        # 1: plain statistics, momentum 0.1
        sm, si, rm, rv, nbt = B.out(Cs), B.out(Cs), B.put(old[0]), B.put(old[1]), B.i64(41)
        K("vmtl_bn_stats", x=xd, M=M, C=C, Cs=Cs, partial=B.out(rows, 2, Cs), nblk_from_conv=0, rows_per_blk_from_conv=0,
          eps=EPS, momentum=0.1, running_mean=rm, running_var=rv, num_batches_tracked=nbt, save_mean=sm, save_invstd=si)
        check_stats("stats", "sweep", mean, var, M, C, sm, si, rm, rv, old, 0.1)
        assert nbt.tolist() == [42]
        # 2: with coefficients, momentum 1.0
        sm2, si2, rm, rv, nbt = B.out(Cs), B.out(Cs), B.put(old[0]), B.put(old[1]), B.i64(-1)
        ca, cc = B.out(Cs), B.out(Cs)
        K("vmtl_bn_stats_coef", x=xd, M=M, C=C, Cs=Cs, partial=B.out(rows, 2, Cs), nblk_from_conv=0,
          rows_per_blk_from_conv=0, eps=EPS, momentum=1.0, running_mean=rm, running_var=rv, num_batches_tracked=nbt,
          save_mean=sm2, save_invstd=si2, gamma=B.put(T.gam), beta=B.put(T.beta), coef_a=ca, coef_c=cc)
        check_stats("stats", "sweep+coef", mean, var, M, C, sm2, si2, rm, rv, old, 1.0)
        check_coefs("stats", "sweep+coef", mean, var, C, T.gam, T.beta, sm2, si2, ca, cc)
        assert nbt.tolist() == [0] and torch.equal(sm, sm2) and torch.equal(si, si2)
        # 3: null gamma / beta, null running buffers, null num_batches_tracked
        sm3, si3, ca, cc = B.out(Cs), B.out(Cs), B.out(Cs), B.out(Cs)
        K("vmtl_bn_stats_coef", x=xd, M=M, C=C, Cs=Cs, partial=B.out(rows, 2, Cs), nblk_from_conv=0,
          rows_per_blk_from_conv=0, eps=EPS, momentum=0.1, running_mean=None, running_var=None, num_batches_tracked=None,
          save_mean=sm3, save_invstd=si3, gamma=None, beta=None, coef_a=ca, coef_c=cc)
        check_coefs("stats", "sweep+coef-null-affine", mean, var, C, None, None, sm3, si3, ca, cc)
        assert torch.equal(sm, sm3) and torch.equal(si, si3)


@functools.lru_cache(maxsize=None)
def rows_case(rpb, M, C, nblk=None):
    """fp32 rows [nblk][2][Cs] of an input (built by the oracle, rounded), their counts and their exact fp64 merge"""
    x = operands(M, C).x
    m, m2, cnt = O.partial_rows(x, rpb, nblk)
    rows = O.rows_tensor(m, m2)
    mean, var = O.merge_rows(rows, cnt, C)
    return x, rows, cnt, mean, var


def check_merged(family, route, mean, var, M, C, save_mean, save_invstd, rm=None, rv=None, old=None, momentum=None):
    """both sides merged the same fp32 rows in fp64: 1 ulp, and 4u on the recovered variance"""
    check(family, route, "save_mean", save_mean, mean, 2 * O.U * mean.abs())
    check(family, route, "var-from-invstd", recovered_var(save_invstd, C), var[:C], 4 * O.U * (var[:C] + O.f32(EPS)))
    assert float(save_invstd[C:].abs().sum()) == 0.0
    if rm is not None:
        rm_ref, rv_ref = O.running(old[0], old[1], mean, var, M, momentum)
        check(family, route, "running_mean", rm, rm_ref, 2 * O.U * rm_ref.abs() + O.f32(momentum) * 2 * O.U * mean[:C].abs())
        check(family, route, "running_var", rv, rv_ref, 2 * O.U * rv_ref.abs())


@pytest.mark.parametrize("rpb,M", GIVEN_ROWS)
def test_statistics_from_given_rows(dev, rpb, M):
    """nblk_from_conv > 0: row blocks of 7, 64 and 1000 pixels with a ragged last row, against the exact fp64 merge."""
    C = 33
    Cs = ceil4(C)
    _, rows, cnt, mean, var = rows_case(rpb, M, C)
    assert cnt[-1] not in (0, rpb) and len(cnt) == 6
    T = operands(M, C)
    old = (T.mean[:C].clone(), T.invstd[:C].clone())
    with Bufs(dev) as B:
        sm, si, rm, rv, nbt = B.out(Cs), B.out(Cs), B.put(old[0]), B.put(old[1]), B.i64(7)
        K("vmtl_bn_stats", x=None, M=M, C=C, Cs=Cs, partial=B.put(rows), nblk_from_conv=len(cnt), rows_per_blk_from_conv=rpb,
          eps=EPS, momentum=0.1, running_mean=rm, running_var=rv, num_batches_tracked=nbt, save_mean=sm, save_invstd=si)
        check_merged("stats", f"rows-of-{rpb}", mean, var, M, C, sm, si, rm, rv, old, 0.1)
        assert nbt.tolist() == [8]


def _with_nan_rows(rows, k):
    return torch.cat([rows, torch.full((k,) + tuple(rows.shape[1:]), float("nan"))], 0)


@pytest.mark.parametrize("k", (1, 5))
def test_rows_past_m_may_hold_anything(dev, k):
    """The row contract: k further rows that lie wholly past M and hold NaN change no bit of any result - through
    vmtl_bn_stats(_coef) behind 1, 2, 16, 17 and 64 live rows, and through vmtl_bn_apply_fused behind 1, 2, 16 and 17 live
    rows and with 64 rows IN ALL (the most it accepts), the last k of them dead."""
    C, rpb = 33, 7
    Cs = ceil4(C)
    for live in NBLK:
        M = live * rpb - 3
        x, rows, cnt, mean, var = rows_case(rpb, M, C)
        T = operands(M, C)
        assert len(cnt) == live
        with Bufs(dev) as B:
            got = []
            for r in (rows, _with_nan_rows(rows, k)):
                o = dict(sm=B.out(Cs), si=B.out(Cs), rm=B.put(T.mean[:C]), rv=B.put(T.invstd[:C]), ca=B.out(Cs), cc=B.out(Cs))
                K("vmtl_bn_stats_coef", x=None, M=M, C=C, Cs=Cs, partial=B.put(r), nblk_from_conv=r.shape[0],
                  rows_per_blk_from_conv=rpb, eps=EPS, momentum=0.1, running_mean=o["rm"], running_var=o["rv"],
                  num_batches_tracked=None, save_mean=o["sm"], save_invstd=o["si"], gamma=B.put(T.gam), beta=B.put(T.beta),
                  coef_a=o["ca"], coef_c=o["cc"])
                got.append(o)
            for name in got[0]:
                assert not torch.isnan(got[1][name]).any(), f"vmtl_bn_stats, {live} live rows + {k}: NaN in {name}"
                assert torch.equal(got[0][name], got[1][name]), f"vmtl_bn_stats, {live} live rows + {k}: {name} moved"
            check_merged("contract", f"stats-{live}+{k}", mean, var, M, C, got[1]["sm"], got[1]["si"])
    for live, total in [(n, n + k) for n in NBLK[:-1]] + [(NBLK[-1] - k, NBLK[-1])]:
        M = live * rpb - 3
        x, rows, cnt, mean, var = rows_case(rpb, M, C)
        T = operands(M, C)
        with Bufs(dev) as B:
            got = []
            for r in (rows, _with_nan_rows(rows, k)):
                assert r.shape[0] in (live, total)
                o = dict(sm=B.out(Cs), si=B.out(Cs), rm=B.put(T.mean[:C]), rv=B.put(T.invstd[:C]), y=B.out(M, Cs))
                K("vmtl_bn_apply_fused", x=B.put(x), partial=B.put(r), nblk=r.shape[0], rows_per_blk=rpb, eps=EPS,
                  momentum=0.1, running_mean=o["rm"], running_var=o["rv"], num_batches_tracked=None, save_mean=o["sm"],
                  save_invstd=o["si"], gamma=B.put(T.gam), beta=B.put(T.beta), mul=None, res=None, y=o["y"], M=M, C=C,
                  Cs=Cs, act=O.NONE)
                got.append(o)
            for name in got[0]:
                assert not torch.isnan(got[1][name]).any(), f"vmtl_bn_apply_fused, {total} rows, {k} dead: NaN in {name}"
                assert torch.equal(got[0][name], got[1][name]), f"vmtl_bn_apply_fused, {total} rows, {k} dead: {name} moved"
            check_merged("contract", f"fused-{total}-{k}", mean, var, M, C, got[1]["sm"], got[1]["si"])


# ------------------------------------------------------------------------------------------------ eval statistics
EVAL_LAYERS = ((3, 4, True, True), (33, 40, False, True), (1025, 1028, True, False))  # C, Cs, coefficients, affine


def test_eval_statistics_three_forms(dev):
    """vmtl_bn_eval_stats, _coef and _batch over three descriptors of different Cs in one launch (max_cs the largest,
    one without coefficients, one with null gamma / beta): batched == per-layer bitwise, both within 2u of fp64."""
    from vision_mtl_amd import ops

    size = _lib().raw("vmtl_bn_eval_desc_bytes")()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    with Bufs(dev) as B:
        recs, per_layer, batched, refs = [], [], [], []
        for C, Cs, coef, affine in EVAL_LAYERS:
            T = operands(8, Cs)
            rm, rv = T.mean[:C].clone(), (T.invstd[:C] ** 2).clone()
            gam, beta = (T.gam[:C].clone(), T.beta[:C].clone()) if affine else (None, None)
            d = dict(rm=B.put(rm), rv=B.put(rv), gam=B.put(gam), beta=B.put(beta))
            a = [B.out(Cs) for _ in range(4 if coef else 2)]
            b = [B.out(Cs) for _ in range(4 if coef else 2)]
            if coef:
                K("vmtl_bn_eval_stats_coef", running_mean=d["rm"], running_var=d["rv"], C=C, Cs=Cs, eps=EPS, save_mean=a[0],
                  save_invstd=a[1], gamma=d["gam"], beta=d["beta"], coef_a=a[2], coef_c=a[3])
            else:
                K("vmtl_bn_eval_stats", running_mean=d["rm"], running_var=d["rv"], C=C, Cs=Cs, eps=EPS, save_mean=a[0],
                  save_invstd=a[1])
            recs.append(struct.pack(ops._EvalBNTable.DESC, ptr(d["rm"]), ptr(d["rv"]), ptr(d["gam"]), ptr(d["beta"]),
                                    ptr(b[0]), ptr(b[1]), ptr(b[2]) if coef else 0, ptr(b[3]) if coef else 0, C, Cs,
                                    EPS, 0).ljust(size, b"\0"))
            per_layer.append(a)
            batched.append(b)
            refs.append((rm, rv, gam, beta, d))
        descs = B.put(torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).view(torch.float32))
        K("vmtl_bn_eval_stats_batch", descs=descs, n=len(recs), max_cs=max(l[1] for l in EVAL_LAYERS))
        for (C, Cs, coef, affine), a, b, (rm, rv, gam, beta, _) in zip(EVAL_LAYERS, per_layer, batched, refs):
            for i, (u, v) in enumerate(zip(a, b)):
                assert torch.equal(u, v), f"C={C}: output {i} of the batched launch differs from the per-layer one"
            mean = torch.zeros(Cs, dtype=torch.float64)
            mean[:C] = rm.double()
            is_ = torch.zeros(Cs, dtype=torch.float64)
            is_[:C] = 1.0 / (rv.double() + O.f32(EPS)).sqrt()
            assert torch.equal(b[0].cpu().double(), mean)
            check("eval", f"C{C}", "save_invstd", b[1], is_, 2 * O.U * is_)
            if coef:
                g = O._pad_c(gam, Cs) if gam is not None else O.lanes(C, Cs)
                bt = O._pad_c(beta, Cs) if beta is not None else torch.zeros(Cs, dtype=torch.float64)
                sc = g * is_
                e_sc = 2 * O.U * sc.abs() + O.U * sc.abs()
                check("eval", f"C{C}", "coef_a", b[2], sc, e_sc)
                check("eval", f"C{C}", "coef_c", b[3], (bt - mean * sc) * O.lanes(C, Cs),
                      mean.abs() * e_sc + O.gamma(2) * (bt.abs() + (mean * sc).abs() + mean.abs() * e_sc))


# ------------------------------------------------------------------------------------------------ apply
@functools.lru_cache(maxsize=None)
def apply_case(M, C, act, gate, affine, bn):
    """(x nudged, mean, invstd, gamma, beta, mul, res, y, bound) on the CPU"""
    T = operands(M, C)
    mean, invstd, gam, beta = _params(T, affine, bn)
    code = O.ACTS[act]
    x = O.nudge(T.x, mean, invstd, gam, beta, code)
    O.check_inputs(*O.normalise(x, mean, invstd, gam, beta), code, C)
    mul = T.mul if "mul" in gate else None
    res = T.res if "res" in gate else None
    y, e = O.apply(x, mean, invstd, gam, beta, mul, res, C, code)
    return x, mean, invstd, gam, beta, mul, res, y, e


def run_apply(dev, M, C, act, gate, affine, bn):
    x, mean, invstd, gam, beta, mul, res, y_ref, e = apply_case(M, C, act, gate, affine, bn)
    Cs = ceil4(C)
    with Bufs(dev) as B:
        y = B.out(M, Cs)
        K("vmtl_bn_apply", x=B.put(x), mean=B.put(mean), invstd=B.put(invstd), gamma=B.put(gam), beta=B.put(beta),
          mul=B.put(mul), res=B.put(res), y=y, M=M, C=C, Cs=Cs, act=O.ACTS[act])
        route = f"{act}/{gate}/{'affine' if affine else 'plain'}/{'bn' if bn else 'nobn'}"
        check("apply", route, "y", y, y_ref, e)
        if Cs > C:  # exactly 0 without res, exactly res with it
            pad = y[:, C:].cpu()
            assert torch.equal(pad, res[:, C:]) if res is not None else float(pad.abs().max()) == 0.0, f"{route}: pad lanes"


@pytest.mark.parametrize("act", ACT_NAMES)
@pytest.mark.parametrize("M,C", FULL)
def test_apply_every_combination(dev, M, C, act):
    """vmtl_bn_apply: {none, mul, res, mul+res} x {affine, null gamma / beta} x {BatchNorm, mean == invstd == null}."""
    for gate in GATES:
        for affine in (True, False):
            for bn in (True, False):
                run_apply(dev, M, C, act, gate, affine, bn)


@pytest.mark.parametrize("M,C", REST)
def test_apply_geometry(dev, M, C):
    i = REST.index((M, C))
    run_apply(dev, M, C, ACT_NAMES[i % 5], GATES[(i + 1) % 4], i % 2 == 0, i != 3)


# act' AT -3, 0, 3 as csrc/common.h (act_grad) documents them: relu'(0) = 0; hardswish' takes the middle formula
# (2z + 3)/6 AT both kinks; hard-sigmoid' is 1/6 on the open interval only.  relu' and hard-sigmoid' are also what torch's
# autograd returns; for hardswish' torch 2.10 returns 0 at -3 and 1 at 3 (the outer branches), where the releases the
# kernels were written against returned -0.5 and 1.5 - a difference on a set of measure zero that the test prints.
KINK_GRADS = {O.RELU: (0.0, 0.0, 1.0), O.HSWISH: (-0.5, 0.5, 1.5), O.HSIGMOID: (0.0, 1.0 / 6.0, 0.0)}


def _kink_inputs():
    """-3, 0, 3 and their fp32 neighbours, one value per row of a [9][4] map"""
    v = torch.tensor([-3.0, 0.0, 3.0])
    inf = torch.tensor(float("inf"))
    pts = torch.stack([torch.nextafter(v, -inf), v, torch.nextafter(v, inf)], 1).reshape(-1)
    return pts[:, None].repeat(1, 4).contiguous()


@pytest.mark.parametrize("act", ACT_NAMES)
def test_kink_conventions_on_the_no_batchnorm_route(dev, act):
    """mean == invstd == null: z == x bit for bit, so inputs AT the kinks stay there.  Forward within the activation's
    own rounding bound (e_z = 0); act' (dx of vmtl_bn_bwd with dy = 1) on the branch csrc/common.h documents - relu'(0)
    = 0, hardswish' on the middle formula AT -3 and 3, hard-sigmoid' = 0 AT -3 and 3 - bit for bit at the kinks (KINK_GRADS),
    and equal to this torch's own fp32 gradient wherever the two conventions agree."""
    import torch.nn.functional as F

    x = _kink_inputs()
    code = O.ACTS[act]
    M, Cs = x.shape
    a_ref, e_a = O.activate(x.double(), torch.zeros_like(x, dtype=torch.float64), code)
    g_ref, e_g = O.act_grad(x.double(), torch.zeros_like(x, dtype=torch.float64), code)
    if code == O.SIGMOID:
        e_a, e_g = O.sigmoid_bar(a_ref), O.sigmoid_bar(g_ref)
    e_a = e_a + 2.0 ** -149  # the neighbours of 0 are subnormal: a result down there is rounded to the 2^-149 grid
    with Bufs(dev) as B:
        xd, y, dx = B.put(x), B.out(M, Cs), B.out(M, Cs)
        K("vmtl_bn_apply", x=xd, mean=None, invstd=None, gamma=None, beta=None, mul=None, res=None, y=y, M=M, C=Cs, Cs=Cs,
          act=code)
        K("vmtl_bn_bwd", x=xd, dy=B.put(torch.ones(M, Cs)), mean=None, invstd=None, gamma=None, beta=None, mul=None,
          dmul=None, partial=None, sum_dz=None, sum_dzx=None, dx=dx, M=M, C=Cs, Cs=Cs, act=code, training=1)
        check("kinks", act, "act", y, a_ref, e_a)
        check("kinks", act, "act'", dx, g_ref, e_g)
        if code in KINK_GRADS:  # AT the kinks: the documented values, bit for bit
            at = [1, 4, 7]  # the rows holding -3, 0, 3
            want = torch.tensor(KINK_GRADS[code], dtype=torch.float32)[:, None].expand(3, Cs)
            assert torch.equal(dx.cpu()[at], want), f"{act}' at -3, 0, 3: {dx.cpu()[at, 0].tolist()}, want {KINK_GRADS[code]}"
            xt = x.clone().requires_grad_(True)
            {O.RELU: F.relu, O.HSWISH: F.hardswish, O.HSIGMOID: F.hardsigmoid}[code](xt).sum().backward()
            same = [1, 4, 7] if code != O.HSWISH else [4]
            print(f"bn-kinks {act}' at -3, 0, 3: kernel {dx.cpu()[at, 0].tolist()}, this torch {xt.grad[at, 0].tolist()}")
            assert torch.equal(dx.cpu()[same], xt.grad[same]), f"{act}': torch gives {xt.grad[at, 0].tolist()}"


# ------------------------------------------------------------------------------------------------ fused apply
def fused_shape(nblk, wide):
    """(M, C, rows per block): 33 channels in rows of 7, or 1025 channels in rows of 2 (M = 1 at one row)"""
    return (2 * nblk - 1, 1025, 2) if wide else (7 * nblk - 3, 33, 7)


@functools.lru_cache(maxsize=None)
def fused_case(nblk, wide, act, gate):
    M, C, rpb = fused_shape(nblk, wide)
    T = operands(M, C)
    code = O.ACTS[act]
    x = T.x
    for _ in range(2):  # the statistics move with the nudged inputs: settle
        m, m2, cnt = O.partial_rows(x, rpb)
        rows = O.rows_tensor(m, m2)
        mean, var = O.merge_rows(rows, cnt, C)
        is_ = O.invstd_of(var, EPS, C)
        x = O.nudge(x, mean, is_, T.gam, T.beta, code)
    m, m2, cnt = O.partial_rows(x, rpb)
    rows = O.rows_tensor(m, m2)
    mean, var = O.merge_rows(rows, cnt, C)
    is_ = O.invstd_of(var, EPS, C)
    d_mean, d_is = 2 * O.U * mean.abs(), 2 * O.U * is_
    O.check_inputs(*O.normalise(x, mean, is_, T.gam, T.beta, d_mean, d_is), code, C)
    mul = T.mul if "mul" in gate else None
    res = T.res if "res" in gate else None
    y, e = O.apply(x, mean, is_, T.gam, T.beta, mul, res, C, code, d_mean, d_is)
    return x, rows, mean, var, mul, res, y, e


@pytest.mark.parametrize("wide", (False, True))
@pytest.mark.parametrize("nblk", NBLK)
def test_fused_apply(dev, nblk, wide):
    """vmtl_bn_apply_fused with 1, 2, 16, 17 and 64 rows (ops._BN_FUSE_ROWS is 16: the upper range is reached here
    only), rows built by the oracle from x and rounded to fp32; y at the apply bound with mean / invstd allowed 1 ulp;
    the published statistics against the exact merge of the same rows."""
    M, C, rpb = fused_shape(nblk, wide)
    Cs = ceil4(C)
    i = NBLK.index(nblk)
    act = "none" if M == 1 else ACT_NAMES[(i + wide) % 5]  # M == 1: invstd = eps^-1/2, e_z is too large for a kink
    gate = GATES[(i + 2 * wide) % 4]
    x, rows, mean, var, mul, res, y_ref, e = fused_case(nblk, wide, act, gate)
    T = operands(M, C)
    old = (T.mean[:C].clone(), T.invstd[:C].clone())
    null_running = wide and nblk == 17
    with Bufs(dev) as B:
        y, sm, si = B.out(M, Cs), B.out(Cs), B.out(Cs)
        rm, rv, nbt = (None, None, None) if null_running else (B.put(old[0]), B.put(old[1]), B.i64(3))
        K("vmtl_bn_apply_fused", x=B.put(x), partial=B.put(rows), nblk=nblk, rows_per_blk=rpb, eps=EPS, momentum=0.1,
          running_mean=rm, running_var=rv, num_batches_tracked=nbt, save_mean=sm, save_invstd=si, gamma=B.put(T.gam),
          beta=B.put(T.beta), mul=B.put(mul), res=B.put(res), y=y, M=M, C=C, Cs=Cs, act=O.ACTS[act])
        route = f"rows{nblk}/C{C}/{act}/{gate}"
        check("fused", route, "y", y, y_ref, e)
        check_merged("fused", route, mean, var, M, C, sm, si, rm, rv, old, 0.1)
        assert float(sm[C:].abs().sum()) == 0.0
        if not null_running:
            assert nbt.tolist() == [4]


def test_fused_apply_refuses_65_rows(dev):
    M, C, rpb = 65 * 7 - 3, 33, 7
    Cs = ceil4(C)
    assert _lib().raw("vmtl_bn_fuse_max_rows")() == 64
    x, rows, _, _, _ = rows_case(rpb, M, C)
    with Bufs(dev) as B:
        with pytest.raises(RuntimeError, match=r"status -1"):
            K("vmtl_bn_apply_fused", x=B.put(x), partial=B.put(rows), nblk=65, rows_per_blk=rpb, eps=EPS, momentum=0.1,
              running_mean=None, running_var=None, num_batches_tracked=None, save_mean=B.out(Cs), save_invstd=B.out(Cs),
              gamma=None, beta=None, mul=None, res=None, y=B.out(M, Cs), M=M, C=C, Cs=Cs, act=O.NONE)


# ------------------------------------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def bwd_case(M, C, act, gated, training, bn):
    T = operands(M, C)
    mean, invstd, gam, beta = _params(T, True, bn)
    code = O.ACTS[act]
    x = O.nudge(T.x, mean, invstd, gam, beta, code)
    mul = T.mul if gated else None
    R = O.bwd_terms(x, T.dy, mean, invstd, gam, beta, mul, C, code)
    O.check_inputs(*R["z"], code, C)
    (s1, b1), (s2, b2) = O.bwd_sums(R, C, code)
    dx, e_dx = O.bwd_dx(*R["dz"], *R["xh"], invstd, gam, s1, b1, s2, b2, M, C, training)
    if code == O.SIGMOID:
        e_dx = O.sigmoid_bar(dx)
    return x, mean, invstd, gam, beta, mul, R["dmul"], (s1, b1), (s2, b2), (dx, e_dx)


def run_bwd(dev, M, C, act, gated, training, bn):
    x, mean, invstd, gam, beta, mul, dmul_ref, s1, s2, dx_ref = bwd_case(M, C, act, gated, training, bn)
    T = operands(M, C)
    Cs = ceil4(C)
    rows = _lib().raw("vmtl_reduce_rows")(M)
    with Bufs(dev) as B:
        dx = B.out(M, Cs)
        dmul = B.out(M, Cs) if gated else None
        partial = B.out(rows, 2, Cs) if bn or gated else None
        sd, sdx = (B.out(C), B.out(C)) if bn else (None, None)
        K("vmtl_bn_bwd", x=B.put(x), dy=B.put(T.dy), mean=B.put(mean), invstd=B.put(invstd), gamma=B.put(gam),
          beta=B.put(beta), mul=B.put(mul), dmul=dmul, partial=partial, sum_dz=sd, sum_dzx=sdx, dx=dx, M=M, C=C, Cs=Cs,
          act=O.ACTS[act], training=int(training))
        route = f"{act}/{'mul+dmul' if gated else 'plain'}/{'train' if training else 'eval'}/{'bn' if bn else 'nobn'}"
        check("bwd", route, "dx", dx, *dx_ref)
        if gated:
            check("bwd", route, "dmul", dmul, *dmul_ref)
        if bn:
            check("bwd", route, "sum_dz", sd, *s1)
            check("bwd", route, "sum_dzx", sdx, *s2)


@pytest.mark.parametrize("act", ACT_NAMES)
@pytest.mark.parametrize("M,C", FULL)
def test_bwd_every_combination(dev, M, C, act):
    """vmtl_bn_bwd: {mul + dmul, none} x {training, eval} x {BatchNorm, none}; sum outputs of exactly C floats."""
    for gated in (True, False):
        for training in (True, False):
            for bn in (True, False):
                run_bwd(dev, M, C, act, gated, training, bn)


@pytest.mark.parametrize("M,C", REST)
def test_bwd_geometry(dev, M, C):
    i = REST.index((M, C))
    run_bwd(dev, M, C, ACT_NAMES[(i + 2) % 5], i % 2 == 1, True, True)


@functools.lru_cache(maxsize=None)
def halves_case(M, C):
    """given rows [red_blocks(M)][2][Cs] of (sum dz, sum dz*xhat) and a given dz: the two halves of vmtl_bn_bwd"""
    T = operands(M, C)
    Cs = ceil4(C)
    nblk = O.red_blocks(M)
    g = torch.Generator().manual_seed(M + 17 * C)
    rows = torch.randn(nblk, 2, Cs, generator=g) * (M / nblk)
    tot = rows.double().sum(0)
    e_tot = O.U * tot.abs() + 2.0 ** -50 * rows.double().abs().sum(0)  # an fp64 sum rounded once to fp32
    return T, rows, tot, e_tot


@pytest.mark.parametrize("M,C", GEOMETRY)
def test_bwd_finalize_and_apply(dev, M, C):
    """vmtl_bn_bwd_finalize with and without coef_a/b/c (pad channels zero, exactly C sum entries), vmtl_bn_bwd_apply in
    training and eval mode on the sums the finalize wrote, and the affine form coef_a*dz + coef_b*x + coef_c evaluated in
    fp64 from the kernel's coefficients against the oracle's dx."""
    T, rows, tot, e_tot = halves_case(M, C)
    Cs = ceil4(C)
    nblk = rows.shape[0]
    z0 = torch.zeros(M, Cs, dtype=torch.float64)
    dz = T.dy * O.lanes(C, Cs).float()  # a producer's dz has zero pad lanes
    xh = (T.x.double() - T.mean.double()) * T.invstd.double() * O.lanes(C, Cs)
    e_xh = O.gamma(2) * xh.abs()
    with Bufs(dev) as B:
        rd, xd, dzd = B.put(rows), B.put(T.x), B.put(dz)
        md, isd, gd = B.put(T.mean), B.put(T.invstd), B.put(T.gam)
        for training in (1, 0):
            route = "train" if training else "eval"
            sd, sdx, ca, cb, cc = B.out(C), B.out(C), B.out(Cs), B.out(Cs), B.out(Cs)
            K("vmtl_bn_bwd_finalize", partial=rd, nblk=nblk, M=M, C=C, Cs=Cs, sum_dz=sd, sum_dzx=sdx, mean=md, invstd=isd,
              gamma=gd, training=training, coef_a=ca, coef_b=cb, coef_c=cc)
            check("halves", route, "sum_dz", sd, tot[0, :C], e_tot[0, :C])
            check("halves", route, "sum_dzx", sdx, tot[1, :C], e_tot[1, :C])
            sd2, sdx2 = B.out(C), B.out(C)
            K("vmtl_bn_bwd_finalize", partial=rd, nblk=nblk, M=M, C=C, Cs=Cs, sum_dz=sd2, sum_dzx=sdx2, mean=None,
              invstd=None, gamma=None, training=training, coef_a=None, coef_b=None, coef_c=None)
            assert torch.equal(sd, sd2) and torch.equal(sdx, sdx2), "the sums depend on whether coefficients are asked for"
            # from here on the kernel's own fp32 sums are exact inputs
            s1, s2 = sd.cpu().double(), sdx.cpu().double()
            zc = torch.zeros(C, dtype=torch.float64)
            (a_ref, b_ref, c_ref), e_aff = O.bwd_affine(T.x, dz, T.mean, T.invstd, T.gam, s1, zc, s2, zc, M, C, training)
            gi = a_ref
            check("halves", route, "coef_a", ca, a_ref, O.U * a_ref.abs())
            check("halves", route, "coef_b", cb, b_ref, O.gamma(5) * b_ref.abs())
            c1, c2 = O._pad_c(s1, Cs) / M, O._pad_c(s2, Cs) / M
            mag_c = gi.abs() * ((T.mean.double() * T.invstd.double() * c2).abs() + c1.abs()) * (1.0 if training else 0.0)
            check("halves", route, "coef_c", cc, c_ref, O.gamma(7) * mag_c)
            dx = B.out(M, Cs)
            K("vmtl_bn_bwd_apply", x=xd, dz=dzd, mean=md, invstd=isd, gamma=gd, sum_dz=sd if training else None,
              sum_dzx=sdx if training else None, dx=dx, M=M, C=C, Cs=Cs, training=training)
            dx_ref, e_dx = O.bwd_dx(dz.double(), z0, xh, e_xh, T.invstd, T.gam, s1, zc, s2, zc, M, C, training)
            check("halves", route, "dx", dx, dx_ref, e_dx)
            affine = ca.cpu().double() * dz.double() + cb.cpu().double() * T.x.double() + cc.cpu().double()
            check("halves", route, "affine-dx", affine * O.lanes(C, Cs), dx_ref, e_aff)


# ------------------------------------------------------------------------------------------------ pool
def _pool_operands(Bn, H, W, C, act, seed):
    T = operands(Bn * H * W, C, seed=seed, scale=0.7)
    x = O.nudge(T.x, T.mean, T.invstd, T.gam, T.beta, O.ACTS[act])
    return T, x


@functools.lru_cache(maxsize=None)
def pool_case(Bn, H, W, C, act, mode="plain"):
    """mode: plain | ties (whole windows at 0 after relu) | nobeta (the bitwise comparison of the exact activations).
    The seed is the first one for which the conditions on the inputs hold."""
    code = O.ACTS[act]
    for seed in range(64):
        T, x = _pool_operands(Bn, H, W, C, act, seed)
        beta = None if mode == "nobeta" else T.beta
        if mode == "nobeta":
            x = O.nudge(T.x, T.mean, T.invstd, T.gam, None, code)
        if mode == "ties":  # every third window wholly below the kink: z = -|z| - 0.1
            z, _ = O.normalise(x, T.mean, T.invstd, T.gam, beta)
            sc = T.gam.double() * T.invstd.double()
            xw, zw = O._windows(x.double(), Bn, H, W), O._windows(z, Bn, H, W)
            scw = sc.expand_as(xw)
            hit = (torch.arange(xw.shape[0]) % 3 == 0)[:, None, None].expand_as(xw)
            xw = torch.where(hit, xw + (-zw.abs() - 0.1 - zw) / scw, xw)
            x = O._unwindows(xw, Bn, H, W).float()
        try:
            O.check_inputs(*O.normalise(x, T.mean, T.invstd, T.gam, beta), code, C)
            O.check_pool_gap(x, T.mean, T.invstd, T.gam, beta, Bn, H, W, C, code)
        except AssertionError:
            continue
        Mp = Bn * (H // 2) * (W // 2)
        dyp = operands(Mp, C, seed=seed + 100).dy
        fwd = O.pool2_fwd(x, T.mean, T.invstd, T.gam, beta, Bn, H, W, C, code)
        bwd = {tr: O.pool2_bwd(x, dyp, T.mean, T.invstd, T.gam, beta, Bn, H, W, C, code, tr) for tr in (True, False)}
        return T, x, beta, dyp, fwd, bwd
    raise AssertionError("no seed satisfies the conditions on the pool inputs")


def run_pool(dev, Bn, H, W, C, act, mode="plain"):
    T, x, beta, dyp, (y_ref, e_y, _), bwd = pool_case(Bn, H, W, C, act, mode)
    Cs, code = ceil4(C), O.ACTS[act]
    M, Mp = Bn * H * W, Bn * (H // 2) * (W // 2)
    rows = _lib().raw("vmtl_reduce_rows")(Mp)
    route = f"{Bn}x{H}x{W}x{C}/{act}/{mode}"
    with Bufs(dev) as B:
        xd, md, isd, gd, bd = B.put(x), B.put(T.mean), B.put(T.invstd), B.put(T.gam), B.put(beta)
        y = B.out(Mp, Cs)
        K("vmtl_bn_act_pool2_fwd", x=xd, mean=md, invstd=isd, gamma=gd, beta=bd, y=y, B=Bn, H=H, W=W, C=C, Cs=Cs, act=code)
        check("pool", route, "y", y, y_ref, e_y)
        if mode == "nobeta":  # exact activation: the same IEEE operations in fp32 give the same bits
            z32 = T.gam * ((x - T.mean) * T.invstd)
            a32 = z32.clamp_min(0) if code == O.RELU else z32
            y32 = O._windows(a32, Bn, H, W).max(1).values * O.lanes(C, Cs).float()
            assert torch.equal(y.cpu(), y32), f"{route}: y is not the fp32 activation of the selected element"
        if mode == "ties":
            dead = (torch.arange(Mp) % 3 == 0)
            assert float(y.cpu()[dead].abs().max()) == 0.0
        for training in (True, False):
            R = bwd[training]
            dx, sd, sdx = B.out(M, Cs), B.out(C), B.out(C)
            K("vmtl_bn_act_pool2_bwd", x=xd, dyp=B.put(dyp), mean=md, invstd=isd, gamma=gd, beta=bd,
              partial=B.out(rows, 2, Cs), sum_dz=sd, sum_dzx=sdx, dx=dx, B=Bn, H=H, W=W, C=C, Cs=Cs, act=code,
              training=int(training))
            tr = "train" if training else "eval"
            check("pool", route, f"sum_dz/{tr}", sd, *R["s1"])
            check("pool", route, f"sum_dzx/{tr}", sdx, *R["s2"])
            check("pool", route, f"dx/{tr}", dx, *R["dx"])


@pytest.mark.parametrize("act", ACT_NAMES)
@pytest.mark.parametrize("Bn,H,W,C", POOL_SHAPES)
def test_pool(dev, Bn, H, W, C, act):
    """vmtl_bn_act_pool2_fwd / _bwd, five activations, gamma negative on every third channel, training and eval."""
    run_pool(dev, Bn, H, W, C, act)
    if act in ("none", "relu"):
        run_pool(dev, Bn, H, W, C, act, "nobeta")


def test_pool_exact_ties_after_relu(dev):
    """whole windows at 0 after ReLU: the first element wins on both sides and its act' is 0"""
    run_pool(dev, 2, 6, 10, 33, "relu", "ties")


def test_pool_nan_wins(dev):
    """a NaN in each window position (activation none, eval mode): y is NaN exactly in the windows that hold one, and
    the pooled gradient goes to the NaN pixel - the other three pixels of such a window get exactly 0."""
    Bn, H, W, C = 2, 6, 10, 33
    Cs, M, Mp = ceil4(C), Bn * H * W, Bn * (H // 2) * (W // 2)
    T, x, beta, dyp, _, _ = pool_case(Bn, H, W, C, "none")
    xw = O._windows(x, Bn, H, W).clone()
    for i in range(0, Mp, 2):
        xw[i, (i // 2) % 4, (i // 2) % C] = float("nan")
    x = O._unwindows(xw, Bn, H, W).contiguous()
    y_ref, e_y, am = O.pool2_fwd(x, T.mean, T.invstd, T.gam, beta, Bn, H, W, C, O.NONE)
    R = O.pool2_bwd(x, dyp, T.mean, T.invstd, T.gam, beta, Bn, H, W, C, O.NONE, False)
    nan_w = torch.isnan(xw).any(1)
    assert {int(am[i, (i // 2) % C]) for i in range(0, Mp, 2)} == {0, 1, 2, 3} and torch.equal(torch.isnan(y_ref), nan_w)
    rows = _lib().raw("vmtl_reduce_rows")(Mp)
    with Bufs(dev) as B:
        xd, md, isd, gd, bd = B.put(x), B.put(T.mean), B.put(T.invstd), B.put(T.gam), B.put(beta)
        y, dx = B.out(Mp, Cs), B.out(M, Cs)
        K("vmtl_bn_act_pool2_fwd", x=xd, mean=md, invstd=isd, gamma=gd, beta=bd, y=y, B=Bn, H=H, W=W, C=C, Cs=Cs, act=O.NONE)
        K("vmtl_bn_act_pool2_bwd", x=xd, dyp=B.put(dyp), mean=md, invstd=isd, gamma=gd, beta=bd, partial=B.out(rows, 2, Cs),
          sum_dz=B.out(C), sum_dzx=B.out(C), dx=dx, B=Bn, H=H, W=W, C=C, Cs=Cs, act=O.NONE, training=0)
        yc, dxc = y.cpu(), dx.cpu()
        assert torch.equal(torch.isnan(yc), nan_w), "y is NaN in other windows than those that hold a NaN"
        keep = ~nan_w
        check("pool", "nan", "y", yc[keep], y_ref[keep], e_y[keep])
        dx_ref, e_dx = R["dx"]
        nan_x = torch.isnan(x) & (torch.arange(Cs) < C)
        assert torch.equal(torch.isnan(dxc), nan_x), "dx is NaN elsewhere than at the NaN pixels"
        check("pool", "nan", "dx/eval", dxc[~nan_x], dx_ref[~nan_x], e_dx[~nan_x])
        others = O._windows(dxc, Bn, H, W)[nan_w[:, None, :].expand(-1, 4, -1) & ~torch.isnan(xw)]
        assert float(others.abs().max()) == 0.0, "a window that holds a NaN routed gradient to another pixel"


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("M,C", GEOMETRY)
def test_column_sums(dev, M, C):
    """vmtl_colsum modes 0 and 1 and vmtl_stitch_bwd with wstride 0 and 1 and a null dx, each with reduce_all 0 and 1."""
    T = operands(M, C)
    Cs = ceil4(C)
    rows = _lib().raw("vmtl_reduce_rows")(M)
    with Bufs(dev) as B:
        ad, bd = B.put(T.x), B.put(T.dy)
        for mode in (0, 1):
            for ra in (0, 1):
                out = B.out(1 if ra else C)
                K("vmtl_colsum", a=ad, b=bd if mode else None, M=M, C=C, Cs=Cs, mode=mode, reduce_all=ra,
                  partial=B.out(rows + 1, Cs), out=out)
                check("colsum", f"mode{mode}/all{ra}", "out", out, *O.colsum(T.x, T.dy, C, mode, ra))
        for wstride, ra, want_dx in ((0, 0, True), (1, 1, True), (0, 1, False), (1, 0, False)):
            w = T.gam[:C].clone() if wstride else T.gam[:1].clone()
            dx, dw = B.out(M, Cs) if want_dx else None, B.out(1 if ra else C)
            K("vmtl_stitch_bwd", x=ad, dy=bd, w=B.put(w), dx=dx, partial=B.out(rows + 1, Cs), dw=dw, M=M, C=C, Cs=Cs,
              wstride=wstride, reduce_all=ra)
            dx_ref, dw_ref = O.stitch_bwd(T.x, T.dy, w, C, wstride, ra)
            route = f"wstride{wstride}/all{ra}/{'dx' if want_dx else 'nodx'}"
            check("stitch", route, "dw", dw, *dw_ref)
            if want_dx:
                check("stitch", route, "dx", dx, *dx_ref)
