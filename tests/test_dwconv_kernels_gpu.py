"""Every kernel variant of csrc/dwconv.hip against the fp64 oracle of tests/dwconv_oracle.py, at the shapes where the
variants differ: each route of the fused forward (3 generic + 18 pair instantiations), of the data gradient (generic + 4)
and of the weight gradient (6 first stages x 2 finalizes, QL 1..16), odd widths and heights, pad lanes, partly filled
panels, two channel chunks, maps smaller than the kernel, pads other than (K-1)/2, and the second trip of the grid-stride
loop.

The entry points are called through ops._k with packed weights and coefficients built here; every output buffer comes
from ops._empty and is filled with NaN before the launch, so an element no kernel wrote fails its comparison (the
poison and launch-guard sweeps of tests/test_poisoned_buffers_gpu.py run this module as well).  Every comparison is
ELEMENTWISE against the oracle's rounding bound (derived in the oracle's docstring from the number of fp32 roundings, not
fitted), and every case asserts the route it was written for through the vmtl_dwconv_*_route queries, which are what the
launchers switch on.  rule_*() below restate the dispatch rules of include/vmtl.h independently;
tests/test_dwconv_host_cpu.py holds them against the queries and checks that the case tables reach every route.

Statistics rows use the project's bars from test_bn_act_dwconv_matches_torch, applied PER ROW: mean tol 1e-5 + atol 1e-6,
variance (M2 / the row's count) tol 1e-4.

Left out: the grid-stride second trip of the stride-2 data-gradient specialisation.  It would need 135 MB tensors and a
much slower CPU reference; it shares the loop macro and the kernel template with the stride-1 case that is here.

Each check prints `dwconv-ratio <node> route=<code> <result> <worst error / bound>`; profiles/dwconv_tests/README.md holds
the figures of one run."""
import functools
from collections import namedtuple

import pytest
import torch

from tests import dwconv_oracle as O
from tests.util import assert_close, ceil4

pytestmark = pytest.mark.gpu

# include/vmtl.h: VMTL_DW_ROUTE_*
SPEC, K5, S2, WLDS, FIN32 = 4, 8, 16, 32, 64
NONE, RELU, HSWISH = 0, 1, 2
ACTS = {"none": NONE, "relu": RELU, "hswish": HSWISH}


def QL(route):
    return 1 << ((route >> 8) & 7)


Case = namedtuple("Case", "K S pad C B H W act")
Geom = namedtuple("Geom", "Cs Ho Wo M KK")


def case(K, S, C, B, H, W, act=NONE, pad=None):
    return Case(K, S, (K - 1) // 2 if pad is None else pad, C, B, H, W, act)


def geom(c):
    Ho, Wo = O.out_size(c.H, c.K, c.S, c.pad), O.out_size(c.W, c.K, c.S, c.pad)
    return Geom(ceil4(c.C), Ho, Wo, c.B * Ho * Wo, c.K * c.K)


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def rule_stats_block(M, Cs, per_thread=2):
    cq = Cs // 4
    rpt = 1 if cq >= 256 else 256 // cq
    rows = max(per_thread * rpt, -(-M // 1024))
    return (rows + 1) & ~1


def rule_fwd(c, generic=False, per_thread=2):
    g = geom(c)
    if generic or g.Wo % 2:
        return c.act
    r = SPEC | c.act | (K5 if c.K == 5 else 0) | (S2 if c.S == 2 else 0)
    if c.K == 5 and rule_stats_block(g.M, g.Cs, per_thread) >= 12 and 9216 + 25 * g.Cs * 4 <= 160 * 1024:
        r |= WLDS
    return r


def rule_data(c, generic=False):
    if not generic and c.pad == (c.K - 1) // 2 and c.W % 2 == 0 and (c.S == 1 or c.H % 2 == 0):
        return SPEC | (K5 if c.K == 5 else 0) | (S2 if c.S == 2 else 0)
    return 0


def rule_weight(c, generic=False):
    g = geom(c)
    r = K5 if c.K == 5 else 0
    if not generic and g.Wo % 2 == 0 and c.pad == (c.K - 1) // 2:
        r |= SPEC | (S2 if c.S == 2 else 0)
    if c.C * g.KK >= 4096:
        r |= FIN32
    ql, sh = 16, 4
    while ql > 1 and ql // 2 >= g.Cs // 4:
        ql, sh = ql // 2, sh - 1
    return r | (sh << 8)


def _lib():
    from vision_mtl_amd._lib import lib

    return lib()


def q_fwd(c):
    g = geom(c)
    return _lib().raw("vmtl_dwconv_bn_fwd_route")(c.B, c.H, c.W, g.Cs, g.Ho, g.Wo, c.K, c.S, c.pad, c.act)


def q_data(c):
    g = geom(c)
    return _lib().raw("vmtl_dwconv_bwd_data_route")(c.B, c.H, c.W, g.Cs, g.Ho, g.Wo, c.K, c.S, c.pad)


def q_weight(c):
    g = geom(c)
    return _lib().raw("vmtl_dwconv_bwd_weight_route")(c.B, c.H, c.W, c.C, g.Cs, g.Ho, g.Wo, c.K, c.S, c.pad)


# ------------------------------------------------------------------------------------------------ the case tables
# fused forward, every route: name -> (K, S, C, H, W, route bits without the activation); B = 3
FWD_SHAPES = {
    "k3s1": (3, 1, 24, 6, 8, SPEC),
    "k3s2-oddW": (3, 2, 24, 7, 11, SPEC | S2),
    "k5s1-wlds": (5, 1, 120, 6, 8, SPEC | K5 | WLDS),
    "k5s2-wlds-oddHW": (5, 2, 72, 9, 7, SPEC | K5 | S2 | WLDS),
    "k5s1-l1": (5, 1, 200, 4, 8, SPEC | K5),
    "k5s2-l1": (5, 2, 200, 8, 12, SPEC | K5 | S2),
    "generic-oddWo": (5, 1, 40, 5, 7, 0),
}

# edge geometry: fused forward (+ a_out + statistics), plain forward, data gradient with and without addend, weight
# gradient on the fused node's a_out.  name -> Case; the routes follow rule_*(), the ones a case was written for are in
# EDGE_EXPECT as (fused forward, data gradient, weight gradient) specialised-or-not.
EDGE_CASES = {}
for _C in (4, 8, 18, 68, 1040):  # QL 1, 2; pad lanes; two weight-gradient panels, one quad in the second; two q0 chunks
    for _K in (3, 5):
        EDGE_CASES[f"C{_C}-k{_K}s1-4x6"] = case(_K, 1, _C, 2, 4, 6, (_C // 4 + _K) % 3)
for _H, _W in ((1, 2), (2, 2), (1, 8), (3, 4), (5, 3)):  # maps smaller than the kernel
    for _K in (3, 5):
        for _S in (1, 2):
            EDGE_CASES[f"small-{_H}x{_W}-k{_K}s{_S}"] = case(_K, _S, 12, 2, _H, _W, (_H + _W + _K + _S) % 3)
for _H, _W in ((5, 7), (6, 11), (7, 8)):  # stride 2: odd W with even Wo, odd H
    for _K in (3, 5):
        EDGE_CASES[f"s2-{_H}x{_W}-k{_K}"] = case(_K, 2, 24, 2, _H, _W, (_H + _K) % 3)
# weight-gradient finalize <32> (C*K*K >= 4096) and <8> behind every first stage
EDGE_CASES["fin32-k5s1-C168"] = case(5, 1, 168, 2, 4, 6, RELU)       # 4200 elements
EDGE_CASES["fin8-k5s1-C160"] = case(5, 1, 160, 2, 4, 6, HSWISH)      # 4000 elements
EDGE_CASES["fin32-k5s2-C168-pair"] = case(5, 2, 168, 2, 4, 8, NONE)
EDGE_CASES["fin32-k5s2-C168-generic"] = case(5, 2, 168, 2, 4, 6, RELU)
EDGE_CASES["fin32-k3s2-C460-pair"] = case(3, 2, 460, 2, 4, 8, HSWISH)  # 4140 elements
EDGE_CASES["fin32-k3s2-C460-generic"] = case(3, 2, 460, 2, 4, 6, NONE)
del _C, _K, _H, _W, _S

EDGE_EXPECT = {
    "s2-5x7-k3": (True, False, True),  # the mixed node: pair forward, generic data gradient, pair weight gradient
    "s2-5x7-k5": (True, False, True),
    "s2-6x11-k3": (True, False, True),
    "s2-7x8-k5": (True, False, True),  # even W, odd H: the stride-2 data gradient needs both even
    "small-1x2-k5s1": (True, True, True),
    "small-1x2-k5s2": (False, False, False),  # Wo = 1
    "small-5x3-k3s1": (False, False, False),
    "C68-k3s1-4x6": (True, True, True),
    "C1040-k5s1-4x6": (True, True, True),
    "fin32-k3s2-C460-generic": (False, True, False),
}

# plain node only: pads other than (K-1)/2, which the generic data and weight gradients take
PAD_CASES = {f"k{K}s{S}-pad{p}": case(K, S, 20, 2, 6, 8, pad=p) for K in (3, 5) for S in (1, 2) for p in (0, K - 1)}

# generic vs specialised on the same inputs
PAIR_SHAPES = {n: v for n, v in FWD_SHAPES.items() if v[5] & SPEC}
GRAD_CASES = {f"k{K}s{S}": case(K, S, 24, 2, 6, 8) for K in (3, 5) for S in (1, 2)}

# large mean, small standard deviation (5x5 s1 and 3x3 s2): 1024 output pixels in two statistics rows of 512
SHIFT_CASES = {"k5s1": case(5, 1, 4, 1, 32, 32), "k3s2": case(3, 2, 4, 1, 64, 64)}

# past the grid cap of 8192 blocks x 256 threads = 2,097,152 work items
CAP_CASES = {
    "past-the-grid-cap-fwd-and-generic-dgrad": case(3, 1, 64, 1, 256, 517),  # 256 * 517 * 16 = 2,117,632 items each
    "past-the-grid-cap-tpl-k3s1-dgrad": case(3, 1, 64, 1, 512, 520),         # 512 * 260 * 16 = 2,129,920 pair items
}

# the 5x5 layer whose LDS copy of the weights passes 64 KB: M = 10404, 12 pixels per block, 9216 + 57600 bytes
LARGE_LDS_CASE = case(5, 1, 576, 1, 102, 102, HSWISH)


def fwd_case(shape, act):
    K, S, C, H, W, _ = FWD_SHAPES[shape]
    return case(K, S, C, 3, H, W, ACTS[act])


def launches():
    """[(node, Case)] for every launch the tables above make WITHOUT an environment override: what the route-coverage
    test of tests/test_dwconv_host_cpu.py evaluates.  node is 'fwd', 'data' or 'weight'."""
    out = []
    for shape in FWD_SHAPES:
        for act in ACTS:
            out.append(("fwd", fwd_case(shape, act)))
    for c in EDGE_CASES.values():
        out += [("fwd", c), ("data", c), ("weight", c)]
    for c in PAD_CASES.values():
        out += [("data", c), ("weight", c)]
    for c in GRAD_CASES.values():
        out += [("data", c), ("weight", c)]
    for c in SHIFT_CASES.values():
        out.append(("fwd", c))
    for c in CAP_CASES.values():
        out.append(("data", c))
    out.append(("fwd", LARGE_LDS_CASE))
    return out


# ------------------------------------------------------------------------------------------------ inputs and references
Inputs = namedtuple("Inputs", "x ca cc wp dy addend")


@functools.lru_cache(maxsize=None)
def inputs(c, shifted=False):
    """fp32 CPU tensors in the kernels' layouts; the pad lanes [C, Cs) of everything are zero"""
    g = geom(c)
    gen = torch.Generator().manual_seed(1009 * c.K + 101 * c.S + 13 * c.C + 7 * c.H + c.W)
    lanes = (torch.arange(g.Cs) < c.C).float()
    if shifted:  # values ~300 with a standard deviation of 0.05; weights summing to 1, nearly all of it in the centre tap,
        # so that the zero padding moves a border output by at most 16 * 2e-5 * 300 = 0.1 and EVERY row has a small std
        x = torch.randn(c.B, c.H, c.W, g.Cs, generator=gen) * 0.05
        ca, cc = torch.ones(g.Cs), torch.full((g.Cs,), 300.0)
        wp = torch.rand(g.KK, g.Cs, generator=gen) * 2e-5
        wp[g.KK // 2] += 1.0 - wp.sum(0)
    else:
        x = torch.randn(c.B, c.H, c.W, g.Cs, generator=gen) * 1.5 + 0.3
        ca, cc = torch.rand(g.Cs, generator=gen) + 0.5, torch.randn(g.Cs, generator=gen) * 0.5
        wp = torch.randn(g.KK, g.Cs, generator=gen) / c.K
    dy = torch.randn(c.B, g.Ho, g.Wo, g.Cs, generator=gen)
    addend = torch.randn(c.B, c.H, c.W, g.Cs, generator=gen)
    return Inputs(*(t * lanes for t in (x, ca, cc, wp, dy, addend)))


@functools.lru_cache(maxsize=None)
def fused_ref(c, shifted=False):
    """(a, bound of a, y, bound of y) of the fused node"""
    T = inputs(c, shifted)
    a, e_a = O.act_with_error(T.x, T.ca, T.cc, c.act)
    y, by = O.fwd(a, T.wp, c.K, c.S, c.pad, e_a)
    return a, e_a, y, by


@functools.lru_cache(maxsize=None)
def plain_ref(c):
    T = inputs(c)
    return O.fwd(T.x, T.wp, c.K, c.S, c.pad)


@functools.lru_cache(maxsize=None)
def data_ref(c, with_addend):
    T = inputs(c)
    return O.bwd_data(T.dy, T.wp, c.H, c.W, c.K, c.S, c.pad, T.addend if with_addend else None)


# ------------------------------------------------------------------------------------------------ launches and checks
def _out(shape, like):
    """an output buffer: from ops._empty, and NaN wherever no kernel writes"""
    from vision_mtl_amd import ops

    return ops._empty(shape, like).fill_(float("nan"))


def _k(name, **kw):
    from vision_mtl_amd import ops

    ops._k(name, **kw)


def _geo_kw(c):
    g = geom(c)
    return dict(B=c.B, H=c.H, W=c.W, Cs=g.Cs, Ho=g.Ho, Wo=g.Wo, K=c.K, stride=c.S, pad=c.pad)


def _within(got, ref, bound, node, route, what, c):
    r = O.worst_ratio(got.cpu(), ref, bound)
    print(f"dwconv-ratio {node} route={route} {what} {r:.3f}")
    assert r <= 1.0, f"{node} {what} of {c}: worst error / rounding bound = {r:.3g} (route {route})"
    g = geom(c)
    if what != "dw" and g.Cs > c.C:
        assert float(got[..., c.C:].abs().max()) == 0.0, f"{node} {what} of {c}: pad lanes are not zero"
    return r


def run_fused(dev, c, want_a=True, want_stats=True, shifted=False):
    """-> (y, a_out or None, partial or None, statistics block) on the device"""
    T, g = inputs(c, shifted), geom(c)
    x = T.x.to(dev)
    y = _out((c.B, g.Ho, g.Wo, g.Cs), x)
    a = _out((c.B, c.H, c.W, g.Cs), x) if want_a else None
    rows = _lib().raw("vmtl_dwconv_bn_stats_rows")(g.M, g.Cs)
    rpb = _lib().raw("vmtl_dwconv_bn_stats_block")(g.M, g.Cs)
    assert rows == -(-g.M // rpb)
    p = _out((rows, 2, g.Cs), x) if want_stats else None
    _k("vmtl_dwconv_bn_fwd", x=x, coef_a=T.ca.to(dev), coef_c=T.cc.to(dev), act=c.act, wp=T.wp.to(dev), y=y, a_out=a,
       partial=p, **_geo_kw(c))
    return y, a, p, rpb


def check_stat_rows(partial, y_ref, rpb, c, route):
    """every statistics row against the exact (mean, M2) of its own pixels"""
    mean, m2, cnt = O.stat_rows(y_ref, rpb)
    st = partial.cpu().double()
    assert st.shape[0] == mean.shape[0], (st.shape, mean.shape)
    worst_m = worst_v = 0.0
    for i in range(st.shape[0]):
        assert_close(st[i, 0], mean[i], tol=1e-5, atol=1e-6, what=f"{c}: mean of statistics row {i}")
        assert_close(st[i, 1] / cnt[i], m2[i] / cnt[i], tol=1e-4, what=f"{c}: variance of statistics row {i}")
        worst_m = max(worst_m, float((st[i, 0] - mean[i]).abs().max() / (1e-5 * mean[i].abs().max() + 1e-6)))
        vmax = float((m2[i] / cnt[i]).abs().max())
        if vmax > 0:
            worst_v = max(worst_v, float((st[i, 1] / cnt[i] - m2[i] / cnt[i]).abs().max() / (1e-4 * vmax)))
    print(f"dwconv-ratio fwd route={route} stat-mean {worst_m:.3f}")
    print(f"dwconv-ratio fwd route={route} stat-var {worst_v:.3f}")


def check_fused(dev, c, want_a, want_stats, route, shifted=False):
    a_ref, e_a, y_ref, by = fused_ref(c, shifted)
    y, a, p, rpb = run_fused(dev, c, want_a, want_stats, shifted)
    _within(y, y_ref, by, "fwd", route, "y", c)
    if want_a:
        _within(a, a_ref, e_a, "fwd", route, "a_out", c)  # NaN (a pixel no tap owned) counts as inf
    if want_stats and not shifted:
        check_stat_rows(p, y_ref, rpb, c, route)
    return y, a, p, rpb


def check_plain_fwd(dev, c):
    T, g = inputs(c), geom(c)
    x = T.x.to(dev)
    y = _out((c.B, g.Ho, g.Wo, g.Cs), x)
    _k("vmtl_dwconv_fwd", x=x, wp=T.wp.to(dev), y=y, **_geo_kw(c))
    _within(y, *plain_ref(c), "plain-fwd", 0, "y", c)


def run_data(dev, c, with_addend):
    T = inputs(c)
    dy = T.dy.to(dev)
    dx = _out((c.B, c.H, c.W, geom(c).Cs), dy)
    if with_addend:
        _k("vmtl_dwconv_bwd_data_add", dy=dy, wp=T.wp.to(dev), addend=T.addend.to(dev), dx=dx, **_geo_kw(c))
    else:
        _k("vmtl_dwconv_bwd_data", dy=dy, wp=T.wp.to(dev), dx=dx, **_geo_kw(c))
    return dx


def check_data(dev, c, route):
    out = []
    for with_addend in (False, True):
        dx = run_data(dev, c, with_addend)
        _within(dx, *data_ref(c, with_addend), "data", route, "dx+addend" if with_addend else "dx", c)
        out.append(dx)
    return out


def run_weight(dev, c, x):
    """x: the device tensor the kernel reads (the input, or the fused node's a_out)"""
    T, g = inputs(c), geom(c)
    rows = _lib().raw("vmtl_dwconv_bwd_weight_rows")(g.M, g.Cs)
    partial = _out((rows, g.KK, g.Cs), x)
    dw = _out((c.C, g.KK), x)
    _k("vmtl_dwconv_bwd_weight", x=x, dy=T.dy.to(dev), partial=partial, dw=dw, C=c.C, **_geo_kw(c))
    return dw


def check_weight(dev, c, x, route):
    dw = run_weight(dev, c, x)
    ref, bound = O.bwd_weight(x.cpu(), inputs(c).dy, c.C, c.K, c.S, c.pad)
    _within(dw, ref, bound, "weight", route, "dw", c)
    return dw


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("shape", list(FWD_SHAPES))
def test_fused_forward_every_route(dev, shape, act):
    """The 21 routes of vmtl_dwconv_bn_fwd, each with a_out and partial present and NULL (four launches); B = 3."""
    c = fwd_case(shape, act)
    route = q_fwd(c)
    assert route == FWD_SHAPES[shape][5] | ACTS[act] == rule_fwd(c), f"{c}: route {route}"
    for want_a in (True, False):
        for want_stats in (True, False):
            check_fused(dev, c, want_a, want_stats, route)


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_edge_geometry(dev, name):
    """Fused forward, plain forward, data gradient with and without addend, and the weight gradient on the fused node's
    a_out, at the channel counts and map sizes listed at EDGE_CASES."""
    c = EDGE_CASES[name]
    routes = q_fwd(c), q_data(c), q_weight(c)
    assert routes == (rule_fwd(c), rule_data(c), rule_weight(c)), f"{c}: routes {routes}"
    if name in EDGE_EXPECT:
        assert tuple(bool(r & SPEC) for r in routes) == EDGE_EXPECT[name], f"{c}: routes {routes}"
    _, a, _, _ = check_fused(dev, c, True, True, routes[0])
    check_plain_fwd(dev, c)
    check_data(dev, c, routes[1])
    check_weight(dev, c, a, routes[2])


@pytest.mark.parametrize("name", list(PAD_CASES))
def test_plain_node_with_other_pads(dev, name):
    """pad 0 and pad K-1 (Ho != H): plain forward, and the generic data and weight gradients they force."""
    c = PAD_CASES[name]
    g = geom(c)
    assert (g.Ho, g.Wo) != (c.H, c.W) and q_fwd(c) == -1  # the fused node refuses pad != (K-1)/2
    routes = q_data(c), q_weight(c)
    assert routes == (rule_data(c), rule_weight(c)) and not (routes[0] | routes[1]) & SPEC, f"{c}: routes {routes}"
    check_plain_fwd(dev, c)
    check_data(dev, c, routes[0])
    check_weight(dev, c, inputs(c).x.to(dev), routes[1])


@pytest.mark.parametrize("name", list(SHIFT_CASES))
def test_fused_statistics_large_mean_small_std(dev, name):
    """|mean| >> std (values ~300, std ~0.05): the shifted sums around a thread's first value.  As in
    test_bn_large_mean_small_std the reference is the fp64 statistics of the SAME output (an fp32 value near 300 carries
    1.5e-5 of representation error, 3e-4 of the standard deviation), per row, variance at tol 1e-4.

    Why rows of 512 pixels (C = 4): a thread's (mean, M2) partial holds its mean in fp32, i.e. rounded to the 3e-5 grid at
    300 (d ~ 0.9e-5 rms), and Chan's merge squares differences of such means: over a row of N pixels the merged variance
    carries a relative error of about 2 d / (std sqrt(N)) = 1.6e-5 at N = 512 - a sixth of the bar - whichever kernel
    produced the partials.  Rows of a few pixels cannot meet 1e-4 at this mean / std ratio with fp32 partials.
    (This case found the row-lane merge keeping a running mean near 300 through 256 merges: 1.5e-4 of the variance; the
    kernels now merge deviations from the first lane's mean.)"""
    c = SHIFT_CASES[name]
    route = q_fwd(c)
    assert route == rule_fwd(c) and route & SPEC, f"{c}: route {route}"
    y, _, p, rpb = check_fused(dev, c, False, True, route, shifted=True)
    assert rpb == 512
    mean, m2, cnt = O.stat_rows(y.cpu(), rpb)
    st = p.cpu().double()
    assert st.shape[0] == 2
    for i in range(st.shape[0]):
        assert 299.0 < float(mean[i, :c.C].min()) and float((m2[i] / cnt[i]).max()) < 1e-2  # what this test is about
        assert_close(st[i, 0], mean[i], tol=1e-5, atol=1e-6, what=f"{c}: mean of statistics row {i}")
        assert_close(st[i, 1] / cnt[i], m2[i] / cnt[i], tol=1e-4, what=f"{c}: variance of statistics row {i}")
        print(f"dwconv-ratio fwd route={route} shifted-stat-var "
              f"{float((st[i, 1] / cnt[i] - m2[i] / cnt[i]).abs().max() / (1e-4 * (m2[i] / cnt[i]).max())):.3f}")


@pytest.mark.parametrize("shape", list(PAIR_SHAPES))
def test_generic_forward_agrees_with_the_pair_kernels(dev, vmtl_env, shape):
    """VMTL_DWBN_GENERIC=1 on the six pair shapes: the route query reports generic, the same bounds hold, and with
    VMTL_DWBN_ROWS 1 and 3 the statistics rows and vmtl_dwconv_bn_stats_block still describe each other."""
    c = fwd_case(shape, "hswish")
    route = q_fwd(c)
    assert route & SPEC
    y_s, a_s, _, _ = check_fused(dev, c, True, True, route)
    vmtl_env("VMTL_DWBN_GENERIC", 1)
    assert q_fwd(c) == rule_fwd(c, generic=True) == HSWISH
    y_g, a_g, _, _ = check_fused(dev, c, True, True, HSWISH)
    print(f"dwconv-diff fwd {shape} y {float((y_s - y_g).abs().max()):.3e} a_out {float((a_s - a_g).abs().max()):.3e}")
    g = geom(c)
    for generic in (1, 0):
        vmtl_env("VMTL_DWBN_GENERIC", generic)
        for per_thread in (1, 3):
            vmtl_env("VMTL_DWBN_ROWS", per_thread)
            route = q_fwd(c)
            assert route == rule_fwd(c, bool(generic), per_thread), f"{c}: route {route}"
            assert _lib().raw("vmtl_dwconv_bn_stats_block")(g.M, g.Cs) == rule_stats_block(g.M, g.Cs, per_thread)
            check_fused(dev, c, False, True, route)


@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_generic_gradients_agree_with_the_specialised(dev, vmtl_env, name):
    """VMTL_DWBN_GENERIC=1 on the four data-gradient and the four weight-gradient shapes."""
    c = GRAD_CASES[name]
    routes = q_data(c), q_weight(c)
    assert routes == (rule_data(c), rule_weight(c)) and routes[0] & routes[1] & SPEC, f"{c}: routes {routes}"
    x = inputs(c).x.to(dev)
    dx_s = check_data(dev, c, routes[0])
    dw_s = check_weight(dev, c, x, routes[1])
    vmtl_env("VMTL_DWBN_GENERIC", 1)
    routes = q_data(c), q_weight(c)
    assert routes == (0, rule_weight(c, generic=True)) and not routes[1] & SPEC, f"{c}: routes {routes}"
    dx_g = check_data(dev, c, routes[0])
    dw_g = check_weight(dev, c, x, routes[1])
    print(f"dwconv-diff grad {name} dx {float((dx_s[0] - dx_g[0]).abs().max()):.3e} dx+addend "
          f"{float((dx_s[1] - dx_g[1]).abs().max()):.3e} dw {float((dw_s - dw_g).abs().max()):.3e}")


@pytest.mark.parametrize("name", list(CAP_CASES))
def test_past_the_grid_cap(dev, name):
    """More work items than 8192 blocks x 256 threads: the second trip of VMTL_GRID_STRIDE in the plain forward and the
    generic data gradient (odd W), and in dwconv_bwd_data_tpl_kernel<3, 1>."""
    c = CAP_CASES[name]
    g = geom(c)
    route = q_data(c)
    if c.W % 2:
        assert route == 0 and c.B * g.Ho * g.Wo * (g.Cs // 4) > 8192 * 256 and c.B * c.H * c.W * (g.Cs // 4) > 8192 * 256
        check_plain_fwd(dev, c)
    else:
        assert route == SPEC and c.B * c.H * (c.W // 2) * (g.Cs // 4) > 8192 * 256
    _within(run_data(dev, c, False), *data_ref(c, False), "data", route, "dx", c)


def test_5x5_weights_through_more_than_64k_of_lds(dev):
    """576 channels, 5x5, 102 x 102: 12 output pixels per block, so the weights go through LDS, and 9216 static + 57600
    dynamic bytes are more than the 64 KB a launch may ask for without opting in (allow_dynamic_lds)."""
    c = LARGE_LDS_CASE
    g = geom(c)
    route = q_fwd(c)
    assert route == SPEC | K5 | WLDS | HSWISH == rule_fwd(c), f"route {route}"
    assert g.M == 10404 and _lib().raw("vmtl_dwconv_bn_stats_block")(g.M, g.Cs) == 12 and 9216 + 25 * g.Cs * 4 == 66816
    check_fused(dev, c, False, True, route)
