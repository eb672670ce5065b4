"""Host side of csrc/dwconv.hip (no GPU needed): the geometry queries answer an empty shape instead of dividing by zero,
the launchers refuse an empty output before any geometry is computed, the route queries agree with the row / block
queries and with the rules restated in tests/test_dwconv_kernels_gpu.py - and the case tables of that module reach EVERY
route the dispatch has.  Pointers are dummy non-null values; every call returns before any launch.

The calls that used to trap (SIGFPE) run in a forked child, so that a trap fails one test and not the session."""
import multiprocessing

import pytest

from tests import test_dwconv_kernels_gpu as G
from vision_mtl_amd._lib import lib

ERR_ARG = -1


def in_child(name, *args):
    """lib().raw(name)(*args) in a forked child: the result, or an assertion naming the signal that killed it"""
    fn = lib().raw(name)  # loaded before the fork
    ctx = multiprocessing.get_context("fork")
    rx, tx = ctx.Pipe(False)

    def run():
        tx.send(fn(*args))

    p = ctx.Process(target=run)
    p.start()
    p.join(60)
    assert p.exitcode == 0, f"{name}{args}: the child ended with {p.exitcode} (-8 = SIGFPE)"
    return rx.recv()


@pytest.mark.parametrize("name,args", [
    ("vmtl_dwconv_bwd_weight_rows", (0, 16)),
    ("vmtl_dwconv_bwd_weight_rows", (16, 0)),
    ("vmtl_dwconv_bwd_weight_rows", (-3, -4)),
    ("vmtl_dwconv_bwd_weight_rows", (16, 3)),
    ("vmtl_dwconv_bn_stats_rows", (16, 0)),
    ("vmtl_dwconv_bn_stats_rows", (0, 16)),
    ("vmtl_dwconv_bn_stats_rows", (-16, -16)),
    ("vmtl_dwconv_bn_stats_rows", (0, 0)),
])
def test_row_queries_of_an_empty_shape_answer_one_row(name, args):
    assert in_child(name, *args) == 1


@pytest.mark.parametrize("args", [(16, 0), (0, 16), (0, 0), (-5, -8), (16, 2)])
def test_stats_block_of_an_empty_shape_is_positive_and_even(args):
    blk = in_child("vmtl_dwconv_bn_stats_block", *args)
    assert blk > 0 and blk % 2 == 0


# B, H, W, C, Cs, Ho, Wo, K, stride, pad: an output extent that is not positive
EMPTY_OUTPUTS = {
    "2x2-k3-pad0": (1, 2, 2, 4, 4, 0, 0, 3, 1, 0),        # (2 - 3) / 1 + 1 == 0 in C: dw_check accepted it
    "1x1-k5-pad0": (1, 1, 1, 4, 4, -3, -3, 5, 1, 0),      # (1 - 5) / 1 + 1 == -3
    "4x2-k3-pad0-Wo0": (1, 4, 2, 4, 4, 2, 0, 3, 1, 0),
    "2x4-k3-pad0-Ho0": (1, 2, 4, 4, 4, 0, 2, 3, 1, 0),
    "2x2-k5-s2-pad1": (2, 2, 2, 8, 8, 1, 1, 5, 2, 1),     # (2 + 2 - 5) / 2 + 1 == 1 in C (-1 / 2 == 0), where floor gives 0
}


@pytest.mark.parametrize("name", list(EMPTY_OUTPUTS))
def test_every_launcher_refuses_an_empty_output(name):
    B, H, W, C, Cs, Ho, Wo, K, S, pad = EMPTY_OUTPUTS[name]
    geo = (B, H, W, Cs, Ho, Wo, K, S, pad)
    assert in_child("vmtl_dwconv_fwd", 1, 1, 1, *geo, None) == ERR_ARG
    assert in_child("vmtl_dwconv_bn_fwd", 1, 1, 1, 0, 1, 1, 1, 1, *geo, None) == ERR_ARG
    assert in_child("vmtl_dwconv_bwd_data", 1, 1, 1, *geo, None) == ERR_ARG
    assert in_child("vmtl_dwconv_bwd_data_add", 1, 1, 1, 1, *geo, None) == ERR_ARG
    assert in_child("vmtl_dwconv_bwd_weight", 1, 1, 1, 1, B, H, W, C, Cs, Ho, Wo, K, S, pad, None) == ERR_ARG
    assert in_child("vmtl_dwconv_bn_fwd_route", *geo, 0) == ERR_ARG
    assert in_child("vmtl_dwconv_bwd_data_route", *geo) == ERR_ARG
    assert in_child("vmtl_dwconv_bwd_weight_route", B, H, W, C, Cs, Ho, Wo, K, S, pad) == ERR_ARG


def test_route_queries_refuse_what_the_launchers_refuse():
    c = G.case(3, 1, 24, 2, 6, 8)
    g = G.geom(c)
    raw = lib().raw
    assert raw("vmtl_dwconv_bn_fwd_route")(c.B, c.H, c.W, g.Cs, g.Ho, g.Wo, 3, 1, 1, 3) == ERR_ARG  # hard-sigmoid
    assert raw("vmtl_dwconv_bn_fwd_route")(c.B, c.H, c.W, g.Cs, g.Ho - 2, g.Wo - 2, 3, 1, 0, 0) == ERR_ARG  # pad
    assert raw("vmtl_dwconv_bn_fwd_route")(c.B, c.H, c.W, 22, g.Ho, g.Wo, 3, 1, 1, 0) == ERR_ARG  # Cs % 4
    assert raw("vmtl_dwconv_bwd_data_route")(c.B, c.H, c.W, g.Cs, g.Ho, g.Wo, 4, 1, 1) == ERR_ARG  # K
    assert raw("vmtl_dwconv_bwd_data_route")(c.B, c.H, c.W, g.Cs, g.Ho, g.Wo + 1, 3, 1, 1) == ERR_ARG  # Wo
    assert raw("vmtl_dwconv_bwd_weight_route")(c.B, c.H, c.W, 25, g.Cs, g.Ho, g.Wo, 3, 1, 1) == ERR_ARG  # C > Cs
    assert raw("vmtl_dwconv_bwd_weight_route")(c.B, c.H, c.W, 0, g.Cs, g.Ho, g.Wo, 3, 1, 1) == ERR_ARG
    assert raw("vmtl_dwconv_bwd_weight_route")(c.B, c.H, c.W, 24, g.Cs, g.Ho, g.Wo, 3, 3, 1) == ERR_ARG  # stride
    # and the same arguments with dummy pointers through the launchers
    assert raw("vmtl_dwconv_bn_fwd")(1, 1, 1, 3, 1, 1, 1, 1, c.B, c.H, c.W, g.Cs, g.Ho, g.Wo, 3, 1, 1, None) == ERR_ARG
    assert raw("vmtl_dwconv_bwd_weight")(1, 1, 1, 1, c.B, c.H, c.W, 25, g.Cs, g.Ho, g.Wo, 3, 1, 1, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("B,C,H,W,K,S,act", [(2, 18, 5, 7, 5, 2, 2), (1, 68, 9, 12, 3, 1, 1), (3, 4, 1, 2, 5, 1, 0),
                                             (2, 12, 6, 8, 3, 2, 2)])
def test_oracle_is_torch_in_fp64_and_torch_in_fp32_stays_inside_its_bounds(B, C, H, W, K, S, act):
    """tests/dwconv_oracle.py against an independent formulation (torch's conv2d and autograd in float64, NCHW), and its
    rounding bounds against torch's own float32 evaluation of the same node - a correct fp32 implementation."""
    import torch
    import torch.nn.functional as F

    from tests import dwconv_oracle as O

    c = G.case(K, S, C, B, H, W, act)
    T = G.inputs(c)
    fact = {0: lambda v: v, 1: F.relu, 2: F.hardswish}[act]

    def torch_node(dt):
        x = T.x[..., :C].permute(0, 3, 1, 2).to(dt).requires_grad_(True)
        w = T.wp[:, :C].t().reshape(C, 1, K, K).to(dt).requires_grad_(True)
        a = fact(x * T.ca[:C].to(dt).view(1, C, 1, 1) + T.cc[:C].to(dt).view(1, C, 1, 1))
        a.retain_grad()
        y = F.conv2d(a, w, None, stride=S, padding=c.pad, groups=C)
        y.backward(T.dy[..., :C].permute(0, 3, 1, 2).to(dt))
        nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
        return nhwc(a), nhwc(y), nhwc(a.grad), w.grad.detach().reshape(C, K * K)

    a64, y64, da64, dw64 = torch_node(torch.float64)
    a32, y32, da32, dw32 = torch_node(torch.float32)
    a, e_a, y, by = G.fused_ref(c)
    dx, bdx = O.bwd_data(T.dy, T.wp, H, W, K, S, c.pad)
    dxa, bdxa = O.bwd_data(T.dy, T.wp, H, W, K, S, c.pad, T.addend)
    dw, bdw = O.bwd_weight(a32, T.dy[..., :C], C, K, S, c.pad)
    dw_exact, _ = O.bwd_weight(a64, T.dy[..., :C], C, K, S, c.pad)
    for got, ref in ((a[..., :C], a64), (y[..., :C], y64), (dx[..., :C], da64), (dw_exact, dw64),
                     (dxa[..., :C], da64 + T.addend[..., :C].double())):
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    ratios = {"a": O.worst_ratio(a32, a[..., :C], e_a[..., :C]), "y": O.worst_ratio(y32, y[..., :C], by[..., :C]),
              "dx": O.worst_ratio(da32, dx[..., :C], bdx[..., :C]), "dw": O.worst_ratio(dw32, dw, bdw),
              "dx+addend": O.worst_ratio(da32 + T.addend[..., :C], dxa[..., :C], bdxa[..., :C])}
    print(ratios)
    assert max(ratios.values()) <= 1.0, ratios
    mean, m2, cnt = O.stat_rows(y, 10)
    flat = y.reshape(-1, y.shape[-1])
    assert float(cnt.sum()) == flat.shape[0] and cnt[-1] == flat.shape[0] - 10 * (len(cnt) - 1)
    tot_mean = (mean * cnt[:, None]).sum(0) / cnt.sum()
    tot_m2 = (m2 + cnt[:, None] * (mean - tot_mean) ** 2).sum(0)
    assert float((tot_mean - flat.mean(0)).abs().max()) <= 1e-12
    assert float((tot_m2 - ((flat - flat.mean(0)) ** 2).sum(0)).abs().max()) <= 1e-9


def test_the_bounds_reject_what_the_global_bar_lets_through():
    """Two subtly wrong forwards of a 5x5 stride-1 node - two taps swapped in ONE channel whose weights are 1e-3 of the
    others', and the zero padding replaced by the edge value in the last column only - stay inside the suite's global
    1e-4 * max|ref| only in the first case, and are far outside the elementwise bound in both."""
    import torch

    from tests import dwconv_oracle as O

    c = G.case(5, 1, 24, 2, 6, 8)
    T = G.inputs(c)
    wp = T.wp.clone()
    wp[:, 3] *= 1e-3
    y, by = O.fwd(T.x, wp, 5, 1, 2)
    swapped = wp.clone()
    swapped[[7, 8], 3] = swapped[[8, 7], 3]
    y_swapped, _ = O.fwd(T.x, swapped, 5, 1, 2)
    assert float((y_swapped - y).abs().max()) <= 1e-4 * float(y.abs().max())  # invisible to the global bar
    assert O.worst_ratio(y_swapped.float(), y, by) > 100
    xp = torch.cat([T.x, T.x[:, :, -1:, :]], 2)  # one more column, holding the edge value
    y_edge, _ = O.fwd(xp, wp, 5, 1, 2)
    assert O.worst_ratio(y_edge[:, :, :8].float(), y, by) > 1000
    assert O.worst_ratio(y.float(), y, by) <= 1.0  # and the correctly rounded result is inside


# ------------------------------------------------------------------------------------------------ coverage as a condition
FWD_ROUTES = {a for a in (0, 1, 2)} | {G.SPEC | k | s | w | a for a in (0, 1, 2) for s in (0, G.S2)
                                       for k, w in ((0, 0), (G.K5, 0), (G.K5, G.WLDS))}
DATA_ROUTES = {0} | {G.SPEC | k | s for k in (0, G.K5) for s in (0, G.S2)}
# (first stage, finalize): generic <9> / <25> and the four pair kernels, each with finalize <8> and <32>
WEIGHT_STAGES = {k | f for k in (0, G.K5) for f in (0, G.FIN32)} | {G.SPEC | k | s | f for k in (0, G.K5)
                                                                      for s in (0, G.S2) for f in (0, G.FIN32)}


def test_the_full_route_sets_have_the_sizes_the_dispatch_has():
    assert (len(FWD_ROUTES), len(DATA_ROUTES), len(WEIGHT_STAGES)) == (21, 5, 12)


def test_the_gpu_case_tables_reach_every_route():
    """100 % of the routes: 21 fused-forward, 5 data-gradient, all 12 (first stage, finalize) pairs of the weight
    gradient and every quad-lane count, evaluated with the queries the launchers switch on."""
    reached = {"fwd": set(), "data": set(), "weight": set()}
    query = {"fwd": G.q_fwd, "data": G.q_data, "weight": G.q_weight}
    rule = {"fwd": G.rule_fwd, "data": G.rule_data, "weight": G.rule_weight}
    for node, c in G.launches():
        r = query[node](c)
        assert r >= 0 and r == rule[node](c), f"{node} {c}: route {r}, the restated rule says {rule[node](c)}"
        reached[node].add(r)
    assert reached["fwd"] == FWD_ROUTES, f"not reached: {sorted(FWD_ROUTES - reached['fwd'])}"
    assert reached["data"] == DATA_ROUTES, f"not reached: {sorted(DATA_ROUTES - reached['data'])}"
    stages = {r & 0xff for r in reached["weight"]}
    assert stages == WEIGHT_STAGES, f"not reached: {sorted(WEIGHT_STAGES - stages)}"
    assert {G.QL(r) for r in reached["weight"]} == {1, 2, 4, 8, 16}
    print(f"routes reached: forward {len(reached['fwd'])}/21, data gradient {len(reached['data'])}/5, weight gradient "
          f"{len(stages)}/12 stage pairs, QL {sorted({G.QL(r) for r in reached['weight']})}")


def test_every_case_is_what_its_table_says():
    assert len(G.FWD_SHAPES) * len(G.ACTS) == 21 and len(G.PAIR_SHAPES) == 6 and len(G.GRAD_CASES) == 4
    assert {c.C for c in G.EDGE_CASES.values()} >= {4, 8, 18, 68, 1040, 160, 168}
    assert set(G.EDGE_EXPECT) <= set(G.EDGE_CASES)
    for c in G.PAD_CASES.values():
        assert c.pad in (0, c.K - 1)
    assert {(c.K, c.S, c.pad) for c in G.PAD_CASES.values()} == {(K, S, p) for K in (3, 5) for S in (1, 2) for p in (0, K - 1)}


# ------------------------------------------------------------------------------------------------ queries against queries
def _weight_rows_rule(M, Cs, ql):
    panels = -(-(Cs // 4) // ql)
    nblk = max(1, min(-(-2048 // panels), -(-M // (4 * (256 // ql))), 512))
    rows = (-(-M // nblk) + 1) & ~1
    return -(-M // rows)


GRID_CS = (4, 8, 168, 172, 560, 564, 1024, 1028, 1544, 1548)
GRID_M = (2, 10, 24, 144, 1024, 10240, 10242, 10404, 20000)


@pytest.mark.parametrize("generic,per_thread", [(0, None), (1, None), (0, 1), (0, 3), (0, 7)])
def test_route_and_geometry_queries_agree(vmtl_env, generic, per_thread):
    """Over a grid of (M, Cs) around the WLDS (12 pixels per block), LDS-limit (64 KB at Cs 564, 160 KB at Cs 1548) and
    channel-chunk (Cs 1024) boundaries: the WLDS bit is the block query's answer and the LDS limit, QL gives the row
    query's answer, and all of it is what the restated rules say - for 5x5 stride 1 on a 1 x M map."""
    vmtl_env("VMTL_DWBN_GENERIC", generic)
    if per_thread is not None:
        vmtl_env("VMTL_DWBN_ROWS", per_thread)
    raw = lib().raw
    seen = set()
    for Cs in GRID_CS:
        for M in GRID_M:
            c = G.case(5, 1, Cs, 1, 1, M)
            g = G.geom(c)
            assert (g.M, g.Cs) == (M, Cs)
            blk, rows = raw("vmtl_dwconv_bn_stats_block")(M, Cs), raw("vmtl_dwconv_bn_stats_rows")(M, Cs)
            assert blk == G.rule_stats_block(M, Cs, per_thread or 2) and blk % 2 == 0 and rows == -(-M // blk)
            r = G.q_fwd(c)
            assert r == G.rule_fwd(c, bool(generic), per_thread or 2), (M, Cs, r)
            assert bool(r & G.WLDS) == (not generic and blk >= 12 and 9216 + 100 * Cs <= 160 * 1024), (M, Cs, r)
            seen.add((bool(r & G.WLDS), blk >= 12, 9216 + 100 * Cs > 65536, 9216 + 100 * Cs > 160 * 1024))
            rw = G.q_weight(c)
            assert rw == G.rule_weight(c, bool(generic)), (M, Cs, rw)
            assert raw("vmtl_dwconv_bwd_weight_rows")(M, Cs) == _weight_rows_rule(M, Cs, G.QL(rw)), (M, Cs, rw)
            assert G.q_data(c) == G.rule_data(c, bool(generic))
    if not generic and per_thread is None:  # both sides of all three boundaries were on the grid
        assert {(True, True, False, False), (True, True, True, False), (False, True, True, True),
                (False, False, False, False), (False, False, True, False)} <= seen, seen
