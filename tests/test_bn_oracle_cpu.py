"""tests/bn_oracle.py itself, without a GPU: (1) a straightforward fp32 torch evaluation of every formula stays inside the
oracle's bound on every shape of the case tables of tests/test_bn_kernels_gpu.py - the bounds can be met; (2) seeded
defects applied to that fp32 evaluation each exceed a bound or a bar on at least one case - the bounds can see them;
(3) the case tables reach every edge of the sweep geometry of csrc/reduce.h they were written for."""
import torch

from tests import bn_oracle as O
from tests import test_bn_kernels_gpu as G
from tests.util import ceil4

SIXTH = torch.tensor(1.0 / 6.0, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ fp32, straightforward
def act32(z, code):
    if code == O.RELU:
        return z.clamp_min(0)
    if code == O.HSWISH:
        return z * (z + 3).clamp(0, 6) * SIXTH
    if code == O.HSIGMOID:
        return (z + 3).clamp(0, 6) * SIXTH
    if code == O.SIGMOID:
        return torch.sigmoid(z)
    return z


def grad32(z, code, outer_at_kink=False):
    one, zero = torch.ones_like(z), torch.zeros_like(z)
    if code == O.RELU:
        return (z > 0).float()
    if code == O.HSWISH:
        if outer_at_kink:  # the seeded defect: <= and >= where torch has < and >
            return torch.where(z <= -3, zero, torch.where(z >= 3, one, (2 * z + 3) * SIXTH))
        return torch.where(z < -3, zero, torch.where(z > 3, one, (2 * z + 3) * SIXTH))
    if code == O.HSIGMOID:
        return torch.where((z > -3) & (z < 3), SIXTH * one, zero)
    if code == O.SIGMOID:
        s = torch.sigmoid(z)
        return s * (1 - s)
    return one


def _v32(v, Cs, fill):
    return torch.full((Cs,), float(fill)) if v is None else v


def z_fwd32(x, mean, invstd, gam, beta):
    if mean is None:
        return x
    Cs = x.shape[-1]
    sc = _v32(gam, Cs, 1) * invstd
    return x * sc + (_v32(beta, Cs, 0) - mean * sc)


def z_bwd32(x, mean, invstd, gam, beta):
    if mean is None:
        return x, x
    Cs = x.shape[-1]
    xh = (x - mean) * invstd
    return _v32(gam, Cs, 1) * xh + _v32(beta, Cs, 0), xh


def apply32(x, mean, invstd, gam, beta, mul, res, C, code, pad_sc=None):
    Cs = x.shape[-1]
    ok = (torch.arange(Cs) < C).float()
    y = act32(z_fwd32(x, mean, invstd, gam, beta), code) * ok
    if pad_sc is not None:  # the seeded defect: a pad channel treated as data with scale pad_sc
        y = y + act32(x * pad_sc, code) * (1 - ok)
    if mul is not None:
        y = y * mul
    if res is not None:
        y = y + res
    return y


def bwd32(x, dy, mean, invstd, gam, beta, mul, C, code, M, training, x_for_xhat=False):
    Cs = x.shape[-1]
    ok = (torch.arange(Cs) < C).float()
    z, xh = z_bwd32(x, mean, invstd, gam, beta)
    dz = dy * ok * (mul if mul is not None else 1.0) * grad32(z, code)
    dmul = dy * ok * act32(z, code)
    s1, s2 = dz.sum(0), (dz * (x if x_for_xhat else xh)).sum(0)
    gi = (_v32(gam, Cs, 1) * invstd if mean is not None else torch.ones(Cs)) * ok
    if training and mean is not None:
        invM = torch.tensor(1.0 / M, dtype=torch.float32)
        dx = gi * (dz - s1 * invM - xh * (s2 * invM))
    else:
        dx = gi * dz
    return dmul, s1[:C], s2[:C], dx


def pool32(x, dyp, mean, invstd, gam, beta, Bn, H, W, C, code, training, argmax_before_act=False):
    Cs = x.shape[-1]
    ok = (torch.arange(Cs) < C).float()
    z, xh = z_bwd32(x, mean, invstd, gam, beta)
    a = act32(z, code)
    aw = O._windows(a, Bn, H, W)
    am, _ = O.argmax_window(O._windows(x, Bn, H, W) if argmax_before_act else aw)
    y = aw.gather(1, am[:, None, :]).squeeze(1) * ok
    sel = torch.zeros(am.shape[0], 4, Cs).scatter_(1, am[:, None, :], 1.0)
    dz = O._unwindows(sel * dyp[:, None, :], Bn, H, W) * ok * grad32(z, code)
    s1, s2 = dz.sum(0), (dz * xh).sum(0)
    gi = _v32(gam, Cs, 1) * invstd * ok
    if training:
        invM = torch.tensor(1.0 / (Bn * H * W), dtype=torch.float32)
        dx = gi * (dz - s1 * invM - xh * (s2 * invM))
    else:
        dx = gi * dz
    return y, s1[:C], s2[:C], dx


WORST = {}


def within(what, got, ref, bound):
    r = O.worst_ratio(got, ref, bound)
    WORST[what] = max(WORST.get(what, 0.0), r)
    assert r <= 1.0, f"{what}: a plain fp32 evaluation is {r:.3g} x the bound away"


def _apply_combos():
    for M, C in G.FULL:
        for act in G.ACT_NAMES:
            for gate in G.GATES:
                for affine in (True, False):
                    for bn in (True, False):
                        yield M, C, act, gate, affine, bn
    for i, (M, C) in enumerate(G.REST):
        yield M, C, G.ACT_NAMES[i % 5], G.GATES[(i + 1) % 4], i % 2 == 0, i != 3


def _bwd_combos():
    for M, C in G.FULL:
        for act in G.ACT_NAMES:
            for gated in (True, False):
                for training in (True, False):
                    for bn in (True, False):
                        yield M, C, act, gated, training, bn
    for i, (M, C) in enumerate(G.REST):
        yield M, C, G.ACT_NAMES[(i + 2) % 5], i % 2 == 1, True, True


def test_fp32_apply_stays_inside_the_bound():
    for M, C, act, gate, affine, bn in _apply_combos():
        x, mean, invstd, gam, beta, mul, res, y, e = G.apply_case(M, C, act, gate, affine, bn)
        within("apply", apply32(x, mean, invstd, gam, beta, mul, res, C, O.ACTS[act]), y, e)
    print(f"worst fp32 error / bound: apply {WORST['apply']:.3f}")


def test_fp32_fused_apply_stays_inside_the_bound():
    """mean / invstd rounded from the exact merge, as the kernel publishes and uses them"""
    for nblk in G.NBLK:
        for wide in (False, True):
            M, C, _ = G.fused_shape(nblk, wide)
            i = G.NBLK.index(nblk)
            act, gate = "none" if M == 1 else G.ACT_NAMES[(i + wide) % 5], G.GATES[(i + 2 * wide) % 4]
            x, rows, mean, var, mul, res, y, e = G.fused_case(nblk, wide, act, gate)
            T = G.operands(M, C)
            is32 = O.invstd_of(var, G.EPS, C).float()
            within("fused", apply32(x, mean.float(), is32, T.gam, T.beta, mul, res, C, O.ACTS[act]), y, e)
    print(f"worst fp32 error / bound: fused apply {WORST['fused']:.3f}")


def test_fp32_backward_stays_inside_the_bound():
    for M, C, act, gated, training, bn in _bwd_combos():
        x, mean, invstd, gam, beta, mul, dmul_ref, s1, s2, dx_ref = G.bwd_case(M, C, act, gated, training, bn)
        T = G.operands(M, C)
        dmul, a1, a2, dx = bwd32(x, T.dy, mean, invstd, gam, beta, mul, C, O.ACTS[act], M, training)
        within("bwd dx", dx, *dx_ref)
        within("bwd dmul", dmul, *dmul_ref)
        if bn:
            within("bwd sum_dz", a1, *s1)
            within("bwd sum_dzx", a2, *s2)
    print("worst fp32 error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items() if k.startswith("bwd")))


def test_fp32_halves_stay_inside_the_bound():
    """bwd_apply from given dz and sums, and the affine form from fp32 coefficients"""
    for M, C in G.GEOMETRY:
        T, rows, tot, _ = G.halves_case(M, C)
        Cs = ceil4(C)
        ok = O.lanes(C, Cs)
        dz = T.dy * ok.float()
        s1, s2 = tot[0, :C].float(), tot[1, :C].float()
        zc, z0 = torch.zeros(C, dtype=torch.float64), torch.zeros(M, Cs, dtype=torch.float64)
        xh = (T.x.double() - T.mean.double()) * T.invstd.double() * ok
        invM = torch.tensor(1.0 / M, dtype=torch.float32)
        c1, c2 = O._pad_c(s1, Cs).float() * invM, O._pad_c(s2, Cs).float() * invM
        gi = T.gam * T.invstd * ok.float()
        dx32 = gi * (dz - c1 - ((T.x - T.mean) * T.invstd) * c2)
        dx, e = O.bwd_dx(dz.double(), z0, xh, O.gamma(2) * xh.abs(), T.invstd, T.gam, s1, zc, s2, zc, M, C, True)
        within("halves dx", dx32, dx, e)
        ca, cb, cc = gi, -gi * T.invstd * c2, gi * (T.mean * T.invstd * c2 - c1)
        _, e_aff = O.bwd_affine(T.x, dz, T.mean, T.invstd, T.gam, s1, zc, s2, zc, M, C, True)
        within("halves affine", (ca.double() * dz.double() + cb.double() * T.x.double() + cc.double()) * ok, dx, e_aff)
    print(f"worst fp32 error / bound: halves dx {WORST['halves dx']:.3f}, affine form {WORST['halves affine']:.3f}")


def test_fp32_pool_stays_inside_the_bound():
    for Bn, H, W, C in G.POOL_SHAPES:
        for act in G.ACT_NAMES:
            T, x, beta, dyp, (y_ref, e_y, _), bwd = G.pool_case(Bn, H, W, C, act)
            for training in (True, False):
                y, a1, a2, dx = pool32(x, dyp, T.mean, T.invstd, T.gam, beta, Bn, H, W, C, O.ACTS[act], training)
                within("pool y", y, y_ref, e_y)
                within("pool sum_dz", a1, *bwd[training]["s1"])
                within("pool sum_dzx", a2, *bwd[training]["s2"])
                within("pool dx", dx, *bwd[training]["dx"])
    print("worst fp32 error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items() if k.startswith("pool")))


def test_fp32_column_sums_stay_inside_the_bound():
    for M, C in G.GEOMETRY:
        T = G.operands(M, C)
        for ra in (0, 1):
            within("colsum", T.x[:, :C].sum().reshape(1) if ra else T.x[:, :C].sum(0), *O.colsum(T.x, T.dy, C, 0, ra))
            p = (T.x * T.dy)[:, :C]
            within("colsum", p.sum().reshape(1) if ra else p.sum(0), *O.colsum(T.x, T.dy, C, 1, ra))
            (dx, e), dw = O.stitch_bwd(T.x, T.dy, T.gam[:C], C, 1, ra)
            within("stitch", p.sum().reshape(1) if ra else p.sum(0), *dw)
            w = torch.zeros(ceil4(C))
            w[:C] = T.gam[:C]
            within("stitch", T.dy * w, dx, e)
    print(f"worst fp32 error / bound: colsum {WORST['colsum']:.3f}, stitch {WORST['stitch']:.3f}")


def stats32(x, C, M_for_var=None):
    """two-pass fp32 statistics; M_for_var: the seeded defect's divisor"""
    M = x.shape[0]
    mean = x.sum(0) / M
    var = ((x - mean) ** 2).sum(0) / (M_for_var or M)
    ok = (torch.arange(x.shape[1]) < C).float()
    return mean * ok, var * ok


def running32(old, mean, var, M, momentum, biased=False, swapped=False):
    m = torch.tensor(momentum, dtype=torch.float32)
    unb = var * (M / (M - 1)) if M > 1 and not biased else var
    a, b = (m, 1 - m) if swapped else (1 - m, m)
    return a * old[0] + b * mean, a * old[1] + b * unb


def _stats_errors(M, C, momentum, **defect):
    """(error / bar) of an fp32 evaluation of the statistics family: save_mean, variance, running_mean, running_var"""
    x, mean, var = G.stats_case(M, C)
    T = G.operands(min(M, 64), C)
    old = (T.mean[:C], T.invstd[:C])
    m32, v32 = stats32(x, C, defect.get("M_for_var"))
    rm, rv = running32(old, m32[:C], v32[:C], M, momentum, defect.get("biased", False), defect.get("swapped", False))
    rm_ref, rv_ref = O.running(old[0], old[1], mean, var, M, momentum)
    bm, bv, mom = G.mean_bar(mean), G.var_bar(var), O.f32(momentum)
    one = torch.ones(C, dtype=torch.float64)
    return (O.worst_ratio(m32[:C], mean[:C], bm * one), O.worst_ratio(v32[:C], var[:C], bv * one + 1e-300),
            O.worst_ratio(rm, rm_ref, mom * bm + O.U * rm_ref.abs()),
            O.worst_ratio(rv, rv_ref, mom * bv * (M / (M - 1) if M > 1 else 1.0) + O.U * rv_ref.abs() + 1e-300))


def test_fp32_statistics_stay_inside_the_bars():
    worst = [0.0] * 4
    for M, C in G.GEOMETRY:
        for momentum in (0.1, 1.0):
            r = _stats_errors(M, C, momentum)
            worst = [max(a, b) for a, b in zip(worst, r)]
    print("worst fp32 error / bar: save_mean %.3f, variance %.3f, running_mean %.3f, running_var %.3f" % tuple(worst))
    assert max(worst) <= 1.0, worst


def test_fp32_eval_statistics_stay_inside_2u():
    """1 / sqrt(rv + eps) with every operation correctly rounded in fp32, on the layers of the GPU test"""
    eps = torch.tensor(G.EPS, dtype=torch.float32)
    worst = 0.0
    for C, Cs, _, _ in G.EVAL_LAYERS:
        rv = G.operands(8, Cs).invstd[:C] ** 2
        is32 = 1.0 / torch.sqrt(rv + eps)
        ref = 1.0 / (rv.double() + O.f32(G.EPS)).sqrt()
        worst = max(worst, O.worst_ratio(is32, ref, 2 * O.U * ref))
    print(f"worst fp32 error / (2u): eval invstd {worst:.3f}")
    assert worst <= 1.0


def test_merge_of_rounded_rows_is_the_statistics_of_the_input():
    """partial_rows + merge_rows against the direct fp64 statistics (the rows are rounded to fp32 in between), and a
    row with count 0 is ignored whatever it holds"""
    for rpb, M in G.GIVEN_ROWS:
        x, rows, cnt, mean, var = G.rows_case(rpb, M, 33)
        m0, v0 = O.exact_stats(x, 33)
        assert float((mean - m0).abs().max()) <= 4 * O.U * float(m0.abs().max())
        assert float((var - v0).abs().max()) <= 1e-6 * float(v0.max())
        dead = torch.cat([rows, torch.full((2, 2, rows.shape[2]), float("nan"))], 0)
        m1, v1 = O.merge_rows(dead, O.row_counts(len(cnt) + 2, rpb, M), 33)
        assert torch.equal(m1, mean) and torch.equal(v1, var)
        assert torch.equal(O.row_counts(len(cnt), rpb, M), cnt)


# ------------------------------------------------------------------------------------------------ seeded defects
def test_defect_last_row_of_a_block_dropped_from_a_column_sum():
    seen = []
    for M, C in G.GEOMETRY:
        T = G.operands(M, C)
        last = O.block_rows(M, O.red_blocks(M))[0] - 1  # the last row of block 0
        keep = torch.arange(M) != last
        ref, bound = O.colsum(T.x, T.dy, C, 0, 0)
        seen.append(O.worst_ratio(T.x[keep][:, :C].sum(0), ref, bound))
    print("error / bound per geometry case:", ["%.3g" % r for r in seen])
    assert max(seen) > 1.0 and sum(r > 1.0 for r in seen) >= 5


def test_defects_of_the_statistics():
    """M - 1 for M in the biased variance; biased for unbiased in running_var; momentum on the old value"""
    worst = {"M-1": 0.0, "biased": 0.0, "swapped": 0.0}
    for M, C in G.GEOMETRY:
        if M == 1:
            continue
        worst["M-1"] = max(worst["M-1"], _stats_errors(M, C, 0.1, M_for_var=M - 1)[1])
        worst["biased"] = max(worst["biased"], _stats_errors(M, C, 1.0, biased=True)[3])
        worst["swapped"] = max(worst["swapped"], *_stats_errors(M, C, 0.1, swapped=True)[2:])
    print(worst)
    assert min(worst.values()) > 1.0, worst


def test_defect_pad_channel_given_sc_1():
    x, mean, invstd, gam, beta, mul, res, y, e = G.apply_case(231, 33, "hswish", "none", True, True)
    assert O.worst_ratio(apply32(x, mean, invstd, gam, beta, mul, res, 33, O.HSWISH), y, e) <= 1.0
    assert O.worst_ratio(apply32(x, mean, invstd, gam, beta, mul, res, 33, O.HSWISH, pad_sc=1.0), y, e) == float("inf")


def test_defect_argmax_before_the_activation_with_a_negative_gamma():
    Bn, H, W, C = 2, 6, 10, 33
    T, x, beta, dyp, (y_ref, e_y, _), bwd = G.pool_case(Bn, H, W, C, "none")
    assert bool((T.gam[:C] < 0).any())
    y, _, _, dx = pool32(x, dyp, T.mean, T.invstd, T.gam, beta, Bn, H, W, C, O.NONE, True, argmax_before_act=True)
    assert O.worst_ratio(y, y_ref, e_y) > 1e3 and O.worst_ratio(dx, *bwd[True]["dx"]) > 1e3
    neg = T.gam[:C] < 0  # only the channels with a negative gamma are wrong
    assert O.worst_ratio(y[:, :C][:, ~neg], y_ref[:, :C][:, ~neg], e_y[:, :C][:, ~neg]) <= 1.0


def test_defect_hardswish_gradient_at_the_kinks_from_the_outer_branch():
    x = G._kink_inputs()
    z = torch.zeros_like(x, dtype=torch.float64)
    g_ref, e_g = O.act_grad(x.double(), z, O.HSWISH)
    assert g_ref[1, 0] == -0.5 and g_ref[7, 0] == 1.5 and g_ref[0, 0] == 0.0 and g_ref[8, 0] == 1.0
    assert O.worst_ratio(grad32(x, O.HSWISH), g_ref, e_g) <= 1.0
    assert O.worst_ratio(grad32(x, O.HSWISH, outer_at_kink=True), g_ref, e_g) > 1e5
    r_ref, _ = O.act_grad(x.double(), z, O.RELU)
    s_ref, _ = O.act_grad(x.double(), z, O.HSIGMOID)
    assert r_ref[:, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]  # relu'(0) = 0
    assert (s_ref[:, 0] * 6).tolist() == [0, 0, 1, 1, 1, 1, 1, 0, 0]  # the open interval


def test_defect_sum_dzx_built_with_x():
    M, C = 231, 33
    x, mean, invstd, gam, beta, mul, _, s1, s2, dx_ref = G.bwd_case(M, C, "relu", False, True, True)
    T = G.operands(M, C)
    _, a1, a2, dx = bwd32(x, T.dy, mean, invstd, gam, beta, mul, C, O.RELU, M, True, x_for_xhat=True)
    assert O.worst_ratio(a1, *s1) <= 1.0 and O.worst_ratio(a2, *s2) > 1e3 and O.worst_ratio(dx, *dx_ref) > 1e3


def test_the_bound_sees_a_wrong_small_element_the_global_bar_does_not():
    """one element among 231 x 33 off by 1e-5 of the tensor's maximum: inside assert_close's 1e-4 * max, outside the bound"""
    x, mean, invstd, gam, beta, mul, res, y, e = G.apply_case(231, 33, "relu", "none", True, True)
    y32 = apply32(x, mean, invstd, gam, beta, mul, res, 33, O.RELU)
    i = int(y[:, :33].abs().argmin())
    y32.view(-1)[(i // 33) * 36 + i % 33] += 1e-5 * float(y.abs().max())
    assert float((y32.double() - y).abs().max()) <= 1e-4 * float(y.abs().max())
    assert O.worst_ratio(y32, y, e) > 10


# ------------------------------------------------------------------------------------------------ the geometry reached
# (M, C): Cs, panels [(quads, row lanes, idle threads)], reduction grid, its distinct block sizes, empty blocks
EXPECT = {
    (1, 3): (4, [(1, 256, 0)], 1, [1], 0),
    (17, 4): (4, [(1, 256, 0)], 2, [9, 8], 0),
    (231, 33): (36, [(9, 28, 4)], 15, [16, 7], 0),
    (35, 1024): (1024, [(256, 1, 0)], 3, [12, 11], 0),
    (40, 1025): (1028, [(256, 1, 0), (1, 256, 0)], 3, [14, 12], 0),
    (18, 1072): (1072, [(256, 1, 0), (12, 21, 4)], 2, [9], 0),
    (16400, 20): (20, [(5, 51, 1)], 1024, [17, 12, 0], 59),
    (4099, 20): (20, [(5, 51, 1)], 257, [16, 3], 0),
}


def test_the_case_tables_reach_every_geometry_edge():
    assert set(EXPECT) == set(G.GEOMETRY)
    for (M, C), (Cs, pan, nr, rows, empty) in EXPECT.items():
        g = O.geometry(M, C)
        assert (g["Cs"], g["panels"], g["red_blocks"], g["red_rows"], g["red_empty"]) == (Cs, pan, nr, rows, empty), g
    g = O.geometry(1, 3)  # one quad, 256 row lanes, one row: 255 lanes without a row
    assert g["red_lane_rows"] == {0, 1} and g["sweep_blocks"] == 1
    g = O.geometry(16400, 20)  # the block cap: 17 rows per block, 965 live blocks, 59 empty
    assert O.cdiv(16400, 16) > O.RED_MAX_BLOCKS and g["red_blocks"] * 17 >= 16400 > (g["red_blocks"] - 60) * 17
    assert g["sweep_blocks"] == 21 and g["sweep_rows"][0] == 781 and g["sweep_lane_rows"] >= {15, 16}
    g = O.geometry(4099, 20)  # odd and even rows per lane in the split load / accumulate loops (VMTL_RIF = 2)
    assert g["sweep_blocks"] == 6 and g["sweep_rows"] == [684, 679] and g["sweep_lane_rows"] >= {13, 14}
    assert g["red_lane_rows"] == {0, 1}
    g = O.geometry(231, 33)  # a ragged last block and four idle threads
    assert g["red_rows"][-1] == 231 - 14 * 16 and g["sweep_blocks"] == 1 and g["sweep_lane_rows"] == {8, 9}
    g = O.geometry(35, 1024)  # one row lane per quad: every lane walks all rows of its block
    assert g["sweep_lane_rows"] == {12, 11} and g["red_lane_rows"] == {12, 11}
    g = O.geometry(40, 1025)  # the second panel is one quad swept by 256 row lanes
    assert g["sweep_lane_rows"] >= {0, 1, 14, 12}
    g = O.geometry(*G.LARGE_MEAN)
    assert (g["red_blocks"], g["red_rows"], g["panels"], g["red_lane_rows"]) == (1024, [512], [(1, 256, 0)], {2})
    # over the table, the tail loop of the RIF-2 sweeps sees odd and even counts, and lanes without any row
    every = set().union(*(O.geometry(M, C)["sweep_lane_rows"] | O.geometry(M, C)["red_lane_rows"] for M, C in G.GEOMETRY))
    assert 0 in every and any(n % 2 for n in every) and any(n and n % 2 == 0 for n in every)
    # the grid cap of sweep_blocks is out of reach: the largest case is far below it
    assert max(O.sweep_blocks(M, ceil4(C)) for M, C in G.GEOMETRY + (G.LARGE_MEAN,)) < 8192
    for Bn, H, W, C in G.POOL_SHAPES:
        assert H % 2 == 0 and W % 2 == 0
    assert G.NBLK[-1] == 64 and 17 in G.NBLK and [M for _, M in G.GIVEN_ROWS] == [5 * r + 3 for r, _ in G.GIVEN_ROWS]


def test_restated_block_counts_are_the_librarys():
    from vision_mtl_amd._lib import lib

    for M in (-5, 0, 1, 15, 16, 17, 16383, 16384, 16385, 16400, 524288):
        assert lib().raw("vmtl_reduce_rows")(M) == O.red_blocks(M)
