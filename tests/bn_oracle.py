"""fp64 oracle of the BatchNorm and column-reduction kernels (csrc/bn.hip on the sweep skeletons of csrc/reduce.h) with
ELEMENTWISE ROUNDING BOUNDS: plain helper module, the sibling of tests/dwconv_oracle.py.

Everything is computed on the CPU in float64 from the same float32 operands the kernel receives, in the kernel's own
layouts: activations [M][Cs], per-channel vectors [Cs] or [C], statistics rows [nblk][2][Cs] = (mean_b, M2_b) of the
rows [b*rpb, min(M, (b+1)*rpb)).  Lanes c >= C of every result are zero (or `res`), whatever the operands hold there.
Every result comes with a bound of the same shape, computed in float64 from MAGNITUDES; none of the constants below is
fitted to a kernel's error.

    u = 2^-24 (fp32 unit roundoff),  gamma_n = n*u / (1 - n*u)

A value that passes through n fp32 roundings carries a relative error of at most gamma_n (Higham, Accuracy and Stability
of Numerical Algorithms, lemma 3.1); a sum of n terms in ANY order, with or without fused multiply-adds, satisfies
|computed - exact| <= gamma_n * sum |term_i| (section 3.1).  A fused multiply-add only removes a rounding.

Normalisation (normalise).  The forward kernels evaluate sc = gamma*invstd, sh = beta - mean*sc, z = x*sc + sh: the
term x*sc passes the roundings of sc, of the product and of the sum (3), mean*sc those of sc, the product, the
subtraction and the sum (4), beta those of the subtraction and the sum (2).  The backward and pool kernels evaluate
xhat = (x - mean)*invstd, z = gamma*xhat + beta: (x - mean) passes the subtraction, two products and the sum (4), beta
one.  With |x - mean| <= |x| + |mean| both forms satisfy
    e_z = gamma_4 * (|x sc| + |mean sc| + |beta|)
(tighter than the gamma_6 a count without looking at the code would give).  Where mean / invstd are themselves results
(the fused apply publishes them rounded from fp64: "1 ulp", d_mean = 2u|mean|, d_invstd = 2u*invstd) their errors are
carried through: + |x g| d_is + |g| (|mean| d_is + d_mean (invstd + d_is)).  Without BatchNorm z = x exactly, e_z = 0.

Activations (activate), a = act(z) from e_z:
  none, relu    1-Lipschitz and exact:  e_a = e_z
  hardswish     as tests/dwconv_oracle.act_with_error: |h'| <= 1.5 and four relative roundings (fl(z + 3), the product
                z*r, the product with fl(1/6), that constant's representation):  e_a = 1.5 e_z + gamma_4 (|h| + 1.5 e_z)
  hard-sigmoid  clamp(z + 3, 0, 6) / 6: Lipschitz 1/6 and three roundings (fl(z + 3), the constant, the product):
                e_a = e_z/6 + gamma_3 (|hs| + e_z/6)
  sigmoid       goes through __expf, whose accuracy no document at hand states.  Sigmoid outputs AND sigmoid gradients
                therefore keep the suite's bar, 1e-4 of the reference's maximum (BASELINE.json north star), as a uniform
                bound: it is the one bound here that is not derived from roundings.
Gate (y = a*mul) and residual (y = a + res): one rounding each, e <- e|mul| + u (|a mul| + e|mul|), then
e <- e + u (|y + res| + e).

Derivatives (act_grad), torch's conventions (relu'(0) = 0; hardswish' = (2z + 3)/6 on [-3, 3], boundaries included;
hard-sigmoid' = 1/6 on the OPEN interval): none and relu exact; hardswish' inside the kinks has Lipschitz 1/3 and three
roundings (2z is exact; + 3, the constant, the product): e_g = e_z/3 + gamma_3 (|h'| + e_z/3); hard-sigmoid' is the
constant fl(1/6): e_g = u/6; outside the kinks both are exactly 0 or 1.

Backward (bwd_terms, sums_bound, bwd_dx):
  dz   = dy * mul * act'(z): two roundings (one without mul):  e_dz = |dy mul| e_g + gamma_2 |dy mul| (|act'| + e_g)
  dmul = dy * act(z): one rounding:  e = |dy| e_a + u |dy| (|a| + e_a)
  xhat = (x - mean)*invstd from exact operands: two roundings, e_xh = gamma_2 |xhat|
  sum_dz  = sum_m dz: n = M + 1 (M terms in whatever order the row lanes, the workgroups and the fp64 finalize take
            them, + 1 for the finalize's rounding of the fp64 total to fp32):
            sum_m e_dz + gamma_{M+1} sum_m (|dz| + e_dz)
  sum_dzx = sum_m dz*xhat: the product of two inexact factors is off by at most
            e_p = (|dz| + e_dz)(|xhat| + e_xh)(1 + u) - |dz xhat|;  sum_m e_p + gamma_{M+1} sum_m (|dz xhat| + e_p)
  dx   = gamma*invstd*(dz - c1 - xhat*c2), c1 = sum_dz * fl(1/M), c2 = sum_dzx * fl(1/M): c1 carries the sum's own
         error and two roundings, e_c1 = (e_s + gamma_2 (|s| + e_s)) / M; dz, c1 and the product xhat*c2 each pass four
         roundings (their own subtraction or product, the second subtraction, fl(gamma*invstd), the last product):
         e_dx = |gamma invstd| (gamma_4 (|dz| + |c1| + |xhat c2|) + (1 + gamma_4)(e_dz + e_c1 + e_x2)),
         e_x2 = (|xhat| + e_xh)(|c2| + e_c2) - |xhat c2|.   Eval mode and the no-BatchNorm route: c1 = c2 = 0.
  The affine form coef_a*dz + coef_b*x + coef_c (bwd_affine) cancels x against mean, so it is bounded in ITS OWN
  magnitudes.  coef_a = gi = fl(gamma*invstd): 1 rounding; coef_b = -gi*invstd*c2: gi, the two products and the two
  roundings of c2 = sum * fl(1/M): 5; coef_c = gi*(mean*invstd*c2 - c1): c2's two, mean*invstd, its product with c2, the
  subtraction, gi and the last product: 7.  With 7 for every term:
         gamma_7 (|gi dz| + |gi invstd c2| (|x| + |mean|) + |gi c1|) + (1 + gamma_7)|gi| (invstd (|x| + |mean|) e_c2 + e_c1)

Statistics are compared with the project's bars (the GPU module states them), not with a rounding bound; the oracle
provides the exact values: partial_rows (the exact rows of an input), merge_rows (the exact fp64 Chan merge of GIVEN
fp32 rows, rows with count 0 ignored whatever they hold), running (the momentum update, unbiased variance for M > 1
and the biased one for M == 1, with momentum and eps taken as the fp32 values the kernels receive).

Pool (pool2_fwd, pool2_bwd): the window arg-max is taken AFTER the activation, the first maximum in window order
(00, 01, 10, 11) wins and NaN wins; y carries the selected element's activation bound; dx covers all four pixels.

Column sums (colsum, stitch_bwd): gamma_{M+1} sum |term| per channel; the all-channel scalar sums the C rounded
per-channel values in fp64 and rounds once more: gamma_{M+C+1} sum |term|.  dx = w*dy is one product: u |dx|.

Conditions on the INPUTS (not on the kernel): nudge() moves every input whose fp64 pre-activation lies within BAND of a
kink (0 for relu; -3 and 3 for hardswish and hard-sigmoid) to 2*BAND away; check_inputs asserts that afterwards no
element lies within the band and that the case's largest e_z is below BAND/10, so that no correct fp32 evaluation can
land on the other side of a kink and NO element is left out of any comparison.  The pool cases also need the two
largest distinct activations of every window to differ by more than 1e-4 of the larger, and (stricter, for values near
0) by more than four times the window's largest activation bound (check_pool_gap).

The sweep geometry of reduce.h is restated at the end (red_blocks, sweep_blocks, panels, lane_rows)."""
import numpy as np
import torch

U = 2.0 ** -24
BAND = 1e-3
NONE, RELU, HSWISH, HSIGMOID, SIGMOID = 0, 1, 2, 3, 4
ACTS = {"none": NONE, "relu": RELU, "hswish": HSWISH, "hsigmoid": HSIGMOID, "sigmoid": SIGMOID}
KINKS = {NONE: (), RELU: (0.0,), HSWISH: (-3.0, 3.0), HSIGMOID: (-3.0, 3.0), SIGMOID: ()}
SIGMOID_BAR = 1e-4  # of the reference's maximum: the suite's bar, see the docstring


def gamma(n):
    assert n * U < 1
    return n * U / (1.0 - n * U)


def f32(v):
    """the fp32 value of a Python float (what a `float` parameter of the C ABI receives), as a Python float"""
    return float(np.float32(v))


def lanes(C, Cs):
    return (torch.arange(Cs) < C).double()


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (0/0 counts as 0, x/0 as inf); NaN in got is inf"""
    err = (got.double() - ref).abs()
    if torch.isnan(err).any():
        return float("inf")
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


def sigmoid_bar(ref):
    return torch.full_like(ref, SIGMOID_BAR * float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ forward
def _vec(v, Cs, fill):
    return torch.full((Cs,), float(fill), dtype=torch.float64) if v is None else v.double()


def normalise(x, mean, invstd, gam, beta, d_mean=None, d_invstd=None):
    """(z, e_z) in float64, all Cs lanes; mean is None: no BatchNorm (z = x, gamma / beta unused)"""
    x = x.double()
    if mean is None:
        return x.clone(), torch.zeros_like(x)
    Cs = x.shape[-1]
    mean, invstd, g, b = mean.double(), invstd.double(), _vec(gam, Cs, 1), _vec(beta, Cs, 0)
    sc = g * invstd
    z = x * sc + (b - mean * sc)
    e = gamma(4) * ((x * sc).abs() + (mean * sc).abs() + b.abs())
    if d_mean is not None:
        e = e + (x * g).abs() * d_invstd + g.abs() * (mean.abs() * d_invstd + d_mean * (invstd + d_invstd))
    return z, e


def act(z, code):
    if code == RELU:
        return z.clamp_min(0)
    if code == HSWISH:
        return z * (z + 3).clamp(0, 6) / 6
    if code == HSIGMOID:
        return (z + 3).clamp(0, 6) / 6
    if code == SIGMOID:
        return torch.sigmoid(z)
    return z.clone()


def activate(z, e_z, code):
    """(a, e_a); for sigmoid e_a is the input error carried through only (|s'| <= 1/4): the routes use sigmoid_bar"""
    a = act(z, code)
    if code in (NONE, RELU):
        return a, e_z
    if code == HSWISH:
        return a, 1.5 * e_z + gamma(4) * (a.abs() + 1.5 * e_z)
    if code == HSIGMOID:
        return a, e_z / 6 + gamma(3) * (a.abs() + e_z / 6)
    return a, e_z / 4


def act_grad(z, e_z, code):
    """(act'(z), e_g) in torch's conventions"""
    one, zero = torch.ones_like(z), torch.zeros_like(z)
    if code == NONE:
        return one, zero
    if code == RELU:
        return (z > 0).double(), zero
    if code == HSWISH:
        inside = (z >= -3) & (z <= 3)
        g = torch.where(z < -3, zero, torch.where(z > 3, one, (2 * z + 3) / 6))
        return g, torch.where(inside, e_z / 3 + gamma(3) * (g.abs() + e_z / 3), zero)
    if code == HSIGMOID:
        g = torch.where((z > -3) & (z < 3), one / 6, zero)
        return g, U * g
    s = torch.sigmoid(z)
    return s * (1 - s), e_z / 4


def apply(x, mean, invstd, gam, beta, mul, res, C, code, d_mean=None, d_invstd=None):
    """y = act(BN(x)) [* mul] [+ res] and its bound; lanes >= C: 0, or res"""
    Cs = x.shape[-1]
    ok = lanes(C, Cs)
    z, e_z = normalise(x, mean, invstd, gam, beta, d_mean, d_invstd)
    y, e = activate(z, e_z, code)
    y, e = y * ok, e * ok
    if mul is not None:
        m = mul.double()
        e = e * m.abs() + U * ((y * m).abs() + e * m.abs())
        y = y * m * ok  # 0 * junk = 0 in the pad lanes
    if res is not None:
        r = res.double()
        y = y + r
        e = e + U * (y.abs() + e)
        e = torch.where(ok.bool().expand_as(e), e, torch.zeros_like(e))  # 0 + res is exact
    if code == SIGMOID:
        e = sigmoid_bar(y)
    return y, e


def nudge(x, mean, invstd, gam, beta, code, band=BAND):
    """fp32 x with every element whose fp64 pre-activation lies within `band` of a kink moved to 2*band away from it"""
    if not KINKS[code]:
        return x
    x = x.double()
    Cs = x.shape[-1]
    sc = (_vec(gam, Cs, 1) * invstd.double()) if mean is not None else torch.ones(Cs, dtype=torch.float64)
    safe = torch.where(sc == 0, torch.ones_like(sc), sc)
    for _ in range(3):
        z, _ = normalise(x, mean, invstd, gam, beta)
        for k in KINKS[code]:
            d = z - k
            bad = (d.abs() < band) & (sc != 0)
            if bad.any():
                s = torch.where(d >= 0, 1.0, -1.0).double()
                x = torch.where(bad, x + (k + 2 * band * s - z) / safe, x)
        x = x.float().double()
    return x.float()


def check_inputs(z, e_z, code, C, band=BAND):
    """the conditions that let every element be compared: nothing within the band of a kink, e_z far below the band"""
    z, e_z = z[..., :C], e_z[..., :C]
    for k in KINKS[code]:
        d = float((z - k).abs().min())
        assert d >= band, f"an input lies {d:.3e} from the kink {k}: nudge it (condition on the inputs)"
    if KINKS[code]:
        assert float(e_z.max()) < band / 10, f"largest e_z {float(e_z.max()):.3e} is not below a tenth of the band"


# ------------------------------------------------------------------------------------------------ backward
def bwd_terms(x, dy, mean, invstd, gam, beta, mul, C, code):
    """dict of (value, bound) pairs: dz, dmul, xh, dzx (= dz*xhat); lanes >= C are zero"""
    Cs = x.shape[-1]
    ok = lanes(C, Cs)
    x64, dy = x.double(), dy.double() * ok
    z, e_z = normalise(x, mean, invstd, gam, beta)
    a, e_a = activate(z, e_z, code)
    g, e_g = act_grad(z, e_z, code)
    m = mul.double() if mul is not None else torch.ones_like(x64)
    gm = (dy * m).abs()
    dz = dy * m * g
    e_dz = gm * e_g + gamma(2) * gm * (g.abs() + e_g)
    dmul = dy * a
    e_dmul = dy.abs() * e_a + U * dy.abs() * (a.abs() + e_a)
    if mean is not None:
        xh = (x64 - mean.double()) * invstd.double() * ok
    else:
        xh = x64 * ok
    e_xh = gamma(2) * xh.abs() if mean is not None else torch.zeros_like(xh)
    dzx = dz * xh
    e_dzx = (dz.abs() + e_dz) * (xh.abs() + e_xh) * (1 + U) - dzx.abs()
    if code == SIGMOID:
        e_dz, e_dmul, e_dzx = sigmoid_bar(dz), sigmoid_bar(dmul), None
    return dict(z=(z, e_z), dz=(dz * ok, e_dz), dmul=(dmul * ok, e_dmul), xh=(xh, e_xh), dzx=(dzx, e_dzx))


def sums_bound(t, e_t):
    """(sum over rows, bound) of terms t carrying errors e_t: n = M + 1"""
    M = t.shape[0]
    return t.sum(0), e_t.sum(0) + gamma(M + 1) * (t.abs() + e_t).sum(0)


def bwd_sums(T, C, code):
    """((sum_dz, bound), (sum_dzx, bound)) as [C] vectors from bwd_terms' result"""
    s1, b1 = sums_bound(*T["dz"])
    if code == SIGMOID:
        s2 = T["dzx"][0].sum(0)
        return (s1[:C], sigmoid_bar(s1[:C])), (s2[:C], sigmoid_bar(s2[:C]))
    s2, b2 = sums_bound(*T["dzx"])
    return (s1[:C], b1[:C]), (s2[:C], b2[:C])


def _pad_c(v, Cs):
    out = torch.zeros(Cs, dtype=torch.float64)
    out[:v.shape[0]] = v.double()
    return out


def bwd_dx(dz, e_dz, xh, e_xh, invstd, gam, s1, e_s1, s2, e_s2, M, C, training):
    """dx and its bound; s1 / s2 ([C], with their carried bounds) are ignored unless training; invstd None: no BatchNorm"""
    Cs = dz.shape[-1]
    ok = lanes(C, Cs)
    gi = _vec(gam if invstd is not None else None, Cs, 1) * (invstd.double() if invstd is not None else 1.0) * ok
    if training and invstd is not None:
        c1, c2 = _pad_c(s1, Cs) / M, _pad_c(s2, Cs) / M
        e_c1 = (_pad_c(e_s1, Cs) + gamma(2) * (_pad_c(s1, Cs).abs() + _pad_c(e_s1, Cs))) / M
        e_c2 = (_pad_c(e_s2, Cs) + gamma(2) * (_pad_c(s2, Cs).abs() + _pad_c(e_s2, Cs))) / M
    else:
        c1 = c2 = e_c1 = e_c2 = torch.zeros(Cs, dtype=torch.float64)
    dx = gi * (dz - c1 - xh * c2)
    e_x2 = (xh.abs() + e_xh) * (c2.abs() + e_c2) - (xh * c2).abs()
    e = gi.abs() * (gamma(4) * (dz.abs() + c1.abs() + (xh * c2).abs()) + (1 + gamma(4)) * (e_dz + e_c1 + e_x2))
    return dx, e


def bwd_affine(x, dz, mean, invstd, gam, s1, e_s1, s2, e_s2, M, C, training):
    """(coef_a, coef_b, coef_c) exact [Cs] and the bound of coef_a*dz + coef_b*x + coef_c evaluated exactly from the
    kernel's fp32 coefficients, against bwd_dx's dx"""
    Cs = x.shape[-1]
    ok = lanes(C, Cs)
    x, dz, mu, is_ = x.double(), dz.double(), mean.double() * ok, invstd.double() * ok
    gi = _vec(gam, Cs, 1) * is_
    if training:
        c1, c2 = _pad_c(s1, Cs) / M, _pad_c(s2, Cs) / M
        e_c1 = (_pad_c(e_s1, Cs) + gamma(2) * (_pad_c(s1, Cs).abs() + _pad_c(e_s1, Cs))) / M
        e_c2 = (_pad_c(e_s2, Cs) + gamma(2) * (_pad_c(s2, Cs).abs() + _pad_c(e_s2, Cs))) / M
    else:
        c1 = c2 = e_c1 = e_c2 = torch.zeros(Cs, dtype=torch.float64)
    ca, cb, cc = gi, -gi * is_ * c2, gi * (mu * is_ * c2 - c1)
    span = x.abs() + mu.abs()
    e = gamma(7) * ((gi * dz).abs() + (gi * is_ * c2).abs() * span + (gi * c1).abs()) \
        + (1 + gamma(7)) * gi.abs() * (is_ * span * e_c2 + e_c1)
    return (ca, cb, cc), e


# ------------------------------------------------------------------------------------------------ statistics
def partial_rows(x, rpb, nblk=None):
    """exact (mean [nblk][Cs], M2 [nblk][Cs], count [nblk]) of the rows [b*rpb, min(M, (b+1)*rpb)) of x [M][Cs]; blocks
    past M (nblk given) have count 0 and hold zeros"""
    x = x.double()
    M, Cs = x.shape
    n = -(-M // rpb) if nblk is None else nblk
    assert n * rpb >= M
    mean = torch.zeros(n, Cs, dtype=torch.float64)
    m2 = torch.zeros_like(mean)
    cnt = torch.zeros(n, dtype=torch.float64)
    for b in range(n):
        blk = x[b * rpb:min(M, (b + 1) * rpb)]
        if blk.shape[0]:
            mean[b] = blk.mean(0)
            m2[b] = ((blk - mean[b]) ** 2).sum(0)
            cnt[b] = blk.shape[0]
    return mean, m2, cnt


def rows_tensor(mean, m2):
    """the fp32 [nblk][2][Cs] tensor the kernels read"""
    return torch.stack([mean, m2], 1).float()


def row_counts(nblk, rpb, M):
    return torch.tensor([max(0, min(rpb, M - b * rpb)) for b in range(nblk)], dtype=torch.float64)


def merge_rows(rows, cnt, C):
    """exact fp64 merge of given fp32 rows [nblk][2][Cs]: (mean [Cs], biased variance [Cs]); rows with count 0 are
    ignored whatever they hold; lanes >= C are zero"""
    live = cnt > 0
    r, n = rows.double()[live], cnt[live][:, None]
    M = n.sum()
    mean = (r[:, 0] * n).sum(0) / M
    var = (r[:, 1] + n * (r[:, 0] - mean) ** 2).sum(0) / M
    ok = lanes(C, rows.shape[-1])
    return mean * ok, var.clamp_min(0) * ok


def exact_stats(x, C):
    """(mean, biased variance) [Cs] of x [M][Cs] in fp64; lanes >= C zero"""
    x = x.double()
    ok = lanes(C, x.shape[-1])
    mean = x.mean(0)
    return mean * ok, ((x - mean) ** 2).mean(0) * ok


def invstd_of(var, eps, C):
    return lanes(C, var.shape[-1]) / (var + f32(eps)).sqrt()


def running(old_mean, old_var, mean, var, M, momentum):
    """the momentum update of the running buffers ([C]): unbiased variance for M > 1, the biased one for M == 1"""
    mom = f32(momentum)
    C = old_mean.shape[0]
    unb = var[:C] * (M / (M - 1)) if M > 1 else var[:C]
    return (1 - mom) * old_mean.double() + mom * mean[:C], (1 - mom) * old_var.double() + mom * unb


def coefficients(mean, invstd, gam, beta, C):
    """(coef_a, coef_c, bound_a, bound_c) [Cs] of exact fp32 mean / invstd: one rounding, and three"""
    Cs = mean.shape[0]
    ok = lanes(C, Cs)
    g, b = _vec(gam, Cs, 1), _vec(beta, Cs, 0)
    sc = g * invstd.double() * ok
    cc = (b - mean.double() * sc) * ok
    return sc, cc, U * sc.abs(), gamma(3) * (b.abs() + (mean.double() * sc).abs()) * ok


# ------------------------------------------------------------------------------------------------ pool
def _windows(t, B, H, W):
    """[B*H/2*W/2][4][Cs] in window order 00, 01, 10, 11 of an NHWC map given as [B*H*W][Cs]"""
    Cs = t.shape[-1]
    v = t.reshape(B, H // 2, 2, W // 2, 2, Cs).permute(0, 1, 3, 2, 4, 5)
    return v.reshape(B * (H // 2) * (W // 2), 4, Cs)


def _unwindows(v, B, H, W):
    Cs = v.shape[-1]
    return v.reshape(B, H // 2, W // 2, 2, 2, Cs).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, Cs)


def argmax_window(a):
    """first maximum in window order, NaN wins (a later NaN replaces an earlier one): [Mp][Cs] indices"""
    am = torch.zeros(a.shape[0], a.shape[2], dtype=torch.long)
    best = a[:, 0].clone()
    for w in range(1, 4):
        v = a[:, w]
        take = (v > best) | torch.isnan(v)
        am = torch.where(take, torch.full_like(am, w), am)
        best = torch.where(take, v, best)
    return am, best


def pool2_fwd(x, mean, invstd, gam, beta, B, H, W, C, code):
    """y [Mp][Cs], its bound, and the arg-max [Mp][Cs]"""
    ok = lanes(C, x.shape[-1])
    z, e_z = normalise(x, mean, invstd, gam, beta)
    a, e_a = activate(z, e_z, code)
    aw, ew = _windows(a, B, H, W), _windows(e_a, B, H, W)
    am, y = argmax_window(aw)
    e = ew.gather(1, am[:, None, :]).squeeze(1)
    y = y * ok
    if code == SIGMOID:
        e = sigmoid_bar(torch.nan_to_num(y))
    return y, e * ok, am


def check_pool_gap(x, mean, invstd, gam, beta, B, H, W, C, code):
    """the two largest DISTINCT activations of every window differ by more than 1e-4 of the larger and by more than four
    times the window's largest activation bound (exact ties stay: the first wins on both sides)"""
    z, e_z = normalise(x, mean, invstd, gam, beta)
    a, e_a = activate(z, e_z, code)
    aw, ew = _windows(a, B, H, W)[..., :C], _windows(e_a, B, H, W)[..., :C]
    top = aw.max(1, keepdim=True).values
    below = torch.where(aw < top, aw, torch.full_like(aw, float("-inf"))).max(1).values
    top = top.squeeze(1)
    has = torch.isfinite(below)
    gap = (top - below)[has]
    assert bool((gap > 1e-4 * top.abs()[has]).all()), "two window candidates are closer than 1e-4 of the larger"
    # near 0 that relative gap says nothing: the candidates must also be apart by more than their own rounding bounds
    assert bool((gap > 4 * ew.max(1).values[has]).all()), "two window candidates are within their rounding bounds"


def pool2_bwd(x, dyp, mean, invstd, gam, beta, B, H, W, C, code, training):
    """dict: s1, s2 ((value, bound) [C]) and dx ((value, bound) [B*H*W][Cs]); M of the BatchNorm is B*H*W"""
    Cs = x.shape[-1]
    ok = lanes(C, Cs)
    M = B * H * W
    z, e_z = normalise(x, mean, invstd, gam, beta)
    a, _ = activate(z, e_z, code)
    g, e_g = act_grad(z, e_z, code)
    am, _ = argmax_window(_windows(a, B, H, W))
    sel = torch.zeros(am.shape[0], 4, Cs, dtype=torch.float64).scatter_(1, am[:, None, :], 1.0)
    dyw = _unwindows(sel * dyp.double()[:, None, :], B, H, W) * ok  # the pooled gradient at its arg-max, 0 elsewhere
    dz = dyw * g
    e_dz = dyw.abs() * e_g + U * dyw.abs() * (g.abs() + e_g)
    xh = (x.double() - mean.double()) * invstd.double() * ok
    e_xh = gamma(2) * xh.abs()
    dzx = dz * xh
    e_dzx = (dz.abs() + e_dz) * (xh.abs() + e_xh) * (1 + U) - dzx.abs()
    # the kernels sum one term per WINDOW (the three zeros of a window are never added): n = Mp + 1 <= M + 1
    s1, b1 = sums_bound(dz, e_dz)
    s2, b2 = sums_bound(dzx, e_dzx)
    if code == SIGMOID:
        e_dz, b1, b2 = sigmoid_bar(dz), sigmoid_bar(s1[:C]), sigmoid_bar(s2[:C])
        b1, b2 = _pad_c(b1, Cs), _pad_c(b2, Cs)
    dx, e_dx = bwd_dx(dz, e_dz, xh, e_xh, invstd, gam, s1[:C], b1[:C], s2[:C], b2[:C], M, C, training)
    if code == SIGMOID:
        e_dx = sigmoid_bar(dx)
    return dict(s1=(s1[:C], b1[:C]), s2=(s2[:C], b2[:C]), dx=(dx, e_dx))


# ------------------------------------------------------------------------------------------------ column sums
def colsum(a, b, C, mode, reduce_all):
    """out [C] (or [1]) and its bound; mode 0: sum a, mode 1: sum a*b"""
    t = a.double() if mode == 0 else a.double() * b.double()
    M = t.shape[0]
    t = t[:, :C]
    if reduce_all:
        return t.sum().reshape(1), (gamma(M + C + 1) * t.abs().sum()).reshape(1)
    return t.sum(0), gamma(M + 1) * t.abs().sum(0)


def stitch_bwd(x, dy, w, C, wstride, reduce_all):
    """(dx, bound), (dw, bound): dx = w[c*wstride]*dy with zero pad lanes, dw = sum x*dy"""
    Cs = x.shape[-1]
    wc = torch.zeros(Cs, dtype=torch.float64)
    wc[:C] = w.double()[torch.arange(C) * wstride]
    dx = dy.double() * wc
    return (dx, U * dx.abs()), colsum(x, dy, C, 1, reduce_all)


# ------------------------------------------------------------------------------------------------ reduce.h, restated
RED_THREADS, RED_MAX_BLOCKS, RIF = 256, 1024, 2


def cdiv(a, b):
    return -(-a // b)


def red_blocks(M):
    return max(1, min(cdiv(M, 16), RED_MAX_BLOCKS))


def sweep_blocks(M, Cs):
    per_blk = max(1, RED_THREADS * 16 // max(1, Cs // 4))
    return max(1, min(cdiv(M, per_blk), 8192))


def panels(Cs):
    """[(quads in the panel, row lanes per quad, idle threads)] for the column panels of 256 quads"""
    CQ, out = Cs // 4, []
    for q0 in range(0, CQ, RED_THREADS):
        cq = min(CQ - q0, RED_THREADS)
        rpt = RED_THREADS // cq
        out.append((cq, rpt, RED_THREADS - rpt * cq))
    return out


def block_rows(M, nblk):
    """rows of each block of a grid of nblk blocks (trailing blocks may be empty)"""
    rpb = cdiv(M, nblk)
    return [max(0, min(rpb, M - b * rpb)) for b in range(nblk)]


def lane_rows(M, Cs, nblk):
    """the set of rows-per-lane counts over every block, panel and row lane of a sweep of [M][Cs] by nblk blocks"""
    seen = set()
    for rows in set(block_rows(M, nblk)):
        for _, rpt, _ in panels(Cs):
            seen |= {len(range(ro, rows, rpt)) for ro in range(rpt)}
    return seen


def geometry(M, C):
    """what a case reaches: both grids of the kernels that sweep [M][ceil4(C)]"""
    Cs = (C + 3) // 4 * 4
    nr, ns = red_blocks(M), sweep_blocks(M, Cs)
    br = block_rows(M, nr)
    return dict(Cs=Cs, panels=panels(Cs), red_blocks=nr, red_rows=sorted(set(br), reverse=True), red_empty=br.count(0),
                sweep_blocks=ns, sweep_rows=sorted(set(block_rows(M, ns)), reverse=True),
                red_lane_rows=lane_rows(M, Cs, nr), sweep_lane_rows=lane_rows(M, Cs, ns))
