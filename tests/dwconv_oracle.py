"""fp64 oracle of the depthwise-conv kernels (csrc/dwconv.hip) with ELEMENTWISE ROUNDING BOUNDS: plain helper module.

Everything is computed on the CPU in float64 from the same float32 inputs the kernel gets, in the kernel's own layouts:
activations NHWC [B][H][W][Cs], weights packed [K*K][Cs] (tap t = dh*K + dw), coefficients [Cs], dw in torch's
(C, K*K) order.  Every result comes with a bound of the same shape, computed in float64 from MAGNITUDES - it is derived
below, not fitted to any kernel's error:

    u = 2^-24 (fp32 unit roundoff),  gamma_n = n*u / (1 - n*u)

A sum of n products evaluated in fp32 in ANY order, with or without fused multiply-adds, satisfies
|computed - exact| <= gamma_n * sum |term_i|  (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: every
term passes through at most n roundings - its product and at most n-1 additions).

  y  = dwconv(a):   n = K*K (the taps of one output; border outputs have fewer, the bound stays valid).
                    bound = gamma_{K*K} * sum_t |a_t| |w_t|
  dx = dwconv^T(dy) [+ addend]:  n = K*K (at most K*K taps reach one input pixel), with addend n = K*K + 1 and |addend|
                    joins the magnitude.   bound = gamma_n * (sum_t |dy_t| |w_t| + |addend|)
  dw[c][t] = sum over the M = B*Ho*Wo output pixels of dy * x(shifted):  n = M + 1 - M for the sum in whatever order
                    the row lanes, wave shuffles, workgroups and the fp64 finalize take it, + 1 for the finalize's
                    rounding of the fp64 total to fp32.   bound = gamma_{M+1} * sum |dy| |x|

The fused node's prologue a = act(ca*x + cc) is itself rounded, and its error enters y through the taps:
  v = ca*x + cc: one rounding as an fma, two as multiply + add: |v_hat - v| <= e_v = 2u (|ca*x| + |cc|).
  none, relu:    1-Lipschitz and exact in fp32:  e_a = e_v                                          (L_act = 1)
  hardswish:     h(v) = v * clamp(v + 3, 0, 6) / 6, |h'| <= 1.5 (reached at v = 3):  the input error gives 1.5 * e_v
                 (L_act = 1.5).  Its own roundings: fl(v + 3) (rounding is monotone, so the clamp's 0 and 6 are still exact
                 and the clamped factor is off by at most u * clamp(v+3, 0, 6)), the product v * r, the product with the
                 constant fl(1/6) and that constant's own representation: four relative errors of u on |h|.
                 e_a = 1.5 * e_v + gamma_4 * (|h(v)| + 1.5 * e_v)
  a_out = a:        bound = e_a
  y (fused):        bound = gamma_{K*K} * sum_t |a_t| |w_t|  +  (1 + gamma_{K*K}) * sum_t e_a,t |w_t|

Statistics rows: per row i of `rpb` output pixels, the exact (mean, M2 = sum (y - mean)^2, count) of the oracle's y over
pixels [i*rpb, min(M, (i+1)*rpb)).  These are compared with the project's statistics bars (see the GPU module), not with
a rounding bound.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
ACT_NONE, ACT_RELU, ACT_HSWISH = 0, 1, 2


def gamma(n):
    assert n * U < 1
    return n * U / (1.0 - n * U)


def out_size(n, K, stride, pad):
    return (n + 2 * pad - K) // stride + 1


def act_with_error(x, ca, cc, act):
    """(a, e_a) in float64: a = act(ca*x + cc) and the bound of its fp32 evaluation (derivation in the module docstring)."""
    x, ca, cc = x.double(), ca.double(), cc.double()
    v = ca * x + cc
    e_v = 2 * U * ((ca * x).abs() + cc.abs())
    if act == ACT_NONE:
        return v, e_v
    if act == ACT_RELU:
        return v.clamp_min(0), e_v
    assert act == ACT_HSWISH
    h = v * (v + 3).clamp(0, 6) / 6
    return h, 1.5 * e_v + gamma(4) * (h.abs() + 1.5 * e_v)


def _taps(ap, Ho, Wo, K, stride):
    """the K*K strided views of the zero-padded NHWC map that meet output pixel (ho, wo): [(t, view [B][Ho][Wo][Cs])]"""
    for dh in range(K):
        for dw in range(K):
            yield dh * K + dw, ap[:, dh:dh + (Ho - 1) * stride + 1:stride, dw:dw + (Wo - 1) * stride + 1:stride, :]


def _pad_hw(a, pad):
    return F.pad(a, (0, 0, pad, pad, pad, pad))


def fwd(a, wp, K, stride, pad, e_a=None):
    """y = dwconv(a) and its bound; a is float64 (or float32) NHWC, e_a the elementwise error of a (fused node)."""
    a, w = a.double(), wp.double()
    B, H, W, Cs = a.shape
    Ho, Wo = out_size(H, K, stride, pad), out_size(W, K, stride, pad)
    ap = _pad_hw(a, pad)
    ep = _pad_hw(e_a, pad) if e_a is not None else None
    y = torch.zeros(B, Ho, Wo, Cs, dtype=torch.float64)
    mag, carried = torch.zeros_like(y), torch.zeros_like(y)
    for t, v in _taps(ap, Ho, Wo, K, stride):
        y += v * w[t]
        mag += v.abs() * w[t].abs()
    if ep is not None:
        for t, v in _taps(ep, Ho, Wo, K, stride):
            carried += v * w[t].abs()
    g = gamma(K * K)
    return y, g * mag + (1 + g) * carried


def bwd_data(dy, wp, H, W, K, stride, pad, addend=None):
    """dx = dwconv^T(dy) [+ addend] and its bound"""
    dy, w = dy.double(), wp.double()
    B, Ho, Wo, Cs = dy.shape
    dxp = torch.zeros(B, H + 2 * pad, W + 2 * pad, Cs, dtype=torch.float64)
    magp = torch.zeros_like(dxp)
    ady = dy.abs()
    for (t, v), (_, m) in zip(_taps(dxp, Ho, Wo, K, stride), _taps(magp, Ho, Wo, K, stride)):
        v += dy * w[t]
        m += ady * w[t].abs()
    dx, mag = dxp[:, pad:pad + H, pad:pad + W, :].clone(), magp[:, pad:pad + H, pad:pad + W, :].clone()
    n = K * K
    if addend is not None:
        dx += addend.double()
        mag += addend.double().abs()
        n += 1
    return dx, gamma(n) * mag


def bwd_weight(x, dy, C, K, stride, pad):
    """dw in the torch (C, K*K) order and its bound; x is what the kernel reads (the fused node's a_out)"""
    x, dy = x.double(), dy.double()
    B, Ho, Wo, Cs = dy.shape
    xp = _pad_hw(x, pad)
    dw = torch.zeros(K * K, Cs, dtype=torch.float64)
    mag = torch.zeros_like(dw)
    ady = dy.abs()
    for t, v in _taps(xp, Ho, Wo, K, stride):
        dw[t] = (v * dy).sum((0, 1, 2))
        mag[t] = (v.abs() * ady).sum((0, 1, 2))
    M = B * Ho * Wo
    return dw[:, :C].t().contiguous(), gamma(M + 1) * mag[:, :C].t().contiguous()


def stat_rows(y, rpb):
    """(mean [rows][Cs], M2 [rows][Cs], count [rows]) of the output pixels [i*rpb, min(M, (i+1)*rpb)), exact in float64"""
    y = y.double().reshape(-1, y.shape[-1])
    M = y.shape[0]
    rows = (M + rpb - 1) // rpb
    mean = torch.zeros(rows, y.shape[1], dtype=torch.float64)
    m2 = torch.zeros_like(mean)
    cnt = torch.zeros(rows, dtype=torch.float64)
    for i in range(rows):
        blk = y[i * rpb:min(M, (i + 1) * rpb)]
        mean[i] = blk.mean(0)
        m2[i] = ((blk - mean[i]) ** 2).sum(0)
        cnt[i] = blk.shape[0]
    return mean, m2, cnt


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (0/0 counts as 0, x/0 as inf); NaN in got is inf"""
    err = (got.double() - ref).abs()
    if torch.isnan(err).any():
        return float("inf")
    if err.numel() == 0:
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())
