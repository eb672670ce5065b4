"""Test-only oracle (not collected) of the depth loss with multi-scale gradient matching (csrc/depth_grad.hip), restated in
fp64 torch from the definition:

    valid v, R = log(pred) - log(target) on valid pixels;  for k < scales, s = 2^k, on the [:, ::s, ::s] subsamples:
    N_k = #valid,  S_k = sum |R[.., 1:] - R[.., :-1]| + sum |R[.., 1:, :] - R[.., :-1, :]| over pairs with both ends valid,
    L_grad = sum_k (S_k / N_k if N_k > 0 else 0),  loss = silog_weight * SILog + grad_weight * L_grad,

with autograd for the gradient (d|a|/da = 0 at a == 0, dL/dpred = 0 at invalid pixels).

signs_from = an fp32 residual image (the device's `resid`): each pair's |dR| is then evaluated as sgn(dR_device) * dR_fp64,
so that arithmetic can be compared where a near-tie was decided the other way; the pairs whose device sign differs from
the fp64 sign come back in `flips` with their |dR_fp64| - a flip is legitimate only inside the rounding band, which is for
the caller to assert.  The sign of an fp32 difference is the sign of the exact difference of the two fp32 values
(subnormals are kept), so it is taken here from the fp32 values in fp64.

case(name): the named inputs, cached; CASES lists them."""
import functools
import math

import torch

GOUT = 0.37
MIN_DEPTH = 1e-3
RESID_TOL = 2.0 ** -19   # per pixel, times max(1, |log pred|, |log target|): one logf pair and a subtraction
MARGIN = 2.0 ** -10      # the smallest |dR| of a margin-built case, before pred is rounded to fp32
MARGIN_SCALES = 4        # the period-16 field of the margin-built cases ties at step 16

SHAPES = {"odd": (2, 5, 13), "one": (1, 1, 1), "row": (1, 1, 40), "col": (1, 40, 1), "edge": (1, 9, 17), "out": (1, 8, 16),
          "seams": (3, 33, 70), "wide": (2, 40, 300), "cap": (5, 512, 512), "long": (1, 1, (1 << 24) + 8)}
# name -> (shape, validity pattern, how pred is built)
CASES = {}
for _s in SHAPES:
    CASES[f"{_s}-holes"] = (_s, "holes", "random")
    if _s not in ("cap", "long"):  # the two large shapes: above the forward's block cap; a row too long for int offsets
        CASES[f"{_s}-holes-margin"] = (_s, "holes", "margin")
for _s in ("odd", "seams"):
    CASES[f"{_s}-checker"] = (_s, "checker", "random")
    CASES[f"{_s}-deadimage"] = (_s, "deadimage", "random")
    CASES[f"{_s}-dead"] = (_s, "dead", "random")
    CASES[f"{_s}-full-margin"] = (_s, "full", "margin")
CASES["edge-checker"] = ("edge", "checker", "random")
MARGIN_CASES = sorted(n for n, c in CASES.items() if c[2] == "margin")


def _valid(pattern, shape, g):
    B, H, W = shape
    if pattern == "holes":
        return torch.rand(B, H, W, generator=g) >= 0.3
    if pattern == "checker":
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        return ((yy + xx) % 2 == 0).expand(B, H, W).clone()
    if pattern == "deadimage":
        v = torch.rand(B, H, W, generator=g) >= 0.3
        v[B // 2] = False
        return v
    if pattern == "dead":
        return torch.zeros(B, H, W, dtype=torch.bool)
    assert pattern == "full"
    return torch.ones(B, H, W, dtype=torch.bool)


@functools.lru_cache(maxsize=None)
def case(name):
    """pred, target (fp32 (B,H,W), target 0 at invalid pixels so that `target > MIN_DEPTH` is the mask), valid (bool)"""
    sname, pattern, kind = CASES[name]
    shape = SHAPES[sname]
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    valid = _valid(pattern, shape, g)
    target = (0.05 + 0.6 * torch.rand(B, H, W, generator=g)).float()
    if kind == "margin":
        px, py = torch.randperm(16, generator=g), torch.randperm(16, generator=g)
        q = px[torch.arange(W) % 16].view(1, 1, W) + 16 * py[torch.arange(H) % 16].view(1, H, 1) - 128
        pred = (target.double() * torch.exp(q.double() / 1024)).float()
    else:
        pred = (target.double() * torch.exp(0.25 * torch.randn(B, H, W, generator=g).double())).clamp(0.01, 0.99).float()
    target = torch.where(valid, target, torch.zeros_like(target))
    return dict(name=name, shape=shape, pred=pred, target=target, valid=valid)


def resid64(pred, target, valid):
    """fp64 R, 0 at invalid pixels (whose pred / target are not looked at)"""
    one = torch.ones((), dtype=torch.float64)
    p, t = torch.where(valid, pred.double(), one), torch.where(valid, target.double(), one)
    return torch.where(valid, torch.log(p) - torch.log(t), torch.zeros((), dtype=torch.float64))


def resid_bound(pred, target, valid):
    """per pixel RESID_TOL * max(1, |log pred|, |log target|); 0 at invalid pixels (resid is exactly 0 there)"""
    one = torch.ones((), dtype=torch.float64)
    lp = torch.log(torch.where(valid, pred.double(), one)).abs()
    lt = torch.log(torch.where(valid, target.double(), one)).abs()
    return torch.where(valid, RESID_TOL * torch.maximum(torch.maximum(lp, lt), one), torch.zeros((), dtype=torch.float64))


def _pairs(img, s):
    """(low end, high end) views of the x pairs and of the y pairs of the [::s, ::s] subsample"""
    sub = img[:, ::s, ::s]
    return (sub[:, :, :-1], sub[:, :, 1:]), (sub[:, :-1, :], sub[:, 1:, :])


def margin(pred, target, valid, scales):
    """the smallest |dR_fp64| over the valid pairs of all scales (inf when there is none)"""
    R = resid64(pred, target, valid)
    m = math.inf
    for k in range(scales):
        for (a, b), (va, vb) in zip(_pairs(R, 1 << k), _pairs(valid, 1 << k)):
            both = va & vb
            if both.any():
                m = min(m, float((b - a).abs()[both].min()))
    return m


def compose(p, target, valid, scales, silog_weight=1.0, grad_weight=0.5, signs_from=None):
    """The loss as a differentiable function of p ((B,H,W), any float dtype, may be part of a larger graph), in p's dtype:
    dict(loss, silog, lgrad, counts, resid[, flips])."""
    B, H, W = p.shape
    one, zero = torch.ones((), dtype=p.dtype), torch.zeros((), dtype=p.dtype)
    R = torch.where(valid, torch.log(torch.where(valid, p, one)) - torch.log(torch.where(valid, target.to(p.dtype), one)), zero)
    index = torch.arange(B * H * W).view(B, H, W)
    dev = None if signs_from is None else signs_from.double()
    lgrad, counts = zero.clone(), []
    fa, fi, fj = [], [], []
    for k in range(scales):
        s = 1 << k
        n = int(valid[:, ::s, ::s].sum())
        counts.append(n)
        sk = zero.clone()
        pr, pv, pi = _pairs(R, s), _pairs(valid, s), _pairs(index, s)
        pd = None if dev is None else _pairs(dev, s)
        for axis in range(2):
            d = pr[axis][1] - pr[axis][0]
            both = pv[axis][0] & pv[axis][1]
            if dev is None:
                term = d.abs()
            else:
                sg = torch.sign(pd[axis][1] - pd[axis][0]).to(p.dtype)
                term = sg * d
                flip = both & (sg != torch.sign(d.detach()))
                fa.append(d.detach().abs()[flip])
                fi.append(pi[axis][0][flip])
                fj.append(pi[axis][1][flip])
            sk = sk + torch.where(both, term, zero).sum()
        if n > 0:
            lgrad = lgrad + sk / n
    silog = zero.clone()
    if silog_weight != 0:
        g = R[valid]
        silog = 10 * torch.sqrt(torch.var(g) + 0.15 * torch.mean(g) ** 2)  # reference losses.py:29-36
    loss = grad_weight * lgrad
    if silog_weight != 0:
        loss = loss + silog_weight * silog
    out = dict(loss=loss, silog=silog, lgrad=lgrad, counts=counts, resid=R)
    if dev is not None:
        out["flips"] = dict(absdr=torch.cat(fa), i=torch.cat(fi), j=torch.cat(fj))
    return out


def reference(pred, target, valid, scales, silog_weight=1.0, grad_weight=0.5, signs_from=None, gout=GOUT):
    """compose() in fp64 on a leaf, detached, plus grad = gout * dloss/dpred, (B,H,W) fp64.
    flips (with signs_from): dict(absdr, i, j) - |dR_fp64| and the flat pixel indices of both ends of every pair whose
    device sign differs from the fp64 sign."""
    p = pred.double().clone().requires_grad_(True)
    out = compose(p, target, valid, scales, silog_weight, grad_weight, signs_from)
    if out["loss"].requires_grad:
        (out["loss"] * gout).backward()
    for k in ("loss", "silog", "lgrad", "resid"):
        out[k] = out[k].detach()
    out["grad"] = torch.zeros_like(out["resid"]) if p.grad is None else p.grad
    return out
