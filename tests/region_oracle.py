"""Test-only oracle of the cross entropy + Dice / Jaccard / Tversky region term (csrc/ce_region.hip), on the CPU in fp64.

  reference(z, t, alpha, beta, smooth, w, ign, ce_weight, region_weight): the whole definition with autograd -
      TP_c, S_c, N_c over the valid pixels of the batch, D_c, T_c, L_region = (1/C) sum_{N_c > 0} (1 - T_c), the weighted
      / ignoring cross entropy, loss = ce_weight * CE + region_weight * L_region and the gradient of GOUT * loss.
  coefficients(...): the closed form a_c, b_c of dL_region/dp_ic = b_c + a_c 1[t_i = c] the kernels use.

Conventions shared with the kernels: the class weights apply to the cross entropy only; an absent class adds 0 and its
coefficients are 0; ce_weight == 0 leaves the cross entropy out (CE reported as 0); every pixel ignored gives
L_region = 0 and CE = NaN."""
import functools

import torch
import torch.nn.functional as F

GOUT = 1.7  # the loss is scaled before backward: grad_output is not 1
IGN = 255
# name: (C, B, H, W).  a: ragged last wave, P = 130; c: the production class count; d: ld = 24 (the wide-ld gradient
# layout); g: the class limit, ld = 36; f: P = 526 683 > 2048 * 256 - the grid-stride loop and every per-block partial row
# h .. l: the remaining register forms (Q = ceil(C / 4) = 3, 4, 6, 7, 8 below the limit)
CASES = {"a": (3, 2, 5, 13), "c": (19, 2, 5, 13), "d": (20, 2, 5, 13), "g": (32, 2, 5, 13), "f": (3, 3, 419, 419),
         "h": (9, 2, 5, 13), "i": (14, 2, 5, 13), "j": (22, 2, 5, 13), "k": (26, 2, 5, 13), "l": (30, 2, 5, 13)}
SMALL = ("a", "c", "d", "g", "h", "i", "j", "k", "l")
VARIANTS = ("c_absent", "c_void_only")  # of case c: one class removed from the labels / present only under void pixels
SETTINGS = ((0.5, 0.5, 0.0), (1.0, 1.0, 0.0), (0.3, 0.7, 1.0))  # (alpha, beta, smooth): Dice, Jaccard, a Tversky


@functools.lru_cache(maxsize=None)
def case(name):
    """Logits randn * 3, labels with about 30 % void pixels, class weights (as ohem_oracle.case); `ign` is the case's
    ignore index.  The variants of c: c_absent relabels every pixel of class 7 as class 8; c_void_only does the same and
    then uses 7 itself as the void label and the ignore index - class 7 is in the label map, but only under void pixels,
    so N_7 = 0 and its coefficients vanish although the kernels meet the label."""
    base = name.split("_")[0]
    C, B, H, W = CASES[base]
    g = torch.Generator().manual_seed(5200 + 17 * sorted(CASES).index(base))
    z = torch.randn(B, C, H, W, generator=g) * 3
    t = torch.randint(0, C, (B, H, W), generator=g)
    void = torch.rand(B, H, W, generator=g) < 0.3
    w = 0.1 + 1.9 * torch.rand(C, generator=g)
    if name != base:
        t[t == 7] = 8
    ign = 7 if name == "c_void_only" else IGN
    t[void] = ign
    valid = t != ign
    return dict(C=C, shape=(B, H, W), z=z, t=t, w=w, ign=ign, valid=valid, V=int(valid.sum()))


def sums(p, t, valid, C):
    """(TP_c, S_c, N_c) of probabilities p (B,C,H,W) over the valid pixels; N_c an int64 tensor."""
    onehot = F.one_hot(t.clamp(0, C - 1), C).permute(0, 3, 1, 2).to(p.dtype) * valid.unsqueeze(1)
    pv = p * valid.unsqueeze(1)
    return (pv * onehot).sum(dim=(0, 2, 3)), pv.sum(dim=(0, 2, 3)), onehot.sum(dim=(0, 2, 3)).round().long()


def region_term(p, t, valid, alpha, beta, smooth):
    """(L_region, T_c, D_c, N_c) by the definition; differentiable in p."""
    C = p.shape[1]
    TP, S, N = sums(p, t, valid, C)
    D = TP + alpha * (S - TP) + beta * (N - TP) + smooth
    present = N > 0
    T = torch.where(present, (TP + smooth) / torch.where(present, D, torch.ones_like(D)), torch.ones_like(D))
    return (1.0 - T)[present].sum() / C, T, D, N


def coefficients(p, t, valid, alpha, beta, smooth):
    """The closed form: (a_c, b_c), zeros for an absent class."""
    C = p.shape[1]
    TP, S, N = sums(p, t, valid, C)
    D = TP + alpha * (S - TP) + beta * (N - TP) + smooth
    m = N > 0
    Ds = torch.where(m, D, torch.ones_like(D))
    b = torch.where(m, alpha * (TP + smooth) / (C * Ds * Ds), torch.zeros_like(D))
    a = torch.where(m, -(1.0 / Ds - (1.0 - alpha - beta) * (TP + smooth) / (Ds * Ds)) / C, torch.zeros_like(D))
    return a, b


def cross_entropy(z, t, valid, w):
    """sum_valid w[t] nll / sum_valid w[t] in the dtype of z (NaN when nothing is valid), with (den, num)"""
    C = z.shape[1]
    tt = t.clamp(0, C - 1)
    nll = -F.log_softmax(z, dim=1).gather(1, tt.unsqueeze(1)).squeeze(1)
    wt = torch.ones_like(nll) if w is None else w.to(z.dtype)[tt]
    num, den = (wt * nll)[valid].sum(), wt[valid].sum()
    return num / den, den, num


def compose(z, t, alpha=0.5, beta=0.5, smooth=0.0, w=None, ign=IGN, ce_weight=1.0, region_weight=1.0):
    """The definition on logits z in z's dtype, differentiable in z: dict(loss, ce, region, ...).  What a step test puts
    in the place of the criterion."""
    valid = torch.ones_like(t, dtype=torch.bool) if ign is None else t != ign
    p = F.softmax(z, dim=1)
    lr, T, D, N = region_term(p, t, valid, alpha, beta, smooth)
    if ce_weight != 0:
        ce, den, num = cross_entropy(z, t, valid, w)
        loss = ce_weight * ce + region_weight * lr
    else:
        ce = den = num = torch.zeros((), dtype=z.dtype)
        loss = region_weight * lr
    return dict(loss=loss, ce=ce, region=lr, p=p, valid=valid, T=T, D=D, N=N, den=den, num=num)


def reference(z, t, alpha=0.5, beta=0.5, smooth=0.0, w=None, ign=IGN, ce_weight=1.0, region_weight=1.0):
    zr = z.double().requires_grad_(True)
    c = compose(zr, t, alpha, beta, smooth, w, ign, ce_weight, region_weight)
    loss, valid = c["loss"], c["valid"]
    grad = torch.zeros_like(zr)
    if loss.requires_grad:  # every pixel ignored and no cross entropy: the loss is the constant 0
        (loss * GOUT).backward()
        grad = zr.grad
    a, b = coefficients(c["p"].detach(), t, valid, alpha, beta, smooth)
    return dict(loss=loss.detach(), ce=c["ce"].detach(), region=c["region"].detach(), grad=grad, coef=torch.cat([a, b]),
                N=c["N"], V=int(valid.sum()), D=c["D"].detach(), T=c["T"].detach(), den=float(c["den"].detach()),
                num=float(c["num"].detach()), valid=valid)
