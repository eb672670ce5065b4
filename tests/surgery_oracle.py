"""fp64 oracle of the two-task gradient surgery (csrc/surgery.hip, vision_mtl_amd/surgery.py), on the CPU.

gram(a, b)                     (n_a, d, n_b) = (<a,a>, <a,b>, <b,b>) as Python floats, summed in fp64 by math.fsum's
                               exactly rounded sum of the (exact) fp64 products
coefficients(method, n_a, d, n_b)  (alpha, beta) in fp64, the closed forms of include/vmtl.h
cosine(n_a, d, n_b)            d / sqrt(n_a n_b), 0 on the pass-through cases
combine(a, b, alpha, beta)     alpha a + beta b in fp64
gram_bound(a, b)               the derived bound of the device's three sums: n * 2^-53 * sum |x_i y_i| each - products of two
                               fp32 values are exact in fp64 and a sum of n terms in ANY order is within (n - 1) u sum|.| (+ O(u^2))
pair(kind, n, seed)            the gradient pairs of the tests, fp32, built so that no branch is taken near its boundary
"""
import math

import torch

METHODS = ("sum", "pcgrad", "mgda", "imtl_g")
KINDS = ("conflict", "agree", "short", "disjoint")
U64 = 2.0 ** -53
U32 = 2.0 ** -24


def gram(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return (math.fsum((a * a).tolist()), math.fsum((a * b).tolist()), math.fsum((b * b).tolist()))


def gram_fast(a, b):
    """gram for long vectors (a million elements): torch's pairwise fp64 sums, ~1e-16 * sqrt(n) of fsum's"""
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a * a).sum()), float((a * b).sum()), float((b * b).sum())


def gram_bound(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    n = a.numel()
    return tuple(n * U64 * float(x.abs().sum()) for x in (a * a, a * b, b * b))


def passes_through(n_a, d, n_b) -> bool:
    """a zero norm or a Gram entry that is not finite: every method hands the plain sum on"""
    return not (all(math.isfinite(v) for v in (n_a, d, n_b)) and n_a > 0.0 and n_b > 0.0)


def mgda_gamma_unclipped(n_a, d, n_b):
    den = n_a - 2.0 * d + n_b
    return None if den <= 0.0 else (n_b - d) / den


def coefficients(method, n_a, d, n_b):
    if method not in METHODS:
        raise ValueError(f"surgery oracle: method must be one of {METHODS}, got {method!r}")
    if passes_through(n_a, d, n_b) or method == "sum":
        return 1.0, 1.0
    if method == "pcgrad":
        return (1.0 - d / n_a, 1.0 - d / n_b) if d < 0.0 else (1.0, 1.0)
    if method == "mgda":
        g = mgda_gamma_unclipped(n_a, d, n_b)
        g = 0.5 if g is None else min(max(g, 0.0), 1.0)
        return g, 1.0 - g
    alpha = math.sqrt(n_b) / (math.sqrt(n_a) + math.sqrt(n_b))
    return alpha, 1.0 - alpha


def cosine(n_a, d, n_b):
    return 0.0 if passes_through(n_a, d, n_b) else d / math.sqrt(n_a * n_b)


def conflicts(n_a, d, n_b) -> bool:
    return not passes_through(n_a, d, n_b) and d < 0.0


def combine(a, b, alpha, beta):
    return alpha * a.detach().double().cpu() + beta * b.detach().double().cpu()


def pair(kind, n, seed=0):
    """(a, b) fp32 CPU vectors of n elements.
    conflict: b = -0.6 a + 0.5 noise (cos about -0.77)   agree: b = 0.4 a + 0.7 noise (cos about +0.5, MGDA's gamma about 0.3)
    short: b = 0.05 a (cos 1; MGDA clips to b, the short one)   disjoint: a on even, b on odd indices (d == 0 exactly)"""
    if kind not in KINDS:
        raise ValueError(kind)
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + 7 * n % 9973 + seed)
    a = torch.randn(n, generator=g)
    noise = torch.randn(n, generator=g)
    if kind == "conflict":
        b = -0.6 * a + 0.5 * noise
    elif kind == "agree":
        b = 0.4 * a + 0.7 * noise
    elif kind == "short":
        b = 0.05 * a
    else:
        even = (torch.arange(n) % 2 == 0)
        a, b = torch.where(even, a, torch.zeros(())), torch.where(even, torch.zeros(()), noise)
    return a.float().contiguous(), b.float().contiguous()


def away_from_boundaries(n_a, d, n_b) -> bool:
    """the PCGrad branch (sign of d) and the MGDA clip are decided the same way by anyone who sums in another order:
    |cos| >= 0.09 or d == 0 exactly, and the unclipped gamma at least 1e-3 away from 0 and 1"""
    if passes_through(n_a, d, n_b):
        return True
    c = cosine(n_a, d, n_b)
    g = mgda_gamma_unclipped(n_a, d, n_b)
    return (d == 0.0 or abs(c) >= 0.09) and g is not None and min(abs(g), abs(g - 1.0)) >= 1e-3
