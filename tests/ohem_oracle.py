"""Test-only oracle of online hard example mining on the cross entropy (csrc/ce_ohem.hip), on the CPU.

  reference(z, t, min_kept_total, thresh, w, ign): the whole definition in fp64 - per-pixel nll, the cut, the kept mask,
      the loss, and the gradient of GOUT * loss by autograd with the mask held fixed (no gradient through the selection).
  select(nll32, valid, K, tau32): the exact cut and kept mask of a GIVEN fp32 nll array, by torch.sort - what the
      device's selection must reproduce bit for bit on its own nll buffer.
  margin(nll64, valid, K, tau): how far the fp64 nll stays from the two decisions a rounding error could flip.

Conventions shared with the kernels: a NaN nll ranks above +inf and is kept; K = min(min_kept_total, V); cut =
min(tau, kappa) with kappa the K-th largest valid nll, and cut = tau when kappa is NaN or K = 0; kept = valid and
not (nll < cut)."""
import functools
import math

import torch
import torch.nn.functional as F

GOUT = 1.7  # the loss is scaled before backward: grad_output is not 1


IGN = 255
# name: (C, B, H, W).  a: ragged last wave, P = 130; c: the production class count; d: the wide-ld gradient layout;
# e: past the 32 logits the register forms hold; f: P = 526 683 > 2048 * 256 - the grid-stride loops, the block cap and
# many blocks feeding one global histogram; g .. k: the remaining register forms (Q = ceil(C / 4) = 3, 4, 6, 7, 8)
CASES = {"a": (3, 2, 5, 13), "c": (19, 2, 5, 13), "d": (20, 2, 5, 13), "e": (33, 2, 5, 13), "f": (3, 3, 419, 419),
         "g": (9, 2, 5, 13), "h": (14, 2, 5, 13), "i": (22, 2, 5, 13), "j": (26, 2, 5, 13), "k": (30, 2, 5, 13)}
SMALL = ("a", "c", "d", "e", "g", "h", "i", "j", "k")
THRESHOLDS = (None, 1.0, 0.7, 1e-6)


@functools.lru_cache(maxsize=None)
def case(name):
    """Logits randn * 3, labels with about 30 % void pixels, class weights; the fp64 nll of the ignoring form."""
    C, B, H, W = CASES[name]
    g = torch.Generator().manual_seed(4100 + 17 * sorted(CASES).index(name))
    z = torch.randn(B, C, H, W, generator=g) * 3
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.3] = IGN
    w = 0.1 + 1.9 * torch.rand(C, generator=g)
    nll, valid = nll64(z, t, IGN)
    return dict(C=C, shape=(B, H, W), z=z, t=t, w=w, nll=nll, valid=valid, V=int(valid.sum()),
                zmax=z.abs().amax(dim=1).double())


def kept_totals(V):
    """the min_kept_total values of the sweep"""
    return (1, 2, V // 2, V - 1, V, V + 5)


def tau_of(thresh):
    return math.inf if thresh is None else -math.log(thresh) + 0.0


def _cut(sorted_desc, K, tau):
    """sorted_desc: the valid nll, descending, NaN first (torch.sort's order).  tau: a 0-d tensor of its dtype."""
    K = min(int(K), sorted_desc.numel())
    if K == 0:
        return tau
    kappa = sorted_desc[K - 1]
    return tau if bool(torch.isnan(kappa)) else torch.minimum(tau, kappa)


def sort_desc(nll, valid):
    return torch.sort(nll[valid], descending=True).values  # torch.sort ranks NaN above every number


def select(nll32, valid, K, tau32, sorted_desc=None):
    """(cut as a 0-d fp32 tensor, kept mask) of the fp32 array nll32; sorted_desc: sort_desc(nll32, valid), to share."""
    assert nll32.dtype == torch.float32
    if sorted_desc is None:
        sorted_desc = sort_desc(nll32, valid)
    cut = _cut(sorted_desc, K, torch.tensor(tau32, dtype=torch.float32))
    return cut, valid & ~(nll32 < cut)


def nll64(z, t, ign):
    """(fp64 nll clamped at 0 with NaN for a valid label outside [0, C), valid mask); differentiable in z."""
    C = z.shape[1]
    valid = torch.ones_like(t, dtype=torch.bool) if ign is None else t != ign
    inside = (t >= 0) & (t < C)
    lp = F.log_softmax(z.double(), dim=1)
    nll = -lp.gather(1, t.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    nll = torch.where(nll > 0, nll, torch.zeros_like(nll))
    return torch.where(inside, nll, torch.full_like(nll, math.nan)), valid


def reference(z, t, min_kept_total, thresh, w=None, ign=None):
    zr = z.double().requires_grad_(True)
    nll, valid = nll64(zr, t, ign)
    key = nll.detach()
    tau = torch.tensor(tau_of(thresh), dtype=torch.float64)
    cut = _cut(sort_desc(key, valid), min_kept_total, tau)
    kept = valid & ~(key < cut)
    wt = torch.ones_like(key) if w is None else w.double()[t.clamp(0, z.shape[1] - 1)]
    loss = (wt * nll)[kept].sum() / wt[kept].sum()
    (loss * GOUT).backward()
    return dict(nll=key, valid=valid, cut=cut, kept=kept, loss=loss.detach(), grad=zr.grad)


def margin(nll, valid, K, tau):
    """The smaller of: the gap between ranks K and K+1 of the valid nll (inf when there is no rank K+1, or K = 0), and
    the distance from tau to the nearest valid nll (inf for tau = 0, which no clamped nll is below, and tau = inf,
    which no finite nll reaches)."""
    s = sort_desc(nll, valid)
    K = min(int(K), s.numel())
    m = math.inf
    if 0 < K < s.numel():
        m = float(s[K - 1] - s[K])
    if 0.0 < tau < math.inf and s.numel():
        m = min(m, float((s - tau).abs().min()))
    return m
