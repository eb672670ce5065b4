"""fp64 restatement of the averaged weights of csrc/weight_avg.hip / dp.ArenaAverage, in plain torch on the CPU.

Modes
  "ema"            e += (1 - d) * (p - e), d = decay
  "ema" + warmup   the same with d = min(decay, (1 + n) / (10 + n)), n = updates so far (timm's rule)
  "swa"            e += (p - e) / (n + 1)
The first update (n == 0) is an exact copy in every mode, as torch's AveragedModel does it; a skipped update (the
optimizer skipped its step) changes neither the average nor n.

The weight of an update is computed in double and rounded once to fp32 - weight_fp32() is the number the kernels apply and
the state block shows - and the oracle applies that fp32 weight in double arithmetic, so what is left between it and a
kernel is the kernel's own fp32 arithmetic.

Bound.  One update computes e + w (p - e) in fp32: with |p - e| <= 2 max(|e|, |p|) and w <= 1, three roundings give at
most 1.25 * 2^-22 * max(|e|, |p|).  PER_UPDATE = 2^-21 of max(|e|, |p|) is allowed per update; an earlier error is
carried with the factor 1 - w <= 1, so the allowances add up over the updates (AverageOracle.bound).  A copy is exact and
resets the allowance to zero."""
import torch

MODES = ("ema", "swa")
PER_UPDATE = 2.0 ** -21


def weight(n, mode="ema", decay=0.999, warmup=False):
    """(w as a Python double, copy flag) of the update that finds n earlier updates."""
    if mode not in MODES:
        raise ValueError(mode)
    if n == 0:
        return 1.0, True
    if mode == "swa":
        return 1.0 / (n + 1), False
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return 1.0 - d, False


def weight_fp32(n, mode="ema", decay=0.999, warmup=False):
    """The weight rounded once to fp32, as a Python float."""
    return float(torch.tensor(weight(n, mode, decay, warmup)[0], dtype=torch.float64).float())


class AverageOracle:
    """e (double), n and the accumulated element-wise allowance after each update()."""

    def __init__(self, p0, mode="ema", decay=0.999, warmup=False):
        self.mode, self.decay, self.warmup = mode, decay, warmup
        self.e = p0.detach().double().clone()  # dp.ArenaAverage starts as a copy of the parameters
        self.bound = torch.zeros_like(self.e)
        self.n = 0

    def update(self, p, skipped=False):
        if skipped:
            return self
        p = p.detach().double()
        _, copy = weight(self.n, self.mode, self.decay, self.warmup)
        if copy:
            self.e = p.clone()
            self.bound = torch.zeros_like(self.e)
        else:
            w = weight_fp32(self.n, self.mode, self.decay, self.warmup)
            self.bound = self.bound + PER_UPDATE * torch.maximum(self.e.abs(), p.abs())
            self.e = self.e + w * (p - self.e)
        self.n += 1
        return self


def assert_within(got, oracle, what=""):
    """|got - oracle.e| <= oracle.bound element-wise; prints the worst ratio before it asserts."""
    err = (got.detach().double().cpu() - oracle.e).abs()
    assert bool(torch.isfinite(err).all()), f"{what}: non-finite values in the average"
    over = err > oracle.bound
    ratio = float((err / oracle.bound.clamp_min(1e-300)).max()) if err.numel() and float(oracle.bound.max()) > 0 else 0.0
    print(f"{what}: max error {float(err.max()):.3e}, worst error / allowance {ratio:.3f}")
    assert not bool(over.any()), f"{what}: {int(over.sum())} element(s) outside the bound, worst ratio {ratio:.3f}"
