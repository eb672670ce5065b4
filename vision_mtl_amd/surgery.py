"""Opt-in gradient surgery at the shared representation of the `basic` model: PCGrad, MGDA and IMTL-G for two tasks.

Both heads of `basic` read ONE tensor, the full-resolution decoder map, and every shared parameter sits below it.  The
per-task gradients of that map are two head data-gradients apart (ops.dual_head keeps them apart when it is handed a
GradSurgery), and every two-task method of the family needs only their 2x2 Gram matrix

    n_a = <g_a, g_a>    d = <g_a, g_b>    n_b = <g_b, g_b>

to derive two coefficients; the trunk then receives alpha * g_a + beta * g_b instead of g_a + g_b.  This is the
representation-level construction of MGDA-UB (Sener & Koltun 2018; `rep_grad` in LibMTL), not parameter-level surgery:
one backward pass, three extra launches (csrc/surgery.hip: a deterministic fp64 reduction, a one-workgroup control step,
a streaming combine).

  "sum"     alpha = beta = 1: the default gradient, with the Gram matrix, cosine and conflict counter as diagnostics
  "pcgrad"  Yu et al. 2020: when d < 0 each gradient loses its component along the other
            (alpha = 1 - d / n_a, beta = 1 - d / n_b); otherwise the sum
  "mgda"    the min-norm point of the segment between the two gradients (alpha = gamma, beta = 1 - gamma)
  "imtl_g"  Liu et al. 2021, gradient part: equal projections onto both unit gradients, alpha + beta = 1

"mgda" and "imtl_g" return a CONVEX combination: at equal norms the trunk gradient has about half the scale of the
default sum (a larger learning rate may be wanted).  The task heads' own parameters are not part of any method.  g_a and
g_b arrive with the static loss weights or the balancer's weights already applied.  Under data parallelism every rank uses
its own shard's Gram matrix; no collective is added.

Everything lives on the device: the kernels read the coefficients by pointer, so a captured step (graphed.GraphedStep)
follows batches whose conflict changes, and nothing on the step path waits for the host.
"""
from __future__ import annotations

import typing as t

import torch

from . import ops

METHODS = tuple(ops.SURGERY_METHODS)


class GradSurgery:
    """A plain object (not an nn.Module: hparams and state_dict() keys do not change).  It owns the state block and the
    reduction workspace, allocated once, on the device of the first call, and never replaced: a captured step that
    used the object keeps reading and writing them, whatever shapes the object serves afterwards.

    stats         the six floats (n_a, d, n_b, alpha, beta, cosine) of the last backward, a device view: reading it is
                  the caller's choice of when to sync (under a captured step it shows the last replay)
    coefficients  (alpha, beta), cosine, counters (steps, conflicts; int64): views of the same block
    conflict_rate()  conflicts / steps as a 0-dim device tensor (NaN before the first step)"""

    def __init__(self, method: str):
        if method not in METHODS:
            raise ValueError(f"GradSurgery: method must be one of {METHODS}, got {method!r}")
        self.method = method
        self._state: t.Optional[torch.Tensor] = None
        self._workspace: t.Optional[torch.Tensor] = None
        self._operands: t.Dict[tuple, torch.Tensor] = {}

    def __repr__(self):
        return f"GradSurgery({self.method!r})"

    def _block(self) -> torch.Tensor:
        if self._state is None:
            raise RuntimeError("GradSurgery: no backward pass has run yet (the state block is allocated on the device of "
                               "the first call)")
        return self._state

    @property
    def stats(self) -> torch.Tensor:
        return self._block()[:6]

    @property
    def coefficients(self) -> torch.Tensor:
        return self._block()[ops.SURGERY_ALPHA:ops.SURGERY_BETA + 1]

    @property
    def cosine(self) -> torch.Tensor:
        return self._block()[ops.SURGERY_COSINE]

    @property
    def counters(self) -> torch.Tensor:
        return ops.surgery_counters(self._block())

    def conflict_rate(self) -> torch.Tensor:
        c = self.counters
        return c[1].to(torch.float32) / c[0].to(torch.float32)

    def reset_counters(self) -> None:
        if self._state is not None:
            self.counters.zero_()

    def _buffers(self, like):
        """(state block, reduction workspace) on like's device.  Both are allocated ONCE per object - the workspace at the
        size of the largest grid vmtl_surgery_gram ever launches - and never replaced: a captured step holds their raw
        addresses, and it must stay valid when the same object later serves another shape (a second GraphedStep, an
        eager step).  The idiom of metrics.EvalAccumulator._ensure_workspace."""
        ops._surgery_operand(like, "the gradient")  # no CPU fallback: refused before anything is allocated
        if self._state is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GradSurgery: the first backward pass must run before the capture (GraphedStep's warm-up "
                                   "steps do)")
            self._state = ops.surgery_state(like)
            self._workspace = ops.surgery_workspace_max(like)
        elif self._state.device != like.device:
            raise RuntimeError(f"GradSurgery: the object lives on {self._state.device} and was handed a gradient on "
                               f"{like.device}; use one GradSurgery per device")
        return self._state, self._workspace

    def head_operand(self, rows: int, cols: int, like: torch.Tensor) -> torch.Tensor:
        """The [rows][cols] block-diagonal data-gradient operand of ops.dual_head, zeroed when first asked for and kept
        for good (one buffer per shape, never replaced, for the reason _buffers gives): the zero lanes and rows are
        static, only the two heads' weight lanes are rewritten every step."""
        key = (rows, cols, like.device)
        buf = self._operands.get(key)
        if buf is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GradSurgery: the first backward pass of a shape must run before the capture")
            buf = self._operands[key] = ops._empty((rows, cols), like).zero_()
        return buf

    def apply(self, gab: torch.Tensor, out: torch.Tensor, rows: int, width: int) -> torch.Tensor:
        """gab: the interleaved map [rows][g_a | g_b] (2 * width floats a row); out [rows][width] <- alpha g_a + beta g_b.
        Three launches: Gram partials, control, combine."""
        state, ws = self._buffers(gab)
        flat = gab.view(-1)
        a, b = flat, flat[width:]
        ops.surgery_gram(a, b, ws, rows=rows, width=width, lda=2 * width, ldb=2 * width)
        ops.surgery_control(ws, state, self.method, rows, width)
        return ops.surgery_combine(a, b, state, out, rows=rows, width=width, lda=2 * width, ldb=2 * width, ldo=width)

    def combine_flat(self, ga: torch.Tensor, gb: torch.Tensor, out: t.Optional[torch.Tensor] = None) -> torch.Tensor:
        """The same three launches on two flat fp32 buffers of equal length (out may be ga)."""
        state, ws = self._buffers(ga)
        ops.surgery_gram(ga, gb, ws)
        ops.surgery_control(ws, state, self.method, 1, ga.numel())
        return ops.surgery_combine(ga, gb, state, out)


def resolve(grad_surgery) -> t.Optional[GradSurgery]:
    """None | a method name | a GradSurgery -> None | GradSurgery (what MTLModule and init_model accept)."""
    if grad_surgery is None or isinstance(grad_surgery, GradSurgery):
        return grad_surgery
    if isinstance(grad_surgery, str):
        return GradSurgery(grad_surgery)
    raise ValueError(f"grad_surgery must be None, one of {METHODS} or a GradSurgery, got {type(grad_surgery).__name__}")
