"""Opt-in task-loss balancing: what replaces the two host floats of the reference's loss sum (lit_module.py:120-131)
when the weights are to be learned or to follow the training run.

  "uncertainty"  homoscedastic-uncertainty weighting (Kendall et al. 2018): sum_k exp(-s_k) L_k + s_k with a learnable
                 log-variance s_k per task.  At s = 0 this is the reference's default loss.
  "dwa"          Dynamic Weight Average (Liu et al. 2019, the MTAN paper): sum_k w_k L_k, the weights re-derived once
                 per epoch from the ratio of the last two epochs' mean losses.
  "geometric"    the geometric loss strategy (Chennupati et al. 2019): exp(mean_k log L_k).  Losses must be positive:
                 a loss <= 0 makes the total (and every gradient) NaN.

Everything lives on the device (csrc/balance.hip): log-variances, DWA weights, the epoch's accumulators and its history.
The kernels read them by pointer, so a captured step (graphed.GraphedStep) follows optimizer.step() and
on_train_epoch_end() without a recapture, and nothing on the step path waits for the host.
"""
from __future__ import annotations

import typing as t

import torch
import torch.distributed as dist
from torch import nn

from . import ops

METHODS = ("uncertainty", "dwa", "geometric")


class TaskBalancer(nn.Module):
    """forward(losses) -> the balanced total of the task losses, `losses` a dict keyed by `tasks` or a sequence in their
    order (0-dim fp32 device tensors).

    log_vars (Parameter, "uncertainty" only): s_k = log sigma_k^2, init_log_vars or zeros.  An optimizer treats it like
    any other parameter (ArenaAdam's weight decay and clipping included).
    dwa_weights / dwa_state (persistent buffers, "dwa" only): the current weights (T floats, 1 until two epochs have
    completed) and the fp64 accumulators + history (layout: include/vmtl.h).  The forward adds the step's losses to the
    accumulators only while torch.is_grad_enabled() - validation steps do not count - and only when all are finite.
    weights: the effective weights d total / d L_k of the last forward, a device tensor (reading it is the caller's choice
    of when to sync; under a captured step it is the graph's own buffer and shows the last replay)."""

    def __init__(self, method: str, tasks: t.Sequence[str] = ("segm", "depth"),
                 init_log_vars: t.Optional[t.Sequence[float]] = None, temperature: float = 2.0):
        super().__init__()
        if method not in METHODS:
            raise ValueError(f"TaskBalancer: method must be one of {METHODS}, got {method!r}")
        tasks = tuple(tasks)
        if not 1 <= len(tasks) <= ops.BALANCE_MAX_TASKS or len(set(tasks)) != len(tasks):
            raise ValueError(f"TaskBalancer: 1..{ops.BALANCE_MAX_TASKS} distinct tasks, got {tasks}")
        if not float(temperature) > 0.0:
            raise ValueError(f"TaskBalancer: temperature must be > 0, got {temperature}")
        if init_log_vars is not None and method != "uncertainty":
            raise ValueError("TaskBalancer: init_log_vars belongs to method 'uncertainty'")
        self.method, self.tasks, self.temperature = method, tasks, float(temperature)
        T = len(tasks)
        if method == "uncertainty":
            s = torch.zeros(T) if init_log_vars is None else torch.as_tensor(init_log_vars, dtype=torch.float32).flatten()
            if s.numel() != T:
                raise ValueError(f"TaskBalancer: init_log_vars must hold {T} floats, got {s.numel()}")
            self.log_vars = nn.Parameter(s.detach().clone())
        elif method == "dwa":
            self.register_buffer("dwa_weights", torch.ones(T, dtype=torch.float32))
            self.register_buffer("dwa_state", torch.zeros(3 * T + 2, dtype=torch.float64))
        self._weights = None

    @property
    def weights(self) -> t.Optional[torch.Tensor]:
        return self._weights

    def _param(self):
        if self.method == "uncertainty":
            return self.log_vars
        return self.dwa_weights if self.method == "dwa" else None

    def forward(self, losses) -> torch.Tensor:
        if isinstance(losses, dict):
            losses = [losses[k] for k in self.tasks]
        losses = list(losses)
        if len(losses) != len(self.tasks):
            raise ValueError(f"TaskBalancer: expected {len(self.tasks)} losses ({self.tasks}), got {len(losses)}")
        param = self._param()
        if param is not None and not param.is_cuda:
            raise RuntimeError("TaskBalancer is on the CPU: move it to the GPU with the model (no CPU fallback on the "
                               "hot path)")
        total, self._weights = ops.balance_losses(losses, self.method, param, getattr(self, "dwa_state", None),
                                                  accumulate=self.method == "dwa" and torch.is_grad_enabled())
        return total

    def on_train_epoch_end(self) -> None:
        """"dwa": turn the epoch's accumulated losses into the next epoch's weights (one launch; a no-op for the other
        methods).  With a process group of more than one rank the accumulators and the step count are sum-reduced
        first, so every rank derives the same weights - call it on every rank."""
        if self.method != "dwa":
            return
        if not self.dwa_state.is_cuda:
            raise RuntimeError("TaskBalancer is on the CPU: move it to the GPU with the model (no CPU fallback)")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.dwa_state[:len(self.tasks) + 1], op=dist.ReduceOp.SUM)
        ops.dwa_epoch_update(self.dwa_state, self.dwa_weights, self.temperature)
