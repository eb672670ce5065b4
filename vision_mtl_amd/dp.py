"""Data-parallel layer: one process per GPU, parameters replicated, gradients in ONE flat fp32
buffer, ONE all-reduce per step over RCCL/xGMI (torch.distributed backend "nccl" is RCCL on ROCm).

The reference has no distributed code at all — this is new, MI355X-first work:
images shard across ranks, every rank runs the same fwd/bwd on its shard with per-replica
BatchNorm statistics (what DDP does by default), gradients are averaged.  ~13.5 M parameters =
54 MB: a single collective per step (no bucketing: on 7 x 153 GB/s point-to-point xGMI links one
54 MB ring all-reduce is ~0.6 ms against a ~15 ms step, and fewer, larger collectives are the right
shape for this fabric).
"""
from __future__ import annotations

import contextlib
import os

import weakref

import torch
import torch.distributed as dist

from . import ops


class FlatArena:
    """Re-homes every parameter of `model` into one contiguous fp32 buffer and gives each a slot in
    a second contiguous gradient buffer.  The backward kernels write parameter gradients directly
    into the slots (see ops._slot), so after loss.backward() `flat_grad` holds the whole gradient.

    Replica consistency: when torch.distributed is initialised the flat parameter buffer and every
    floating-point buffer (BatchNorm running statistics) are broadcast from rank 0 here, so ranks
    whose models were initialised under different seeds start identical (what DDP does in its
    constructor).  BatchNorm statistics are per replica afterwards (PyTorch-DDP default; the reference is
    single-device, there is no SyncBN to mirror): running buffers drift apart by the shard statistics and
    `broadcast_buffers()` re-aligns them to rank 0's (call it before evaluating / checkpointing).

    Gradient semantics: a backward pass OVERWRITES the slot of every parameter its kernels compute a
    gradient for (it does not accumulate: one fwd+bwd per optimizer step, as the reference's loop,
    training_lit.py:82-87).  Gradients that reach an arena parameter through ordinary autograd (a
    torch-native loss term on a parameter) are added in place by AccumulateGrad instead; a parameter
    that gets BOTH kinds in one backward pass would depend on their order, so that raises.  zero_grad()
    is one memset of the flat buffer (needed only for the autograd-accumulated kind).

    Use from a driver loop that owns the optimizer step (bench.py, ArenaAdam below).  Do not combine
    with optimizer.zero_grad(set_to_none=True): .grad must stay bound to the arena (rebind_grads() re-attaches it).

    COLLECTIVE CONSTRUCTOR: with an initialised process group, FlatArena(model) broadcasts rank 0's parameters and
    buffers (broadcast=True, the default) - EVERY rank must construct its arena, in the same order, or the ranks that do
    wait forever.  Pass broadcast=False for a rank-local arena (and call broadcast_parameters() yourself later).

    extra_params: trainable parameters that live outside `model` (the log-variances of a balancing.TaskBalancer, which
    belongs to the MTLModule around the model).  They are appended AFTER the model's, so the model's offsets are those
    of FlatArena(model) and the parameter order is MTLModule.parameters()': ArenaAdam.state_dict() then matches
    torch.optim.Adam(module.parameters()) parameter for parameter."""

    def __init__(self, model: torch.nn.Module, broadcast: bool = True, extra_params=None):
        params = [p for p in model.parameters() if p.requires_grad]
        if not params:
            raise ValueError("model has no trainable parameters")
        for p in extra_params or ():
            if not isinstance(p, torch.nn.Parameter) or not p.requires_grad or p.dtype != torch.float32:
                raise ValueError("FlatArena: extra_params must be trainable float32 nn.Parameters")
            if any(p is q for q in params):
                raise ValueError("FlatArena: an extra parameter is already in the arena")
            if p.device != params[0].device:
                raise ValueError(f"FlatArena: an extra parameter is on {p.device}, the model on {params[0].device}")
            params.append(p)
        dev = params[0].device  # build the arena AFTER model.to(device): .to() would drop the views
        total = sum(p.numel() for p in params)
        self.flat_param = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.params, self.offsets, off = params, [], 0
        self._kernel_written = set()  # ids of parameters whose slot a HIP backward kernel writes (ops._slot); per step
        self._zero_bias = set()       # ids of bias parameters whose slot is KNOWN to hold zeros (see ops._bias_grad)
        self._scale_consumer = None   # weak reference to the ArenaAdam that folds pending_scale into its update
        self._hooks = []
        for p in params:
            n = p.numel()
            slot = self.flat_param[off:off + n].view(p.shape)
            slot.copy_(p.data)
            p.data = slot
            p.grad = self.flat_grad[off:off + n].view(p.shape)
            p._vmtl_gslot = p.grad
            p._vmtl_arena = self
            self._hooks.append(p.register_hook(self._make_mixed_use_guard(p)))
            self.offsets.append(off)
            off += n
        self.numel = total
        self.model = model
        self._adam = None
        self._optim = None  # (workspace, control block) of the clipping / extended-update launches
        self.pending_scale = 1.0  # 1/world still to be applied to flat_grad (see all_reduce_mean / ArenaAdam)
        self._applied_average = None  # the ArenaAverage whose weights stand in flat_param right now (ArenaAverage.applied)
        if broadcast:
            self.broadcast_parameters()

    # ---- replica consistency
    def broadcast_parameters(self, src: int = 0) -> None:
        """Rank `src`'s parameters and floating-point buffers to every rank (no-op without a process group)."""
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return
        dist.broadcast(self.flat_param, src=src)
        self.broadcast_buffers(src)
        ops.packs.invalidate()

    def broadcast_buffers(self, src: int = 0) -> None:
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return
        for b in self.model.buffers():
            dist.broadcast(b, src=src)

    def checksum(self) -> float:
        """Cheap cross-rank consistency probe: max over ranks of |sum(params) - rank 0's sum| (0.0 when identical)."""
        s = self.flat_param.double().sum().reshape(1)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            ref = s.clone()
            dist.broadcast(ref, src=0)
            d = (s - ref).abs()
            dist.all_reduce(d, op=dist.ReduceOp.MAX)
            return float(d.item())
        return 0.0

    # ---- gradient bookkeeping
    def _make_mixed_use_guard(self, p):
        # The hook lives in the tensor's C++ autograd metadata, where Python's cycle collector cannot see it: a closure
        # holding the arena (or p) strongly would keep arena, parameters and model alive for the life of the process
        # (and with them their packed operands, re-packed every step: bench.py's later configurations measured up to
        # 1 ms/step slower).  It holds a weak reference and the parameter's id instead.
        wself, pid = weakref.ref(self), id(p)

        def guard(grad):
            arena = wself()
            if arena is not None and grad is not None and pid in arena._kernel_written:  # kernels hand autograd None
                raise RuntimeError(
                    "a parameter of the FlatArena receives a gradient through ordinary autograd AND from a HIP "
                    "backward kernel that overwrites its slot in the same backward pass: the result would depend on "
                    "their order.  Keep torch-native loss terms off parameters the vmtl kernels differentiate.")
            return grad
        return guard

    def close(self) -> None:
        """Detach from the model: hooks removed, kernels stop writing into the slots (the parameters keep their storage
        inside the flat buffer and their .grad views, which stay valid tensors)."""
        for h in self._hooks:
            h.remove()
        self._hooks = []
        for p in self.params:
            for attr in ("_vmtl_gslot", "_vmtl_arena"):
                if hasattr(p, attr):
                    delattr(p, attr)
        self._scale_consumer = None
        self._kernel_written.clear()
        if getattr(self.model, "dp_arena", None) is self:
            self.model.dp_arena = None

    def zero_grad(self) -> None:
        """One memset of the whole gradient buffer (slots written by kernels do not need it: they are overwritten)."""
        self.flat_grad.zero_()
        self.pending_scale = 1.0

    def slots_clobbered(self) -> None:
        """Tell the arena that flat_grad was written from outside (a test poisoning it, a checkpoint restore): slots
        whose gradient is structurally zero are then zeroed again by the next backward pass instead of being trusted."""
        self._zero_bias.clear()

    def rebind_grads(self) -> None:
        """Re-attach every parameter's .grad to its arena slot (after an optimizer.zero_grad(set_to_none=True), torch
        2.x's default, which only drops the Python binding: the kernels keep writing into the slots)."""
        for p, off in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * off:
                p.grad = self.flat_grad[off:off + p.numel()].view(p.shape)

    def all_reduce_mean(self):
        """Average the flat gradient over all ranks: ONE collective.  On RCCL (backend nccl) the averaging is the
        collective's own reduction op (no extra pass over the 54 MB buffer) and 1.0 is returned; on backends without
        AVG (gloo: the CPU tests) the sum is reduced and the factor 1/world is returned for the caller to fold into
        its next pass over the gradient (ArenaAdam: grad_scale of the fused Adam launch)."""
        ops.side.join()  # no-op unless a backward pass ended abnormally with side-stream work un-joined
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            if dist.get_backend() == "nccl":
                dist.all_reduce(self.flat_grad, op=dist.ReduceOp.AVG)
                return 1.0
            dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM)
            return 1.0 / dist.get_world_size()
        return 1.0

    def sync_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """Return `loss` with the gradient averaging hooked onto its backward pass: when the autograd
        engine finishes `loss.backward()` (engine callback, queued from the root of the graph) the side
        stream is joined and the flat gradient is all-reduced once over RCCL - so the reference's
        `loss.backward(); optimizer.step()` (training_lit.py:85-87) needs no change (SURVEY.md section 8b,
        last row).  MTLModule does this for the train stage when `dp_arena` is set.  A remaining 1/world factor
        (gloo only) is applied in place unless an ArenaAdam is attached, which folds it into its update."""
        return _SyncGrads.apply(loss, self)

    def _end_of_backward(self):
        scale = self.all_reduce_mean()
        self._kernel_written.clear()  # the guard covers one backward pass; the next forward re-registers its slots
        if scale != 1.0:
            consumer = self._scale_consumer() if self._scale_consumer is not None else None
            if consumer is not None:
                # the attached ArenaAdam folds the factor into its fused update (no extra pass over 54 MB).  Until its
                # step() - or adam_step() - runs, flat_grad holds the SUM over ranks: anything else that reads gradients
                # in between (clipping, logging) must multiply by arena.pending_scale - grad_norm() and
                # clip_grad_norm_() below do, torch.nn.utils.clip_grad_norm_ does not
                self.pending_scale = scale
            else:
                self.flat_grad.mul_(scale)

    # ---- global-norm clipping (csrc/optim.hip)
    def _optim_buffers(self):
        """(workspace, control block) of the norm / clip / extended-update launches, allocated once per arena."""
        if self._optim is None:
            self._optim = (ops.optim_workspace(self.numel, self.flat_param), ops.optim_control_block(self.flat_param))
        return self._optim

    def _adam_state(self):
        if self._adam is None:
            z = torch.zeros_like(self.flat_param)
            self._adam = {"m": z, "v": z.clone(), "step": torch.zeros(1, dtype=torch.float32, device=z.device)}
        return self._adam

    def grad_norm(self) -> torch.Tensor:
        """2-norm of the TRUE gradient as a 0-dim device tensor (no host sync): a 1/world factor still owed to flat_grad
        (pending_scale) is honoured, flat_grad is not written.  The tensor is a view of the arena's control block: the
        next grad_norm() / clip_grad_norm_() / extended adam_step() overwrites it (clone() to keep a value)."""
        ws, ctl = self._optim_buffers()
        ops.side.join()
        return ops.grad_norm(self.flat_grad, self.pending_scale, ws, ctl)

    def clip_grad_norm_(self, max_norm) -> torch.Tensor:
        """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) over the arena in two launches (one read of the
        gradient for the norm, one scale pass), for callers who keep torch.optim.Adam over the parameter views.  Returns
        the norm before clipping (0-dim device tensor, a view like grad_norm()'s).  A pending 1/world factor is part of the
        gradient that is measured and is CONSUMED by the scale pass: pending_scale is 1.0 afterwards, so a following
        optimizer does not apply it again."""
        if max_norm is None or not float(max_norm) >= 0.0:
            raise ValueError(f"clip_grad_norm_: max_norm must be >= 0, got {max_norm}")
        ws, ctl = self._optim_buffers()
        ops.side.join()
        scale, self.pending_scale = self.pending_scale, 1.0
        return ops.scale_by_clip(self.flat_grad, float(max_norm), scale, ws, ctl)

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, *, max_grad_norm=None,
                  decoupled_weight_decay=False, skip_nonfinite=False, average=None):
        """torch.optim.Adam semantics (reference training_lit.py:51,87) as ONE fused launch over the arena.

        max_grad_norm (clip the global norm of the true gradient first), decoupled_weight_decay (AdamW),
        skip_nonfinite (leave everything untouched when the gradient norm is inf / NaN) or a 0-dim device tensor as lr
        select the extended path instead (ops.adam_step_ex: norm pass when clipping or skipping, control launch, update):
        the step counter is then incremented on the device, in the same tensor.

        average (an ArenaAverage over this arena) selects the extended path too, ending in ops.adam_step_wavg: the new
        parameters go into the average in the same pass, so the caller calls no average.update()."""
        if self._applied_average is not None:
            raise RuntimeError("FlatArena.adam_step: the averaged weights are applied (ArenaAverage.applied / swap): a step "
                               "now would train the average instead of the live parameters")
        if average is not None:
            return self._adam_step_averaged(average, lr, betas, eps, weight_decay, grad_scale, max_grad_norm,
                                            decoupled_weight_decay, skip_nonfinite)
        extended = (max_grad_norm is not None or decoupled_weight_decay or skip_nonfinite
                    or isinstance(lr, torch.Tensor))
        st = self._adam_state()
        ops.side.join()
        # a 1/world factor still owed to the gradient (gloo: all_reduce_mean returned it to _end_of_backward) is consumed
        # HERE, whoever calls: a direct adam_step() after a discarded ArenaAdam cannot silently drop it
        grad_scale, self.pending_scale = grad_scale * self.pending_scale, 1.0
        if extended:
            ws, ctl = self._optim_buffers()
            ops.adam_step_ex(self.flat_param, self.flat_grad, st["m"], st["v"], st["step"], lr, betas, eps,
                             weight_decay, grad_scale, max_grad_norm=max_grad_norm,
                             decoupled_weight_decay=decoupled_weight_decay, skip_nonfinite=skip_nonfinite,
                             workspace=ws, ctl=ctl)
        else:
            st["step"] += 1
            ops.adam_step(self.flat_param, self.flat_grad, st["m"], st["v"], st["step"], lr, betas, eps, weight_decay,
                          grad_scale)
        self._kernel_written.clear()
        ops.packs.invalidate()  # parameters changed through raw pointers: packed operands are stale

    def _adam_step_averaged(self, average, lr, betas, eps, weight_decay, grad_scale, max_grad_norm, decoupled_weight_decay,
                            skip_nonfinite):
        """adam_step(average=...): the extended update with the average in the same pass (+ the buffers launch)."""
        if not isinstance(average, ArenaAverage) or average.arena is not self:
            raise ValueError("FlatArena.adam_step: average must be an ArenaAverage over this arena")
        st = self._adam_state()
        ops.side.join()
        grad_scale, self.pending_scale = grad_scale * self.pending_scale, 1.0
        ws, ctl = self._optim_buffers()
        ops.adam_step_wavg(self.flat_param, self.flat_grad, st["m"], st["v"], average.flat_avg, average.state, st["step"],
                           lr, betas, eps, weight_decay, grad_scale, mode=average.mode, decay=average.decay,
                           warmup=average.warmup, max_grad_norm=max_grad_norm,
                           decoupled_weight_decay=decoupled_weight_decay, skip_nonfinite=skip_nonfinite, workspace=ws,
                           ctl=ctl)
        if average._table is not None:
            ops.wavg_buffers(average._table, average.state)
        self._kernel_written.clear()
        ops.packs.invalidate()


class ArenaAdam(torch.optim.Optimizer):
    """torch.optim.Adam's interface over FlatArena.adam_step (one fused launch over the flat buffers).
    `param_groups`, `zero_grad` and the `state_dict` WIRE FORMAT are torch.optim.Adam's: state_dict() emits
    {"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [{..., "params": [0..n-1]}]} with the
    moments sliced per parameter out of the flat buffers (parameter order = model.parameters(), the order
    torch.optim.Adam(module.parameters()) uses), and load_state_dict() accepts exactly that - so the reference's
    scheduler (`ReduceLROnPlateau`, training_lit.py:51-55) drives it unchanged and session_{epoch}.pt files
    written by `save_ckpt` (pipeline_utils.py:139-167) move between this optimizer and torch.optim.Adam in both
    directions.  Anything else raises (never a silent partial load).

    decoupled_weight_decay=True is AdamW (torch.optim.AdamW is Adam with this flag): it lives in param_groups[0] as in
    torch and travels with the state dict.  max_grad_norm clips the global norm of the true gradient (a pending 1/world
    factor included) inside the update - the clipped gradient is never written back - and skip_nonfinite leaves
    parameters, moments and the step counter untouched when that norm is inf / NaN; both are plain attributes, not
    optimizer state (clipping is not optimizer state in torch either).  After a step() with any of these set, `grad_norm`
    (before clipping; NaN when neither clipping nor skipping asked for a norm) and `skipped_steps` are 0-dim device
    tensors, views of the arena's control block: reading them is the caller's choice of when to sync.

    capturable=True: param_groups[0]["lr"] is a 0-dim fp32 DEVICE tensor handed to the kernel by pointer (torch's
    schedulers fill_ a tensor lr in place, so a captured step() follows ReduceLROnPlateau); state_dict() emits it as a
    float.  Moments, workspace and control block are allocated here, and step() issues nothing but the vmtl launches, so
    it can be captured into a hipGraph on its own.  ops.packs.invalidate() stays host-side bookkeeping that a replay
    does not repeat: whoever REPLAYS a captured step() must call ops.packs.invalidate() after it - or use GraphedStep,
    whose graph re-packs the operands every step.

    average: an ArenaAverage over the same arena (opt-in; a plain attribute like max_grad_norm, not optimizer state).
    step() then takes the extended path and its update launch also folds the new parameters into the average
    (ops.adam_step_wavg), honouring skip_nonfinite: the caller calls no average.update().  Without it step() issues the
    launches it always issued."""

    def __init__(self, arena: "FlatArena", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *,
                 decoupled_weight_decay=False, max_grad_norm=None, skip_nonfinite=False, capturable=False, average=None):
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"ArenaAdam: max_grad_norm must be >= 0 or None, got {max_grad_norm}")
        if isinstance(lr, torch.Tensor):
            if not capturable:
                raise ValueError("ArenaAdam: a tensor lr needs capturable=True (as torch.optim.Adam has it)")
            lr = float(lr)
        if average is not None and (not isinstance(average, ArenaAverage) or average.arena is not arena):
            raise ValueError("ArenaAdam: average must be an ArenaAverage over the same arena")
        self.arena = arena
        self.average = average
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self.capturable = bool(capturable)
        if capturable:
            lr = torch.tensor(float(lr), dtype=torch.float32, device=arena.flat_param.device)
            arena._adam_state()
            arena._optim_buffers()
        super().__init__([arena.flat_param], dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                                  decoupled_weight_decay=bool(decoupled_weight_decay)))
        arena._scale_consumer = weakref.ref(self)  # weak: a discarded optimizer stops deferring the 1/world factor

    @property
    def grad_norm(self):
        """Norm of the last step's true gradient before clipping (None before the first extended step)."""
        o = self.arena._optim
        return None if o is None else o[1][ops.CTL_NORM]

    @property
    def skipped_steps(self):
        """How many steps skip_nonfinite has skipped so far (None before the first extended step)."""
        o = self.arena._optim
        return None if o is None else o[1][ops.CTL_SKIPPED]

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        kw = {} if self.average is None else {"average": self.average}  # absent by default: the call it always made
        self.arena.adam_step(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"],
                             max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite,
                             decoupled_weight_decay=bool(g["decoupled_weight_decay"]), **kw)
        return loss

    def zero_grad(self, set_to_none: bool = False):
        """One memset of the flat gradient buffer (`set_to_none` is ignored: .grad must stay bound to the arena)."""
        self.arena.zero_grad()

    def state_dict(self):
        a, st = self.arena, self.arena._adam
        group = {k: (float(v) if k == "lr" and isinstance(v, torch.Tensor) else v)
                 for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(a.params)))
        state = {}
        if st is not None:
            for i, (p, off) in enumerate(zip(a.params, a.offsets)):
                n = p.numel()
                state[i] = {"step": st["step"].detach().clone().reshape(()).cpu(),
                            "exp_avg": st["m"][off:off + n].view(p.shape).clone(),
                            "exp_avg_sq": st["v"][off:off + n].view(p.shape).clone()}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        a = self.arena
        if not isinstance(sd, dict) or "param_groups" not in sd or "state" not in sd:
            raise ValueError("ArenaAdam.load_state_dict: expected a torch.optim.Adam state_dict ('state' + 'param_groups')")
        groups = sd["param_groups"]
        ids = [i for g in groups for i in g["params"]]
        if ids != list(range(len(a.params))):
            raise ValueError(f"ArenaAdam.load_state_dict: the checkpoint covers {len(ids)} parameters, the arena holds "
                             f"{len(a.params)} (parameter order must be model.parameters())")
        hyper = [{k: v for k, v in g.items() if k != "params"} for g in groups]
        if any(h != hyper[0] for h in hyper[1:]):
            raise ValueError("ArenaAdam.load_state_dict: parameter groups with different hyper-parameters are not supported")
        for k in ("amsgrad", "maximize"):
            if hyper[0].get(k):
                raise ValueError(f"ArenaAdam.load_state_dict: {k}=True is not implemented by the fused update")
        lr_t = self.param_groups[0]["lr"] if self.capturable else None
        self.param_groups[0].update({k: v for k, v in hyper[0].items() if k in self.param_groups[0]})
        if lr_t is not None:  # the kernel reads lr through this tensor's address: refill it, never rebind it
            self.param_groups[0]["lr"] = lr_t.fill_(float(hyper[0].get("lr", lr_t)))
        state = sd["state"]
        if not state:
            a._adam = None
            return
        if sorted(state.keys()) != list(range(len(a.params))):
            raise ValueError("ArenaAdam.load_state_dict: 'state' must hold every parameter (a partially stepped optimizer "
                             "cannot be represented by one fused step counter)")
        dev = a.flat_param.device
        m, v = torch.zeros_like(a.flat_param), torch.zeros_like(a.flat_param)
        steps = set()
        for i, (p, off) in enumerate(zip(a.params, a.offsets)):
            e, n = state[i], p.numel()
            if tuple(e["exp_avg"].shape) != tuple(p.shape) or tuple(e["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError(f"ArenaAdam.load_state_dict: moment shapes of parameter {i} do not match {tuple(p.shape)}")
            m[off:off + n].copy_(e["exp_avg"].reshape(-1))
            v[off:off + n].copy_(e["exp_avg_sq"].reshape(-1))
            steps.add(float(e["step"]))
        if len(steps) != 1:
            raise ValueError("ArenaAdam.load_state_dict: parameters with different step counts cannot share the fused update")
        a._adam = {"m": m, "v": v, "step": torch.full((1,), steps.pop(), dtype=torch.float32, device=dev)}


class ArenaAdamW(ArenaAdam):
    """torch.optim.AdamW over the arena: ArenaAdam with decoupled weight decay and AdamW's default weight_decay."""

    def __init__(self, arena: "FlatArena", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        super().__init__(arena, lr, betas, eps, weight_decay, decoupled_weight_decay=True, **kw)


class ArenaAverage:
    """An averaged copy of the arena's parameters, kept on the device as ONE flat buffer next to `flat_param`, and
    evaluation under it.  mode "ema": e += (1 - decay) * (p - e) per update (timm's ModelEmaV2, torch's
    AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay))); warmup=True uses min(decay, (1 + n) / (10 + n)) with n the
    updates so far (timm's warm-up rule).  mode "swa": the equal average e += (p - e) / (n + 1) (AveragedModel's
    default).  The first update is an exact copy, as in torch; the average starts as a copy of the parameters, so it is
    valid before the first update and after a run whose first steps were all skipped.

    update(optimizer=None): control launch + one streaming pass (+ one launch for the buffers), no host sync and no
    allocation, so it can be captured on its own or after a capturable ArenaAdam.step().  With the ArenaAdam passed, an
    update after a step that skip_nonfinite skipped is skipped too (counter and average keep their bits).
    ArenaAdam(arena, ..., average=avg) folds the update into the optimizer's own pass instead: call no update() then.

    use_buffers=False (torch's default): the averaged model uses the live model's buffers (BatchNorm running
    statistics); nothing is stored or exchanged for them.  use_buffers=True: the floating-point buffers of arena.model are
    averaged with the same weight by one launch over a descriptor table and exchanged by applied(); integer buffers
    (num_batches_tracked) stay the live model's.

    applied(): a context manager under which the model computes with the averaged weights: `flat_param` and the average
    (and the averaged buffers) are exchanged in place by ops.swap_ on entry and again on exit.  No address changes, so
    parameter views, .grad bindings, BatchNorm-table signatures and captured graphs (GraphedEval) stay valid; the packed
    operands are invalidated both ways.  It refuses to nest, and update() / FlatArena.adam_step() raise inside it.
    swap() is the bare exchange.  MTLModule.weight_average = avg makes validation_step, test_step, predict_step and
    GraphedEval run inside applied().

    n_averaged: a 0-dim int64 device tensor, a view of the state block (ops.wavg_state); reading it is the caller's
    choice of when to sync.

    Checkpoints: state_dict() / load_state_dict() use the wire format of
    torch.optim.swa_utils.AveragedModel(arena.model).state_dict(): "n_averaged" plus "module.<key>" for every key of
    arena.model.state_dict(), in the torch layout, so a checkpoint moves between this object and torch's in both
    directions.  Entries this object does not average (buffers without use_buffers, integer buffers, parameters
    outside the arena) carry the live model's values on the way out - what AveragedModel holds for them - and are checked
    for shape but not stored on the way in.  The arena's extra_params (a TaskBalancer's log-variances) travel as
    "arena_extra.<i>", i counting them in arena order; an arena without extra parameters emits none, and torch's
    AveragedModel does not know them (drop them before handing the dict to it).  Anything that does not match raises.
    averaged_state_dict(module) is module.state_dict() with the averaged values in place of the live ones: hand it to
    save_ckpt to write the model_{epoch}.pt of the averaged model.

    Data-parallel runs: parameters are replicated and every rank applies the same update to the same values, so every
    rank holds the same average without a collective (averaged buffers follow each rank's own BatchNorm statistics, as
    the live ones do; FlatArena.broadcast_buffers aligns the live ones only).  This has NOT run on more than one GPU."""

    EXTRA_KEY = "arena_extra."

    def __init__(self, arena: "FlatArena", decay=0.999, mode="ema", warmup=False, use_buffers=False):
        if not isinstance(arena, FlatArena):
            raise ValueError(f"ArenaAverage: arena must be a FlatArena, got {type(arena).__name__}")
        if mode not in ops.WAVG_MODES:
            raise ValueError(f"ArenaAverage: mode must be one of {sorted(ops.WAVG_MODES)}, got {mode!r}")
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"ArenaAverage: decay must be a float in [0, 1], got {decay!r}")
        if warmup and mode != "ema":
            raise ValueError("ArenaAverage: warmup is the EMA decay warm-up; it does not combine with mode='swa'")
        self.arena = arena
        self.decay, self.mode, self.warmup, self.use_buffers = float(decay), mode, bool(warmup), bool(use_buffers)
        self.flat_avg = arena.flat_param.detach().clone()
        self.state = ops.wavg_state(arena.flat_param)
        self._n_model = sum(1 for p in arena.model.parameters() if p.requires_grad)  # arena.params[_n_model:]: extras
        self._buffers, self._buf_avg, self._table = [], [], None
        if self.use_buffers:
            self._buffers = [b for b in arena.model.buffers() if b.is_floating_point()]
            if any(b.dtype != torch.float32 or not b.is_contiguous() for b in self._buffers):
                raise ValueError("ArenaAverage: use_buffers=True takes contiguous float32 buffers")
            flat = torch.cat([b.detach().reshape(-1) for b in self._buffers]) if self._buffers else None
            off = 0
            for b in self._buffers:
                self._buf_avg.append(flat[off:off + b.numel()].view(b.shape))
                off += b.numel()
            if self._buffers and arena.flat_param.is_cuda:
                self._table = ops.wavg_buffer_table([(b.view(-1), a.view(-1)) for b, a in zip(self._buffers, self._buf_avg)])

    @property
    def n_averaged(self) -> torch.Tensor:
        return ops.wavg_n_averaged(self.state)

    @property
    def is_applied(self) -> bool:
        return self.arena._applied_average is self

    def _not_applied(self, what):
        if self.arena._applied_average is not None:
            raise RuntimeError(f"ArenaAverage.{what}: the averaged weights are applied (inside applied()): flat_param "
                               "holds the average, not the live parameters")

    # ---- the update
    @torch.no_grad()
    def update(self, optimizer=None) -> None:
        self._not_applied("update")
        ctl = None
        if optimizer is not None:
            if getattr(optimizer, "arena", None) is not self.arena:
                raise ValueError("ArenaAverage.update: optimizer must be the ArenaAdam of the same arena")
            if getattr(optimizer, "average", None) is self:
                raise ValueError("ArenaAverage.update: this optimizer already averages in its step() (average=): "
                                 "calling update() as well would average every step twice")
            o = self.arena._optim  # None: no extended step has run, so none was skipped
            ctl = None if o is None else o[1]
        ops.wavg_control(self.state, self.mode, self.decay, self.warmup, ctl=ctl)
        ops.wavg_update(self.flat_avg, self.arena.flat_param, self.state)
        if self._table is not None:
            ops.wavg_buffers(self._table, self.state)
        elif self._buffers:
            ops._flat(self._buffers[0], "buffer")  # a CPU model: the no-CPU-fallback error

    # ---- evaluation under the average
    @torch.no_grad()
    def swap(self) -> None:
        """Exchange flat_param with the average (and the averaged buffers with the live ones), bit for bit, in place."""
        ops.side.join()
        ops.packs.join()  # a side-stream packing pass still reading the parameters is ordered before the exchange
        ops.swap_(self.arena.flat_param, self.flat_avg)
        if self._table is not None:
            ops.swap_table_(self._table)
        elif self._buffers:
            ops._flat(self._buffers[0], "buffer")
        ops.packs.invalidate()  # parameters changed through raw pointers: packed operands are stale

    @contextlib.contextmanager
    def applied(self):
        if self.arena._applied_average is not None:
            raise RuntimeError("ArenaAverage.applied: averaged weights are already applied to this arena (no nesting)")
        self.swap()
        self.arena._applied_average = self
        try:
            yield self
        finally:
            self.arena._applied_average = None
            self.swap()

    # ---- checkpoints
    def _slices(self):
        """id(parameter) -> its slice of the average, shaped like the parameter."""
        a = self.arena
        return {id(p): self.flat_avg[off:off + p.numel()].view(p.shape) for p, off in zip(a.params, a.offsets)}

    def _averaged_of(self):
        """id(tensor) -> averaged tensor, for every parameter of the arena and every averaged buffer."""
        m = self._slices()
        m.update({id(b): avg for b, avg in zip(self._buffers, self._buf_avg)})
        return m

    def _extras(self):
        a = self.arena
        return list(zip(a.params[self._n_model:], a.offsets[self._n_model:]))

    @torch.no_grad()
    def state_dict(self) -> dict:
        self._not_applied("state_dict")
        avg = self._averaged_of()
        out = {"n_averaged": self.n_averaged.detach().clone()}
        for k, t in self.arena.model.state_dict(keep_vars=True).items():
            out["module." + k] = avg.get(id(t), t).detach().clone()
        for i, (p, off) in enumerate(self._extras()):
            out[f"{self.EXTRA_KEY}{i}"] = self.flat_avg[off:off + p.numel()].view(p.shape).clone()
        return out

    @torch.no_grad()
    def load_state_dict(self, sd) -> None:
        self._not_applied("load_state_dict")
        if not isinstance(sd, dict) or "n_averaged" not in sd:
            raise ValueError("ArenaAverage.load_state_dict: expected an AveragedModel state_dict ('n_averaged' + 'module.*')")
        live = self.arena.model.state_dict(keep_vars=True)
        expect = {"n_averaged": None}
        expect.update({"module." + k: t for k, t in live.items()})
        expect.update({f"{self.EXTRA_KEY}{i}": p for i, (p, _) in enumerate(self._extras())})
        missing, extra = sorted(set(expect) - set(sd)), sorted(set(sd) - set(expect))
        if missing or extra:
            raise ValueError(f"ArenaAverage.load_state_dict: missing keys {missing}, unexpected keys {extra}")
        n = torch.as_tensor(sd["n_averaged"])
        if n.numel() != 1 or n.is_floating_point() or n.is_complex() or int(n) < 0:
            raise ValueError(f"ArenaAverage.load_state_dict: n_averaged must be one non-negative integer, got {n!r}")
        for k, t in expect.items():
            if t is not None and tuple(sd[k].shape) != tuple(t.shape):
                raise ValueError(f"ArenaAverage.load_state_dict: {k} has shape {tuple(sd[k].shape)}, the model "
                                 f"{tuple(t.shape)}")
        avg = self._averaged_of()
        for k, t in expect.items():  # everything was checked: nothing is written before the whole dict matched
            dst = None if t is None else avg.get(id(t))
            if dst is not None:
                dst.copy_(sd[k])
        self.n_averaged.fill_(int(n))

    @torch.no_grad()
    def averaged_state_dict(self, module: torch.nn.Module) -> dict:
        """module.state_dict() (an MTLModule around arena.model, or the model itself) with the averaged values in place
        of the live ones: same keys, same order, fresh tensors."""
        self._not_applied("averaged_state_dict")
        avg = self._averaged_of()
        return type(module.state_dict())((k, avg.get(id(t), t).detach().clone())
                                         for k, t in module.state_dict(keep_vars=True).items())


class _SyncGrads(torch.autograd.Function):
    """Identity on the loss; its backward (the first node the engine runs) queues FlatArena._end_of_backward."""

    @staticmethod
    def forward(ctx, loss, arena):
        ctx.arena = arena
        return loss.view_as(loss)

    @staticmethod
    def backward(ctx, g):
        torch.autograd.Variable._execution_engine.queue_callback(ctx.arena._end_of_backward)
        return g, None


def world_size() -> int:
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def init_distributed():
    """Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torch.distributed.run contract).  Returns
    (rank, world, local_rank); initialises RCCL only when world > 1."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        # VMTL_DIST_BACKEND=gloo: rehearsal of the multi-rank path on a box with fewer GPUs than ranks (ranks then share
        # devices round-robin; RCCL refuses two ranks on one device)
        backend = os.environ.get("VMTL_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if torch.cuda.is_available():
            if backend != "nccl":
                local_rank %= max(torch.cuda.device_count(), 1)
            torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    elif torch.cuda.is_available():
        torch.cuda.set_device(local_rank)
    return rank, world, local_rank


def shard_batch(batch: dict, rank: int, world: int) -> dict:
    """Equal contiguous shards of the leading (image) axis; the global batch must divide evenly."""
    out = {}
    for k, v in batch.items():
        if v.shape[0] % world:
            raise ValueError(f"global batch {v.shape[0]} does not divide over {world} ranks")
        n = v.shape[0] // world
        out[k] = v[rank * n:(rank + 1) * n]
    return out
