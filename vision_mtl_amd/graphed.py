"""Product-side captured training step: the reference's train iteration (training_lit.py:81-98) at hipGraph
replay speed.

The reference drives the step surface from an eager Python loop::

    for batch in train_dataloader:
        optimizer.zero_grad()
        batch = module.transfer_batch_to_device(batch, device)
        loss = module.training_step(batch, 0)
        loss.backward()
        optimizer.step()

One step of `basic` is ~560 kernel launches of 4-25 us each: issued one by one from Python the step is host-bound
(bench.py reports both numbers: config.ms_per_step_eager vs ms_per_step).  `GraphedStep` captures forward + losses +
backward ONCE into a hipGraph over static input buffers and a FlatArena (gradients land in the arena's slots, which
stay bound to `p.grad`), then every call copies the new batch into the static buffers and replays::

    gstep = GraphedStep(module, example_batch)            # once, after module.to(device)
    for batch in train_dataloader:
        optimizer.zero_grad()
        loss = gstep(batch)                               # replaces transfer_batch_to_device + training_step
        loss.backward()                                   # no-op handle kept for source compatibility
        optimizer.step()

What stays outside the graph on purpose: the data-parallel gradient all-reduce (one RCCL collective, issued right
after the replay by the same end-of-backward routine the eager path uses) and the optimizer (torch.optim.Adam over
the arena's parameter views, or dp.ArenaAdam: one fused launch).  BatchNorm running statistics, the per-step packing
of the GEMM operands and the per-step metrics are kernels inside the graph.
"""
from __future__ import annotations

import contextlib

import torch

from . import dp, ops
from .precision import conv_precision, get_conv_precision


class _Replayed(torch.autograd.Function):
    """The loss of a replayed step as a tensor with a grad_fn: `loss.backward()` in the caller's loop is accepted and
    does nothing (the captured backward pass already wrote every parameter gradient into the arena)."""

    @staticmethod
    def forward(ctx, value, anchor):
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return None, None


class _StaticBatch:
    """What a captured step shares: static input buffers the caller's batches are copied into, and the model input
    made from them inside the graph (dataset sample layout re-laid by one kernel, or the recorded device transform)."""

    def _init_static(self, module, example_batch: dict) -> None:
        self.device = next(module.model.parameters()).device
        # a raw batch (data.collate_raw) whose sample transform runs inside the graph: recorded once, like the precision
        self.device_transform = getattr(module, "device_transform", None)
        self.static = {k: self._static_like(v) for k, v in example_batch.items()}
        self._fill(example_batch)
        self._sample_layout = (self.device_transform is None and self.static["img"].dim() == 4
                               and self.static["img"].shape[-1] == 3 and self.static["img"].shape[1] != 3)
        self.conv_precision = get_conv_precision()

    def _static_like(self, v: torch.Tensor) -> torch.Tensor:
        return torch.empty(v.shape, dtype=torch.float32 if v.is_floating_point() else v.dtype, device=self.device)

    def _fill(self, batch: dict) -> None:
        name = type(self).__name__
        for k, dst in self.static.items():
            src = batch[k]
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"{name}: batch[{k!r}] has shape {tuple(src.shape)}, the captured step expects "
                                 f"{tuple(dst.shape)} (capture one {name} per batch shape; drop_last=True)")
            dst.copy_(src, non_blocking=src.device.type == "cpu" and src.is_pinned())

    def _model_batch(self) -> dict:
        batch = dict(self.static)
        if self.device_transform is not None:
            batch = self.device_transform(batch)
        elif self._sample_layout:
            batch["img"] = ops.hwc_to_model_input(self.static["img"])
        return batch


class GraphedStep(_StaticBatch):
    """fwd + losses + bwd of `module.training_step` captured once, replayed per batch.

    module: an MTLModule already on its device; example_batch: a batch of the shapes / dtypes / layout every later
    batch will have (host or device; an image in dataset sample layout (B,H,W,3) keeps the one-kernel re-layout of
    data.upload_batch inside the graph).  arena: an existing dp.FlatArena of module.model (default: module.dp_arena,
    else a new one - built here, so construct the GraphedStep on every rank).  warmup: eager steps before capture
    (allocator pools, code objects, packed-operand table).  NOTE: the warm-up steps and the capture rehearsal run real
    training steps on `example_batch` (BatchNorm running statistics move, no optimizer step is taken; the buffers of a
    module.task_balancer - DWA weights, accumulators, history - are put back as they were, and its parameters join the
    default arena: a caller's arena must hold them, dp.FlatArena(model, extra_params=...)).  The step is captured
    under the convolution precision in force at construction (recorded as `conv_precision`), and every replay keeps it
    whatever vision_mtl_amd.set_conv_precision says later.  Likewise `module.device_transform` (data.DeviceTransform)
    at construction: the static buffers then hold raw batches (data.collate_raw) and the transform is captured too.
    `module.train_augment` (data.DeviceAugment) at construction is captured as well, after the transform or re-layout
    (stage "train" only); construction leaves its counter as it was, every replay advances it by one on the device."""

    def __init__(self, module, example_batch: dict, arena: "dp.FlatArena | None" = None, warmup: int = 2,
                 stage: str = "train"):
        if not torch.cuda.is_available():
            raise RuntimeError("GraphedStep needs an MI355X: the hot path has no CPU fallback")
        self.module, self.stage = module, stage
        balancer = getattr(module, "task_balancer", None)
        extra = [] if balancer is None else [p for p in balancer.parameters() if p.requires_grad]
        if arena is None:
            arena = module.dp_arena
        if arena is None:
            arena = dp.FlatArena(module.model, extra_params=extra)
        elif any(getattr(p, "_vmtl_arena", None) is not arena for p in extra):
            raise ValueError("GraphedStep: the arena does not hold the task balancer's parameters; build it as "
                             "dp.FlatArena(module.model, extra_params=list(module.task_balancer.parameters()))")
        self.arena = arena
        self._init_static(module, example_batch)  # static buffers; conv precision and module.device_transform recorded
        # a data.DeviceAugment, recorded like the transform: its two launches join the graph, its counter lives on the
        # device, so every replay draws fresh parameters
        self.train_augment = getattr(module, "train_augment", None) if stage == "train" else None
        attached, module.dp_arena = module.dp_arena, None  # the collective stays outside the graph (see __call__)
        # the warm-up and rehearsal steps run with gradients enabled: a "dwa" balancer would count them into its epoch
        snap = [] if balancer is None else [(b, b.clone()) for b in balancer.buffers()]
        aug_counter = None if self.train_augment is None else self.train_augment.counter
        try:
            so = module.step_outputs[stage]
            mark = {k: len(v) for k, v in so.items()}
            for _ in range(max(1, warmup)):
                self._step().backward()
            torch.cuda.synchronize(self.device)
            # rehearsal on a side stream (what torch.cuda.graph does internally needs the allocations of one step to
            # have happened on a non-default stream), then the capture itself
            s = _rehearsal_stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                self._step().backward()
            torch.cuda.current_stream(self.device).wait_stream(s)
            for k, v in so.items():
                del v[mark[k]:]
            self.graph = torch.cuda.CUDAGraph()
            with conv_precision(self.conv_precision), torch.cuda.graph(self.graph):
                loss = self._step()
                loss.backward()
                # everything the step appended to step_outputs (loss + the four metrics), as ONE static vector
                self._keys = [k for k, v in so.items() if len(v) > mark[k]]
                self._stats = torch.stack([so[k][-1].detach().reshape(()).float() for k in self._keys])
                self._loss = loss.detach()
            for k, v in so.items():
                del v[mark[k]:]
            # the graph reads the packed-operand descriptor tables by address: keep them alive should the cache rebuild
            self._pack_tables = (ops.packs.table, ops.packs.table_side)
        finally:
            module.dp_arena = attached
            with torch.no_grad():
                for b, v in snap:
                    b.copy_(v)
            if aug_counter is not None:  # the warm-up and rehearsal steps drew: the stream continues where it was
                self.train_augment.set_counter(aug_counter)
        self._anchor = torch.zeros((), device=self.device, requires_grad=True)
        self.replays = 0

    # ---- helpers
    def _step(self) -> torch.Tensor:
        if self.train_augment is None:
            return self.module.shared_step(self._model_batch(), self.stage)
        return self.module.shared_step(self.train_augment(self._model_batch()), self.stage)

    # ---- the step
    def __call__(self, batch: dict) -> torch.Tensor:
        self._fill(batch)
        self.graph.replay()
        self.replays += 1
        if self.module.dp_arena is not None or dp.world_size() > 1:
            self.arena._end_of_backward()  # ONE all-reduce of the flat gradient (no-op on one rank)
        # optimizer.zero_grad() defaults to set_to_none=True in torch 2.x: re-bind .grad to the arena slots
        if self.arena.params[0].grad is None or self.arena.params[-1].grad is None:
            self.arena.rebind_grads()
        stats = self._stats.clone()  # one tiny copy: the static vector is overwritten by the next replay
        so = self.module.step_outputs[self.stage]
        for i, k in enumerate(self._keys):
            so[k].append(stats[i])
        return _Replayed.apply(stats[self._keys.index("loss")] if "loss" in self._keys else self._loss, self._anchor)


class GraphedEval(_StaticBatch):
    """One forward-only step (no_grad) captured once, replayed per batch: the validation / test / predict loops of
    the reference (training_lit.py:115-150, 186-216) at hipGraph replay speed::

        geval = GraphedEval(module, example_batch, stage="val")      # module.train(): the reference validates in
        with torch.no_grad():                                        # train mode (BatchNorm uses batch statistics
            for batch in val_dataloader:                             # and moves its running buffers)
                loss = geval(batch)                                  # = module.validation_step(batch)

        module.eval()
        gpred = GraphedEval(module, example_batch, stage="predict")
        preds = [gpred(batch) for batch in predict_dataloader]       # = module.predict_step(batch)

    stage "val" / "test": shared_step; the call returns the loss and appends loss + metrics to
    module.step_outputs[stage] as the eager step does.  stage "predict": predict_step, with or without "mask" / "depth"
    in the batch; the call returns {"segm", "depth"} as fresh tensors (the reference keeps every batch's predictions)
    and appends to step_outputs["predict"] when the targets are there.  `module.predict_augment`
    (inference.PredictAugment) at construction is captured with it - every view's forward, the merge and the finish are
    nodes of the one graph - and "confidence" is returned as well when the object asks for it; a call raises ValueError
    when the attribute is another object than the one captured.

    When a BatchNorm of the model is in eval mode the step runs inside ops.eval_bn_table: the first node of the graph
    derives every eval-mode layer's statistics from the running buffers as they are at replay time.  Parameters are
    read in place (the per-step weight packing is a node of the graph), so a replay after optimizer.step() sees the new
    weights.  Construction has no side effects: the BatchNorm running buffers are restored in place after the
    warm-up / rehearsal steps, step_outputs is left as it was and no gradient is written.  Like GraphedStep, the step
    keeps the convolution precision, module.device_transform and batch shapes in force at construction; a call raises
    ValueError on another batch shape or when module.training (or a BatchNorm's mode) differs from the capture.
    bn_table=False keeps the per-layer eval-statistics launches (A/B measurement).

    `module.weight_average` (a dp.ArenaAverage): a call exchanges the averaged weights in before the replay and out after
    it, as the eager evaluation steps do (ArenaAverage.applied).  The exchanges are ordinary launches outside the graph and
    move no address, so the graph is the one captured without an average - also one captured before the average existed.
    Construction never applies the average; it records whether the attribute was set, and a call raises ValueError when
    that has changed since.  The record is the attribute `weight_average` of this object: a caller who sets
    module.weight_average later and wants an existing capture to follow it assigns the same object here as well -
    nothing is recaptured."""

    STAGES = ("val", "test", "predict")

    def __init__(self, module, example_batch: dict, stage: str = "val", warmup: int = 2, bn_table: bool = True):
        if stage not in self.STAGES:
            raise ValueError(f"GraphedEval: stage must be one of {self.STAGES}, got {stage!r}")
        if not torch.cuda.is_available():
            raise RuntimeError("GraphedEval needs an MI355X: the hot path has no CPU fallback")
        if stage != "predict" and not ("mask" in example_batch and "depth" in example_batch):
            raise ValueError(f"GraphedEval(stage={stage!r}): the batch needs 'mask' and 'depth'")
        self.module, self.stage = module, stage
        self._init_static(module, example_batch)
        # an inference.PredictAugment, recorded like the transform: its views, merge and finish launches join the graph
        self.predict_augment = getattr(module, "predict_augment", None) if stage == "predict" else None
        self.weight_average = getattr(module, "weight_average", None)
        bns = [m for m in module.model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        self.training = module.training
        self._modes = tuple(m.training for m in bns)
        self._bns = bns
        self.bn_table = bool(bn_table) and not all(self._modes)
        self._table = None
        so = module.step_outputs[stage]
        mark = {k: len(v) for k, v in so.items()}
        snap = [(m, [b.clone() for b in self._buffers(m)]) for m in bns]
        try:
            with torch.no_grad():
                for _ in range(max(1, warmup)):
                    self._step()  # builds the packed-operand and BatchNorm tables outside the capture
                torch.cuda.synchronize(self.device)
                s = _rehearsal_stream(self.device)
                s.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(s):
                    self._step()
                torch.cuda.current_stream(self.device).wait_stream(s)
                for k, v in so.items():
                    del v[mark[k]:]
                self.graph = torch.cuda.CUDAGraph()
                with conv_precision(self.conv_precision), torch.cuda.graph(self.graph):
                    out = self._step()
                    # everything the step appended to step_outputs (loss + the four metrics), as ONE static vector
                    self._keys = [k for k, v in so.items() if len(v) > mark[k]]
                    self._stats = (torch.stack([so[k][-1].detach().reshape(()).float() for k in self._keys])
                                   if self._keys else None)
                    self._out = out
            # the graph reads these by address: keep them alive should a cache rebuild its tables
            self._pack_tables = (ops.packs.table, ops.packs.table_side)
        finally:
            for k, v in so.items():
                del v[mark[k]:]
            with torch.no_grad():
                for m, saved in snap:
                    for b, v in zip(self._buffers(m), saved):
                        b.copy_(v)
        self.replays = 0

    @staticmethod
    def _buffers(m):
        return [b for b in (m.running_mean, m.running_var, m.num_batches_tracked) if b is not None]

    def _step(self):
        ctx = ops.eval_bn_table(self.module.model) if self.bn_table else contextlib.nullcontext()
        with ctx as table:
            if table is not None:
                self._table = table
            batch = self._model_batch()
            if self.stage == "predict":
                return self.module._predict_step(batch)  # on the weights as they stand: see __call__
            return self.module.shared_step(batch, self.stage)

    def __call__(self, batch: dict):
        if self.module.training != self.training or tuple(m.training for m in self._bns) != self._modes:
            raise ValueError(f"GraphedEval: captured with module.training={self.training}, called with "
                             f"module.training={self.module.training} (or a BatchNorm changed mode); capture one "
                             "GraphedEval per mode")
        if self.stage == "predict" and getattr(self.module, "predict_augment", None) is not self.predict_augment:
            raise ValueError(f"GraphedEval: captured with module.predict_augment={self.predict_augment!r}, called with "
                             f"{getattr(self.module, 'predict_augment', None)!r}; capture one GraphedEval per predict_augment")
        average = getattr(self.module, "weight_average", None)
        if average is not self.weight_average:
            raise ValueError(f"GraphedEval: built with module.weight_average={self.weight_average!r}, called with "
                             f"{average!r}; build one GraphedEval per weight_average")
        self._fill(batch)
        if average is None:
            self.graph.replay()
        else:
            with average.applied():
                self.graph.replay()
        self.replays += 1
        stats = None
        if self._stats is not None:
            stats = self._stats.clone()  # one tiny copy: the static vector is overwritten by the next replay
            so = self.module.step_outputs[self.stage]
            for i, k in enumerate(self._keys):
                so[k].append(stats[i])
        if self.stage == "predict":
            out = {"segm": self._out["segm"].clone(), "depth": self._out["depth"].clone()}
            if "confidence" in self._out:  # inference.PredictAugment(return_confidence=True)
                out["confidence"] = self._out["confidence"].clone()
            return out
        return stats[self._keys.index("loss")] if "loss" in self._keys else self._out.clone()


_STREAMS = {}


def _rehearsal_stream(device) -> torch.cuda.Stream:
    """One per device and process: HIP maps streams onto few hardware queues round-robin."""
    s = _STREAMS.get(device.index)
    if s is None:
        s = _STREAMS[device.index] = torch.cuda.Stream(device=device)
    return s
