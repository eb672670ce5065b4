"""Per-step metrics of reference vision_mtl/lit_module.py:48-69,106-118 on the HIP kernels:
one confusion-matrix pass yields accuracy (micro), Jaccard (class mean) and F-beta (support
weighted); MAE is the L1 kernel.  Values stay on the device (no host sync on the step path)."""
from __future__ import annotations

import typing as t

import torch

from . import ops
from ._lib import lib


def _k(name, **kw):
    lib().callk(name, stream=torch.cuda.current_stream().cuda_stream, **kw)


def confusion_matrix(pred: torch.Tensor, target: torch.Tensor, num_classes: int,
                     ignore_index: t.Optional[int] = None) -> torch.Tensor:
    """cm[t, p] = #pixels with target t predicted as p; int32 (C, C) on the device.  ignore_index: pixels whose target
    equals it are not counted."""
    if not pred.is_cuda:
        raise RuntimeError("confusion_matrix: predictions are not on the GPU (no CPU fallback)")
    pred, target = pred.contiguous(), target.contiguous()
    if pred.dtype != torch.int64 or target.dtype != torch.int64 or pred.numel() != target.numel():
        raise TypeError("confusion_matrix expects int64 predictions and targets of equal size")
    cm = torch.empty((num_classes, num_classes), dtype=torch.int32, device=pred.device)
    if ignore_index is None:
        _k("vmtl_confusion_matrix", pred=pred, target=target, cm=cm, P=pred.numel(), C=num_classes)
    else:
        _k("vmtl_confusion_matrix_ex", pred=pred, target=target, cm=cm, P=pred.numel(), C=num_classes,
           ignore_index=int(ignore_index))
    return cm


def _derived(cm: torch.Tensor, beta: float = 1.0, ignore_index: t.Optional[int] = None) -> torch.Tensor:
    """(accuracy, Jaccard, F-beta) of a confusion matrix.  ignore_index (the one the matrix was built with): a class in
    [0, C) is left out of the Jaccard class mean; accuracy and F-beta follow from its empty row."""
    out = torch.empty((3,), dtype=torch.float32, device=cm.device)
    if ignore_index is None:
        _k("vmtl_segm_metrics", cm=cm, C=cm.shape[0], beta=beta, out=out)
    else:
        _k("vmtl_segm_metrics_ex", cm=cm, C=cm.shape[0], beta=beta, ignore_index=int(ignore_index), out=out)
    return out


class _CMMetric:
    index = 0

    def __init__(self, num_classes: int, beta: float = 1.0, ignore_index: t.Optional[int] = None):
        self.num_classes, self.beta, self.ignore_index = num_classes, beta, ignore_index

    def to(self, *a, **k):
        return self

    def from_confusion(self, cm: torch.Tensor) -> torch.Tensor:
        return _derived(cm, self.beta, self.ignore_index)[self.index]

    def __call__(self, preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return self.from_confusion(confusion_matrix(preds, target, self.num_classes, self.ignore_index))


class Accuracy(_CMMetric):
    index = 0


class JaccardIndex(_CMMetric):
    index = 1


class FBetaScore(_CMMetric):
    index = 2


class MeanAbsoluteError:
    def to(self, *a, **k):
        return self

    def __call__(self, preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return ops.l1_loss(preds.detach(), target)


# ---------------------------------------------------------------------------------------- dataset-level metrics
# (csrc/eval_accum.hip).  The classes above score one batch; the host then averages the batches,
# which is not the mIoU of the evaluation set (a class missing from a batch scores 0 in it) and knows no depth metric
# but the MAE.  EvalAccumulator keeps a confusion matrix and the depth sums on the device over a whole epoch.

EVAL_SCALARS = ("pixel_acc", "mean_acc", "miou", "fbeta", "abs_err", "rel_err", "sq_rel", "rmse", "rmse_log", "log10",
                "silog", "delta1", "delta2", "delta3", "n_valid", "n_pixels")  # out[16] of vmtl_eval_finalize, in order
EVAL_ACC_SIZE = 16  # VMTL_EVAL_ACC_SIZE
MAX_CLASSES = 64


def all_reduce_state(cm: torch.Tensor, acc: torch.Tensor, group=None) -> None:
    """Sum an accumulator's two state tensors over the ranks, in place (what EvalAccumulator.all_reduce does).  cm and
    the counts of acc are integers, so they come out exact; the floating sums are the fp64 sum of the ranks' sums.
    A process without an initialised torch.distributed group is its own world: nothing to do."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    dist.all_reduce(cm, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group)


class EvalAccumulator:
    """Confusion matrix (int64) and depth sums (float64) of a whole evaluation set, kept on the device.

    update() adds one batch with one or two launches and no host sync, so it can sit inside a captured step;
    compute() is one launch and ONE device-to-host copy per epoch.  The class means of compute() leave out the classes
    that never occur (IoU NaN) and the ignore index - the Cityscapes / MTAN convention, NOT the per-step JaccardIndex's
    (absent class = 0); the depth prediction is clamped below at min_depth before every term (see include/vmtl.h).

    ignore_index: targets to skip (None: none); min_depth: a depth pixel is valid when target > min_depth unless
    update() is given a `valid` mask; beta: of the F-beta score.  The state tensors `cm`, `acc` and the workspace keep
    their addresses for the object's life (a captured step holds them).  device="cpu" gives a holder for state
    (state_dict, merge, all_reduce over gloo); update() and compute() need the GPU."""

    def __init__(self, num_classes: int, ignore_index: t.Optional[int] = None, min_depth: float = 1e-3,
                 beta: float = 1.0, device: t.Union[str, torch.device] = "cuda"):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"EvalAccumulator: num_classes must be an int in [1, {MAX_CLASSES}], got {num_classes!r}")
        if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int)
                                         or ignore_index < 0):
            raise ValueError(f"EvalAccumulator: ignore_index must be None or an int >= 0, got {ignore_index!r}")
        if not (isinstance(min_depth, (int, float)) and 0.0 <= float(min_depth) < float("inf")):
            raise ValueError(f"EvalAccumulator: min_depth must be a finite float >= 0, got {min_depth!r}")
        if not (isinstance(beta, (int, float)) and 0.0 < float(beta) < float("inf")):
            raise ValueError(f"EvalAccumulator: beta must be a finite float > 0, got {beta!r}")
        self.num_classes, self.ignore_index = num_classes, ignore_index
        self.min_depth, self.beta = float(min_depth), float(beta)
        self.device = torch.device(device)
        self.cm = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=self.device)
        self.acc = torch.zeros((EVAL_ACC_SIZE,), dtype=torch.float64, device=self.device)
        self._out = torch.empty((len(EVAL_SCALARS) + num_classes,), dtype=torch.float64, device=self.device)
        self._ws = None
        if self.device.type == "cuda":  # the size at the grid cap: update() normally never has to grow it
            self._ensure_workspace(1 << 40)

    # ---- state
    def _config(self) -> dict:
        return {"num_classes": self.num_classes, "ignore_index": self.ignore_index, "min_depth": self.min_depth,
                "beta": self.beta}

    def _ensure_workspace(self, pixels: int) -> torch.Tensor:
        need = lib().raw("vmtl_eval_accum_workspace_bytes")(pixels) // 8
        if self._ws is None or self._ws.numel() < need:
            if self._ws is not None and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("EvalAccumulator: the workspace would have to grow inside a graph capture; run one "
                                   "update of this size before capturing")
            self._ws = torch.empty((need,), dtype=torch.float64, device=self.device)
        return self._ws

    def reset(self) -> None:
        self.cm.zero_()
        self.acc.zero_()

    def state_dict(self) -> dict:
        return dict(self._config(), cm=self.cm.clone(), acc=self.acc.clone())

    def load_state_dict(self, state: dict) -> None:
        mine = self._config()
        for k, v in mine.items():
            if k not in state or state[k] != v:
                raise ValueError(f"EvalAccumulator.load_state_dict: {k} is {v!r} here, {state.get(k)!r} in the state")
        cm, acc = state["cm"], state["acc"]
        if cm.dtype != torch.int64 or tuple(cm.shape) != tuple(self.cm.shape):
            raise ValueError(f"EvalAccumulator.load_state_dict: cm must be int64 {tuple(self.cm.shape)}, got "
                             f"{cm.dtype} {tuple(cm.shape)}")
        if acc.dtype != torch.float64 or tuple(acc.shape) != tuple(self.acc.shape):
            raise ValueError(f"EvalAccumulator.load_state_dict: acc must be float64 {tuple(self.acc.shape)}, got "
                             f"{acc.dtype} {tuple(acc.shape)}")
        self.cm.copy_(cm)  # in place: the addresses stay
        self.acc.copy_(acc)

    def merge(self, other: "EvalAccumulator") -> None:
        """Add another accumulator's state (another shard of the same evaluation set) to this one."""
        if not isinstance(other, EvalAccumulator) or other._config() != self._config():
            raise ValueError("EvalAccumulator.merge: the other accumulator was built with other arguments")
        self.cm.add_(other.cm.to(self.device))
        self.acc.add_(other.acc.to(self.device))

    def all_reduce(self, group=None) -> None:
        """Sum the state over the ranks (torch.distributed); every rank then computes the dataset's metrics."""
        all_reduce_state(self.cm, self.acc, group)

    # ---- the step path
    @staticmethod
    def _dense(x: torch.Tensor, dtype: torch.dtype, what: str) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError(f"EvalAccumulator.update: {what} is not on the GPU (no CPU fallback)")
        if x.dtype != dtype:
            if not (dtype.is_floating_point and x.is_floating_point()):
                raise TypeError(f"EvalAccumulator.update: {what} must be {dtype}, got {x.dtype}")
            x = x.to(dtype)
        # dense in pixel order already (size-1 dimensions carry no order: the (B,H,W,1) view of a (B,1,H,W) map is): no copy
        return x if x.is_contiguous() else x.contiguous()

    def update(self, segm_pred: t.Optional[torch.Tensor] = None, mask: t.Optional[torch.Tensor] = None,
               depth_pred: t.Optional[torch.Tensor] = None, depth: t.Optional[torch.Tensor] = None,
               valid: t.Optional[torch.Tensor] = None, step_cm: t.Optional[torch.Tensor] = None) -> None:
        """Add one batch.  Segmentation: int64 predictions and targets (`segm_pred`, `mask`), or `step_cm`, the int32
        (C, C) matrix confusion_matrix() built for this step with the same ignore_index.  Depth: `depth_pred`, `depth`
        of equal numel, optionally `valid` (bool / uint8, same numel) in place of the target > min_depth rule.  Either
        part may be left out."""
        if self.device.type != "cuda":
            raise RuntimeError("EvalAccumulator.update: the state is not on the GPU (no CPU fallback)")
        if (segm_pred is None) != (mask is None):
            raise ValueError("EvalAccumulator.update: segm_pred and mask go together")
        if (depth_pred is None) != (depth is None):
            raise ValueError("EvalAccumulator.update: depth_pred and depth go together")
        if step_cm is not None and segm_pred is not None:
            raise ValueError("EvalAccumulator.update: give segm_pred / mask or step_cm, not both")
        if valid is not None and depth is None:
            raise ValueError("EvalAccumulator.update: valid needs depth_pred and depth")
        if segm_pred is None and step_cm is None and depth is None:
            raise ValueError("EvalAccumulator.update: nothing to add")
        P = Pd = 0
        if segm_pred is not None:
            segm_pred = self._dense(segm_pred, torch.int64, "segm_pred")
            mask = self._dense(mask, torch.int64, "mask")
            P = segm_pred.numel()
            if mask.numel() != P or P == 0:
                raise ValueError(f"EvalAccumulator.update: segm_pred has {P} pixels, mask {mask.numel()}")
        if step_cm is not None:
            step_cm = self._dense(step_cm, torch.int32, "step_cm")
            if tuple(step_cm.shape) != tuple(self.cm.shape):
                raise ValueError(f"EvalAccumulator.update: step_cm must be {tuple(self.cm.shape)}, got "
                                 f"{tuple(step_cm.shape)}")
        ws = None
        if depth is not None:
            depth_pred = self._dense(depth_pred.detach(), torch.float32, "depth_pred")
            depth = self._dense(depth, torch.float32, "depth")
            Pd = depth.numel()
            if depth_pred.numel() != Pd or Pd == 0:
                raise ValueError(f"EvalAccumulator.update: depth_pred has {depth_pred.numel()} pixels, depth {Pd}")
            if valid is not None:
                if valid.dtype == torch.bool:
                    valid = valid.view(torch.uint8) if valid.is_contiguous() else valid.contiguous().view(torch.uint8)
                valid = self._dense(valid, torch.uint8, "valid")
                if valid.numel() != Pd:
                    raise ValueError(f"EvalAccumulator.update: valid has {valid.numel()} pixels, depth {Pd}")
            ws = self._ensure_workspace(Pd)
        _k("vmtl_eval_accumulate", pred=segm_pred, target=mask, step_cm=step_cm, P=P, C=self.num_classes,
           ignore_index=-1 if self.ignore_index is None else self.ignore_index, dpred=depth_pred, dtarget=depth,
           valid=valid, min_depth=self.min_depth, Pd=Pd, cm=self.cm, acc=self.acc, workspace=ws)

    def compute(self) -> dict:
        """The dataset's metrics: {name: float for name in EVAL_SCALARS} plus "iou", a CPU float64 tensor (C,)
        (NaN for a class left out of the mean).  One launch, one device-to-host copy."""
        if self.device.type != "cuda":
            raise RuntimeError("EvalAccumulator.compute: the state is not on the GPU (no CPU fallback)")
        n = len(EVAL_SCALARS)
        _k("vmtl_eval_finalize", cm=self.cm, acc=self.acc, C=self.num_classes, beta=self.beta,
           ignore_index=-1 if self.ignore_index is None else self.ignore_index, out=self._out, iou=self._out[n:])
        host = self._out.cpu()
        res = dict(zip(EVAL_SCALARS, host[:n].tolist()))
        res["iou"] = host[n:].clone()
        return res
