"""Host-side mirror of reference vision_mtl/losses.py (+ the CrossEntropyLoss the reference takes
from torch.nn at lit_module.py:31) on the HIP loss kernels."""
from __future__ import annotations

import typing as t

import torch
from torch import nn

from . import ops


class SILogLoss(nn.Module):
    """reference vision_mtl/losses.py:7-36.  pred / target: (B,H,W,1) (or any equal-numel pair).

    The reference first resizes ``pred`` to ``target.shape[-2:]`` with a bilinear interpolate;
    for the (B,H,W,1) tensors of this pipeline that is an identity, so the
    fused kernel requires equal shapes and raises otherwise rather than silently resampling."""

    def __init__(self, min_depth: float = 1e-3):
        super().__init__()
        self.min_depth = min_depth

    def forward(self, pred: torch.Tensor, target: torch.Tensor, mask: t.Optional[torch.Tensor] = None,
                interpolate: bool = True, min_depth: t.Optional[float] = None) -> torch.Tensor:
        if pred.dim() < 2 or target.dim() < 2:
            raise IndexError("SILogLoss expects at least 2-D pred/target (the reference indexes shape[-2:])")
        if interpolate and pred.shape[-2:] != target.shape[-2:]:
            raise NotImplementedError("SILogLoss: pred/target spatial sizes differ; resample before the loss")
        if pred.shape != target.shape:
            raise ValueError(f"SILogLoss: shape mismatch {tuple(pred.shape)} vs {tuple(target.shape)}")
        # mask: the valid pixels (bool / uint8, target's shape); min_depth is then not applied (losses.py:29-31)
        return ops.silog(pred, target, self.min_depth if min_depth is None else min_depth, mask=mask)


def _check_depth_pair(who: str, pred: torch.Tensor, target: torch.Tensor, interpolate: bool) -> None:
    """SILogLoss.forward's shape errors, under the caller's name"""
    if pred.dim() < 2 or target.dim() < 2:
        raise IndexError(f"{who} expects at least 2-D pred/target (the reference indexes shape[-2:])")
    if interpolate and pred.shape[-2:] != target.shape[-2:]:
        raise NotImplementedError(f"{who}: pred/target spatial sizes differ; resample before the loss")
    if pred.shape != target.shape:
        raise ValueError(f"{who}: shape mismatch {tuple(pred.shape)} vs {tuple(target.shape)}")


class GradientMatchingLoss(nn.Module):
    """The multi-scale scale-invariant gradient-matching term of MegaDepth (Li & Snavely 2018) / MiDaS, on log depth,
    alone (ops.depth_loss with silog_weight = 0, grad_weight = 1): sum over scales s = 1, 2, .. 2^(scales-1) of the mean
    absolute x- and y-difference of log(pred) - log(target) on the [::s, ::s] subsample, over valid pixel pairs, divided
    by the subsample's valid pixel count of the whole batch.  pred: (B,H,W,1), (B,1,H,W) or (B,H,W)."""

    def __init__(self, scales: int = 4, min_depth: float = 1e-3):
        super().__init__()
        self.scales = ops.depth_loss_scales(scales)
        self.min_depth = min_depth

    def forward(self, pred: torch.Tensor, target: torch.Tensor, mask: t.Optional[torch.Tensor] = None,
                min_depth: t.Optional[float] = None) -> torch.Tensor:
        return ops.depth_loss(pred, target, self.min_depth if min_depth is None else min_depth, mask=mask,
                              grad_weight=1.0, scales=self.scales, silog_weight=0.0)


class SILogGradLoss(nn.Module):
    """SILogLoss + grad_weight * GradientMatchingLoss(scales) from one autograd node (one pass over pred / target, one
    gradient buffer).  Same call signature and shape errors as SILogLoss; no parameters or buffers."""

    def __init__(self, grad_weight: float = 0.5, scales: int = 4, min_depth: float = 1e-3):
        super().__init__()
        grad_weight = ops.depth_loss_weight(grad_weight, "grad_weight")
        if grad_weight == 0.0:
            raise ValueError("SILogGradLoss: grad_weight must be > 0 (SILogLoss is the criterion without the term)")
        self.grad_weight = grad_weight
        self.scales = ops.depth_loss_scales(scales)
        self.min_depth = min_depth

    def forward(self, pred: torch.Tensor, target: torch.Tensor, mask: t.Optional[torch.Tensor] = None,
                interpolate: bool = True, min_depth: t.Optional[float] = None) -> torch.Tensor:
        _check_depth_pair("SILogGradLoss", pred, target, interpolate)
        return ops.depth_loss(pred, target, self.min_depth if min_depth is None else min_depth, mask=mask,
                              grad_weight=self.grad_weight, scales=self.scales, silog_weight=1.0)


class CrossEntropyLoss(nn.Module):
    """torch.nn.CrossEntropyLoss (reduction "mean", no smoothing): logits (B,C,H,W), target int64 (B,H,W).

    weight: one float per class (torch's `weight`); ignore_index: a target value whose pixels count neither in the sum
    nor in the denominator.  Its default is None - NOT torch's -100: nothing is ignored, and a label outside [0, C)
    makes the loss NaN instead of vanishing.  With both at their defaults this is the reference's criterion on the
    unweighted kernels.  `weight` is a buffer (it follows .to(device)) that stays out of state_dict: checkpoints keep
    the reference's keys.

    ohem_min_kept (opt-in): online hard example mining - the mean runs over the valid pixels whose true-class probability
    is below ohem_thresh (in (0, 1]; None: pure top-K), and never over fewer than ohem_min_kept pixels per image
    (ops.cross_entropy_ohem).  Mining is on iff ohem_min_kept is given.

    region_weight (opt-in): the loss becomes this cross entropy + region_weight * the Tversky region term with
    (region_alpha, region_beta, region_smooth) - Dice by default - from one node (ops.segm_region_loss).  `weight`
    keeps applying to the cross entropy only.  It does not combine with mining."""

    def __init__(self, weight: t.Optional[torch.Tensor] = None, ignore_index: t.Optional[int] = None,
                 ohem_min_kept: t.Optional[int] = None, ohem_thresh: t.Optional[float] = None,
                 region_weight: t.Optional[float] = None, region_alpha: float = 0.5, region_beta: float = 0.5,
                 region_smooth: float = 0.0):
        super().__init__()
        if region_weight is not None:
            if ohem_min_kept is not None or ohem_thresh is not None:
                raise ValueError("CrossEntropyLoss: region_weight does not combine with ohem_min_kept / ohem_thresh "
                                 "(mining the region term is not supported)")
            region_weight = ops.region_loss_number(region_weight, "region_weight", "CrossEntropyLoss", positive=True)
            region_alpha = ops.region_loss_number(region_alpha, "region_alpha", "CrossEntropyLoss", positive=True)
            region_beta = ops.region_loss_number(region_beta, "region_beta", "CrossEntropyLoss", positive=True)
            region_smooth = ops.region_loss_number(region_smooth, "region_smooth", "CrossEntropyLoss")
        self.region_weight = region_weight
        self.region = (region_alpha, region_beta, region_smooth)
        if ohem_min_kept is None:
            if ohem_thresh is not None:
                raise ValueError("CrossEntropyLoss: ohem_thresh needs ohem_min_kept (mining is on iff ohem_min_kept is set)")
        else:
            if isinstance(ohem_min_kept, bool) or not isinstance(ohem_min_kept, int):
                raise TypeError(f"CrossEntropyLoss: ohem_min_kept must be an int or None, got {ohem_min_kept!r}")
            if ohem_min_kept < 1:
                raise ValueError(f"CrossEntropyLoss: ohem_min_kept must be at least 1, got {ohem_min_kept}")
            ops.ohem_tau(ohem_thresh)  # TypeError / ValueError for anything but None or a float in (0, 1]
        self.ohem_min_kept = ohem_min_kept
        self.ohem_thresh = ohem_thresh
        if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int)):
            raise TypeError(f"CrossEntropyLoss: ignore_index must be an int or None, got {ignore_index!r}")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).detach().clone()
            if weight.dim() != 1 or weight.numel() == 0:
                raise ValueError(f"CrossEntropyLoss: weight must be a 1-D tensor of per-class floats, got shape "
                                 f"{tuple(weight.shape)}")
        self.ignore_index = ignore_index
        self.register_buffer("weight", weight, persistent=False)

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self.region_weight is not None:
            return ops.segm_region_loss(logits, target, self.region_weight, *self.region, weight=self.weight,
                                        ignore_index=self.ignore_index)
        if self.ohem_min_kept is not None:
            return ops.cross_entropy_ohem(logits, target, self.ohem_min_kept, self.ohem_thresh, weight=self.weight,
                                          ignore_index=self.ignore_index)
        return ops.cross_entropy(logits, target, weight=self.weight, ignore_index=self.ignore_index)

    def forward_with_predictions(self, logits: torch.Tensor, target: torch.Tensor):
        """(loss, argmax_c logits): the loss pass finds each pixel's maximum anyway (one launch instead of two)."""
        if self.region_weight is not None:
            return ops.segm_region_loss_with_argmax(logits, target, self.region_weight, *self.region, weight=self.weight,
                                                    ignore_index=self.ignore_index)
        if self.ohem_min_kept is not None:
            return ops.cross_entropy_ohem_with_argmax(logits, target, self.ohem_min_kept, self.ohem_thresh,
                                                      weight=self.weight, ignore_index=self.ignore_index)
        return ops.cross_entropy_with_argmax(logits, target, weight=self.weight, ignore_index=self.ignore_index)


class TverskyLoss(nn.Module):
    """The region term alone (ops.segm_region_loss with ce_weight = 0): the multiclass TverskyLoss of
    segmentation_models_pytorch on logits (B,C,H,W) and an int64 target (B,H,W),
    (1/C) sum_{c present} (1 - (TP_c + smooth) / (TP_c + alpha FP_c + beta FN_c + smooth)) over the pixels whose target
    is not ignore_index.  Every pixel ignored: exactly 0.  No parameters or buffers."""

    def __init__(self, alpha: float = 0.5, beta: float = 0.5, smooth: float = 0.0, ignore_index: t.Optional[int] = None):
        super().__init__()
        who = type(self).__name__
        self.alpha = ops.region_loss_number(alpha, "alpha", who, positive=True)
        self.beta = ops.region_loss_number(beta, "beta", who, positive=True)
        self.smooth = ops.region_loss_number(smooth, "smooth", who)
        if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int)):
            raise TypeError(f"{who}: ignore_index must be an int or None, got {ignore_index!r}")
        self.ignore_index = ignore_index

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return ops.segm_region_loss(logits, target, 1.0, self.alpha, self.beta, self.smooth,
                                    ignore_index=self.ignore_index, ce_weight=0.0)

    def forward_with_predictions(self, logits: torch.Tensor, target: torch.Tensor):
        return ops.segm_region_loss_with_argmax(logits, target, 1.0, self.alpha, self.beta, self.smooth,
                                                ignore_index=self.ignore_index, ce_weight=0.0)


class DiceLoss(TverskyLoss):
    """TverskyLoss with alpha = beta = 0.5: 1 - 2 TP / (S + N) per present class."""

    def __init__(self, smooth: float = 0.0, ignore_index: t.Optional[int] = None):
        super().__init__(0.5, 0.5, smooth, ignore_index)


class JaccardLoss(TverskyLoss):
    """TverskyLoss with alpha = beta = 1: 1 - TP / (S + N - TP) per present class."""

    def __init__(self, smooth: float = 0.0, ignore_index: t.Optional[int] = None):
        super().__init__(1.0, 1.0, smooth, ignore_index)


class L1Loss(nn.Module):
    """mean |pred - target| — the depth MAE metric of reference lit_module.py:68,112, usable as a loss."""

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return ops.l1_loss(pred, target)
