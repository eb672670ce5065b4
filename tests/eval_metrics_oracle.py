"""Test helper: the DEFINITION of the dataset-level evaluation metrics (csrc/eval_accum.hip, include/vmtl.h), in fp64
torch on the CPU.

State: cm[t, p] int64 over the pixels whose target is not the ignore index and whose target and prediction are in
[0, C); acc float64[16] over the valid depth pixels (target > float32(min_depth), or the mask), with the prediction
clamped below at float32(min_depth) first:
    [0] n  [1] sum|p-t|  [2] sum|p-t|/t  [3] sum(p-t)^2/t  [4] sum(p-t)^2  [5] sum g^2  [6] sum g, g = ln p - ln t
    [7] sum|log10 p - log10 t|  [8..10] #max(p/t, t/p) < 1.25, 1.25^2, 1.25^3   [11..15] zero
Metrics: class means over the classes that occur (union, or support for the accuracy, non-zero), never the ignore index."""
import math

import torch

SCALARS = ("pixel_acc", "mean_acc", "miou", "fbeta", "abs_err", "rel_err", "sq_rel", "rmse", "rmse_log", "log10", "silog",
           "delta1", "delta2", "delta3", "n_valid", "n_pixels")
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
COUNT_SLOTS = (0, 8, 9, 10)
SUM_SLOTS = (1, 2, 3, 4, 5, 6, 7)


def confusion(pred, target, C, ignore_index=None):
    pred, target = pred.reshape(-1).long().cpu(), target.reshape(-1).long().cpu()
    keep = (target >= 0) & (target < C) & (pred >= 0) & (pred < C)
    if ignore_index is not None:
        keep &= target != ignore_index
    return torch.bincount(target[keep] * C + pred[keep], minlength=C * C).reshape(C, C)


def depth_terms(pred, target, min_depth=1e-3, valid=None):
    """-> (acc float64[16], mag float64[16]: the sum of |term| behind every floating sum, margin: the smallest relative
    distance of a valid pixel's ratio from a delta threshold (inf without valid pixels))."""
    pred, target = pred.reshape(-1).float().cpu(), target.reshape(-1).float().cpu()
    md = torch.tensor(min_depth, dtype=torch.float32)
    keep = target > md if valid is None else valid.reshape(-1).cpu() != 0
    p = torch.maximum(pred, md)[keep].double()  # the clamp is in fp32, as the kernel's
    t = target[keep].double()
    d = p - t
    g = torch.log(p) - torch.log(t)
    ratio = torch.maximum(p / t, t / p)
    terms = [d.abs(), d.abs() / t, d * d / t, d * d, g * g, g, (torch.log10(p) - torch.log10(t)).abs()]
    acc, mag = torch.zeros(16, dtype=torch.float64), torch.zeros(16, dtype=torch.float64)
    acc[0] = t.numel()
    for slot, term in zip(SUM_SLOTS, terms):
        acc[slot], mag[slot] = term.sum(), term.abs().sum()
    margin = math.inf
    for slot, th in zip(COUNT_SLOTS[1:], THRESHOLDS):
        acc[slot] = int((ratio < th).sum())
        if t.numel():
            margin = min(margin, float(((ratio - th).abs() / th).min()))
    return acc, mag, margin


def finalize(cm, acc, beta=1.0, ignore_index=None):
    """-> {name: float for name in SCALARS, "iou": float64 (C,)}"""
    cm, acc = cm.double().cpu(), acc.double().cpu()
    C = cm.shape[0]
    nan = float("nan")
    tp, row, col = cm.diag(), cm.sum(1), cm.sum(0)
    fn, fp = row - tp, col - tp
    total = float(row.sum())
    union = tp + fp + fn
    classes = torch.ones(C, dtype=torch.bool)
    if ignore_index is not None and 0 <= ignore_index < C:
        classes[ignore_index] = False
    iou = torch.full((C,), nan, dtype=torch.float64)
    in_iou = classes & (union > 0)
    iou[in_iou] = tp[in_iou] / union[in_iou]
    in_acc = classes & (row > 0)
    b2 = beta * beta
    den = (1 + b2) * tp + b2 * fn + fp
    f = torch.where(den > 0, (1 + b2) * tp / den.clamp(min=1e-300), torch.zeros_like(den))
    out = {"iou": iou, "n_pixels": total, "n_valid": float(acc[0])}
    if total > 0:
        out["pixel_acc"] = float(tp.sum()) / total
        out["mean_acc"] = float((tp[in_acc] / row[in_acc]).mean()) if bool(in_acc.any()) else nan
        out["miou"] = float(iou[in_iou].mean()) if bool(in_iou.any()) else nan
        out["fbeta"] = float((row * f).sum()) / total
    else:
        out.update(pixel_acc=nan, mean_acc=nan, miou=nan, fbeta=nan)
        out["iou"] = torch.full((C,), nan, dtype=torch.float64)
    n = float(acc[0])
    if n > 0:
        eg2, eg = float(acc[5]) / n, float(acc[6]) / n
        out.update(abs_err=float(acc[1]) / n, rel_err=float(acc[2]) / n, sq_rel=float(acc[3]) / n,
                   rmse=math.sqrt(float(acc[4]) / n), rmse_log=math.sqrt(eg2), log10=float(acc[7]) / n,
                   silog=math.sqrt(max(eg2 - eg * eg, 0.0)), delta1=float(acc[8]) / n, delta2=float(acc[9]) / n,
                   delta3=float(acc[10]) / n)
    else:
        out.update({k: nan for k in SCALARS[4:14]})
    return out


def dataset_metrics(segm_pred, mask, depth_pred, depth, C, ignore_index=None, min_depth=1e-3, beta=1.0, valid=None):
    return finalize(confusion(segm_pred, mask, C, ignore_index), depth_terms(depth_pred, depth, min_depth, valid)[0],
                    beta, ignore_index)
