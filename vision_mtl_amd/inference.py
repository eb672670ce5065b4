"""Inference-side options of the predict step: flip / multi-scale test-time augmentation and predictions at the labels'
resolution.  The counterpart of data.DeviceAugment, which trains with
the same scale and flip transforms::

    module.predict_augment = PredictAugment(scales=(0.75, 1.0, 1.25), flip=True, output_size=(1024, 2048))
    preds = module.predict_step(batch)              # or GraphedEval(module, batch, stage="predict")(batch)

Opt-in and forward-only: with `module.predict_augment is None` the predict step is the reference's.  Host plumbing only -
the views, the merge and the output-size reduction are three HIP kernels (csrc/tta.hip) and the model's own forward."""
from __future__ import annotations

import math

import torch

from . import ops

MERGES = tuple(ops.TTA_MODES)


class PredictAugment:
    """scales: the view sizes relative to the batch's own, each rounded to a multiple of `size_multiple` (the model's
    stride); flip: every scale also mirrored in x; output_size: (Ho, Wo) of the returned predictions (default: the
    batch's size); merge: "prob" averages softmax probabilities, "logit" averages logits; compensate_depth: multiply a
    view's depth by its scale before averaging - the inverse of DeviceAugment's "depth divided by the scale";
    return_confidence: also return the largest softmax probability of the merged map per output pixel."""

    def __init__(self, scales=(1.0,), flip: bool = False, output_size=None, merge: str = "prob", size_multiple: int = 32,
                 compensate_depth: bool = False, return_confidence: bool = False):
        try:
            scales = tuple(float(s) for s in scales)
        except TypeError:
            raise ValueError(f"PredictAugment: scales must be a non-empty sequence of finite floats > 0, got {scales!r}") from None
        if not scales or any(not math.isfinite(s) or s <= 0 for s in scales):
            raise ValueError(f"PredictAugment: scales must be a non-empty sequence of finite floats > 0, got {scales!r}")
        if merge not in MERGES:
            raise ValueError(f"PredictAugment: merge must be one of {MERGES}, got {merge!r}")
        if output_size is not None:
            output_size = ops._tta_size(output_size, "PredictAugment: output_size")
        if isinstance(size_multiple, bool) or not isinstance(size_multiple, int) or size_multiple < 1:
            raise ValueError(f"PredictAugment: size_multiple must be an int >= 1, got {size_multiple!r}")
        self.scales, self.flip, self.output_size, self.merge = scales, bool(flip), output_size, merge
        self.size_multiple = size_multiple
        self.compensate_depth, self.return_confidence = bool(compensate_depth), bool(return_confidence)

    def __repr__(self):
        return (f"PredictAugment(scales={self.scales}, flip={self.flip}, output_size={self.output_size}, "
                f"merge={self.merge!r}, size_multiple={self.size_multiple}, compensate_depth={self.compensate_depth}, "
                f"return_confidence={self.return_confidence})")

    def views(self, H: int, W: int) -> list:
        """The ordered view table [(h, w, flip, scale)] for a batch of size (H, W): the scales as given, unflipped before
        flipped, duplicate (h, w, flip) rows dropped.  Host only."""
        m = self.size_multiple
        table, seen = [], set()
        for s in self.scales:
            h, w = max(m, round(s * H / m) * m), max(m, round(s * W / m) * m)
            for flip in ((False, True) if self.flip else (False,)):
                if (h, w, flip) not in seen:
                    seen.add((h, w, flip))
                    table.append((h, w, flip, s))
        return table

    def out_size(self, H: int, W: int) -> tuple:
        return (H, W) if self.output_size is None else self.output_size

    @torch.no_grad()
    def __call__(self, model, img) -> dict:
        """{"segm": int64 (B,Ho,Wo), "depth": float32 (B,Ho,Wo,1)[, "confidence": float32 (B,Ho,Wo)]} of the merged
        views of `img` ((B,3,H,W), as the model takes it).  Per view: ops.tta_view (not for the identity view, which is
        the batch itself), the model's forward, ops.tta_accumulate; then one ops.tta_finish."""
        B, _, H, W = img.shape
        table = self.views(H, W)
        acc = acc_depth = None
        for k, (h, w, flip, s) in enumerate(table):
            view = img if (h, w, flip) == (H, W, False) else ops.tta_view(img, (h, w), flip)
            out = model(view)
            logits, depth_logits = out["segm"], out["depth"]
            if acc is None:
                C = logits.shape[1]
                if C > ops.TTA_MAX_CLASSES:
                    raise ValueError(f"PredictAugment: at most {ops.TTA_MAX_CLASSES} classes are supported, the model "
                                     f"returns {C}")
                acc, acc_depth = ops._empty((B, C, H, W), logits), ops._empty((B, H, W), logits)
            ops.tta_accumulate(logits, depth_logits, acc, acc_depth, flip=flip, weight=1.0,
                               depth_gain=s if self.compensate_depth else 1.0, merge=self.merge, first=k == 0)
        segm, depth, conf = ops.tta_finish(acc, acc_depth, 1.0 / len(table), self.out_size(H, W), merge=self.merge,
                                           confidence=self.return_confidence)
        res = {"segm": segm, "depth": depth.unsqueeze(-1)}
        if conf is not None:
            res["confidence"] = conf
        return res
