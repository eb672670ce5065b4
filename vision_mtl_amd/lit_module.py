"""Host-side mirror of reference vision_mtl/lit_module.py: the step surface run_pipe()/predict()
call (training_lit.py:81-98,115-168,186-216).  A plain nn.Module (the reference's LightningModule is
used without a Trainer), same method names, attributes and step_outputs layout.

Losses, post-processing and the per-step metrics are HIP kernels; nothing on the step path
synchronises with the host.
"""
from __future__ import annotations

import math
import typing as t
from typing import Any

import torch
from torch import nn

from . import metrics as M
from . import ops
from .balancing import TaskBalancer
from .losses import CrossEntropyLoss, SILogGradLoss, SILogLoss
from .models.basic_model import BasicMTLModel
from .surgery import GradSurgery, resolve as resolve_surgery
from .utils.loss_utils import summarize_epoch_metrics


class MTLModule(nn.Module):
    def __init__(self, model: nn.Module, num_classes: int, optim_dict: t.Optional[dict] = None,
                 lr: t.Optional[float] = None, device: str = "cuda", loss_segm_weight: float = 1.0,
                 loss_depth_weight: float = 1.0, segm_ignore_index: t.Optional[int] = None,
                 segm_class_weights: t.Optional[t.Sequence[float]] = None,
                 loss_balancing: t.Union[None, str, TaskBalancer] = None, dwa_temperature: float = 2.0,
                 segm_ohem_min_kept: t.Optional[int] = None, segm_ohem_thresh: t.Optional[float] = None,
                 depth_grad_weight: t.Optional[float] = None, depth_grad_scales: int = 4,
                 segm_region_weight: t.Optional[float] = None, segm_region_alpha: float = 0.5,
                 segm_region_beta: float = 0.5, segm_region_smooth: float = 0.0,
                 grad_surgery: t.Union[None, str, GradSurgery] = None):
        """segm_ignore_index / segm_class_weights (opt-in): the `ignore_index` and per-class `weight`
        of the segmentation criterion; the ignore index also keeps those pixels out of the segmentation metrics.
        loss_balancing (opt-in): "uncertainty" | "dwa" | "geometric" or a balancing.TaskBalancer
        over the tasks ("segm", "depth"); it becomes the submodule `task_balancer` and takes the place of the two static
        weights, which must then stay 1.0.  dwa_temperature: the softmax temperature of "dwa".
        segm_ohem_min_kept / segm_ohem_thresh (opt-in): online hard example mining in the
        segmentation loss of the TRAINING step - it becomes the submodule `segm_train_criterion`; validation, test and
        predict keep reporting the un-mined loss of `segm_criterion` with the same weights and ignore index.
        depth_grad_weight / depth_grad_scales (opt-in): `depth_criterion` becomes
        SILog + depth_grad_weight * the multi-scale gradient-matching term (losses.SILogGradLoss), in every stage: it is
        part of the loss definition, like the class weights.
        segm_region_weight / segm_region_alpha / _beta / _smooth (opt-in): `segm_criterion`
        becomes cross entropy + segm_region_weight * the Dice / Tversky region term (losses.CrossEntropyLoss with
        region_weight), in every stage, like depth_grad_weight; it does not combine with segm_ohem_min_kept.
        grad_surgery (opt-in): "sum" | "pcgrad" | "mgda" | "imtl_g" or a surgery.GradSurgery -
        the training step's backward pass combines the two tasks' gradients of the shared decoder map by that method.  It
        is set on the model (`BasicMTLModel.grad_surgery`; `csnet` and `mtan` have no single shared representation and
        are refused) and acts on the gradient, so it combines with everything above that acts on the losses."""
        super().__init__()
        grad_surgery = resolve_surgery(grad_surgery)
        if grad_surgery is not None and not isinstance(model, BasicMTLModel):  # checked before anything is built
            raise ValueError(f"MTLModule: grad_surgery needs a model whose tasks share one representation "
                             f"(BasicMTLModel), got {type(model).__name__}")
        region = {}
        if segm_region_weight is not None:  # checked before anything is built
            if segm_ohem_min_kept is not None or segm_ohem_thresh is not None:
                raise ValueError("MTLModule: segm_region_weight does not combine with segm_ohem_min_kept / "
                                 "segm_ohem_thresh (mining the region term is not supported)")
            if not 2 <= num_classes <= ops.CE_REGION_MAX_CLASSES:
                raise ValueError(f"MTLModule: segm_region_weight takes 2 to {ops.CE_REGION_MAX_CLASSES} classes, got "
                                 f"num_classes = {num_classes}")
            region = dict(
                region_weight=ops.region_loss_number(segm_region_weight, "segm_region_weight", "MTLModule", positive=True),
                region_alpha=ops.region_loss_number(segm_region_alpha, "segm_region_alpha", "MTLModule", positive=True),
                region_beta=ops.region_loss_number(segm_region_beta, "segm_region_beta", "MTLModule", positive=True),
                region_smooth=ops.region_loss_number(segm_region_smooth, "segm_region_smooth", "MTLModule"))
        if loss_balancing is not None:
            if loss_segm_weight != 1.0 or loss_depth_weight != 1.0:
                raise ValueError("MTLModule: loss_balancing replaces the static loss weights: leave loss_segm_weight and "
                                 f"loss_depth_weight at 1.0 (got {loss_segm_weight}, {loss_depth_weight})")
            if isinstance(loss_balancing, str):
                loss_balancing = TaskBalancer(loss_balancing, temperature=dwa_temperature)
            elif not isinstance(loss_balancing, TaskBalancer):
                raise ValueError(f"MTLModule: loss_balancing must be None, a method name or a TaskBalancer, got "
                                 f"{type(loss_balancing).__name__}")
            if loss_balancing.tasks != ("segm", "depth"):
                raise ValueError(f"MTLModule: the balancer's tasks must be ('segm', 'depth'), got {loss_balancing.tasks}")
        if segm_class_weights is not None:
            segm_class_weights = torch.as_tensor(segm_class_weights, dtype=torch.float32).detach().flatten()
            if segm_class_weights.numel() != num_classes:
                raise ValueError(f"MTLModule: segm_class_weights must hold num_classes = {num_classes} floats, got "
                                 f"{segm_class_weights.numel()}")
        self.hparams = {"num_classes": num_classes, "optim_dict": optim_dict, "lr": lr, "device": device,
                        "loss_segm_weight": loss_segm_weight, "loss_depth_weight": loss_depth_weight,
                        "segm_ignore_index": segm_ignore_index,
                        "segm_class_weights": None if segm_class_weights is None else segm_class_weights.tolist()}
        if loss_balancing is not None:  # the default module keeps the hparams it always had
            self.hparams.update(loss_balancing=loss_balancing.method, dwa_temperature=loss_balancing.temperature)
        if grad_surgery is not None:  # the default module keeps the hparams it always had
            self.hparams.update(grad_surgery=grad_surgery.method)
            model.grad_surgery = grad_surgery
        self.num_classes = num_classes
        self.model = model
        if region:  # the default module keeps the hparams and the criterion it always had
            self.hparams.update({"segm_" + k: v for k, v in region.items()})
        self.segm_criterion = CrossEntropyLoss(weight=segm_class_weights, ignore_index=segm_ignore_index, **region)
        if segm_class_weights is not None:  # the model usually arrives on its device: the weights join it there
            p = next(model.parameters(), None)
            if p is not None:
                self.segm_criterion.to(p.device)
        if segm_ohem_min_kept is not None or segm_ohem_thresh is not None:  # absent by default, as the balancer
            self.hparams.update(segm_ohem_min_kept=segm_ohem_min_kept, segm_ohem_thresh=segm_ohem_thresh)
            self.segm_train_criterion = CrossEntropyLoss(weight=segm_class_weights, ignore_index=segm_ignore_index,
                                                         ohem_min_kept=segm_ohem_min_kept, ohem_thresh=segm_ohem_thresh)
            if segm_class_weights is not None:
                self.segm_train_criterion.to(self.segm_criterion.weight.device)
        self.segm_ignore_index = segm_ignore_index
        if depth_grad_weight is None:
            self.depth_criterion = SILogLoss()
        else:  # same child name, no parameters or buffers: checkpoints keep their keys
            if (isinstance(depth_grad_weight, bool) or not isinstance(depth_grad_weight, (int, float))
                    or not math.isfinite(depth_grad_weight) or depth_grad_weight <= 0):
                raise ValueError(f"MTLModule: depth_grad_weight must be a finite float > 0, got {depth_grad_weight!r}")
            if (isinstance(depth_grad_scales, bool) or not isinstance(depth_grad_scales, int)
                    or not 1 <= depth_grad_scales <= ops.DEPTH_GRAD_SCALES_MAX):
                raise ValueError(f"MTLModule: depth_grad_scales must be an int in 1..{ops.DEPTH_GRAD_SCALES_MAX}, got "
                                 f"{depth_grad_scales!r}")
            self.hparams.update(depth_grad_weight=float(depth_grad_weight), depth_grad_scales=depth_grad_scales)
            self.depth_criterion = SILogGradLoss(grad_weight=float(depth_grad_weight), scales=depth_grad_scales)
        if loss_balancing is not None:  # absent by default: state_dict() keys and parameters() stay the reference's
            p = next(model.parameters(), None)
            self.task_balancer = loss_balancing if p is None else loss_balancing.to(p.device)
        self.optim_dict = optim_dict
        self.loss_segm_weight = loss_segm_weight
        self.loss_depth_weight = loss_depth_weight
        self.step_outputs = {k: {"loss": [], "accuracy": [], "jaccard_index": [], "fbeta_score": [], "mae": []}
                             for k in ["train", "val", "test", "predict"]}
        # reference lit_module.py:48-69 (torchmetrics 0.7.3 Accuracy-micro / FBeta-weighted / Jaccard / MAE)
        ign = segm_ignore_index
        self.metrics = {"accuracy": M.Accuracy(num_classes, ignore_index=ign),
                        "fbeta_score": M.FBetaScore(num_classes, beta=1.0, ignore_index=ign),
                        "jaccard_index": M.JaccardIndex(num_classes, ignore_index=ign), "mae": M.MeanAbsoluteError()}
        self.automatic_optimization = False
        self.compute_metrics = True  # bench.py turns this off to time exactly fwd + losses + bwd
        self._nan = {}  # device -> the NaN placeholder of the skipped metrics (built once, not filled every step)
        self.dp_arena = None  # a dp.FlatArena: training_step's loss then averages gradients over ranks at end of backward
        # a data.DeviceTransform: transfer_batch_to_device then takes raw batches (data.collate_raw) and runs the sample
        # transform on the device (GraphedStep records it at construction)
        self.device_transform = None
        # a data.DeviceAugment: training_step applies it to the device batch (validation, test and predict never do;
        # GraphedStep(stage="train") records it at construction and captures it)
        self.train_augment = None
        # an inference.PredictAugment: predict_step merges flipped / rescaled views and returns predictions at its output
        # size (training, validation and test never look at it; GraphedEval(stage="predict") records it at construction)
        self.predict_augment = None
        # a dp.ArenaAverage (EMA / SWA of the arena's parameters): validation_step, test_step and predict_step run with the
        # averaged weights exchanged in (ArenaAverage.applied), training_step never does; GraphedEval records at
        # construction whether it was set.  An attribute like train_augment: hparams and state_dict() keys do not change
        self.weight_average = None
        self._mining = False  # True inside a training step's calc_losses

    @property
    def grad_surgery(self) -> t.Optional[GradSurgery]:
        """The model's surgery.GradSurgery (None by default): its .stats / .coefficients / .conflict_rate() are device
        tensors that show the last training step."""
        return getattr(self.model, "grad_surgery", None)

    @grad_surgery.setter
    def grad_surgery(self, value) -> None:
        value = resolve_surgery(value)
        if value is not None and not isinstance(self.model, BasicMTLModel):
            raise ValueError(f"MTLModule: grad_surgery needs a BasicMTLModel, got {type(self.model).__name__}")
        self.model.grad_surgery = value

    def forward(self, x: torch.Tensor) -> dict:
        return self.model(x)

    # ---- reference lit_module.py:75-95
    def shared_step(self, batch: dict, stage: str) -> torch.Tensor:
        img, gt_mask, gt_depth = batch["img"], batch["mask"], batch["depth"]
        raw_out = self(img)
        # the segmentation prediction comes out of the cross-entropy pass (calc_losses) when the criterion can emit it
        out = self.postprocess_raw_out(raw_out, defer_segm_predictions=hasattr(self.segm_criterion, "forward_with_predictions"))
        self._mining = stage == "train"  # calc_losses keeps its signature: the training step alone mines
        try:
            all_losses = self.calc_losses(gt_mask, gt_depth, out)
        finally:
            self._mining = False
        all_metrics = self.calc_metrics(gt_mask, gt_depth, out)
        self.update_step_stats(stage, all_losses, all_metrics)
        if stage == "train" and self.dp_arena is not None and torch.is_grad_enabled():
            return self.dp_arena.sync_loss(all_losses["loss"])
        return all_losses["loss"]

    def update_step_stats(self, stage: str, all_losses: dict, all_metrics: dict) -> None:
        so = self.step_outputs[stage]
        so["loss"].append(all_losses["loss"].detach())
        for k in ("accuracy", "jaccard_index", "fbeta_score", "mae"):
            so[k].append(all_metrics[k])

    def calc_metrics(self, gt_mask, gt_depth, out: dict) -> dict:
        if not self.compute_metrics:
            nan = self._nan.get(gt_mask.device)
            if nan is None:
                nan = self._nan[gt_mask.device] = torch.full((), float("nan"), device=gt_mask.device)
            return {"accuracy": nan, "jaccard_index": nan, "fbeta_score": nan, "mae": nan}
        if self.segm_ignore_index is None:  # the default step makes the call it always made
            cm = M.confusion_matrix(out["segm_predictions"], gt_mask, self.num_classes)
        else:
            cm = M.confusion_matrix(out["segm_predictions"], gt_mask, self.num_classes,
                                    ignore_index=self.segm_ignore_index)
        return {"accuracy": self.metrics["accuracy"].from_confusion(cm),
                "jaccard_index": self.metrics["jaccard_index"].from_confusion(cm),
                "fbeta_score": self.metrics["fbeta_score"].from_confusion(cm),
                "mae": self.metrics["mae"](out["depth_predictions"].detach(), gt_depth)}

    def calc_losses(self, gt_mask, gt_depth, out: dict) -> dict:  # reference lit_module.py:120-131
        criterion = self.segm_criterion
        if self._mining:  # a training step: the mining criterion, when there is one
            criterion = getattr(self, "segm_train_criterion", criterion)
        if out.get("segm_predictions") is None and hasattr(criterion, "forward_with_predictions"):
            loss_segm, out["segm_predictions"] = criterion.forward_with_predictions(out["segm_logits"], gt_mask)
        else:
            loss_segm = criterion(out["segm_logits"], gt_mask)
        loss_depth = self.depth_criterion(out["depth_predictions"], gt_depth)
        balancer = getattr(self, "task_balancer", None)
        if balancer is not None:  # learned / dynamic weights, read on the device (csrc/balance.hip)
            loss = balancer({"segm": loss_segm, "depth": loss_depth})
        elif loss_segm.is_cuda and loss_segm.dim() == 0 and loss_depth.dim() == 0:
            loss = ops.add_losses(loss_segm, loss_depth, self.loss_segm_weight, self.loss_depth_weight)
        else:
            loss = self.loss_segm_weight * loss_segm + self.loss_depth_weight * loss_depth
        return {"loss": loss, "loss_segm": loss_segm, "loss_depth": loss_depth}

    def postprocess_raw_out(self, out: dict, defer_segm_predictions: bool = False) -> dict:  # reference lit_module.py:133-144
        segm_logits, depth_logits = out["segm"], out["depth"]
        return {"segm_logits": segm_logits,
                # argmax(softmax(z)) == argmax(z); deferred: calc_losses fills it from the cross-entropy pass
                "segm_predictions": None if defer_segm_predictions else ops.argmax_channels(segm_logits),
                "depth_predictions": ops.sigmoid(depth_logits).permute(0, 2, 3, 1)}

    def training_step(self, batch: dict, batch_idx: Any = 0):
        if self.train_augment is not None:
            batch = self.train_augment(batch)
        return self.shared_step(batch=batch, stage="train")

    def validation_step(self, batch: dict, batch_idx: Any = 0):
        if self.weight_average is None:  # the default step makes the call it always made
            return self.shared_step(batch=batch, stage="val")
        with self.weight_average.applied():
            return self.shared_step(batch=batch, stage="val")

    def test_step(self, batch: dict, batch_idx: Any = 0):
        if self.weight_average is None:
            return self.shared_step(batch=batch, stage="test")
        with self.weight_average.applied():
            return self.shared_step(batch=batch, stage="test")

    def predict_step(self, batch: dict, batch_idx: int = 0, dataloader_idx: int = 0):
        if self.weight_average is None:
            return self._predict_step(batch)
        with self.weight_average.applied():
            return self._predict_step(batch)

    def _predict_step(self, batch: dict) -> dict:
        """predict_step on the weights as they stand (GraphedEval captures this: the exchange is not part of its graph)."""
        if self.predict_augment is not None:
            return self._predict_augmented(batch)
        out = self.postprocess_raw_out(self(batch["img"]))
        if "mask" in batch and "depth" in batch:
            gt_mask, gt_depth = batch["mask"], batch["depth"]
            self.update_step_stats("predict", self.calc_losses(gt_mask, gt_depth, out),
                                   self.calc_metrics(gt_mask, gt_depth, out))
        return {"segm": out["segm_predictions"], "depth": out["depth_predictions"]}

    def _predict_augmented(self, batch: dict) -> dict:
        """predict_step under `predict_augment`: the merged predictions at the object's output size.  With targets in the
        batch (at that size) the four metrics go through calc_metrics as in the plain step; the "loss" entry is the NaN
        placeholder - a merged prediction has no logits to put a criterion on."""
        img = batch["img"]
        has_targets = "mask" in batch and "depth" in batch
        if has_targets:  # checked before any launch
            B, _, H, W = img.shape
            Ho, Wo = self.predict_augment.out_size(H, W)
            gt_mask, gt_depth = batch["mask"], batch["depth"]
            if tuple(gt_mask.shape) != (B, Ho, Wo) or tuple(gt_depth.shape) not in ((B, Ho, Wo, 1), (B, Ho, Wo)):
                raise ValueError(f"MTLModule.predict_step: predict_augment returns predictions of size {(Ho, Wo)}: mask "
                                 f"must be {(B, Ho, Wo)} and depth {(B, Ho, Wo, 1)}, got {tuple(gt_mask.shape)} and "
                                 f"{tuple(gt_depth.shape)}")
        res = self.predict_augment(self.model, img)
        if has_targets:
            out = {"segm_predictions": res["segm"], "depth_predictions": res["depth"].view(gt_depth.shape)}
            nan = self._nan.get(img.device)
            if nan is None:
                nan = self._nan[img.device] = torch.full((), float("nan"), device=img.device)
            self.update_step_stats("predict", {"loss": nan}, self.calc_metrics(gt_mask, gt_depth, out))
        return res

    def shared_epoch_end(self, stage: Any):
        return summarize_epoch_metrics(self.step_outputs[stage], metric_name_prefix=stage)

    def on_train_epoch_end(self):
        balancer = getattr(self, "task_balancer", None)
        if balancer is not None:  # "dwa": the epoch's mean losses become the next epoch's weights
            balancer.on_train_epoch_end()
        return self.shared_epoch_end("train")

    def on_validation_epoch_end(self):
        return self.shared_epoch_end("val")

    def on_test_epoch_end(self):
        return self.shared_epoch_end("test")

    def on_predict_epoch_end(self):
        return self.shared_epoch_end("predict")

    def configure_optimizers(self):  # reference lit_module.py:193-209 (unused by run_pipe)
        if self.optim_dict:
            return self.optim_dict
        optimizer = torch.optim.Adam(params=self.parameters(), lr=self.hparams["lr"])
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer=optimizer, patience=5, factor=0.95)
        return {"optimizer": optimizer,
                "lr_scheduler": {"scheduler": scheduler, "interval": "epoch", "monitor": "train_loss"}}

    def transfer_batch_to_device(self, batch: dict, device, dataloader_idx: int = 0):
        """reference lit_module.py:211-219.  Pinned host tensors (DataLoader(pin_memory=True), data.collate) go up
        asynchronously on the current stream; an image batch kept in dataset sample layout (B,H,W,3) is re-laid on
        the device by one kernel straight into the model's input storage (data.upload_batch).  With device_transform
        set, the batch is a raw one (data.collate_raw) and the transform runs on the device after the copy."""
        from .data import upload_batch

        if isinstance(batch, dict):
            up = upload_batch(batch, device, transform=self.device_transform)
            for key in batch.keys():
                batch[key] = up[key]
            return batch
        return batch.to(device, non_blocking=batch.device.type == "cpu" and batch.is_pinned())

    def parameters(self, recurse: bool = True):  # reference lit_module.py:232-234
        for p in self.model.parameters():
            yield p
        balancer = getattr(self, "task_balancer", None)
        if balancer is not None:  # the log-variances of "uncertainty" train with the model, after its parameters
            for p in balancer.parameters():
                yield p
