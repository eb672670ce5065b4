"""Host-side mirror of the construction API, reference vision_mtl/utils/pipeline_utils.py:22-30,80-136."""
from __future__ import annotations

import argparse
import typing as t

import torch

from ..lit_module import MTLModule
from ..models.basic_model import BasicMTLModel
from ..models.cross_stitch_model import CSNet, check_stitch_mixing
from ..models.mtan_model import MTANMiniUnet
from ..models.unet_mobilenetv3 import get_model_with_dense_preds


class DataConfig(t.Protocol):
    num_classes: int


def build_model(args: argparse.Namespace, data_cfg: DataConfig) -> t.Union[BasicMTLModel, MTANMiniUnet, CSNet]:
    """reference utils/pipeline_utils.py:80-136: dispatch on args.model_name in {basic, mtan, csnet}."""
    encoder_weights = getattr(args, "backbone_weights", "imagenet")
    if args.model_name == "basic":
        return BasicMTLModel(segm_classes=data_cfg.num_classes, decoder_first_channel=540, num_decoder_layers=5,
                             encoder_weights=encoder_weights)
    if args.model_name == "mtan":
        return MTANMiniUnet(in_channels=3, map_tasks_to_num_channels={"depth": 1, "segm": data_cfg.num_classes},
                            task_subnets_hidden_channels=128, encoder_first_channel=32, encoder_num_channels=4)
    if args.model_name == "csnet":
        mixing = check_stitch_mixing(getattr(args, "cross_stitch_mixing", "diagonal"))  # before the networks are built
        backbone_params = dict(encoder_name="timm-mobilenetv3_large_100", encoder_weights=encoder_weights,
                               decoder_first_channel=256, num_decoder_layers=5)
        models = {
            "depth": get_model_with_dense_preds(segm_classes=1, activation=None, backbone_params=backbone_params),
            "segm": get_model_with_dense_preds(segm_classes=data_cfg.num_classes, activation=None,
                                               backbone_params=backbone_params),
        }
        # "diagonal": the reference's arithmetic; "full": the opt-in cross-stitch unit proper
        return CSNet(models, channel_wise_stitching=getattr(args, "channel_wise_stitching", True),
                     stitch_mixing=mixing)
    raise NotImplementedError(f"Unknown model name: {args.model_name}")


def init_model(args: argparse.Namespace, data_cfg: DataConfig) -> MTLModule:
    """reference utils/pipeline_utils.py:22-30.

    Averaged weights (dp.ArenaAverage) are not wired here: they live next to a dp.FlatArena,
    which the caller builds after the model is on its device, so args.weight_average / weight_average_decay /
    weight_average_warmup are not read - set module.weight_average once the arena exists."""
    grad_surgery = getattr(args, "grad_surgery", None)
    if grad_surgery is not None:  # checked before the networks are built
        from ..surgery import resolve

        grad_surgery = resolve(grad_surgery)
        if args.model_name != "basic":
            raise ValueError(f"init_model: grad_surgery needs the single shared representation of model_name 'basic', got "
                             f"{args.model_name!r} (INTEGRATION.md section 17)")
    model = build_model(args, data_cfg)
    # opt-in: an ignored label / per-class weights (a sequence of num_classes floats) for the segmentation loss
    module = MTLModule(model=model, num_classes=data_cfg.num_classes, lr=getattr(args, "lr", None),
                       device=getattr(args, "device", "cuda"),
                       segm_ignore_index=getattr(args, "segm_ignore_index", None),
                       segm_class_weights=getattr(args, "segm_class_weights", None),
                       # opt-in: "uncertainty" | "dwa" | "geometric" task-loss balancing
                       loss_balancing=getattr(args, "loss_balancing", None),
                       dwa_temperature=getattr(args, "dwa_temperature", 2.0),
                       # opt-in: online hard example mining in the training step's segmentation loss
                       segm_ohem_min_kept=getattr(args, "segm_ohem_min_kept", None),
                       segm_ohem_thresh=getattr(args, "segm_ohem_thresh", None),
                       # opt-in: SILog + weight * multi-scale gradient matching as the depth loss
                       depth_grad_weight=getattr(args, "depth_grad_weight", None),
                       depth_grad_scales=getattr(args, "depth_grad_scales", 4),
                       # opt-in: cross entropy + weight * Dice / Tversky region term as the
                       # segmentation loss
                       segm_region_weight=getattr(args, "segm_region_weight", None),
                       segm_region_alpha=getattr(args, "segm_region_alpha", 0.5),
                       segm_region_beta=getattr(args, "segm_region_beta", 0.5),
                       segm_region_smooth=getattr(args, "segm_region_smooth", 0.0),
                       # opt-in: "sum" | "pcgrad" | "mgda" | "imtl_g" gradient surgery at the
                       # shared decoder map of `basic`
                       grad_surgery=grad_surgery)
    # opt-in: test-time augmentation / output-size predictions of the predict step; an
    # attribute like train_augment, nothing goes into hparams
    scales, flip = getattr(args, "predict_scales", None), getattr(args, "predict_flip", None)
    out_size, merge = getattr(args, "predict_output_size", None), getattr(args, "predict_merge", None)
    if any(v is not None for v in (scales, flip, out_size, merge)):
        from ..inference import PredictAugment

        module.predict_augment = PredictAugment(scales=(1.0,) if scales is None else scales, flip=bool(flip),
                                                output_size=None if out_size is None else tuple(out_size),
                                                merge="prob" if merge is None else merge)
    if getattr(args, "ckpt_dir", None):
        from .ckpt import load_ckpt_model

        module.load_state_dict(load_ckpt_model(args.ckpt_dir)["model"])
    return module


def fetch_data_cfg(dataset_name: str):
    """reference utils/pipeline_utils.py:288-294 with the constants of cfg.py:63-155."""
    if dataset_name == "cityscapes":
        return argparse.Namespace(num_classes=19, height=128, width=256, batch_size=8)
    if dataset_name == "nyuv2":
        return argparse.Namespace(num_classes=14, height=256, width=256, batch_size=4)
    raise ValueError(f"Unknown dataset name: {dataset_name}")
