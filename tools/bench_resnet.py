#!/usr/bin/env python
"""ms/step and img/s of `basic` with a ResNet encoder (default resnet34) at 128x256: the captured training step
(graphed.GraphedStep: fwd + losses + bwd) and the captured predict step (graphed.GraphedEval, eval mode), in fp32 and
bf16 convolution precision, at bs 8 and 32.  Then the stride-2 data gradients of the encoder's strided convs
(vmtl_conv2d_dgrad_s2) timed against the stride-1 data gradient of the same channel counts at the same input extent.

    python tools/bench_resnet.py [--encoder resnet34] [--steps 20] [--warmup 3] [--only train|predict|dgrad]
                                 [--batch 32] [--prec fp32]

Prints one JSON line per measurement.  For the per-kernel profile run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_resnet.py --only train --batch 32 --prec fp32`."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _events(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def _module(encoder, dev):
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.models.basic_model import BasicMTLModel

    torch.manual_seed(0)
    model = BasicMTLModel(19, encoder_name=encoder, encoder_weights=None).to(dev)
    return MTLModule(model, num_classes=19, device=str(dev))


def bench_train(encoder, B, H, W, prec, steps, warmup, dev):
    from vision_mtl_amd import conv_precision, dp
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep

    module = _module(encoder, dev)
    module.model.train()
    arena = dp.FlatArena(module.model)
    batch = synthetic_batch(B, H, W, 19, seed=1, masked=0.1)
    with conv_precision(prec):
        g = GraphedStep(module, batch, arena=arena)
    ms = _events(lambda: g(batch), steps, warmup)
    return dict(step="train", encoder=encoder, batch=B, hw=[H, W], prec=prec, ms_per_step=round(ms, 3),
                img_per_s=round(B / ms * 1e3, 1))


def bench_predict(encoder, B, H, W, prec, steps, warmup, dev):
    from vision_mtl_amd import conv_precision
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedEval

    module = _module(encoder, dev)
    module.eval()
    batch = {"img": synthetic_batch(B, H, W, 19, seed=1)["img"]}
    with conv_precision(prec):
        g = GraphedEval(module, batch, stage="predict")
    with torch.no_grad():
        ms = _events(lambda: g(batch), steps, warmup)
    return dict(step="predict", encoder=encoder, batch=B, hw=[H, W], prec=prec, ms_per_step=round(ms, 3),
                img_per_s=round(B / ms * 1e3, 1))


def bench_dgrad(B, H, W, steps, warmup, dev):
    """The strided convs of resnet34's encoder at input H x W (stem 7x7 at the image, 3x3 conv1 and 1x1 downsample of
    layers 2-4) - the phase-decomposed data gradient vs the stride-1 data gradient (same Cin / Cout / K at the same input
    extent, vmtl_conv2d_fwd on the tap-flipped operand) in TF/s of algorithmic FLOPs."""
    from vision_mtl_amd import ops

    layers = [("stem", 3, 64, 7, 3, H, W)]
    h, w = H // 4, W // 4
    for cin, cout in ((64, 128), (128, 256), (256, 512)):
        layers += [(f"{cout}.conv1", cin, cout, 3, 1, h, w), (f"{cout}.downsample", cin, cout, 1, 0, h, w)]
        h, w = h // 2, w // 2
    out = []
    for name, cin, cout, K, pad, hh, ww in layers:
        Cs, ldy = ops.ceil4(cin), ops.ceil4(cout)
        wt = torch.randn(cout, cin, K, K, device=dev)
        Ho, Wo = (hh + 2 * pad - K) // 2 + 1, (ww + 2 * pad - K) // 2 + 1
        dy2 = torch.randn(B, Ho, Wo, ldy, device=dev)
        g2 = ops.ConvGeom.of((B, hh, ww, Cs), ldy, K, K, 2, pad)
        s2 = _events(lambda: ops._dgrad_s2(dy2, wt, g2, 0), steps, warmup)
        dy1 = torch.randn(B, hh, ww, ldy, device=dev)
        KK = K * K
        wd = ops.packs.get(wt, "dgrad", ops.Layout.dgrad(cout, cin, KK, ldy))
        dx = torch.empty(B, hh, ww, Cs, device=dev)
        g1 = ops.ConvGeom.of((B, hh, ww, Cs), ldy, K, K, 1, pad).dgrad()
        s1 = _events(lambda: ops._conv_launch(dy1, wd, None, dx, g1, Cout=cin, cin=cout), steps, warmup)
        f2, f1 = 2.0 * B * Ho * Wo * cout * KK * cin, 2.0 * B * hh * ww * cout * KK * cin
        out.append(dict(step="dgrad", layer=name, batch=B, in_hw=[hh, ww], K=K, cin=cin, cout=cout,
                        s2_ms=round(s2, 4), s2_tflops=round(f2 / s2 / 1e9, 2), s1_ms=round(s1, 4),
                        s1_tflops=round(f1 / s1 / 1e9, 2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder", default="resnet34", choices=["resnet18", "resnet34"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--only", choices=["train", "predict", "dgrad"])
    ap.add_argument("--batch", type=int, help="one batch size (default: 8 and 32)")
    ap.add_argument("--prec", choices=["fp32", "bf16"], help="one precision (default: both)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [a.batch] if a.batch else [8, 32]
    precs = [a.prec] if a.prec else ["fp32", "bf16"]
    for kind, fn in (("train", bench_train), ("predict", bench_predict)):
        if a.only in (None, kind):
            for B in batches:
                for p in precs:
                    print(json.dumps(fn(a.encoder, B, a.height, a.width, p, a.steps, a.warmup, dev)), flush=True)
    if a.only in (None, "dgrad"):
        for r in bench_dgrad(batches[-1], a.height, a.width, a.steps, a.warmup, dev):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
