"""Training-step time of the captured step (vision_mtl_amd.graphed.GraphedStep) in the three convolution precisions:
fp32, bf16 and bf16_pw (bf16 plus the pointwise GEMMs; GPU box only: there is no CPU fallback).  All modes are captured on
the same model, then timed in alternating blocks; each configuration reports ms/step and img/s per mode, the speed-up of
bf16 and bf16_pw over fp32, and the loss of the last replay of each against the fp32 one.  Prints ONE JSON line.

    python tools/bench_precision.py [--steps 20] [--rounds 3] [--only basic_bs32]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [("basic_bs32", "basic", 32, 128, 256, 19), ("basic_bs8", "basic", 8, 128, 256, 19),
           ("csnet_bs32", "csnet", 32, 128, 256, 19), ("mtan_bs16", "mtan", 16, 256, 256, 14)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="replays per timed block")
    ap.add_argument("--rounds", type=int, default=3, help="alternating (fp32, bf16, bf16_pw) blocks; the median is reported")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_precision.py needs an MI355X (the hot path has no CPU fallback)")
    from vision_mtl_amd import conv_precision, dp
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import build_model

    dev = torch.device("cuda:0")
    PRECS = ("fp32", "bf16", "bf16_pw")
    out = {}
    for tag, name, bs, H, W, C in CONFIGS:
        if args.only and args.only not in tag:
            continue
        torch.manual_seed(11)
        model = build_model(argparse.Namespace(model_name=name, backbone_weights=None, channel_wise_stitching=False),
                            argparse.Namespace(num_classes=C)).to(dev).train()
        module = MTLModule(model, num_classes=C, device=str(dev))
        module.compute_metrics = False
        batch = {k: v.to(dev) for k, v in synthetic_batch(bs, H, W, C, seed=11).items()}
        arena = dp.FlatArena(model)
        module.dp_arena = None
        steps = {}
        for prec in PRECS:
            with conv_precision(prec):
                steps[prec] = GraphedStep(module, batch, arena=arena, warmup=1)
        times = {prec: [] for prec in PRECS}
        losses = {}
        for _ in range(args.rounds):
            for prec in PRECS:
                g = steps[prec].graph
                g.replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    g.replay()
                e1.record()
                e1.synchronize()
                times[prec].append(e0.elapsed_time(e1) / args.steps)
                losses[prec] = float(steps[prec]._loss)
        res = {}
        for prec in PRECS:
            ms = statistics.median(times[prec])
            res[prec] = {"ms_per_step": round(ms, 3), "img_per_s": round(bs / ms * 1e3, 1), "final_loss": losses[prec]}
        for prec in PRECS[1:]:
            res[prec + "_speedup"] = round(res["fp32"]["ms_per_step"] / res[prec]["ms_per_step"], 3)
            res[prec + "_loss_rel_diff"] = abs(losses[prec] - losses["fp32"]) / abs(losses["fp32"])
        out[tag] = res
        print(f"{tag}: {res}", file=sys.stderr, flush=True)
        del steps, module, model, arena
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    print(json.dumps({"bench_precision": out}))


if __name__ == "__main__":
    main()
