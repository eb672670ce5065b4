"""Eager vs replayed forward-only steps (vision_mtl_amd.graphed.GraphedEval): the validation step (train mode, no_grad) and
the predict step (eval mode), ms per step on one GPU, plus the launches of the captured predict step with and without
the batched eval-mode BatchNorm statistics (ops.eval_bn_table).

    python tools/bench_eval.py [--steps 30] [--warmup 5] [--only basic]

Batches are synthetic and already on the device in both paths (the replay adds one device-to-device copy into its
static buffers).  One JSON line per configuration, then a markdown table."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

CONFIGS = [("basic", 128, 256, 8), ("basic", 128, 256, 32), ("csnet", 256, 256, 16), ("mtan", 256, 256, 16)]
C = 19


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _launches(module, example, bn_table):
    """GraphedEval(stage="predict") built while every ops._k launch issued under capture is counted."""
    from vision_mtl_amd import ops
    from vision_mtl_amd.graphed import GraphedEval

    names, orig = [], ops._k

    def rec(name, *a, **kw):
        if torch.cuda.is_current_stream_capturing():
            names.append(name)
        return orig(name, *a, **kw)

    ops._k = rec
    try:
        g = GraphedEval(module, example, stage="predict", bn_table=bn_table)
    finally:
        ops._k = orig
    return g, len(names)


def run(name, H, W, bs, steps, warmup):
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedEval
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import build_model

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ns = argparse.Namespace(model_name=name, backbone_weights=None, channel_wise_stitching=True)
    module = MTLModule(build_model(ns, argparse.Namespace(num_classes=C)).to(dev), num_classes=C, device=str(dev))
    batch = {k: v.to(dev) for k, v in synthetic_batch(bs, H, W, C, seed=1, masked=0.1).items()}
    pbatch = {"img": batch["img"]}
    res = {"model": name, "H": H, "W": W, "bs": bs}
    with torch.no_grad():
        module.train()
        res["val_eager_ms"] = _time(lambda: module.validation_step(dict(batch)), steps, warmup)
        gval = GraphedEval(module, batch, stage="val")
        res["val_replay_ms"] = _time(lambda: gval(batch), steps, warmup)
        module.eval()
        res["predict_eager_ms"] = _time(lambda: module.predict_step(dict(pbatch)), steps, warmup)
        gp, res["predict_launches"] = _launches(module, pbatch, True)
        gp0, res["predict_launches_no_table"] = _launches(module, pbatch, False)
        res["predict_replay_ms"] = _time(lambda: gp(pbatch), steps, warmup)
        res["predict_replay_no_table_ms"] = _time(lambda: gp0(pbatch), steps, warmup)
    for k, v in res.items():
        if k.endswith("_ms"):
            res[k] = round(v, 3)
    for so in module.step_outputs.values():
        for v in so.values():
            v.clear()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="run the configurations of this model only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs an MI355X")
    rows = []
    for name, H, W, bs in CONFIGS:
        if args.only and name != args.only:
            continue
        r = run(name, H, W, bs, args.steps, args.warmup)
        print(json.dumps(r), flush=True)
        rows.append(r)
        torch.cuda.empty_cache()
    print(f"\n{torch.cuda.get_device_name(0)}, {args.steps} timed steps after {args.warmup} warm-up, ms/step\n")
    print("| config | val eager | val replayed | predict eager | predict replayed | predict replayed, no table "
          "| predict launches (table / no table) |")
    print("|---|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['model']} {r['H']}x{r['W']} bs {r['bs']} | {r['val_eager_ms']:.2f} | {r['val_replay_ms']:.2f} | "
              f"{r['predict_eager_ms']:.2f} | {r['predict_replay_ms']:.2f} | {r['predict_replay_no_table_ms']:.2f} | "
              f"{r['predict_launches']} / {r['predict_launches_no_table']} |")


if __name__ == "__main__":
    main()
