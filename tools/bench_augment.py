"""Device-side joint training augmentation (data.DeviceAugment, csrc/augment.hip) on one MI355X.

Prints one JSON line per measurement:
  kernels - draw + apply on one bs-32 batch already on the GPU, at 128x256 and 256x256, from the model's NHWC storage
            (ld 4) and from dataset sample layout (ld 3): HIP events around `--iters` calls replayed from one captured
            graph (and, for comparison, issued eagerly from Python), warm, median of `--repeats`, against the bytes the
            gather must move (every input and output pixel once: an upper bound on the reads, a crop at scale s touches
            1/s^2 of the input);
  step    - GraphedStep for `basic` at 128x256, bs 32, in ms/step, with the augmentation in the graph and without;
            the two captured steps share one model and arena and run interleaved in one process.

    python tools/bench_augment.py [--out profiles/augment/bench_augment.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, C = 32, 19


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)

    from vision_mtl_amd import dp, ops
    from vision_mtl_amd.data import DeviceAugment, collate, synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import build_model

    dev = torch.device("cuda:0")
    for H, W in ((128, 256), (256, 256)):
        host = synthetic_batch(B, H, W, C, seed=11, masked=0.1)
        hwc = host["img"].permute(0, 2, 3, 1).contiguous().to(dev)
        rest = {"mask": host["mask"].to(dev), "depth": host["depth"].to(dev)}
        for ld, img in ((4, ops.hwc_to_model_input(hwc)), (3, hwc)):
            aug = DeviceAugment(seed=11)
            batch = dict(rest, img=img)
            for _ in range(3):
                aug(batch)
            torch.cuda.synchronize()
            # the device time of the two launches: `iters` calls captured into one graph (no host gaps), replayed
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(a.iters):
                    aug(batch)
            graph.replay()
            torch.cuda.synchronize()
            times, eager = [], []
            for _ in range(a.repeats):
                for into, run in ((times, graph.replay), (eager, lambda: [aug(batch) for _ in range(a.iters)])):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    e1.synchronize()
                    into.append(e0.elapsed_time(e1) * 1e3 / a.iters)
            us = statistics.median(times)
            nbytes = B * H * W * (4 * ld + 8 + 4) + B * H * W * (16 + 8 + 4)
            emit({"what": "kernels", "batch": B, "size": [H, W], "ld": ld, "us_per_batch": round(us, 2),
                  "us_all_repeats": [round(t, 2) for t in times], "bytes": nbytes,
                  "GB_per_s": round(nbytes / us / 1e3, 1),
                  "us_per_batch_eager": round(statistics.median(eager), 2),
                  "note": "draw + apply; us_per_batch: replayed from a graph of `iters` calls (device time), "
                          "us_per_batch_eager: issued from Python, launch gaps included"}, a.out)

    import argparse as _ap

    H, W = 128, 256
    torch.manual_seed(0)
    samples = synthetic_batch(B, H, W, C, seed=11, masked=0.1)
    pinned = collate([{"img": samples["img"][i].permute(1, 2, 0).contiguous(), "mask": samples["mask"][i],
                       "depth": samples["depth"][i]} for i in range(B)])
    # ONE model, module and FlatArena behind both captured steps (see tools/bench_device_resize.py)
    model = build_model(_ap.Namespace(model_name="basic", backbone_weights=None), _ap.Namespace(num_classes=C))
    module = MTLModule(model.to(dev).train(), num_classes=C, device=str(dev))
    module.compute_metrics = False
    arena = dp.FlatArena(model)
    module.train_augment = DeviceAugment(seed=11)
    g_aug = GraphedStep(module, pinned, arena=arena)  # records the augmentation
    module.train_augment = None
    g_plain = GraphedStep(module, pinned, arena=arena)
    steps = {"augmented": g_aug, "plain": g_plain}
    res = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, gs in steps.items():
            gs(pinned)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                gs(pinned)
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    emit({"what": "step", "model": "basic", "batch": B, "size": [H, W], "steps": a.steps,
          "ms_per_step": {k: round(statistics.median(v), 3) for k, v in res.items()},
          "ms_all_rounds": {k: [round(x, 3) for x in v] for k, v in res.items()},
          "note": "each step includes the pinned host->device copy of its sample-layout batch"}, a.out)


if __name__ == "__main__":
    main()
