"""NYUv2 sample transform: the host chain against the device transform (data.DeviceTransform, csrc/resize.hip).

Prints one JSON line per measurement:
  host    - the reference's per-sample chain (ToTensor + Resize((256, 256), antialias=True) on image, mask and uint16
            depth, then data.prepare_sample) in ms per 480x640 sample, on 1 and 16 threads (PNG decode not included);
  device  - the transform of one bs-32 raw batch already on the GPU: HIP events around `--iters` launches, warm, median
            of `--repeats`, with the bytes it moves per second;
  step    - GraphedStep for `basic` at 256x256, bs 32, in ms/step: fed raw pinned batches with the device transform in
            the graph, against fed pre-resized pinned batches; the two run interleaved in one process.

    python tools/bench_device_resize.py [--out profiles/device_resize/bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HI, WI, HO, WO, B = 480, 640, 256, 256, 32


def raw_sample(g):
    return {"img": g.integers(0, 256, (HI, WI, 3), dtype=np.uint8), "mask": g.integers(0, 14, (HI, WI), dtype=np.uint8),
            "depth": g.integers(0, 65536, (HI, WI)).astype(np.uint16)}


def host_chain(s):
    from vision_mtl_amd.data import prepare_sample

    rs = lambda x: F.interpolate(x[None], size=(HO, WO), mode="bilinear", align_corners=False, antialias=True)[0]
    img = rs(torch.from_numpy(s["img"]).permute(2, 0, 1).float().div(255)).permute(1, 2, 0)
    mask = rs(torch.from_numpy(s["mask"])[None].float().div(255))[0]
    d = torch.from_numpy(s["depth"])
    depth = rs(d[None].float())[0].round().to(d.dtype)
    return prepare_sample({"img": img, "mask": mask, "depth": depth}, 14, max_depth=10.0, dataset="nyuv2")


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-samples", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    g = np.random.default_rng(0)
    samples = [raw_sample(g) for _ in range(B)]

    for threads in (1, 16):
        torch.set_num_threads(threads)
        host_chain(samples[0])
        t0 = time.perf_counter()
        for i in range(a.host_samples):
            host_chain(samples[i % B])
        ms = (time.perf_counter() - t0) * 1e3 / a.host_samples
        emit({"what": "host", "threads": threads, "ms_per_sample": round(ms, 3),
              "samples_per_s": round(1e3 / ms, 1)}, a.out)
    torch.set_num_threads(16)

    from vision_mtl_amd.data import DeviceTransform, collate, collate_raw

    dev = torch.device("cuda:0")
    raw = collate_raw(samples)
    raw_dev = {k: v.to(dev) for k, v in raw.items()}
    tf = DeviceTransform((HO, WO), 10.0)
    for _ in range(3):
        tf(raw_dev)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            tf(raw_dev)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    us = statistics.median(times)
    nbytes = B * HI * WI * (3 + 1 + 2) + B * HO * WO * (16 + 8 + 4)
    emit({"what": "device", "batch": B, "in": [HI, WI], "out": [HO, WO], "us_per_batch": round(us, 2),
          "us_all_repeats": [round(t, 2) for t in times], "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)},
         a.out)

    import argparse as _ap

    from vision_mtl_amd import dp
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import build_model

    torch.manual_seed(0)
    pre = collate([host_chain(s) for s in samples])

    # ONE model, module and FlatArena behind both captured steps: a captured step replays the packed-operand table of
    # the model it was captured on, and building a second model (or arena) would rebuild that table under the first
    model = build_model(_ap.Namespace(model_name="basic", backbone_weights=None), _ap.Namespace(num_classes=14))
    module = MTLModule(model.to(dev).train(), num_classes=14, device=str(dev))
    module.compute_metrics = False
    arena = dp.FlatArena(model)
    module.device_transform = tf
    g_raw = GraphedStep(module, raw, arena=arena)  # records the transform
    module.device_transform = None
    g_pre = GraphedStep(module, pre, arena=arena)
    steps = {"raw_device_transform": (g_raw, raw), "pre_resized": (g_pre, pre)}
    res = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, (gs, batch) in steps.items():
            gs(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                gs(batch)
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    emit({"what": "step", "model": "basic", "batch": B, "size": [HO, WO], "steps": a.steps,
          "ms_per_step": {k: round(statistics.median(v), 3) for k, v in res.items()},
          "ms_all_rounds": {k: [round(x, 3) for x in v] for k, v in res.items()},
          "note": "each step includes the pinned host->device copy of its batch (raw 480x640 vs pre-resized 256x256)"},
         a.out)


if __name__ == "__main__":
    main()
