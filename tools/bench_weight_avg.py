"""The averaged weights of csrc/weight_avg.hip over flat buffers of the `basic` and `mtan` arenas' sizes, GPU box only.

  update          vmtl_wavg_control + vmtl_wavg_update (12 bytes per element: p and e read, e written)
  step_ex         vmtl_optim_control + vmtl_adam_step_ex, the yardstick of this run (28 bytes per element)
  two_launch      step_ex, then update (40 bytes per element, 4 launches)
  fused           vmtl_optim_control + vmtl_wavg_control + vmtl_adam_step_wavg (36 bytes per element, 3 launches)
  torch_lerp      torch._foreach_lerp_ over per-parameter views of the same buffers (what get_ema_multi_avg_fn runs)
  torch_averaged  torch.optim.swa_utils.AveragedModel.update_parameters (EMA) over a module holding those views
  swap            vmtl_swap_ (16 bytes per element)
  three_copies    the exchange through a third buffer with three copy_ (24 bytes per element)

Each variant's calls are timed with HIP events over a warmed-up window of `reps` calls; the variants alternate window by
window, `rounds` windows each; reported are the median and the spread (min, max) over the windows and the GB/s of the
bytes a call has to move.  Every call works on the next of several buffer sets, enough of them that even the variants
that touch p and e alone walk over twice the 256 MiB Infinity Cache per round, as in training, where a forward and a
backward pass run between two optimizer steps.  `fused_gain_us` is two_launch - fused (medians) and `spread_us` the
larger of the two variants' (max - min): the fused entry point earns its place only when the gain exceeds the spread.

--step: a captured GraphedEval replay (validation step, eval mode, batch 8 at 128x256, 19 classes) with and without
module.weight_average, i.e. the cost of the two exchanges around the replay.
Prints ONE JSON line.

    python tools/bench_weight_avg.py [--reps 100] [--rounds 9] [--step] [--out profiles/weight_avg/bench_weight_avg.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CACHE_BYTES = 256 << 20
LR = 5e-4
DECAY = 0.999


def _model(name):
    from vision_mtl_amd.utils.pipeline_utils import build_model

    return build_model(argparse.Namespace(model_name=name, backbone_weights=None, channel_wise_stitching=True),
                       argparse.Namespace(num_classes=19))


def _window(fn, nsets, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % nsets)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def _ab(fns, nsets, reps, rounds):
    for fn in fns.values():
        for i in range(max(nsets, 3)):
            fn(i % nsets)
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(_window(fn, nsets, reps))
    return out


def _summary(us, nbytes, launches):
    med = statistics.median(us)
    return {"us_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "bytes": nbytes,
            "GBps_median": round(nbytes / med / 1e3, 1), "launches": launches}


class _Views(torch.nn.Module):
    def __init__(self, views):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(v, requires_grad=False) for v in views])


def bench_model(dev, name, reps, rounds):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    from vision_mtl_amd import ops

    shapes = [tuple(p.shape) for p in _model(name).parameters() if p.requires_grad]
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    nsets = max(2, -(-2 * CACHE_BYTES // (8 * n)))  # sized by the smallest working set: update and swap touch p and e only
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(nsets):
        p = torch.randn(n, device=dev, generator=g) * 0.1
        s = {"p": p, "g": torch.randn(n, device=dev, generator=g) * 0.01, "m": torch.zeros_like(p),
             "v": torch.zeros_like(p), "e": p.clone(), "tmp": torch.empty_like(p), "step": torch.ones(1, device=dev),
             "ws": ops.optim_workspace(n, p), "ctl": ops.optim_control_block(p), "state": ops.wavg_state(p)}
        views, eviews, off = [], [], 0
        for shp in shapes:
            k = int(torch.Size(shp).numel())
            views.append(s["p"][off:off + k].view(shp))
            eviews.append(s["e"][off:off + k].view(shp))
            off += k
        s["views"], s["eviews"] = views, eviews
        s["live"] = _Views(views)
        s["averaged"] = AveragedModel(s["live"], multi_avg_fn=get_ema_multi_avg_fn(DECAY))
        s["averaged"].update_parameters(s["live"])  # the first update copies: the timed ones average
        sets.append(s)

    def update(i):
        s = sets[i]
        ops.wavg_control(s["state"], "ema", DECAY)
        ops.wavg_update(s["e"], s["p"], s["state"])

    def step_ex(i):
        s = sets[i]
        ops.adam_step_ex(s["p"], s["g"], s["m"], s["v"], s["step"], LR, workspace=s["ws"], ctl=s["ctl"])

    def two_launch(i):
        s = sets[i]
        ops.adam_step_ex(s["p"], s["g"], s["m"], s["v"], s["step"], LR, workspace=s["ws"], ctl=s["ctl"])
        ops.wavg_control(s["state"], "ema", DECAY, ctl=s["ctl"])
        ops.wavg_update(s["e"], s["p"], s["state"])

    def fused(i):
        s = sets[i]
        ops.adam_step_wavg(s["p"], s["g"], s["m"], s["v"], s["e"], s["state"], s["step"], LR, mode="ema", decay=DECAY,
                           workspace=s["ws"], ctl=s["ctl"])

    def torch_lerp(i):
        s = sets[i]
        torch._foreach_lerp_(s["eviews"], s["views"], 1.0 - DECAY)

    def torch_averaged(i):
        s = sets[i]
        s["averaged"].update_parameters(s["live"])

    def swap(i):
        s = sets[i]
        ops.swap_(s["p"], s["e"])

    def three_copies(i):
        s = sets[i]
        s["tmp"].copy_(s["p"])
        s["p"].copy_(s["e"])
        s["e"].copy_(s["tmp"])

    fns = {"update": update, "step_ex": step_ex, "two_launch": two_launch, "fused": fused, "swap": swap,
           "three_copies": three_copies, "torch_lerp": torch_lerp}
    us = _ab(fns, nsets, reps, rounds)
    # host-bound (hundreds of small tensors, a host-side counter): fewer calls per window
    us.update(_ab({"torch_averaged": torch_averaged}, nsets, max(reps // 5, 5), rounds))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(s["p"]).all()) and bool(torch.isfinite(s["e"]).all()) for s in sets)
    nb = {"update": (12 * n, 2), "step_ex": (28 * n, 2), "two_launch": (40 * n, 4), "fused": (36 * n, 3),
          "swap": (16 * n, 1), "three_copies": (24 * n, 3), "torch_lerp": (12 * n, None), "torch_averaged": (12 * n, None)}
    res = {k: _summary(v, *nb[k]) for k, v in us.items()}
    gain = res["two_launch"]["us_median"] - res["fused"]["us_median"]
    spread = max(res[k]["us_max"] - res[k]["us_min"] for k in ("two_launch", "fused"))
    return {"model": name, "floats": n, "parameters": len(shapes), "buffer_sets": nsets, "calls": res,
            "fused_gain_us": round(gain, 2), "spread_us": round(spread, 2)}


def bench_step(dev, name, steps, rounds):
    """A captured validation replay with and without module.weight_average: ms per call, median over `rounds` windows."""
    import time

    from vision_mtl_amd import dp
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedEval
    from vision_mtl_amd.lit_module import MTLModule

    torch.manual_seed(0)
    model = _model(name).to(dev)
    module = MTLModule(model, num_classes=19, device=str(dev)).eval()
    arena = dp.FlatArena(model)
    batch = {k: v.to(dev) for k, v in synthetic_batch(8, 128, 256, 19, seed=1, masked=0.1).items()}
    out = {}
    with torch.no_grad():
        for key, use_buffers in (("replay", None), ("replay_averaged", False), ("replay_averaged_buffers", True)):
            module.weight_average = None if use_buffers is None else dp.ArenaAverage(arena, use_buffers=use_buffers)
            geval = GraphedEval(module, batch, stage="val")
            for _ in range(5):
                geval(batch)
            wins = []
            for _ in range(rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    geval(batch)
                torch.cuda.synchronize()
                wins.append((time.perf_counter() - t0) / steps * 1e3)
            out[key] = {"ms_median": round(statistics.median(wins), 4), "ms_min": round(min(wins), 4),
                        "ms_max": round(max(wins), 4)}
            for so in module.step_outputs.values():
                for v in so.values():
                    v.clear()
    module.weight_average = None
    return {"model": name, "floats": arena.numel, "batch": [8, 128, 256], "steps": steps, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--models", default="basic,mtan")
    ap.add_argument("--step", action="store_true", help="also time a captured GraphedEval replay with and without the average")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_avg.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
           "models": [bench_model(dev, m, args.reps, args.rounds) for m in args.models.split(",")]}
    if args.step:
        torch.cuda.empty_cache()
        res["replay"] = [bench_step(dev, m, 30, args.rounds) for m in args.models.split(",")]
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
