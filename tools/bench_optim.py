"""The optimizer step over flat buffers of the `basic` and `mtan` arenas' sizes, GPU box only: the parent's fused Adam
(vmtl_adam_step), the extended update of csrc/optim.hip with and without global-norm clipping, the in-place clip
followed by the parent's update, and torch's own clip_grad_norm_ + Adam(fused=True) over the parameter views.

The yardstick is vmtl_adam_step on the same buffers IN THIS RUN.  Each variant's step (all of its launches) is timed with
HIP events over a warmed-up window of `reps` steps; the variants alternate window by window, `rounds` windows each;
reported are the median and the spread (min, max) over the windows and the GB/s of the bytes a step has to move
(update: p, g, m, v read and p, m, v written = 28n; norm: +4n; in-place clip: +4n for the norm and +8n for the scale
pass).  Every step works on the next of several buffer sets so that the window's working set exceeds the 256 MiB
Infinity Cache, as it does in training, where a forward and a backward pass run between two optimizer steps.
The in-place clip runs with grad_scale 2 and a bound of half the doubled gradient's norm: every call then clips by
0.5 (to within 1e-6 / norm) and leaves the gradient as it found it, so each window times the scale pass and not its no-op shortcut.
Prints ONE JSON line.

    python tools/bench_optim.py [--reps 100] [--rounds 9] [--out profiles/optim_clip/bench_optim.json]
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


def _shapes(name):
    from vision_mtl_amd.utils.pipeline_utils import build_model

    model = build_model(argparse.Namespace(model_name=name, backbone_weights=None), argparse.Namespace(num_classes=19))
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


def _window(fn, nsets, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % nsets)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per step


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
    return {"us_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
            "bytes": nbytes, "GBps_median": round(nbytes / med / 1e3, 1), "launches": launches}


def bench_model(dev, name, reps, rounds):
    from vision_mtl_amd import ops

    shapes = _shapes(name)
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    nsets = max(2, -(-2 * CACHE_BYTES // (16 * n)))
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(nsets):
        p = torch.randn(n, device=dev, generator=g) * 0.1
        gr = torch.randn(n, device=dev, generator=g) * 0.01
        sets.append({"p": p, "g": gr, "m": torch.zeros_like(p), "v": torch.zeros_like(p),
                     "step": torch.ones(1, device=dev), "ws": ops.optim_workspace(n, p),
                     "ctl": ops.optim_control_block(p)})
    norm0 = float(sets[0]["g"].double().norm())
    clip = 0.5 * norm0
    # torch's own path over per-parameter views of the same flat buffers
    for s in sets:
        views, off = [], 0
        for shp in shapes:
            k = int(torch.Size(shp).numel())
            t = s["p"][off:off + k].view(shp).requires_grad_(True)
            t.grad = s["g"][off:off + k].view(shp)
            views.append(t)
            off += k
        s["views"] = views
        s["topt"] = torch.optim.Adam(views, lr=LR, fused=True)

    def parent(i):
        s = sets[i]
        ops.adam_step(s["p"], s["g"], s["m"], s["v"], s["step"], LR)

    def update_ex(i):
        s = sets[i]
        ops.adam_step_ex(s["p"], s["g"], s["m"], s["v"], s["step"], LR, workspace=s["ws"], ctl=s["ctl"])

    def norm_clip_update(i):
        s = sets[i]
        ops.adam_step_ex(s["p"], s["g"], s["m"], s["v"], s["step"], LR, max_grad_norm=clip, workspace=s["ws"],
                         ctl=s["ctl"])

    def clip_then_parent(i):
        s = sets[i]
        ops.scale_by_clip(s["g"], norm0, 2.0, s["ws"], s["ctl"])
        ops.adam_step(s["p"], s["g"], s["m"], s["v"], s["step"], LR)

    def torch_clip_fused_adam(i):
        s = sets[i]
        torch.nn.utils.clip_grad_norm_(s["views"], clip)
        s["topt"].step()

    def norm_only(i):
        s = sets[i]
        ops.grad_sumsq(s["g"], s["ws"])

    fns = {"parent_adam_step": parent, "update_ex": update_ex, "norm_clip_update_ex": norm_clip_update,
           "clip_inplace_then_parent": clip_then_parent, "norm_pass_only": norm_only}
    us = _ab(fns, nsets, reps, rounds)
    # torch's path last and on its own: clip_grad_norm_ shrinks the gradient for good (the variants above leave it alone)
    us.update(_ab({"torch_clip_fused_adam": torch_clip_fused_adam}, nsets, max(reps // 5, 5), rounds))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(s["p"]).all()) for s in sets)
    nb = {"parent_adam_step": (28 * n, 1), "update_ex": (28 * n, 2), "norm_clip_update_ex": (32 * n, 3),
          "clip_inplace_then_parent": (40 * n, 3), "norm_pass_only": (4 * n, 1),
          "torch_clip_fused_adam": (40 * n, None)}
    return {"model": name, "floats": n, "parameters": len(shapes), "buffer_sets": nsets,
            "steps": {k: _summary(v, *nb[k]) for k, v in us.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--models", default="basic,mtan")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
           "copy_rate_GBps": 6290, "models": [bench_model(dev, m, args.reps, args.rounds) for m in args.models.split(",")]}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
