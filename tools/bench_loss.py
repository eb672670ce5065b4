"""The weighted / ignoring cross entropy (vmtl_ce_fwd_ex with argmax, vmtl_ce_bwd_ex into NHWC rows) against the
unweighted entry points (vmtl_ce_fwd_argmax, vmtl_ce_bwd_strided) in the same process, GPU box only.

Shapes: 32x19x128x256 (Cityscapes at the benchmark's batch) and 16x14x256x256 (NYUv2); targets with ~30 % void pixels
(label 255) for the new kernels, none for the old ones (they have no way to skip them).  The new kernels move the bytes
the old ones move plus a C-float table, so the yardstick is the old kernels' time IN THIS RUN.  Each launch is timed with
HIP events over a warmed-up window of `reps` launches; the two variants alternate, `rounds` windows each; reported are
the median and the spread (min, max) over the windows, and the GB/s of the bytes a launch has to move (forward: logits +
targets read, argmax written; backward: logits + targets read, ceil4(C+1)-wide rows written).  Every launch works on the
next of several tensor sets so that the window's working set exceeds the 256 MiB Infinity Cache.  Prints ONE JSON line.

    python tools/bench_loss.py [--reps 50] [--rounds 7] [--out profiles/loss_ignore/bench_loss.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(32, 19, 128, 256), (16, 14, 256, 256)]
CACHE_BYTES = 256 << 20
IGN = 255


def _window(fn, nsets, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % nsets)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per launch


def _ab(fns, nsets, reps, rounds):
    """{name: us per launch of every window}; the variants alternate window by window"""
    for fn in fns.values():
        for i in range(max(nsets, 3)):
            fn(i % nsets)
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(_window(fn, nsets, reps))
    return out


def _summary(us, nbytes):
    med = statistics.median(us)
    return {"us_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
            "GBps_median": round(nbytes / med / 1e3, 1)}


def bench_shape(dev, B, C, H, W, reps, rounds):
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib

    HW, P = H * W, B * H * W
    ld = ops.ceil4(C + 1)
    fwd_bytes = P * (4 * C + 8 + 8)
    bwd_bytes = P * (4 * C + 8 + 4 * ops.ceil4(C))  # both shapes: ld == ceil4(C), the rows kernel
    nsets = max(2, -(-2 * CACHE_BYTES // bwd_bytes))
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(nsets):
        z = torch.randn(B, C, H, W, device=dev, generator=g) * 3
        t = torch.randint(0, C, (B, H, W), device=dev, generator=g)
        tv = t.clone()
        tv[torch.rand(B, H, W, device=dev, generator=g) < 0.3] = IGN
        sets.append((z, t, tv, torch.empty(B, H, W, dtype=torch.int64, device=dev), torch.empty(B, H, W, ld, device=dev)))
    w = 0.1 + 1.9 * torch.rand(C, device=dev, generator=g)
    loss, stats, gout = torch.empty((), device=dev), torch.empty(2, device=dev), torch.ones((), device=dev)
    ws = torch.empty(lib().raw("vmtl_ce_ex_workspace_bytes")(P) // 8, dtype=torch.float64, device=dev)
    geo = dict(B=B, HW=HW, C=C, sb=C * HW, sc=HW, sp=1)
    dgeo = dict(dsb=HW * ld, dsc=1, dsp=ld)

    def fwd_old(i):
        z, t, _, am, _ = sets[i]
        ops._k("vmtl_ce_fwd_argmax", logits=z, target=t, loss=loss, workspace=ws, argmax=am, **geo)

    def fwd_new(i):
        z, _, tv, am, _ = sets[i]
        ops._k("vmtl_ce_fwd_ex", logits=z, target=tv, weight=w, ignore_index=IGN, loss=loss, stats=stats, workspace=ws,
               argmax=am, **geo)

    def bwd_old(i):
        z, t, _, _, d = sets[i]
        ops._k("vmtl_ce_bwd_strided", logits=z, target=t, grad_out=gout, dlogits=d, **geo, **dgeo)

    def bwd_new(i):
        z, _, tv, _, d = sets[i]
        ops._k("vmtl_ce_bwd_ex", logits=z, target=tv, weight=w, ignore_index=IGN, stats=stats, grad_out=gout, dlogits=d,
               **geo, **dgeo)

    fwd_new(0)  # stats of a real forward for the backward windows (any set: only the scale of the gradient depends on it)
    f = _ab({"unweighted": fwd_old, "weighted_ignoring": fwd_new}, nsets, reps, rounds)
    b = _ab({"unweighted": bwd_old, "weighted_ignoring": bwd_new}, nsets, reps, rounds)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(sets[0][4][..., :C]).all())
    return {"shape": [B, C, H, W], "row_floats": ld, "tensor_sets": nsets,
            "fwd_argmax": {k: _summary(v, fwd_bytes) for k, v in f.items()},
            "bwd_nhwc_rows": {k: _summary(v, bwd_bytes) for k, v in b.items()},
            "note": "forward = main kernel + finalize launch (both variants)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
           "shapes": [bench_shape(dev, *s, args.reps, args.rounds) for s in SHAPES]}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
