"""The depth loss with multi-scale gradient matching (vmtl_depth_grad_fwd + vmtl_depth_grad_bwd, csrc/depth_grad.hip)
against the SILog pair it extends (vmtl_silog_fwd + vmtl_silog_bwd) on the same inputs, in the same process, GPU box only.

Shapes: 32x128x256 (Cityscapes at the benchmark's batch) and 16x256x256 (NYUv2); ~10 % invalid depth (target 0);
grad_weight 0.5, `--scales` scales (default 4).  Each call is timed with HIP events over a warmed-up window of `reps`
calls; the variants alternate window by window, `rounds` windows each; reported are the median and the spread (min, max)
in microseconds, and the bytes per pixel that the median implies were the call one streaming pass at a copy kernel's rate
(us * 1e-6 * HBM_BYTES_PER_S / pixels) next to the bytes per pixel the call has to move.  Every call works on the next of
several tensor sets so that the window's working set exceeds the 256 MiB Infinity Cache.

--step adds milliseconds per replayed training step of graphed.GraphedStep (`basic`, 32x128x256, C = 19, metrics on)
without and with the term, one model alive at a time, the plain step measured first and again last.  Prints ONE JSON line.

    python tools/bench_depth_grad.py [--reps 30] [--rounds 7] [--scales 4] [--step] [--out profiles/depth_grad/bench_depth_grad.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(32, 128, 256), (16, 256, 256)]
CACHE_BYTES = 256 << 20
HBM_BYTES_PER_S = 6.3e12  # about what a plain copy kernel sustains on the MI355X (datasheet peak: 8.0e12)
GRAD_WEIGHT = 0.5
MIN_DEPTH = 1e-3
# bytes per pixel a call has to move: SILog reads pred + target (8) forward and again backward, writes dpred (4);
# the new node also writes resid (4) in the residual pass, reads resid + target in the stencil pass (8) and reads pred,
# target, resid and writes dpred backward (16); neighbour re-reads are expected to hit in L2
NEED = {"silog": {"fwd": 8, "bwd": 12}, "depth_grad": {"fwd": 20, "bwd": 16}}


def _window(fn, nsets, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % nsets)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def _ab(fns, nsets, reps, rounds):
    """{name: us per call of every window}; the variants alternate window by window"""
    for fn in fns.values():
        for i in range(max(nsets, 3)):
            fn(i % nsets)
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(_window(fn, nsets, reps))
    return out


def _summary(us, pixels=None, need=None, digits=2):
    med = statistics.median(us)
    out = {"median": round(med, digits), "min": round(min(us), digits), "max": round(max(us), digits)}
    if pixels:
        out["implied_bytes_per_pixel"] = round(med * 1e-6 * HBM_BYTES_PER_S / pixels, 1)
        out["needed_bytes_per_pixel"] = need
    return out


def bench_shape(dev, B, H, W, scales, reps, rounds):
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib

    P = B * H * W
    nsets = max(2, -(-2 * CACHE_BYTES // (16 * P)))  # pred, target, resid, dpred per set
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(nsets):
        t = 0.05 + 0.6 * torch.rand(B, H, W, device=dev, generator=g)
        p = (t * torch.exp(0.25 * torch.randn(B, H, W, device=dev, generator=g))).clamp(0.01, 0.99)
        t[torch.rand(B, H, W, device=dev, generator=g) < 0.1] = 0.0
        sets.append((p, t, torch.empty(B, H, W, device=dev), torch.empty(B, H, W, device=dev)))
    loss, terms, gout = torch.empty((), device=dev), torch.empty(2, device=dev), torch.ones((), device=dev)
    stats_s, stats_d = torch.empty(3, device=dev), torch.empty(3, device=dev)
    counts = torch.empty(scales, dtype=torch.int64, device=dev)
    ws_s = torch.empty(lib().raw("vmtl_silog_workspace_bytes")(P) // 8, dtype=torch.float64, device=dev)
    ws_d = torch.empty(lib().raw("vmtl_depth_grad_workspace_bytes")(B, H, W, scales) // 8, dtype=torch.float64, device=dev)
    geom = dict(B=B, H=H, W=W, scales=scales, silog_weight=1.0, grad_weight=GRAD_WEIGHT)

    def fwd_s(i):
        p, t, _, _ = sets[i]
        ops._k("vmtl_silog_fwd", pred=p, target=t, min_depth=MIN_DEPTH, loss=loss, stats=stats_s, workspace=ws_s, P=P)

    def bwd_s(i):
        p, t, _, d = sets[i]
        ops._k("vmtl_silog_bwd", pred=p, target=t, stats=stats_s, grad_out=gout, min_depth=MIN_DEPTH, dpred=d, P=P)

    def fwd_d(i):
        p, t, r, _ = sets[i]
        ops._k("vmtl_depth_grad_fwd", pred=p, target=t, mask=None, min_depth=MIN_DEPTH, loss=loss, terms=terms,
               stats=stats_d, counts=counts, resid=r, workspace=ws_d, **geom)

    def bwd_d(i):
        p, t, r, d = sets[i]
        ops._k("vmtl_depth_grad_bwd", pred=p, target=t, mask=None, min_depth=MIN_DEPTH, resid=r, stats=stats_d,
               counts=counts, grad_out=gout, dpred=d, **geom)

    def pair_s(i):
        fwd_s(i)
        bwd_s(i)

    def pair_d(i):
        fwd_d(i)
        bwd_d(i)

    for i in range(nsets):  # every set's resid belongs to its own pred / target before a backward window reads it
        fwd_d(i)
    fwd_s(0)
    f = _ab({"silog": fwd_s, "depth_grad": fwd_d}, nsets, reps, rounds)
    b = _ab({"silog": bwd_s, "depth_grad": bwd_d}, nsets, reps, rounds)
    pr = _ab({"silog": pair_s, "depth_grad": pair_d}, nsets, reps, rounds)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(sets[0][3]).all())
    need = lambda k, what: NEED[k][what] if what != "pair" else NEED[k]["fwd"] + NEED[k]["bwd"]
    return {"shape": [B, H, W], "scales": scales, "tensor_sets": nsets, "unit": "us per call", "counts": counts.tolist(),
            "fwd": {k: _summary(v, P, need(k, "fwd")) for k, v in f.items()},
            "bwd": {k: _summary(v, P, need(k, "bwd")) for k, v in b.items()},
            "fwd_plus_bwd": {k: _summary(v, P, need(k, "pair")) for k, v in pr.items()},
            "note": "silog forward = sweep + finalize; depth_grad forward = residual sweep + stencil + finalize"}


def bench_step(dev, args):
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.utils.pipeline_utils import fetch_data_cfg, init_model

    C = fetch_data_cfg("cityscapes").num_classes
    B, H, W = 32, 128, 256
    batch = {k: v.to(dev) for k, v in synthetic_batch(B, H, W, C, seed=11, masked=0.1).items()}
    ms = {}
    # one model alive at a time (a captured step re-packs the GEMM operands of every live model); the plain step runs
    # first and again last: the difference between its two results is what the order of construction alone is worth
    for tag, weight in (("silog", None), ("silog_grad", GRAD_WEIGHT), ("silog_again", None)):
        torch.manual_seed(11)
        ns = argparse.Namespace(model_name="basic", backbone_weights=None, depth_grad_weight=weight,
                                depth_grad_scales=args.scales)
        module = init_model(ns, argparse.Namespace(num_classes=C)).to(dev).train()
        gstep = GraphedStep(module, batch)
        ms[tag] = _ab({tag: lambda i: gstep(batch)}, 1, args.step_reps, args.rounds)[tag]
        gstep.arena.close()
        del gstep, module
        gc.collect()
        torch.cuda.empty_cache()
    return {"unit": "ms per replayed step", "model": "basic", "shape": [B, H, W], "grad_weight": GRAD_WEIGHT,
            "scales": args.scales, "steps": {k: _summary([x / 1e3 for x in v], digits=4) for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scales", type=int, default=4)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_grad.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
           "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S,
           "kernels": [bench_shape(dev, *s, args.scales, args.reps, args.rounds) for s in SHAPES]}
    if args.step:
        res["step"] = bench_step(dev, args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
