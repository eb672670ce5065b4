"""Online hard example mining in the cross entropy (vmtl_ce_ohem_fwd with argmax + vmtl_ce_ohem_bwd into NHWC rows,
csrc/ce_ohem.hip) against the weighted / ignoring pair it extends (vmtl_ce_fwd_ex with argmax + vmtl_ce_bwd_ex) on the
same inputs, in the same process, GPU box only.

Shapes: 32x19x128x256 (Cityscapes at the benchmark's batch) and 32x14x256x256 (NYUv2); ~30 % void pixels (label 255),
class weights on, min_kept = HW/16 pixels per image, thresh 0.7.  Two regimes:
  "tau"   near-uniform logits (randn * 0.1: every true-class probability is near 1/C < 0.7) - K or more pixels reach tau,
          the cut is tau and the two radix rounds return at once (early training);
  "kappa" confident logits (the true class raised by 12: every probability is above 0.7) - nothing reaches tau, the cut is
          the K-th largest nll and all three radix rounds run (late training).
Each call is timed with HIP events over a warmed-up window of `reps` calls; the variants alternate window by window,
`rounds` windows each; reported are the median and the spread (min, max) in microseconds.  Every call works on the next
of several tensor sets so that the window's working set exceeds the 256 MiB Infinity Cache.

--step adds milliseconds per replayed training step of graphed.GraphedStep (`basic`, 32x128x256, C = 19, ignore index and
class weights on, metrics on) without and with mining (thresh 0.7, min_kept = HW/16), one model alive at a time, the
un-mined step measured first and again last.  Prints ONE JSON line.

    python tools/bench_ohem.py [--reps 30] [--rounds 7] [--step] [--out profiles/ohem/bench_ohem.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(32, 19, 128, 256), (32, 14, 256, 256)]
CACHE_BYTES = 256 << 20
IGN = 255
THRESH = 0.7


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


def _summary(us, digits=2):
    return {"median": round(statistics.median(us), digits), "min": round(min(us), digits), "max": round(max(us), digits)}


def bench_shape(dev, B, C, H, W, regime, reps, rounds):
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib

    HW, P = H * W, B * H * W
    ld = ops.ceil4(C + 1)
    total = B * (HW // 16)
    tau = ops.ohem_tau(THRESH)
    nsets = max(2, -(-2 * CACHE_BYTES // (P * (4 * C + 8 + 4 * ld))))
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(nsets):
        t = torch.randint(0, C, (B, H, W), device=dev, generator=g)
        if regime == "tau":
            z = torch.randn(B, C, H, W, device=dev, generator=g) * 0.1
        else:
            z = torch.randn(B, C, H, W, device=dev, generator=g)
            z.scatter_add_(1, t.unsqueeze(1), torch.full((B, 1, H, W), 12.0, device=dev))
        t[torch.rand(B, H, W, device=dev, generator=g) < 0.3] = IGN
        sets.append((z, t, torch.empty(B, H, W, dtype=torch.int64, device=dev), torch.empty(B, H, W, ld, device=dev),
                     torch.empty(B, H, W, device=dev)))
    w = 0.1 + 1.9 * torch.rand(C, device=dev, generator=g)
    loss, gout = torch.empty((), device=dev), torch.ones((), device=dev)
    stats2, stats4 = torch.empty(2, device=dev), torch.empty(4, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    ws_ex = torch.empty(lib().raw("vmtl_ce_ex_workspace_bytes")(P) // 8, dtype=torch.float64, device=dev)
    ws_oh = torch.empty(lib().raw("vmtl_ce_ohem_workspace_bytes")(P) // 8, dtype=torch.float64, device=dev)
    geo = dict(B=B, HW=HW, C=C, sb=C * HW, sc=HW, sp=1)
    dgeo = dict(dsb=HW * ld, dsc=1, dsp=ld)

    def fwd_ex(i):
        z, t, am, _, _ = sets[i]
        ops._k("vmtl_ce_fwd_ex", logits=z, target=t, weight=w, ignore_index=IGN, loss=loss, stats=stats2, workspace=ws_ex,
               argmax=am, **geo)

    def bwd_ex(i):
        z, t, _, d, _ = sets[i]
        ops._k("vmtl_ce_bwd_ex", logits=z, target=t, weight=w, ignore_index=IGN, stats=stats2, grad_out=gout, dlogits=d,
               **geo, **dgeo)

    def fwd_oh(i):
        z, t, am, _, nll = sets[i]
        ops._k("vmtl_ce_ohem_fwd", logits=z, target=t, weight=w, ignore_index=IGN, nll_thresh=tau, min_kept_total=total,
               loss=loss, stats=stats4, counts=counts, nll=nll, workspace=ws_oh, argmax=am, **geo)

    def bwd_oh(i):
        z, t, _, d, nll = sets[i]
        ops._k("vmtl_ce_ohem_bwd", logits=z, target=t, weight=w, ignore_index=IGN, stats=stats4, nll=nll, grad_out=gout,
               dlogits=d, **geo, **dgeo)

    def pair_ex(i):
        fwd_ex(i)
        bwd_ex(i)

    def pair_oh(i):
        fwd_oh(i)
        bwd_oh(i)

    pair_oh(0)
    torch.cuda.synchronize()
    cut, (V, kept) = float(stats4[2]), counts.tolist()
    assert (cut == float(torch.tensor(tau, dtype=torch.float32))) == (regime == "tau"), (regime, cut)
    f = _ab({"ce_ex": fwd_ex, "ce_ohem": fwd_oh}, nsets, reps, rounds)
    b = _ab({"ce_ex": bwd_ex, "ce_ohem": bwd_oh}, nsets, reps, rounds)
    p = _ab({"ce_ex": pair_ex, "ce_ohem": pair_oh}, nsets, reps, rounds)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(sets[0][3][..., :C]).all())
    return {"shape": [B, C, H, W], "regime": regime, "thresh": THRESH, "min_kept_total": total, "valid": V, "kept": kept,
            "cut": cut, "row_floats": ld, "tensor_sets": nsets, "unit": "us per call",
            "fwd_argmax": {k: _summary(v) for k, v in f.items()}, "bwd_nhwc_rows": {k: _summary(v) for k, v in b.items()},
            "fwd_plus_bwd": {k: _summary(v) for k, v in p.items()},
            "note": "ce_ex forward = main kernel + finalize; ce_ohem forward = memset + pixel pass + 2 radix rounds + sum "
                    "pass + finalize"}


def bench_step(dev, args):
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.utils.pipeline_utils import fetch_data_cfg, init_model

    C = fetch_data_cfg("cityscapes").num_classes
    B, H, W = 32, 128, 256
    batch = synthetic_batch(B, H, W, C, seed=11, masked=0.1)
    batch["mask"][torch.rand(B, H, W, generator=torch.Generator().manual_seed(12)) < 0.3] = IGN
    batch = {k: v.to(dev) for k, v in batch.items()}
    weights = (0.1 + 1.9 * torch.rand(C, generator=torch.Generator().manual_seed(C))).tolist()
    ms = {}
    # one model alive at a time (a captured step re-packs the GEMM operands of every live model); the un-mined step runs
    # first and again last: the difference between its two results is what the order of construction alone is worth
    for tag, min_kept in (("unmined", None), ("ohem", H * W // 16), ("unmined_again", None)):
        torch.manual_seed(11)
        ns = argparse.Namespace(model_name="basic", backbone_weights=None, segm_ignore_index=IGN,
                                segm_class_weights=weights, segm_ohem_min_kept=min_kept,
                                segm_ohem_thresh=None if min_kept is None else THRESH)
        module = init_model(ns, argparse.Namespace(num_classes=C)).to(dev).train()
        gstep = GraphedStep(module, batch)
        ms[tag] = _ab({tag: lambda i: gstep(batch)}, 1, args.step_reps, args.rounds)[tag]
        gstep.arena.close()
        del gstep, module
        gc.collect()
        torch.cuda.empty_cache()
    return {"unit": "ms per replayed step", "model": "basic", "shape": [B, H, W], "thresh": THRESH,
            "min_kept": H * W // 16, "steps": {k: _summary([x / 1e3 for x in v], 4) for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ohem.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
           "kernels": [bench_shape(dev, *s, regime, args.reps, args.rounds) for s in SHAPES for regime in ("tau", "kappa")]}
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
