"""Cross entropy + Dice / Tversky region term from one node (vmtl_ce_region_fwd with argmax + vmtl_ce_region_bwd into
NHWC rows, csrc/ce_region.hip) against the weighted / ignoring pair it extends (vmtl_ce_fwd_ex with argmax +
vmtl_ce_bwd_ex) on the same inputs, in the same process, GPU box only.

Shapes: 32x19x128x256 (Cityscapes at the benchmark's batch) and 16x14x256x256 (NYUv2); randn * 3 logits, ~30 % void
pixels (label 255), class weights on, Dice (alpha = beta = 0.5, smooth 0), region weight 0.5.  Each call is timed with HIP
events over a warmed-up window of `reps` calls; the variants alternate window by window, `rounds` windows each; reported
are the median and the spread (min, max) in microseconds.  Every call works on the next of several tensor sets so that
the window's working set exceeds the 256 MiB Infinity Cache.

--step adds milliseconds per replayed training step of graphed.GraphedStep (`basic`, 32x128x256, C = 19, ignore index and
class weights on, metrics on) without and with the term, one model alive at a time, the plain step measured first and
again last.  Prints ONE JSON line.

    python tools/bench_region.py [--reps 30] [--rounds 7] [--step] [--out profiles/region_loss/bench_region.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(32, 19, 128, 256), (16, 14, 256, 256)]
CACHE_BYTES = 256 << 20
IGN = 255
ALPHA, BETA, SMOOTH, REGION_WEIGHT = 0.5, 0.5, 0.0, 0.5


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


def bench_shape(dev, B, C, H, W, reps, rounds):
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib

    HW, P = H * W, B * H * W
    ld = ops.ceil4(C + 1)
    nsets = max(2, -(-2 * CACHE_BYTES // (P * (4 * C + 8 + 4 * ld))))
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(nsets):
        t = torch.randint(0, C, (B, H, W), device=dev, generator=g)
        z = torch.randn(B, C, H, W, device=dev, generator=g) * 3
        t[torch.rand(B, H, W, device=dev, generator=g) < 0.3] = IGN
        sets.append((z, t, torch.empty(B, H, W, dtype=torch.int64, device=dev), torch.empty(B, H, W, ld, device=dev)))
    w = 0.1 + 1.9 * torch.rand(C, device=dev, generator=g)
    loss, gout = torch.empty((), device=dev), torch.ones((), device=dev)
    stats_ex, stats_rg, terms, coef = (torch.empty(n, device=dev) for n in (2, 2, 2, 2 * C))
    counts = torch.empty(C + 1, dtype=torch.int64, device=dev)
    ws_ex = torch.empty(lib().raw("vmtl_ce_ex_workspace_bytes")(P) // 8, dtype=torch.float64, device=dev)
    ws_rg = torch.empty(lib().raw("vmtl_ce_region_workspace_bytes")(P, C) // 8, dtype=torch.float64, device=dev)
    geo = dict(B=B, HW=HW, C=C, sb=C * HW, sc=HW, sp=1)
    dgeo = dict(dsb=HW * ld, dsc=1, dsp=ld)
    rg = dict(ce_weight=1.0, region_weight=REGION_WEIGHT)

    def fwd_ex(i):
        z, t, am, _ = sets[i]
        ops._k("vmtl_ce_fwd_ex", logits=z, target=t, weight=w, ignore_index=IGN, loss=loss, stats=stats_ex,
               workspace=ws_ex, argmax=am, **geo)

    def bwd_ex(i):
        z, t, _, d = sets[i]
        ops._k("vmtl_ce_bwd_ex", logits=z, target=t, weight=w, ignore_index=IGN, stats=stats_ex, grad_out=gout,
               dlogits=d, **geo, **dgeo)

    def fwd_rg(i):
        z, t, am, _ = sets[i]
        ops._k("vmtl_ce_region_fwd", logits=z, target=t, weight=w, ignore_index=IGN, alpha=ALPHA, beta=BETA,
               smooth=SMOOTH, loss=loss, terms=terms, stats=stats_rg, coef=coef, counts=counts, workspace=ws_rg,
               argmax=am, **rg, **geo)

    def bwd_rg(i):
        z, t, _, d = sets[i]
        ops._k("vmtl_ce_region_bwd", logits=z, target=t, weight=w, ignore_index=IGN, stats=stats_rg, coef=coef,
               grad_out=gout, dlogits=d, **rg, **geo, **dgeo)

    def pair_ex(i):
        fwd_ex(i)
        bwd_ex(i)

    def pair_rg(i):
        fwd_rg(i)
        bwd_rg(i)

    pair_ex(0)
    pair_rg(0)
    torch.cuda.synchronize()
    ce, lr = terms.tolist()
    f = _ab({"ce_ex": fwd_ex, "ce_region": fwd_rg}, nsets, reps, rounds)
    b = _ab({"ce_ex": bwd_ex, "ce_region": bwd_rg}, nsets, reps, rounds)
    p = _ab({"ce_ex": pair_ex, "ce_region": pair_rg}, nsets, reps, rounds)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(sets[0][3][..., :C]).all())
    # what has to move per direction: the logits once, the target, and on the way back the NHWC rows (plus the argmax)
    min_bytes = {"fwd_argmax": P * (4 * C + 8 + 8), "bwd_nhwc_rows": P * (4 * C + 8 + 4 * ops.ceil4(C))}
    return {"shape": [B, C, H, W], "alpha": ALPHA, "beta": BETA, "smooth": SMOOTH, "region_weight": REGION_WEIGHT,
            "valid": counts[C].item(), "ce": ce, "l_region": lr, "row_floats": ld, "tensor_sets": nsets,
            "unit": "us per call", "min_bytes": min_bytes,
            "fwd_argmax": {k: _summary(v) for k, v in f.items()}, "bwd_nhwc_rows": {k: _summary(v) for k, v in b.items()},
            "fwd_plus_bwd": {k: _summary(v) for k, v in p.items()},
            "note": "ce_ex forward = main kernel + finalize; ce_region forward = pixel pass + finalize"}


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
    # one model alive at a time (a captured step re-packs the GEMM operands of every live model); the plain step runs
    # first and again last: the difference between its two results is what the order of construction alone is worth
    for tag, rw in (("plain", None), ("region", REGION_WEIGHT), ("plain_again", None)):
        torch.manual_seed(11)
        ns = argparse.Namespace(model_name="basic", backbone_weights=None, segm_ignore_index=IGN,
                                segm_class_weights=weights, segm_region_weight=rw, segm_region_alpha=ALPHA,
                                segm_region_beta=BETA, segm_region_smooth=SMOOTH)
        module = init_model(ns, argparse.Namespace(num_classes=C)).to(dev).train()
        gstep = GraphedStep(module, batch)
        ms[tag] = _ab({tag: lambda i: gstep(batch)}, 1, args.step_reps, args.rounds)[tag]
        gstep.arena.close()
        del gstep, module
        gc.collect()
        torch.cuda.empty_cache()
    return {"unit": "ms per replayed step", "model": "basic", "shape": [B, H, W], "region_weight": REGION_WEIGHT,
            "steps": {k: _summary([x / 1e3 for x in v], 4) for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_region.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
           "kernels": [bench_shape(dev, *s, args.reps, args.rounds) for s in SHAPES]}
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
