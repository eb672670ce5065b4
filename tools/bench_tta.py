"""The three test-time-augmentation launches (vmtl_tta_view, vmtl_tta_accumulate, vmtl_tta_finish; csrc/tta.hip) against
the torch composition they replace, on the same inputs, in the same process, GPU box only.

Cases (B x C x H x W -> output size): 32x19x128x256 -> 128x256 (Cityscapes at the benchmark's batch), 8x19x128x256 ->
1024x2048 (Cityscapes at label resolution) and 16x14x256x256 -> 256x256 (NYUv2).  The view is the 1.25x mirrored one
(sizes rounded to a multiple of 32), "accumulate" merges that view's logits into the base-size accumulators in "prob"
mode (first = 0: read + add), "finish" turns the accumulators into predictions at the output size, without and with the
confidence map.  The torch side is what a user would write instead:

    view        torch.flip(F.interpolate(img, (h, w), mode="bilinear"), [3])
    accumulate  acc += softmax(F.interpolate(flip(logits), (H, W))); acc_depth += F.interpolate(flip(sigmoid(depth)))
    finish      F.interpolate(acc, (Ho, Wo)).argmax(1); inv * F.interpolate(acc_depth, (Ho, Wo))   [+ max / sum]

Each call is timed with HIP events over a warmed-up window of `reps` calls; the variants alternate window by window,
`rounds` windows each; reported are the median and the spread (min, max) in microseconds.  Every call works on the next
of several tensor sets so that a window's working set exceeds the 256 MiB Infinity Cache.  For `finish` the achieved
GB/s against its compulsory traffic is reported - the accumulators read once plus 12 B per output pixel written (int64
arg-max + fp32 depth), 16 B with the confidence map - next to the GB/s of a plain device copy measured in the same run.

--step adds milliseconds per replayed graphed.GraphedEval predict step of `basic` (32x128x256, C = 19, no targets):
plain, flip only, and three scales (0.75, 1.0, 1.25) + flip; one model alive at a time, the plain step first and again
last.  Prints ONE JSON line.

    python tools/bench_tta.py [--reps 20] [--rounds 7] [--step] [--out profiles/tta/bench_tta.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(32, 19, 128, 256, 128, 256), (8, 19, 128, 256, 1024, 2048), (16, 14, 256, 256, 256, 256)]
CACHE_BYTES = 256 << 20
SCALE = 1.25
MAX_SETS = 6


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


def _summary(us, nbytes=None, digits=2):
    med = statistics.median(us)
    out = {"median": round(med, digits), "min": round(min(us), digits), "max": round(max(us), digits)}
    if nbytes:
        out["compulsory_bytes"] = nbytes
        out["achieved_gb_per_s"] = round(nbytes / (med * 1e-6) / 1e9, 1)
    return out


def _interp(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False)


def copy_bandwidth(dev, reps, rounds):
    """GB/s (bytes read + bytes written) of dst.copy_(src) on 1 GiB tensors, rotating over three pairs"""
    n = (1 << 30) // 4
    pairs = [(torch.rand(n, device=dev), torch.empty(n, device=dev)) for _ in range(3)]
    us = _ab({"copy": lambda i: pairs[i][1].copy_(pairs[i][0])}, 3, reps, rounds)["copy"]
    return _summary(us, 2 * 4 * n)


def bench_case(dev, B, C, H, W, Ho, Wo, reps, rounds):
    from vision_mtl_amd import ops

    h, w = round(SCALE * H / 32) * 32, round(SCALE * W / 32) * 32
    out_px, base_px, view_px = B * Ho * Wo, B * H * W, B * h * w
    set_bytes = 4 * ((C + 1) * (view_px + base_px) + 4 * (base_px + view_px)) + 16 * out_px
    nsets = min(MAX_SETS, max(2, -(-2 * CACHE_BYTES // set_bytes)))
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(nsets):
        img = torch.rand(B, H, W, 4, device=dev, generator=g)
        sets.append(dict(img=img, img_nchw=img[..., :3].permute(0, 3, 1, 2).contiguous(),
                         view=torch.empty(B, h, w, 4, device=dev),
                         logits=3.0 * torch.randn(B, C, h, w, device=dev, generator=g),
                         depth=torch.randn(B, 1, h, w, device=dev, generator=g),
                         acc=torch.rand(B, C, H, W, device=dev, generator=g), acc_d=torch.rand(B, H, W, device=dev, generator=g),
                         segm=torch.empty(B, Ho, Wo, dtype=torch.int64, device=dev), out_d=torch.empty(B, Ho, Wo, device=dev),
                         conf=torch.empty(B, Ho, Wo, device=dev)))
    inv = 0.25

    def view_hip(i):
        s = sets[i]
        ops._k("vmtl_tta_view", img=s["img"], ld=4, out=s["view"], B=B, H=H, W=W, Ho=h, Wo=w, flip=1)

    def view_torch(i):
        return torch.flip(_interp(sets[i]["img_nchw"], (h, w)), [3])

    def acc_hip(i):
        s = sets[i]
        ops._k("vmtl_tta_accumulate", logits=s["logits"], depth_logits=s["depth"], acc=s["acc"], acc_depth=s["acc_d"], B=B,
               C=C, h=h, w=w, H=H, W=W, flip=1, weight=1.0, depth_gain=1.0, mode=0, first=0)

    def acc_torch(i):
        s = sets[i]
        s["acc"].add_(torch.softmax(_interp(torch.flip(s["logits"], [3]), (H, W)), 1))
        s["acc_d"].add_(_interp(torch.flip(torch.sigmoid(s["depth"]), [3]), (H, W))[:, 0])

    def fin_hip(i, conf=False):
        s = sets[i]
        ops._k("vmtl_tta_finish", acc=s["acc"], acc_depth=s["acc_d"], inv_weight=inv, segm=s["segm"], depth=s["out_d"],
               confidence=s["conf"] if conf else None, B=B, C=C, H=H, W=W, Ho=Ho, Wo=Wo, mode=0)

    def fin_torch(i, conf=False):
        s = sets[i]
        m = _interp(s["acc"], (Ho, Wo))
        res = [m.argmax(1), inv * _interp(s["acc_d"][:, None], (Ho, Wo))[:, 0]]
        if conf:
            res.append(m.max(1).values / m.sum(1))
        return res

    v = _ab({"hip": view_hip, "torch": view_torch}, nsets, reps, rounds)
    a = _ab({"hip": acc_hip, "torch": acc_torch}, nsets, reps, rounds)
    for s in sets:  # the accumulate windows added to them: back to probabilities-like values
        s["acc"].uniform_(0, 1)
        s["acc_d"].uniform_(0, 1)
    f = _ab({"hip": fin_hip, "torch": fin_torch, "hip_conf": lambda i: fin_hip(i, True),
             "torch_conf": lambda i: fin_torch(i, True)}, nsets, reps, rounds)
    torch.cuda.synchronize()
    # same inputs, same answer: the timed torch composition is also the check
    ref = fin_torch(0, True)
    fin_hip(0, True)
    torch.cuda.synchronize()
    agree = float((sets[0]["segm"] == ref[0]).double().mean())
    assert agree > 0.999, agree
    assert float((sets[0]["out_d"] - ref[1]).abs().max()) < 1e-5 and float((sets[0]["conf"] - ref[2]).abs().max()) < 1e-5
    acc_bytes = 4 * (C + 1) * base_px
    nb = {"hip": acc_bytes + 12 * out_px, "hip_conf": acc_bytes + 16 * out_px}
    return {"case": f"{B}x{C}x{H}x{W} -> {Ho}x{Wo}", "view": [h, w], "tensor_sets": nsets, "unit": "us per launch",
            "argmax_agreement_with_torch": agree,
            "view_launch": {k: _summary(x) for k, x in v.items()},
            "accumulate": {k: _summary(x) for k, x in a.items()},
            "finish": {k: _summary(x, nb.get(k)) for k, x in f.items()},
            "note": "torch = the F.interpolate / softmax / argmax composition the launch replaces; finish bytes = the "
                    "accumulators read once + 12 (16 with confidence) B per output pixel written"}


def bench_step(dev, args):
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedEval
    from vision_mtl_amd.inference import PredictAugment
    from vision_mtl_amd.utils.pipeline_utils import fetch_data_cfg, init_model

    C = fetch_data_cfg("cityscapes").num_classes
    B, H, W = 32, 128, 256
    batch = {"img": synthetic_batch(B, H, W, C, seed=11)["img"].to(dev)}
    variants = (("plain", None), ("flip", dict(flip=True)), ("three_scales_flip", dict(scales=(0.75, 1.0, 1.25), flip=True)),
                ("plain_again", None))
    ms, views = {}, {}
    for tag, kw in variants:  # one model alive at a time (a captured step re-packs the GEMM operands of every live model)
        torch.manual_seed(11)
        module = init_model(argparse.Namespace(model_name="basic", backbone_weights=None), argparse.Namespace(num_classes=C))
        module = module.to(dev).eval()
        if kw is not None:
            module.predict_augment = PredictAugment(**kw)
            views[tag] = len(module.predict_augment.views(H, W))
        geval = GraphedEval(module, batch, stage="predict")
        ms[tag] = _ab({tag: lambda i: geval(batch)}, 1, args.step_reps, args.rounds)[tag]
        del geval, module
        gc.collect()
        torch.cuda.empty_cache()
    return {"unit": "ms per replayed predict step", "model": "basic", "shape": [B, H, W], "views": views,
            "steps": {k: _summary([x / 1e3 for x in v], digits=4) for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
           "copy": copy_bandwidth(dev, args.reps, args.rounds),
           "kernels": [bench_case(dev, *c, args.reps, args.rounds) for c in CASES]}
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
