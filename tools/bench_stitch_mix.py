"""The full cross-stitch mix (csrc/stitch_mix.hip) at the eleven production stitch shapes of `csnet` (128x256, bs 32),
GPU box only.  Per site and weight layout, in one run and on the same tensors:

  mix_fwd / mix_bwd    vmtl_stitch_mix / vmtl_stitch_mix_bwd (data gradients + the whole weight gradient), one launch each
  diag_fwd / diag_bwd  the reference-faithful kernels, vmtl_stitch / vmtl_stitch_bwd, once per task (two launches)
  copy_fwd / copy_bwd  device-to-device copies moving the same number of bytes

timed with HIP events over a warmed-up window, reported as GB/s of the bytes each launch has to move (stored tensors of
M x Cs floats: forward 2 reads + 2 writes, backward 4 reads + 2 writes, for both tasks together).  The mix moves exactly
what the two diagonal launches move, so the comparison is bandwidth.  Each launch works on the next of up to 16 tensor
sets, enough at the large sites for the window's working set to exceed the 256 MiB Infinity Cache twice over ("tensor_sets"
in the output; the small deep sites stay cache-resident, as they do inside a training step).

--step adds the training-step time of the captured step (graphed.GraphedStep, the harness of tools/bench_precision.py)
in both stitch modes and both layouts, timed in alternating blocks.  Prints ONE JSON line.

    python tools/bench_stitch_mix.py [--bs 32] [--reps 50] [--rounds 3] [--step] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CACHE_BYTES = 256 << 20


def _build(channel_wise, mixing):
    from vision_mtl_amd.utils.pipeline_utils import build_model

    torch.manual_seed(11)
    return build_model(argparse.Namespace(model_name="csnet", backbone_weights=None, channel_wise_stitching=channel_wise,
                                          cross_stitch_mixing=mixing), argparse.Namespace(num_classes=19))


def stitch_sites(dev, bs, H, W):
    """(site name, M, C, Cs) of every mix launch of one forward pass, recorded from the model itself"""
    from vision_mtl_amd import ops

    model = _build(True, "full").to(dev).eval()
    model._compile()
    names = [arg for op, arg in model._program if op == "mix"]
    seen, orig = [], ops.stitch_mix

    def record(x0, x1, weights, C):
        B, h, w, Cs = x0.shape
        seen.append((B * h * w, C, Cs))
        return orig(x0, x1, weights, C)

    ops.stitch_mix = record
    try:
        with torch.no_grad():
            model(torch.zeros(bs, 3, H, W, device=dev))
    finally:
        ops.stitch_mix = orig
    torch.cuda.synchronize()
    assert len(seen) == len(names) == 11, (len(seen), len(names))
    return [(n,) + s for n, s in zip(names, seen)]


def _time(fn, nsets, reps, rounds):
    """median over `rounds` windows of the time of one fn(i) call, i cycling over the tensor sets"""
    for i in range(max(nsets, 3)):
        fn(i % nsets)
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i % nsets)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ms)


def bench_site(dev, M, C, Cs, channel_wise, reps, rounds):
    from vision_mtl_amd._lib import lib

    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    tensor_bytes = M * Cs * 4
    nsets = max(1, min(16, -(-2 * CACHE_BYTES // (8 * tensor_bytes))))
    g = torch.Generator(device=dev).manual_seed(3)
    sets = [[torch.randn(M, Cs, device=dev, generator=g) for _ in range(8)] for _ in range(nsets)]  # x0 x1 g0 g1 + 4 outputs
    for s in sets:
        for t in s:
            t[:, C:] = 0.0
    w = torch.rand((2, 2, C) if channel_wise else (2, 2), device=dev, generator=g)
    dw = torch.empty_like(w)
    rows = L.raw("vmtl_reduce_rows")(M)
    partial = torch.empty(4 * rows + 4, Cs, device=dev)
    ws = 1 if channel_wise else 0
    blk = C if channel_wise else 1

    def mix_fwd(i):
        x0, x1, _, _, y0, y1, _, _ = sets[i]
        L.callk("vmtl_stitch_mix", x0=x0, x1=x1, w=w, y0=y0, y1=y1, M=M, C=C, Cs=Cs, wstride=ws, stream=stream)

    def mix_bwd(i):
        x0, x1, g0, g1, _, _, d0, d1 = sets[i]
        L.callk("vmtl_stitch_mix_bwd", x0=x0, x1=x1, dy0=g0, dy1=g1, w=w, dx0=d0, dx1=d1, partial=partial, dw=dw, M=M, C=C,
                Cs=Cs, wstride=ws, stream=stream)

    def diag_fwd(i):
        s = sets[i]
        for t in range(2):
            L.callk("vmtl_stitch", x=s[t], w=w.view(-1)[3 * t * blk:], y=s[4 + t], M=M, C=C, Cs=Cs, wstride=ws, stream=stream)

    def diag_bwd(i):
        s = sets[i]
        for t in range(2):
            o = 3 * t * blk
            L.callk("vmtl_stitch_bwd", x=s[t], dy=s[2 + t], w=w.view(-1)[o:], dx=s[6 + t], partial=partial,
                    dw=dw.view(-1)[o:o + blk], M=M, C=C, Cs=Cs, wstride=ws, reduce_all=0 if channel_wise else 1, stream=stream)

    def copy_fwd(i):
        s = sets[i]
        s[4].copy_(s[0])
        s[5].copy_(s[1])

    def copy_bwd(i):
        s = sets[i]
        s[4].copy_(s[0])
        s[5].copy_(s[1])
        s[6].copy_(s[2])

    moved = {"fwd": 4 * tensor_bytes, "bwd": 6 * tensor_bytes}
    res = {"M": M, "C": C, "Cs": Cs, "tensor_sets": nsets}
    for name, fn in (("mix_fwd", mix_fwd), ("diag_fwd", diag_fwd), ("copy_fwd", copy_fwd), ("mix_bwd", mix_bwd),
                     ("diag_bwd", diag_bwd), ("copy_bwd", copy_bwd)):
        ms = _time(fn, nsets, reps, rounds)
        res[name] = {"us": round(ms * 1e3, 2), "GBps": round(moved[name[-3:]] / (ms * 1e-3) / 1e9, 1)}
    return res


def bench_step(dev, bs, H, W, steps, rounds):
    """ms/step of the captured training step, diagonal vs full mixing, per layout; alternating timed blocks"""
    from vision_mtl_amd import dp
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.lit_module import MTLModule

    out = {}
    for layout, cw in (("layer_wise", False), ("channel_wise", True)):
        gsteps, keep = {}, []
        for mixing in ("diagonal", "full"):
            model = _build(cw, mixing).to(dev).train()
            module = MTLModule(model, num_classes=19, device=str(dev))
            module.compute_metrics = False
            batch = {k: v.to(dev) for k, v in synthetic_batch(bs, H, W, 19, seed=11).items()}
            arena = dp.FlatArena(model)
            module.dp_arena = None
            gsteps[mixing] = GraphedStep(module, batch, arena=arena, warmup=1)
            keep.append((model, module, arena))
        times = {m: [] for m in gsteps}
        for _ in range(rounds):
            for mixing, gs in gsteps.items():
                gs.graph.replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    gs.graph.replay()
                e1.record()
                e1.synchronize()
                times[mixing].append(e0.elapsed_time(e1) / steps)
        res = {}
        for mixing in gsteps:
            ms = statistics.median(times[mixing])
            res[mixing] = {"ms_per_step": round(ms, 3), "img_per_s": round(bs / ms * 1e3, 1),
                           "final_loss": float(gsteps[mixing]._loss)}
        res["full_over_diagonal"] = round(res["full"]["ms_per_step"] / res["diagonal"]["ms_per_step"], 3)
        out[layout] = res
        print(f"step {layout}: {res}", file=sys.stderr, flush=True)
        del gsteps, keep
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows; the median is reported")
    ap.add_argument("--step", action="store_true", help="also time the captured training step in both stitch modes")
    ap.add_argument("--steps", type=int, default=20, help="replays per timed block of --step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stitch_mix.py needs an MI355X (the hot path has no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"config": {"bs": args.bs, "H": args.height, "W": args.width, "reps": args.reps, "rounds": args.rounds}, "sites": {}}
    for name, M, C, Cs in stitch_sites(dev, args.bs, args.height, args.width):
        site = {}
        for layout, cw in (("channel_wise", True), ("layer_wise", False)):
            site[layout] = bench_site(dev, M, C, Cs, cw, args.reps, args.rounds)
            torch.cuda.empty_cache()
        out["sites"][name] = site
        print(f"{name}: {site}", file=sys.stderr, flush=True)
    if args.step:
        out["step"] = bench_step(dev, args.bs, args.height, args.width, args.steps, args.rounds)
    print(json.dumps({"bench_stitch_mix": out}))


if __name__ == "__main__":
    main()
