"""Micro-benchmark (GPU box) of the implicit-GEMM kernels on the `basic` decoder shapes at bs 32,
called through the C ABI.  VMTL_FORCE_TILE=<id> / VMTL_FORCE_WG_SPLITS=<n> override the host heuristics.
--precision fp32|bf16|both: operand precision of the covered kernels (VMTL_PREC_*); `both` times the two modes
alternately on every shape in one process and ends with one JSON line of per-shape times and bf16 speed-ups.
--wgrad-routes: instead, the weight gradient of every selected 3x3 layer through the product route (ops._wgrad_into: kernel +
slab sum) under each of the settings in --route-env ("NAME=VALUE[,NAME=VALUE];..." - default: the strip kernel's routing from
before its tail rows / 80-float pixels against today's), --repeats alternating rounds; one JSON line per layer.
--pipe-routes: instead, the launches of decoder blocks 0-2 of the headline (forward, UP2 forward, data gradient with the fused
BatchNorm backward, and every weight-gradient launch: conv2, skip part, low-resolution 4x4 / stride 2 part) and MTAN's 128-row
weight gradients, each through the C ABI under each setting of --route-env, alternating; one JSON line per launch."""
import argparse
import json
import sys

import torch

import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_mtl_amd._lib import lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="")
ap.add_argument("--stats", action="store_true", help="forward launches also write the BatchNorm partial rows (as in a training step)")
ap.add_argument("--precision", choices=["fp32", "bf16", "both"], default="fp32")
ap.add_argument("--wgrad-routes", action="store_true")
ap.add_argument("--pipe-routes", action="store_true")
ap.add_argument("--max-slabs", type=int, default=0, help="--pipe-routes: slabs allocated per weight gradient when a setting forces more slices")
ap.add_argument("--route-env", default="VMTL_WGRAD_SMALL_WIDE=0;VMTL_WGRAD_SMALL_WIDE=1")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warm-rounds", type=int, default=2, help="--wgrad-routes: unrecorded rounds in front of each layer's recorded ones")
args = ap.parse_args()
PRECS = ["fp32", "bf16"] if args.precision == "both" else [args.precision]
dev = torch.device("cuda:0")
L = lib()
st = torch.cuda.current_stream().cuda_stream


def c4(c):
    return (c + 3) // 4 * 4


# (name, B, H, W, Cin, Cout, K)
LAYERS = [("blk0.c1", 32, 8, 16, 1072, 540, 3), ("blk0.c2", 32, 8, 16, 540, 540, 3),
          ("blk1.c1", 32, 16, 32, 580, 270, 3), ("blk1.c2", 32, 16, 32, 270, 270, 3),
          ("blk2.c1", 32, 32, 64, 294, 135, 3), ("blk2.c2", 32, 32, 64, 135, 135, 3),
          ("blk3.c1", 32, 64, 128, 151, 67, 3), ("blk3.c2", 32, 64, 128, 67, 67, 3),
          ("blk4.c1", 32, 128, 256, 67, 33, 3), ("blk4.c2", 32, 128, 256, 33, 33, 3),
          ("head20", 32, 128, 256, 33, 20, 3),
          # same GEMM shapes as blk2.c2 / blk3.c2 without tap re-reads (1x1): isolates the im2col operand traffic
          ("pw.blk2c2", 32, 32, 64, 1215, 135, 1), ("pw.blk3c2", 32, 64, 128, 603, 67, 1),
          # MTAN attention 1x1 convs at full resolution (bs 16, 256x256): output-heavy, 4-6 K steps
          ("pw.mtan192", 16, 256, 256, 128, 192, 1), ("pw.mtan128", 16, 256, 256, 192, 128, 1),
          # MTAN (bs 16, 256x256, first encoder width 32): the C -> C 3x3 convs of the four resolutions
          ("mtan.s0", 16, 256, 256, 32, 32, 3), ("mtan.s1", 16, 128, 128, 64, 64, 3),
          ("mtan.s2", 16, 64, 64, 128, 128, 3), ("mtan.s3", 16, 32, 32, 256, 256, 3),
          # csnet's full-resolution decoder tail (bs 32, 128x256) and MTAN's first conv
          ("cs.32-16", 32, 128, 256, 32, 16, 3), ("cs.16-16", 32, 128, 256, 16, 16, 3), ("cs.16-19", 32, 128, 256, 16, 19, 3),
          ("cs.16-1", 32, 128, 256, 16, 1, 3), ("cs.80-32", 32, 64, 128, 80, 32, 3), ("mtan.c0", 16, 256, 256, 3, 32, 3),
          # the skip half of blk3.c1 (its own weight-gradient launch) and MTAN's 64 -> 64 at 256x256
          ("blk3.skip", 32, 64, 128, 16, 67, 3), ("mtan.64@256", 16, 256, 256, 64, 64, 3)]


def call(name, prec, *a):
    """fp32: the legacy entry point; bf16: its _p variant with VMTL_PREC_BF16 in front of the stream argument"""
    if prec == "fp32":
        L.call(name, *a)
    else:
        L.call(name + "_p", *a[:-1], 1, a[-1])


def timeit(fn):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.reps


def wgrad_routes():
    """kernel + unpack of each layer's weight gradient per routing setting, alternating; us per call"""
    from vision_mtl_amd import ops

    settings = [dict(kv.split("=") for kv in s.split(",") if kv) for s in args.route_env.split(";")]
    names = sorted({k for s in settings for k in s})
    for name, B, H, W, Cin, Cout, K in LAYERS:
        if K != 3 or (args.only and name not in args.only.split(",")):  # here --only is a comma-separated list of names
            continue
        Cs, ldy = c4(Cin), c4(Cout)
        x = torch.randn(B, H, W, Cs, device=dev)
        dy = torch.randn(B, H, W, ldy, device=dev)
        dw = torch.empty(Cout, Cin, 3, 3, device=dev)
        g = ops.ConvGeom.of(x.shape, ldy, 3, 3, 1, 1)
        lay = ops.Layout.fwd(Cout, Cin, 9, Cs)
        rec = ops._RECORD
        times = [[] for _ in settings]
        launches = [None] * len(settings)
        for rnd in range(-args.warm_rounds, args.repeats):  # rounds < 0 are not recorded: the first ~100 ms of a process run slower
            for i, s in enumerate(settings):
                for n in names:
                    os.environ.pop(n, None)
                os.environ.update(s)
                L.raw("vmtl_reload_env")()
                ops._RECORD = []
                ops._wgrad_into(x, dy, g, lay, dw, 1.0)
                launches[i] = [(n, kw.get("nslabs", kw.get("splits"))) for n, kw, _, _ in ops._RECORD]
                ops._RECORD = rec
                t = round(timeit(lambda: ops._wgrad_into(x, dy, g, lay, dw, 1.0)) * 1e3, 1)
                if rnd >= 0:
                    times[i].append(t)
        for n in names:
            os.environ.pop(n, None)
        L.raw("vmtl_reload_env")()
        print(json.dumps({"layer": name, "B": B, "H": H, "W": W, "Cin": Cin, "Cout": Cout,
                          "routes": [{"env": s, "launch": l, "us": t} for s, l, t in zip(settings, launches, times)]}), flush=True)


def pipe_routes():
    """us per call of each launch under each setting of --route-env, alternating rounds (rounds < 0 unrecorded)"""
    settings = [dict(kv.split("=") for kv in s.split(",") if kv) for s in args.route_env.split(";")]
    names = sorted({k for s in settings for k in s})
    KS = L.raw("vmtl_conv2d_ksplit")
    UKS = L.raw("vmtl_conv2d_up2_ksplit")

    def fwd(B, H, W, Cin, Cout):
        Cs, ldy = c4(Cin), c4(Cout)
        x, wp = torch.randn(B, H, W, Cs, device=dev), torch.randn(Cout, 9 * Cs, device=dev) * 0.01
        y = torch.empty(B, H, W, ldy, device=dev)
        ws = torch.empty(max(KS(B, H, W, ldy, 9 * Cs), 1), B, H, W, ldy, device=dev)
        keep = (x, wp, y, ws)
        return keep, lambda: L.call("vmtl_conv2d_fwd_ws", x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), ws.data_ptr(), B, H, W, Cs,
                                    H, W, ldy, Cout, Cout, 3, 3, 1, 1, st)

    def bnbwd(B, H, W, Cin, Cout):  # data gradient of a Cin -> Cout conv: contracts dy (Cout) into dx (Cin)
        Cs, ldy = c4(Cin), c4(Cout)
        dy, wd = torch.randn(B, H, W, ldy, device=dev), torch.randn(Cin, 9 * ldy, device=dev) * 0.01
        dx, ezx = torch.empty(B, H, W, Cs, device=dev), torch.randn(B, H, W, Cs, device=dev)
        ezs = torch.empty(L.raw("vmtl_conv2d_stats_rows")(B, H, W, Cs) + 1, 2, Cs, device=dev)
        vec = [torch.rand(Cs, device=dev) + 0.5 for _ in range(4)]
        keep = (dy, wd, dx, ezx, ezs, vec)
        return keep, lambda: L.call("vmtl_conv2d_bnbwd", dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), ezs.data_ptr(), ezx.data_ptr(),
                                    vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), 1, B, H, W, ldy, H, W,
                                    Cs, Cin, Cin, 3, 3, 1, 1, st)

    def up2(B, H2, W2, C0, C1, Cout):
        C0s, C1s, ldy = c4(C0), c4(C1), c4(Cout)
        xl, sk = torch.randn(B, H2, W2, C0s, device=dev), torch.randn(B, 2 * H2, 2 * W2, C1s, device=dev)
        wp = torch.randn(4, Cout, 4 * C0s + 9 * C1s, device=dev) * 0.01
        y = torch.empty(B, 2 * H2, 2 * W2, ldy, device=dev)
        ws = torch.empty(max(UKS(B, H2, W2, ldy, 4 * C0s + 9 * C1s), 1), B, 2 * H2, 2 * W2, ldy, device=dev)
        keep = (xl, sk, wp, y, ws)
        return keep, lambda: L.call("vmtl_conv2d_up2_fwd_ws", xl.data_ptr(), sk.data_ptr(), wp.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                    B, H2, W2, C0s, C1s, ldy, Cout, st)

    def wgrad(B, H, W, Cin, Ho, Wo, Nw, KH, stride, pad):
        Cs, ldy = c4(Cin), c4(Nw)
        x, dy = torch.randn(B, H, W, Cs, device=dev), torch.randn(B, Ho, Wo, ldy, device=dev)
        # the slice count is asked again at every call (memoised): a setting may force it (VMTL_FORCE_WG_SPLITS, a slice-length sweep)
        splits = lambda: L.raw("vmtl_conv2d_wgrad_splits")(B * Ho * Wo, Nw, KH * KH * Cs)
        slabs = torch.empty(max(splits(), args.max_slabs), Nw, KH * KH * Cs, device=dev)
        keep = (x, dy, slabs)
        return keep, lambda: L.call("vmtl_conv2d_wgrad", x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), splits(), B, H, W, Cs, Ho, Wo, ldy,
                                    Nw, KH, KH, stride, pad, st)

    # basic at bs 32, 128x256: block b's convs run on (8, 16) << b maps; conv1 = UP2 of (C0 low-res, C1 skip) channels
    BLK = [(8, 16, 960, 112, 540), (16, 32, 540, 40, 270), (32, 64, 270, 24, 135)]
    ops = []
    for b, (H, W, C0, C1, C) in enumerate(BLK):
        ops += [(f"blk{b}.c2 fwd", fwd, (32, H, W, C, C)), (f"blk{b}.c2 dgrad+bnbwd", bnbwd, (32, H, W, C, C)),
                (f"blk{b}.c1 up2 fwd", up2, (32, H // 2, W // 2, C0, C1, C)),
                (f"blk{b}.c2 wgrad", wgrad, (32, H, W, C, H, W, C, 3, 1, 1)),
                (f"blk{b}.c1 wgrad skip", wgrad, (32, H, W, C1, H, W, C, 3, 1, 1)),
                (f"blk{b}.c1 wgrad low 4x4s2", wgrad, (32, H, W, C, H // 2, W // 2, C0, 4, 2, 1))]
    ops += [("mtan.s2 wgrad", wgrad, (16, 64, 64, 128, 64, 64, 128, 3, 1, 1)), ("mtan.s3 wgrad", wgrad, (16, 32, 32, 256, 32, 32, 256, 3, 1, 1))]
    for name, make, a in ops:
        if args.only and not any(o in name for o in args.only.split(",")):
            continue
        for n in names:
            os.environ.pop(n, None)
        L.raw("vmtl_reload_env")()
        keep, fn = make(*a)  # buffers sized under the default settings (the settings change no split count)
        times = [[] for _ in settings]
        for rnd in range(-args.warm_rounds, args.repeats):
            for i, s in enumerate(settings):
                for n in names:
                    os.environ.pop(n, None)
                os.environ.update(s)
                L.raw("vmtl_reload_env")()
                t = round(timeit(fn) * 1e3, 2)
                if rnd >= 0:
                    times[i].append(t)
        for n in names:
            os.environ.pop(n, None)
        L.raw("vmtl_reload_env")()
        print(json.dumps({"launch": name, "shape": a, "routes": [{"env": s, "us": t} for s, t in zip(settings, times)]}), flush=True)
        del keep


if args.pipe_routes:
    pipe_routes()
    sys.exit(0)

if args.wgrad_routes:
    wgrad_routes()
    sys.exit(0)

tots = {p: {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0} for p in PRECS}
flops = 0.0
table = {}
for name, B, H, W, Cin, Cout, K in LAYERS:
    if args.only and args.only not in name:
        continue
    Cs, ldy, KK = c4(Cin), c4(Cout), K * K
    x = torch.randn(B, H, W, Cs, device=dev)
    dy = torch.randn(B, H, W, ldy, device=dev)
    wp = torch.randn(Cout, KK * Cs, device=dev) * 0.01
    wd = torch.randn(Cin, KK * ldy, device=dev) * 0.01
    y = torch.empty(B, H, W, ldy, device=dev)
    dx = torch.empty(B, H, W, Cs, device=dev)
    M = B * H * W
    fl = 2.0 * M * Cout * Cin * KK
    stats = None
    if args.stats:
        stats_t = torch.empty(L.raw("vmtl_conv2d_stats_rows")(B, H, W, ldy) + 1, 2, ldy, device=dev)
        stats = stats_t.data_ptr()
    ezs = torch.empty(L.raw("vmtl_conv2d_stats_rows")(B, H, W, Cs) + 1, 2, Cs, device=dev)
    ezx = torch.randn(B, H, W, Cs, device=dev)
    vec = [torch.rand(Cs, device=dev) + 0.5 for _ in range(4)]
    S = L.raw("vmtl_conv2d_wgrad_splits")(M, Cout, KK * Cs)
    slabs = torch.empty(S, Cout, KK * Cs, device=dev)
    flops += fl
    for prec in PRECS:  # alternating modes, shape by shape
        t_f = timeit(lambda: call("vmtl_conv2d_fwd", prec, x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), stats, B, H, W, Cs, H, W,
                                    ldy, Cout, Cout, K, K, 1, K // 2, 0, 0, st))
        t_d = timeit(lambda: call("vmtl_conv2d_fwd", prec, dy.data_ptr(), wd.data_ptr(), None, dx.data_ptr(), None, B, H, W, ldy, H,
                                    W, Cs, Cin, Cin, K, K, 1, K // 2, 0, 0, st))
        # the data gradient with the producer's BatchNorm + ReLU backward in its epilogue (vmtl_conv2d_bnbwd)
        t_z = timeit(lambda: call("vmtl_conv2d_bnbwd", prec, dy.data_ptr(), wd.data_ptr(), dx.data_ptr(), ezs.data_ptr(), ezx.data_ptr(),
                                    vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), 1, B, H, W, ldy, H,
                                    W, Cs, Cin, Cin, K, K, 1, K // 2, st))
        t_w = timeit(lambda: call("vmtl_conv2d_wgrad", prec, x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), S, B, H, W, Cs, H, W, ldy,
                                    Cout, K, K, 1, K // 2, st))
        t_ws = None
        if prec == "fp32" and K == 3 and L.raw("vmtl_conv3x3_wgrad_small_supported")(Cs, ldy, W):  # the strip-walking halo kernel on the same layer
            ns = L.raw("vmtl_conv3x3_wgrad_small_slabs_for")(B, H, W, Cs, ldy, Cout)
            slabs_s = torch.empty(ns, Cout, KK * Cs, device=dev)
            t_ws = timeit(lambda: L.call("vmtl_conv3x3_wgrad_small", x.data_ptr(), dy.data_ptr(), slabs_s.data_ptr(), ns, B, H, W, Cs,
                                         ldy, Cout, st))
        tot = tots[prec]
        tot["fwd"] += t_f
        tot["dgrad"] += t_d
        tot["wgrad"] += t_w
        table.setdefault(name, {})[prec] = {"fwd_us": round(t_f * 1e3, 1), "dgrad_us": round(t_d * 1e3, 1),
                                            "bnbwd_us": round(t_z * 1e3, 1), "wgrad_us": round(t_w * 1e3, 1)}
        print(f"{name:8s} {prec} M={M:8d} Cin={Cin:5d} Cout={Cout:4d}  fwd {t_f * 1e3:7.1f} us {fl / t_f / 1e9:6.1f} TF | "
              f"dgrad {t_d * 1e3:7.1f} us {fl / t_d / 1e9:6.1f} TF (+bnbwd {t_z * 1e3:6.1f}) | wgrad(S={S:3d}) {t_w * 1e3:7.1f} us {fl / t_w / 1e9:6.1f} TF"
              + (f" | halo wgrad {t_ws * 1e3:7.1f} us {fl / t_ws / 1e9:6.1f} TF" if t_ws else ""))
for prec, tot in tots.items():
    print(f"TOTAL {prec} fwd {tot['fwd']:.3f} ms ({flops / tot['fwd'] / 1e9:.1f} TF)  dgrad {tot['dgrad']:.3f} ms ({flops / tot['dgrad'] / 1e9:.1f} TF)"
          f"  wgrad {tot['wgrad']:.3f} ms ({flops / tot['wgrad'] / 1e9:.1f} TF)  sum {sum(tot.values()):.3f} ms")
if len(PRECS) == 2:
    speedup = {n: {k[:-3]: round(v["fp32"][k] / v["bf16"][k], 2) for k in v["fp32"]} for n, v in table.items()}
    print(json.dumps({"bench_conv": table, "bf16_speedup": speedup,
                      "total_ms": {p: round(sum(t.values()), 3) for p, t in tots.items()}}))
