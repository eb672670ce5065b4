"""Micro-benchmark (GPU box) of the pointwise (1x1) GEMM entry points (csrc/conv_pw.hip) in fp32 and bf16, called through
the C ABI on the launches of the captured steps listed in profiles/r03_experiments/step_table_mtan.txt (MTAN's attention
modules, bs 16 at 256x256) and step_table_basic.txt (the MobileNetV3 encoder chain of `basic`, bs 32 at 128x256).
The two precisions alternate shape by shape in one process; hipEvents around `--reps` launches after one warm-up launch, as
tools/bench_conv.py.  One line per shape, then ONE JSON line with the per-shape times and the bf16 speed-ups.

    python tools/bench_pw.py [--reps 10] [--only mtan]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_mtl_amd._lib import lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--only", default="", help="substring of the shape tag (mtan / basic / an entry-point kind)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_pw.py needs an MI355X (the hot path has no CPU fallback)")
dev = torch.device("cuda:0")
L = lib()
st = torch.cuda.current_stream().cuda_stream

# (model, kind, M, Ks, ldy [, K1 | N1]): kind = the entry point without its vmtl_conv1x1_ prefix; cat_fwd reads
# [K1 | Ks - K1] source columns, cat_dgrad writes [N1 | ldy - N1] destination columns
SHAPES = [
    ("mtan", "cat_fwd", 1048576, 192, 128, 64), ("mtan", "cat_dgrad", 1048576, 128, 192, 64),
    ("mtan", "bn_fwd", 1048576, 128, 32), ("mtan", "bnbwd", 1048576, 32, 128),
    ("mtan", "cat_fwd", 262144, 256, 128, 128), ("mtan", "cat_dgrad", 262144, 128, 256, 128),
    ("mtan", "cat_fwd", 262144, 64, 128, 32), ("mtan", "cat_dgrad", 262144, 128, 64, 32),
    ("mtan", "bn_fwd", 262144, 128, 64), ("mtan", "bnbwd", 262144, 64, 128),
    ("mtan", "cat_fwd", 65536, 384, 128, 256), ("mtan", "cat_dgrad", 65536, 128, 384, 256),
    ("mtan", "bn_fwd", 65536, 128, 128), ("mtan", "bnbwd", 65536, 128, 128),
    ("mtan", "cat_fwd", 16384, 640, 128, 512), ("mtan", "cat_dgrad", 16384, 128, 640, 512),
    ("mtan", "bn_fwd", 16384, 128, 256), ("mtan", "bnbwd", 16384, 256, 128),
    ("mtan", "fwd", 1048576, 4, 128),
    ("basic", "bn_res_fwd", 262144, 16, 64), ("basic", "bnbwd_add", 262144, 64, 16),
    ("basic", "bn_res_fwd", 4096, 112, 672), ("basic", "bn_fwd", 4096, 112, 672),
    ("basic", "bn_res_fwd", 1024, 160, 960), ("basic", "fwd", 1024, 960, 160), ("basic", "bnbwd_add", 1024, 960, 160),
]


def timeit(fn):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.reps


def launcher(kind, M, Ks, ldy, split):
    """closure(precision code) of one launch of vmtl_conv1x1_<kind>[_p]; the tensors stay alive in the closure"""
    r = lambda *s: torch.randn(*s, device=dev)
    variant = 1 if kind in ("bn_res_fwd", "bnbwd_add") else 0
    rows = L.raw("vmtl_conv1x1_stats_rows")(M, ldy, Ks, variant)
    kw = dict(wp=r(ldy, Ks) * 0.05)
    if kind in ("fwd", "cat_fwd", "bn_fwd", "bn_res_fwd"):
        kw.update(bias=None, y=torch.empty(M, ldy, device=dev), stats=torch.empty(rows, 2, ldy, device=dev), M=M, ldy=ldy,
                  Nw=ldy, Cout=ldy)
        if kind == "cat_fwd":
            kw.update(x=r(M, split), K1=split, x2=r(M, Ks - split), K2s=Ks - split)
        else:
            kw.update(x=r(M, Ks), Ks=Ks)
        if kind.startswith("bn_"):
            kw.update(coef_a=torch.rand(Ks, device=dev) + 0.5, coef_c=r(Ks) * 0.1, act_in=0 if kind == "bn_res_fwd" else 1,
                      a_out=torch.empty(M, Ks, device=dev))
        if kind == "bn_res_fwd":
            kw.update(res=r(M, Ks))
    elif kind == "cat_dgrad":
        kw.update(dy=r(M, Ks), dx=torch.empty(M, split, device=dev), N1=split, dx2=torch.empty(M, ldy - split, device=dev),
                  N2s=ldy - split, N2=ldy - split, M=M, Ks=Ks)
    else:  # bnbwd, bnbwd_add
        kw.update(dy=r(M, Ks), dz=torch.empty(M, ldy, device=dev), stats=torch.empty(rows, 2, ldy, device=dev), ez_x=r(M, ldy),
                  ez_mean=r(ldy) * 0.1, ez_invstd=torch.rand(ldy, device=dev) + 0.5, ez_gamma=torch.rand(ldy, device=dev) + 0.5,
                  ez_beta=r(ldy) * 0.1, ez_act=0 if kind == "bnbwd_add" else 1, M=M, Ks=Ks, ldy=ldy, Nw=ldy, Cout=ldy)
        if kind == "bnbwd_add":
            kw.update(addend=r(M, ldy))
    name = "vmtl_conv1x1_" + kind

    def launch(prec):
        if prec:
            L.callk(name + "_p", stream=st, precision=prec, **kw)
        else:
            L.callk(name, stream=st, **kw)

    return launch


table, tot = {}, {"fp32": 0.0, "bf16": 0.0}
for model, kind, M, Ks, ldy, *split in SHAPES:
    tag = f"{model}.{kind}.M{M}.K{Ks}.N{ldy}"
    if args.only and args.only not in tag:
        continue
    launch = launcher(kind, M, Ks, ldy, split[0] if split else 0)
    fl = 2.0 * M * Ks * ldy
    t = {}
    for prec, code in (("fp32", 0), ("bf16", 1)):  # alternating precisions, shape by shape
        t[prec] = timeit(lambda: launch(code))
        tot[prec] += t[prec]
    table[tag] = {"fp32_us": round(t["fp32"] * 1e3, 1), "bf16_us": round(t["bf16"] * 1e3, 1),
                  "bf16_speedup": round(t["fp32"] / t["bf16"], 3)}
    print(f"{tag:40s} fp32 {t['fp32'] * 1e3:8.1f} us {fl / t['fp32'] / 1e9:6.1f} TF | bf16 {t['bf16'] * 1e3:8.1f} us "
          f"{fl / t['bf16'] / 1e9:6.1f} TF | x{t['fp32'] / t['bf16']:.2f}", flush=True)
    del launch
    torch.cuda.empty_cache()
print(json.dumps({"bench_pw": table, "total_ms": {p: round(v, 3) for p, v in tot.items()}}))
