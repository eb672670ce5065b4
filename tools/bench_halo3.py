"""Micro-benchmark (GPU box) of vmtl_conv3x3_halo (csrc/conv3x3_halo.hip) against the implicit GEMM on every shape the
VMTL_MID_HALO route covers, through the C ABI with the epilogue each call site uses: forward with statistics (the halo
kernel also with its BatchNorm prologue), plain data gradient, fused BatchNorm-backward data gradient.  Prints one line per
shape with both times, the TF executed by each (2 * M * Nw * 9 * Cs), the speed-up and the largest difference."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision_mtl_amd._lib import lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")
L = lib()
st = torch.cuda.current_stream().cuda_stream

# name, B, H, W, Cs (input storage), Nw (weight rows = logical output channels), mode: fwd / dgrad / bnbwd
SHAPES = [
    ("basic b3 conv2 fwd 68->67", 32, 64, 128, 68, 67, "fwd"),
    ("basic b3 conv2 bnbwd 68->67", 32, 64, 128, 68, 67, "bnbwd"),
    ("basic b3 conv1 dskip 68->16", 32, 64, 128, 68, 16, "dgrad"),
    ("basic_256 b3 conv2 fwd 68->67", 32, 128, 128, 68, 67, "fwd"),
    ("basic bs8 b3 conv2 fwd 68->67", 8, 64, 128, 68, 67, "fwd"),
    ("basic bs8 b3 conv2 bnbwd 68->67", 8, 64, 128, 68, 67, "bnbwd"),
    ("mtan 64->64 fwd", 16, 128, 128, 64, 64, "fwd"),
    ("mtan 64->64 dgrad", 16, 128, 128, 64, 64, "dgrad"),
    ("mtan 64->64 bnbwd", 16, 128, 128, 64, 64, "bnbwd"),
    ("mtan 64->32 dgrad", 16, 128, 128, 64, 32, "dgrad"),
    ("csnet 64->64 fwd", 32, 32, 64, 64, 64, "fwd"),
    ("csnet 64->64 dgrad", 32, 32, 64, 64, 64, "dgrad"),
    ("mtan 64->64 fwd at 64x64", 16, 64, 64, 64, 64, "fwd"),
]


def timeit(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / args.reps * 1e3


for name, B, H, W, Cs, Nw, mode in SHAPES:
    ldy = (Nw + 3) // 4 * 4
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, H, W, Cs, device=dev, generator=g)
    wp = torch.randn(Nw, 9 * Cs, device=dev, generator=g) * (9 * Cs) ** -0.5
    y0, y1 = torch.zeros(B, H, W, ldy, device=dev), torch.zeros(B, H, W, ldy, device=dev)
    ez = dict(ez_x=torch.randn(B, H, W, ldy, device=dev, generator=g), ez_mean=torch.zeros(ldy, device=dev),
              ez_invstd=torch.ones(ldy, device=dev), ez_gamma=torch.ones(ldy, device=dev),
              ez_beta=torch.zeros(ldy, device=dev), ez_act=1)
    none_ez = dict(ez_x=None, ez_mean=None, ez_invstd=None, ez_gamma=None, ez_beta=None, ez_act=0)
    geo = dict(B=B, H=H, W=W, Cs=Cs, Ho=H, Wo=W, ldy=ldy, Nw=Nw, Cout=Nw, KH=3, KW=3, stride=1, pad=1)
    hrows = L.raw("vmtl_conv3x3_halo_stat_rows")(B, H, W)
    hst = torch.empty(max(hrows, 1), 2, ldy, device=dev)
    if mode == "fwd":
        ist = torch.empty(L.raw("vmtl_conv2d_stats_rows")(B, H, W, ldy), 2, ldy, device=dev)
        old = lambda: L.callk("vmtl_conv2d_fwd", x=x, wp=wp, bias=None, y=y0, stats=ist, act=0, shuffle=0, stream=st, **geo)
        new = lambda: L.callk("vmtl_conv3x3_halo", x=x, pa=None, pc=None, act_in=0, a_out=None, wp=wp, bias=None, y=y1,
                              stats=hst, ep_mode=1, B=B, H=H, W=W, Cs=Cs, ldy=ldy, Nw=Nw, Cout=Nw, stream=st, **none_ez)
    elif mode == "dgrad":
        assert L.raw("vmtl_conv2d_ksplit")(B, H, W, ldy, 9 * Cs) == 1
        old = lambda: L.callk("vmtl_conv2d_fwd", x=x, wp=wp, bias=None, y=y0, stats=None, act=0, shuffle=0, stream=st, **geo)
        new = lambda: L.callk("vmtl_conv3x3_halo", x=x, pa=None, pc=None, act_in=0, a_out=None, wp=wp, bias=None, y=y1,
                              stats=None, ep_mode=0, B=B, H=H, W=W, Cs=Cs, ldy=ldy, Nw=Nw, Cout=Nw, stream=st, **none_ez)
    else:
        ist = torch.empty(L.raw("vmtl_conv2d_stats_rows")(B, H, W, ldy), 2, ldy, device=dev)
        old = lambda: L.callk("vmtl_conv2d_bnbwd", x=x, wp=wp, y=y0, stats=ist, stream=st, **ez, **geo)
        new = lambda: L.callk("vmtl_conv3x3_halo", x=x, pa=None, pc=None, act_in=0, a_out=None, wp=wp, bias=None, y=y1,
                              stats=hst, ep_mode=2, B=B, H=H, W=W, Cs=Cs, ldy=ldy, Nw=Nw, Cout=Nw, stream=st, **ez)
    t0, t1 = timeit(old), timeit(new)
    diff = float((y1 - y0).abs().max() / y0.abs().max())
    xflop = 2.0 * B * H * W * Nw * 9 * Cs
    line = (f"{name:32s} igemm {t0:7.1f} us {xflop / t0 / 1e6:6.1f} TF | halo {t1:7.1f} us {xflop / t1 / 1e6:6.1f} TF"
            f" | {t0 / t1:.2f}x  max rel diff {diff:.1e}")
    if mode == "fwd":  # with the BatchNorm + ReLU prologue writing the activated input back (the _BNActConv route)
        pa, pc, a = torch.rand(Cs, device=dev, generator=g), torch.randn(Cs, device=dev, generator=g), torch.empty_like(x)
        pro = lambda: L.callk("vmtl_conv3x3_halo", x=x, pa=pa, pc=pc, act_in=1, a_out=a, wp=wp, bias=None, y=y1,
                              stats=hst, ep_mode=1, B=B, H=H, W=W, Cs=Cs, ldy=ldy, Nw=Nw, Cout=Nw, stream=st, **none_ez)
        t2 = timeit(pro)
        line += f" | halo+prologue {t2:7.1f} us"
    print(line, flush=True)
