"""The branch-free, really-prefetching loaders of pw_gemm_kernel (csrc/conv_pw.hip) and of the narrow weight-gradient
tiles (csrc/conv_wgrad.hip, PD = 3, scalar-chunk loader) against the loaders they replaced, which the same build keeps
behind VMTL_PW_PIPE=0 / VMTL_WG_PIPE=0.

Every buffer a kernel sees here - operands included - is a tests/poison.py "guard" buffer: a view between two guard
bands of NaN sentinels, outputs NaN-filled.  The new loaders select ADDRESSES (an out-of-range buffer offset, a zero
page) where the old ones selected values, so a wrong select reads a neighbouring row, a guard band, or nothing: the
first two put different numbers or NaN into the result, the last leaves poison in an output - and a store outside an
operand breaks a guard band, which Poison.close() reports.

  * old route against new route: torch.equal on every output (the MFMA order did not change);
  * every pointwise case against an fp64 GEMM of the same operands at the tolerance the existing kernel tests use for
    these kernels: tests.util.assert_close's 1e-4 of max|ref| for fp32, and for bf16 the 1e-5 of
    tests/test_pw_bf16_gpu.py against the fp64 product of the bf16-rounded operands.

Shapes (the smallest that can go wrong): Ks in {4 .. 112} = 1 to 7 k-groups, fewer than / equal to / more than the
prefetch depth, each run with the 4 waves stacked along M (KW = 1) and splitting K (KW = 4, VMTL_PW_KW); M in
{1, 33, 100, 1000} (less than a tile, a ragged second tile, several workgroups); Nw in {3, 19, 67} (32- and 64-column
tiles, ragged in both).  Two entry points cannot take two of these values and use the nearest legal one:
vmtl_conv1x1_cat_fwd needs K1, K2s >= 4 (Ks = 8 stands in for Ks = 4; every K1 used is no multiple of 16), and
vmtl_conv1x1_cat_dgrad needs N1 >= 4 (Nw = 7 stands in for Nw = 3)."""
import itertools

import pytest
import torch

from tests import poison
from tests.util import assert_close

pytestmark = pytest.mark.gpu

KS = (4, 12, 16, 20, 40, 48, 72, 112)
MS = (1, 33, 100, 1000)
NWS = (3, 19, 67)
K1_OF = {8: 4, 12: 4, 16: 12, 20: 8, 40: 20, 48: 36, 72: 44, 112: 52}  # two-source split: K1 % 4 == 0, K1 % 16 != 0
N1_OF = {7: 4, 19: 8, 67: 32}                                           # two-destination split: N1 % 4 == 0
ACT_NONE, ACT_RELU, ACT_HSWISH = 0, 1, 2

FAMILIES = ("fwd", "bn_fwd", "bn_res_fwd", "bnbwd", "bnbwd_add", "cat_fwd", "cat_dgrad")


def _cdiv(a, b):
    return -(-a // b)


def _lib():
    from vision_mtl_amd._lib import lib

    return lib()


def _r(t):
    """the bf16 image of an fp32 tensor, in fp64"""
    return t.to(torch.bfloat16).double()


class _Bufs:
    """guard-banded device buffers: operands (filled from CPU tensors) and poisoned outputs"""

    def __init__(self, dev):
        self.p = poison.Poison("guard")
        self.like = torch.empty(0, device=dev)

    def put(self, t):
        d = self.p.empty(tuple(t.shape), self.like)
        d.copy_(t)
        return d

    def out(self, *shape):
        return self.p.empty(shape, self.like)


def _act(v, code):
    if code == ACT_RELU:
        return v.clamp_min(0)
    if code == ACT_HSWISH:
        return v * (v + 3).clamp(0, 6) / 6
    return v


def _pw_problem(family, M, Ks, Nw, seed):
    """CPU operands of one case (fp32) and its geometry"""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    ldy = (Nw + 3) // 4 * 4
    c = dict(M=M, Ks=Ks, Nw=Nw, ldy=ldy, x=rnd(M, Ks), wp=rnd(Nw, Ks) / Ks ** 0.5, bias=rnd(Nw))
    if family in ("bn_fwd", "bn_res_fwd"):
        c.update(pa=rnd(Ks), pc=rnd(Ks), act=ACT_RELU if family == "bn_fwd" else ACT_HSWISH)
        if family == "bn_res_fwd":
            c["res"] = rnd(M, Ks)
    if family in ("bnbwd", "bnbwd_add"):
        c.update(ez_x=rnd(M, ldy), ez_mean=rnd(ldy), ez_invstd=rnd(ldy).abs() + 0.5, ez_gamma=rnd(ldy), ez_beta=rnd(ldy))
        if family == "bnbwd_add":
            c["addend"] = rnd(M, ldy)
    return c


def _pw_launch(L, B, family, c, d, prec):
    """one launch into fresh poisoned outputs; returns {name: tensor}"""
    M, Ks, Nw, ldy = c["M"], c["Ks"], c["Nw"], c["ldy"]
    variant = 1 if family in ("bn_res_fwd", "bnbwd_add") else 0
    rows = L.raw("vmtl_conv1x1_stats_rows")(M, ldy, Ks, variant)
    geo = dict(M=M, Ks=Ks, ldy=ldy, Nw=Nw, Cout=Nw)
    name = "vmtl_conv1x1_" + family
    if family == "fwd":
        outs = dict(y=B.out(M, ldy), stats=B.out(rows, 2, ldy))
        kw = dict(x=d["x"], wp=d["wp"], bias=d["bias"], **outs, **geo)
    elif family in ("bn_fwd", "bn_res_fwd"):
        outs = dict(a_out=B.out(M, Ks), y=B.out(M, ldy), stats=B.out(rows, 2, ldy))
        kw = dict(x=d["x"], coef_a=d["pa"], coef_c=d["pc"], act_in=c["act"], wp=d["wp"], bias=d["bias"], **outs, **geo)
        if family == "bn_res_fwd":
            kw["res"] = d["res"]
    elif family in ("bnbwd", "bnbwd_add"):
        outs = dict(dz=B.out(M, ldy), stats=B.out(rows, 2, ldy))
        kw = dict(dy=d["x"], wp=d["wp"], ez_x=d["ez_x"], ez_mean=d["ez_mean"], ez_invstd=d["ez_invstd"],
                  ez_gamma=d["ez_gamma"], ez_beta=d["ez_beta"], ez_act=ACT_RELU, **outs, **geo)
        if family == "bnbwd_add":
            kw["addend"] = d["addend"]
    elif family == "cat_fwd":
        K1 = K1_OF[Ks]
        outs = dict(y=B.out(M, ldy), stats=B.out(rows, 2, ldy))
        kw = dict(x=d["x1"], K1=K1, x2=d["x2"], K2s=Ks - K1, wp=d["wp"], bias=d["bias"], **outs, M=M, ldy=ldy, Nw=Nw, Cout=Nw)
    else:  # cat_dgrad
        N1 = N1_OF[Nw]
        outs = dict(dx=B.out(M, N1), dx2=B.out(M, ldy - N1))
        kw = dict(dy=d["x"], wp=d["wp"], N1=N1, N2s=ldy - N1, N2=Nw - N1, M=M, Ks=Ks, **outs)
    if prec:
        L.callk(name + "_p", precision=prec, stream=None, **kw)
    else:
        L.callk(name, stream=None, **kw)
    return outs


def _block_rows(L, c, variant):
    return L.raw("vmtl_conv1x1_stats_block")(c["M"], c["ldy"], c["Ks"], variant)


def _check_fp64(L, family, c, out, prec, what):
    """the new route's outputs against fp64 references (CPU)"""
    M, Ks, Nw, ldy = c["M"], c["Ks"], c["Nw"], c["ldy"]
    o = {k: v.double().cpu() for k, v in out.items()}
    for k, v in o.items():
        assert not torch.isnan(v).any(), f"{what}: poison left in (or read into) {k}"
    f = _r if prec else (lambda t: t.double())
    tol = 1e-5 if prec else 1e-4
    w = f(c["wp"])
    if family in ("fwd", "cat_fwd", "bn_fwd", "bn_res_fwd"):
        if family in ("bn_fwd", "bn_res_fwd"):
            a = _act(c["pa"].double() * c["x"].double() + c["pc"].double(), c["act"])
            if family == "bn_res_fwd":
                a = a + c["res"].double()
            assert_close(o["a_out"], a, what=f"{what} a_out")
            # the product operand is the bf16 image of the fp32 value a_out received
            a = _r(out["a_out"].float().cpu()) if prec else a
        else:
            a = f(c["x"])
        y = a @ w.t() + c["bias"].double()
        assert_close(o["y"][:, :Nw], y, tol=tol, what=f"{what} y")
        assert float(o["y"][:, Nw:].abs().max() if ldy > Nw else 0.0) == 0.0, f"{what}: pad columns of y"
        rpb = _block_rows(L, c, 1 if family == "bn_res_fwd" else 0)
        for t in range(o["stats"].shape[0]):  # (mean, M2) of the row block, from the output the kernel itself stored
            blk = o["y"][t * rpb:(t + 1) * rpb]
            mean = blk.mean(0)
            assert_close(o["stats"][t, 0], mean, what=f"{what} stats mean", atol=1e-6)
            assert_close(o["stats"][t, 1], ((blk - mean) ** 2).sum(0), what=f"{what} stats M2", atol=1e-5)
    elif family in ("bnbwd", "bnbwd_add"):
        acc = f(c["x"]) @ w.t()
        acc = torch.cat([acc, torch.zeros(M, ldy - Nw, dtype=torch.float64)], 1)
        if family == "bnbwd_add":
            acc = acc + c["addend"].double()
            acc[:, Nw:] = 0.0
        xh = (c["ez_x"].double() - c["ez_mean"].double()) * c["ez_invstd"].double()
        z = c["ez_gamma"].double() * xh + c["ez_beta"].double()
        z[:, Nw:] = 0.0  # gamma = beta = 0 past Cout: relu'(0) = 0
        dz = acc * (z > 0)
        far = z.abs() > 1e-5  # an element whose pre-activation rounds onto the other side of the kink is not an error
        assert_close(torch.where(far, o["dz"], dz), dz, tol=tol, what=f"{what} dz")
        rpb = _block_rows(L, c, 1 if family == "bnbwd_add" else 0)
        for t in range(o["stats"].shape[0]):
            blk, xb = o["dz"][t * rpb:(t + 1) * rpb], xh[t * rpb:(t + 1) * rpb]
            assert_close(o["stats"][t, 0], blk.sum(0), what=f"{what} stats sum dz", atol=1e-5)
            assert_close(o["stats"][t, 1], (blk * xb).sum(0), what=f"{what} stats sum dz*xhat", atol=1e-5)
    else:  # cat_dgrad
        N1 = N1_OF[Nw]
        full = f(c["x"]) @ w.t()
        assert_close(o["dx"], full[:, :N1], tol=tol, what=f"{what} dx")
        assert_close(o["dx2"][:, :Nw - N1], full[:, N1:], tol=tol, what=f"{what} dx2")
        assert float(o["dx2"][:, Nw - N1:].abs().max() if ldy > Nw else 0.0) == 0.0, f"{what}: pad columns of dx2"


@pytest.mark.parametrize("prec", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_pw_gemm_new_loader_equals_old_and_fp64(dev, vmtl_env, family, prec):
    L = _lib()
    B = _Bufs(dev)
    ks = tuple(8 if k == 4 else k for k in KS) if family == "cat_fwd" else KS
    nws = tuple(7 if n == 3 else n for n in NWS) if family == "cat_dgrad" else NWS
    cases = []
    for i, (Ks, M, Nw) in enumerate(itertools.product(ks, MS, nws)):
        c = _pw_problem(family, M, Ks, Nw, 7000 + i)
        d = {k: B.put(v) for k, v in c.items() if torch.is_tensor(v)}
        if family == "cat_fwd":
            K1 = K1_OF[Ks]
            d["x1"], d["x2"] = B.put(c["x"][:, :K1].contiguous()), B.put(c["x"][:, K1:].contiguous())
        cases.append((c, d))
    launches = 0
    for kw in (1, 4):
        vmtl_env("VMTL_PW_KW", kw)
        got = {}
        for pipe in (0, 1):
            vmtl_env("VMTL_PW_PIPE", pipe)
            got[pipe] = [_pw_launch(L, B, family, c, d, prec) for c, d in cases]
            launches += len(cases)
        torch.cuda.synchronize()
        for (c, _), old, new in zip(cases, got[0], got[1]):
            what = f"conv1x1_{family} {'bf16' if prec else 'fp32'} KW={kw} M={c['M']} Ks={c['Ks']} Nw={c['Nw']}"
            for k in old:
                assert torch.equal(old[k], new[k]), f"{what}: {k} differs between VMTL_PW_PIPE=0 and =1"
            _check_fp64(L, family, c, new, prec, what)
    B.p.close()  # no store outside any buffer, operands included
    print(f"{launches} launches, {B.p.count} guarded buffers, all guards intact")


# ---------------------------------------------------------------------------------------------- weight gradient
# (kind, KH, stride, pad, Cs): 3x3 stride 1, 4x4 stride 2, pointwise
WG_KINDS = {"3x3": (3, 1, 1, 8), "4x4s2": (4, 2, 1, 8), "pw": (1, 1, 0, 40)}
# M -> (B, Ho, Wo) with Wo % 32 == 0 (the scalar-chunk loader), and the forced slice counts: slices of 1, 2, 3, 4, 7 chunks
WG_M = {32: ((1, 1, 32), (1,)), 96: ((3, 1, 32), (1, 3)), 224: ((1, 7, 32), (1, 7)), 1024: ((2, 16, 32), (8, 16, 32))}
# tile heights 16, 20, 32, 36 (PD = 3: the peeled loop) and 48, 64 (PD = 2: measured slower with the peeled loop, so they
# keep the guarded one under either setting - they stay in the sweep for the day that changes)
WG_NW = (16, 20, 32, 33, 48, 64)


def _wg_case(L, B, vmtl_env, Bn, Ho, Wo, KH, stride, pad, Cs, Nw, splits, seed, what, expect_chunks=None):
    H, W = (Ho - 1) * stride + KH - 2 * pad, (Wo - 1) * stride + KH - 2 * pad
    M, ldy, Ktot = Bn * Ho * Wo, (Nw + 3) // 4 * 4, KH * KH * Cs
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Bn, H, W, Cs, generator=g)
    dy = torch.randn(M, ldy, generator=g)
    dy[:, Nw:] = 0.0
    xd, dyd = B.put(x), B.put(dy)
    vmtl_env("VMTL_FORCE_WG_SPLITS", splits)
    sp = L.raw("vmtl_conv2d_wgrad_splits")(M, Nw, Ktot)
    if expect_chunks is not None:
        assert sp == splits and _cdiv(_cdiv(M, sp), 32) == expect_chunks, (what, sp)
    slabs = {}
    for pipe in (0, 1):
        vmtl_env("VMTL_WG_PIPE", pipe)
        slabs[pipe] = B.out(sp, Nw, Ktot)
        L.callk("vmtl_conv2d_wgrad", x=xd, dy=dyd, slabs=slabs[pipe], splits=sp, B=Bn, H=H, W=W, Cs=Cs, Ho=Ho, Wo=Wo,
                ldy=ldy, Nw=Nw, KH=KH, KW=KH, stride=stride, pad=pad, stream=None)
    torch.cuda.synchronize()
    assert torch.equal(slabs[0], slabs[1]), f"{what}: slabs differ between VMTL_WG_PIPE=0 and =1"
    # fp64: dW[co][kh][kw][ci] = sum over pixels of dy * the shifted input (fp32 MFMAs: assert_close's 1e-4)
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (Nw, Cs, KH, KH),
                                      dy[:, :Nw].double().view(Bn, Ho, Wo, Nw).permute(0, 3, 1, 2), stride=stride, padding=pad)
    assert_close(slabs[1].double().sum(0).cpu(), ref.permute(0, 2, 3, 1).reshape(Nw, Ktot), what=what)


@pytest.mark.parametrize("kind", list(WG_KINDS))
@pytest.mark.parametrize("Nw", WG_NW)
def test_wgrad_peeled_loop_equals_guarded_loop(dev, vmtl_env, kind, Nw):
    L = _lib()
    B = _Bufs(dev)
    KH, stride, pad, Cs = WG_KINDS[kind]
    vmtl_env("VMTL_WG_MIN_STEPS", 1)  # lets VMTL_FORCE_WG_SPLITS cut slices shorter than four chunks
    n = 0
    for M, ((Bn, Ho, Wo), all_splits) in WG_M.items():
        for splits in all_splits:
            chunks = M // 32 // splits
            _wg_case(L, B, vmtl_env, Bn, Ho, Wo, KH, stride, pad, Cs, Nw, splits, 9000 + M + splits,
                     f"wgrad {kind} Nw={Nw} M={M} slices of {chunks} chunk(s)", expect_chunks=chunks)
            n += 1
    B.p.close()
    print(f"{n} shapes x 2 routes, {B.p.count} guarded buffers, all guards intact")


def test_wgrad_general_loader_is_unchanged(dev, vmtl_env):
    """Wo % 32 != 0 takes the general loader, which keeps the guarded loop under either setting"""
    L = _lib()
    B = _Bufs(dev)
    for Nw in (33, 64):
        _wg_case(L, B, vmtl_env, 2, 10, 20, 3, 1, 1, 8, Nw, 0, 9900 + Nw, f"wgrad 3x3 Wo=20 Nw={Nw}")
    B.p.close()
