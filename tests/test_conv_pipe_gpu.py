"""Two K chunks in flight in conv_igemm_kernel (64x144 tile, PF = 2) and in the tall weight-gradient tiles (128 / 144 rows,
PD = 2, peeled loop), and the weight gradient's row-group loader, against the routes they replace, which the same build
keeps behind VMTL_IG_PIPE=0 / VMTL_WG_PIPE=0 / VMTL_WG_FAST=0.

Every buffer a kernel sees is a tests/poison.py "guard" buffer (operands included): the new loops select ADDRESSES (an
out-of-range buffer offset for a chunk past the K range or the slice) where the old ones skipped the load, so a wrong
select reads a neighbour or a guard band - different numbers or NaN in the result - and a store outside a buffer breaks
a guard band, which Poison.close() reports.

  * old route against new route: torch.equal (fragment reads and MFMA order did not change);
  * every case against an fp64 reference at tests.util.assert_close's 1e-4 of max|ref|."""
import pytest
import torch
import torch.nn.functional as F

from tests import poison
from tests.util import assert_close

pytestmark = pytest.mark.gpu

FP32 = 0
TILE = 11


def _cdiv(a, b):
    return -(-a // b)


def _c4(c):
    return (c + 3) // 4 * 4


def _lib():
    from vision_mtl_amd._lib import lib

    return lib()


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


def _clean(what, **outs):
    o = {k: v.double().cpu() for k, v in outs.items()}
    for k, v in o.items():
        assert not torch.isnan(v).any(), f"{what}: poison left in (or read into) {k}"
    return o


# ------------------------------------------------------------------------------------------------ implicit GEMM
B_, H_, W_ = 2, 6, 10  # M = 120: one whole and one ragged 64-row tile
NWS = (19, 150)        # one ragged column tile; a whole one and a ragged one


def _conv_problem(KH, Cs, Nw, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B_, H_, W_, Cs, generator=g)
    w = torch.randn(Nw, Cs, KH, KH, generator=g) / (Cs * KH * KH) ** 0.5
    wp = w.permute(0, 2, 3, 1).reshape(Nw, KH * KH * Cs).contiguous()  # [n][tap * Cs + ci]
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=KH // 2).permute(0, 2, 3, 1)
    return x, wp, ref


def _geo(KH, Cs, Nw):
    return dict(B=B_, H=H_, W=W_, Cs=Cs, Ho=H_, Wo=W_, ldy=_c4(Nw), Nw=Nw, Cout=Nw, KH=KH, KW=KH, stride=1, pad=KH // 2)


def _both_routes(vmtl_env, launch, want=2):
    """the launch under VMTL_IG_PIPE=0 and =1; what each launch itself ran is read back from the launcher (not recomputed
    here): the one-chunk loop, then `want` chunks in flight"""
    got = {}
    last = _lib().raw("vmtl_conv2d_last_pipe_depth")
    for pipe in (0, 1):
        vmtl_env("VMTL_IG_PIPE", pipe)
        got[pipe] = launch()
        assert last() == (want if pipe else 1), f"VMTL_IG_PIPE={pipe}: the launch ran depth {last()}"
    torch.cuda.synchronize()
    return got[0], got[1]


def _expect_depth(L, Cs, C2s, nk, grid, up2, want):
    assert L.raw("vmtl_conv2d_pipe_depth")(TILE, Cs, C2s, nk, grid, up2, FP32) == want, (Cs, C2s, nk, grid, up2)


PLAIN = [(1, 32), (1, 64), (1, 96), (1, 128), (1, 160),  # 1-5 chunks: fewer than, equal to, more than the peel
         (3, 32),                                         # 9 chunks, taps change on chunk boundaries
         (3, 36),                                         # a tap change inside a chunk, ragged last chunk
         (3, 8)]                                          # narrow segments: must route to the one-chunk loop


@pytest.mark.parametrize("KH,Cs", PLAIN)
def test_igemm_two_chunks_equal_one_chunk_and_fp64(dev, vmtl_env, KH, Cs):
    L = _lib()
    Bf = _Bufs(dev)
    vmtl_env("VMTL_FORCE_TILE", TILE)
    vmtl_env("VMTL_IG_PIPE_MIN_CHUNKS", 1)  # lets K ranges shorter than the routed minimum of four chunks reach the new loop
    for Nw in NWS:
        x, wp, ref = _conv_problem(KH, Cs, Nw, 100 * Cs + Nw + KH)
        geo = _geo(KH, Cs, Nw)
        xd, wd = Bf.put(x), Bf.put(wp)
        vmtl_env("VMTL_IG_PIPE", 1)
        _expect_depth(L, Cs, 0, _cdiv(KH * KH * Cs, 32), 2 * _cdiv(geo["ldy"], 144), 0, 2 if Cs >= 32 else 1)

        def launch():
            y = Bf.out(B_, H_, W_, geo["ldy"])
            L.callk("vmtl_conv2d_fwd", x=xd, wp=wd, bias=None, y=y, stats=None, act=0, shuffle=0, stream=None, **geo)
            return y

        old, new = _both_routes(vmtl_env, launch, 2 if Cs >= 32 else 1)
        what = f"igemm {KH}x{KH} Cs={Cs} Nw={Nw}"
        assert torch.equal(old, new), f"{what}: y differs between VMTL_IG_PIPE=0 and =1"
        o = _clean(what, y=new)
        assert_close(o["y"][..., :Nw], ref, what=what)
        assert float(o["y"][..., Nw:].abs().max()) == 0.0, f"{what}: pad columns"
    Bf.p.close()


def test_igemm_routed_minimum_keeps_short_k_ranges_on_the_old_loop(dev):
    L = _lib()
    for nk, want in ((1, 1), (3, 1), (4, 2), (5, 2)):
        _expect_depth(L, 32, 0, nk, 4, 0, want)


UP2 = [(32, 0), (36, 36), (64, 32)]  # (C0s, C1s): no skip; the segment boundary inside a chunk; on a chunk boundary
H2_, W2_ = 3, 5                      # M = 30 rows per phase: one ragged row tile each


@pytest.mark.parametrize("C0s,C1s", UP2)
def test_igemm_up2_two_chunks_equal_one_chunk_and_fp64(dev, vmtl_env, C0s, C1s):
    L = _lib()
    Bf = _Bufs(dev)
    vmtl_env("VMTL_FORCE_TILE", TILE)
    vmtl_env("VMTL_IG_PIPE_MIN_CHUNKS", 1)
    vmtl_env("VMTL_IG_PIPE_UP2", 1)  # the UP2 class is off by default (it measured slower): switched on, it must still be right
    for Nw in NWS:
        g = torch.Generator().manual_seed(31 * C0s + C1s + Nw)
        xl = torch.randn(B_, H2_, W2_, C0s, generator=g)
        sk = torch.randn(B_, 2 * H2_, 2 * W2_, C1s, generator=g) if C1s else None
        w = torch.randn(Nw, C0s + C1s, 3, 3, generator=g) / ((C0s + C1s) * 9) ** 0.5
        ldy, Ktot = _c4(Nw), 4 * C0s + 9 * C1s
        up = xl.double().permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
        cat = torch.cat([up, sk.double().permute(0, 3, 1, 2)], 1) if C1s else up
        ref = F.conv2d(cat, w.double(), padding=1).permute(0, 2, 3, 1)
        xd, wd = Bf.put(xl), Bf.put(w)
        skd = Bf.put(sk) if C1s else None
        wp = Bf.out(4, Nw, Ktot)
        L.callk("vmtl_pack_up2_fwd", w=wd, dst=wp, Cout=Nw, C0=C0s, C0s=C0s, C1=C1s, C1s=C1s, stream=None)
        vmtl_env("VMTL_IG_PIPE", 1)
        _expect_depth(L, C0s, C1s, _cdiv(Ktot, 32), 4 * _cdiv(ldy, 144), 1, 2)

        def launch():
            y = Bf.out(B_, 2 * H2_, 2 * W2_, ldy)
            L.callk("vmtl_conv2d_up2_fwd", xl=xd, skip=skd, wp_eff=wp, y=y, stats=None, B=B_, H2=H2_, W2=W2_, C0s=C0s,
                    C1s=C1s, ldy=ldy, Cout=Nw, stream=None)
            return y

        old, new = _both_routes(vmtl_env, launch)
        what = f"igemm UP2 C0s={C0s} C1s={C1s} Nw={Nw}"
        assert torch.equal(old, new), f"{what}: y differs between VMTL_IG_PIPE=0 and =1"
        o = _clean(what, y=new)
        assert_close(o["y"][..., :Nw], ref, what=what)
        assert float(o["y"][..., Nw:].abs().max()) == 0.0, f"{what}: pad columns"
    Bf.p.close()


def test_igemm_statistics_epilogue_is_unchanged(dev, vmtl_env):
    L = _lib()
    Bf = _Bufs(dev)
    vmtl_env("VMTL_FORCE_TILE", TILE)
    KH, Cs, Nw = 3, 36, 150
    x, wp, ref = _conv_problem(KH, Cs, Nw, 77)
    geo = _geo(KH, Cs, Nw)
    ldy, M = geo["ldy"], B_ * H_ * W_
    bias = torch.randn(Nw, generator=torch.Generator().manual_seed(78))
    xd, wd, bd = Bf.put(x), Bf.put(wp), Bf.put(bias)
    rows = L.raw("vmtl_conv2d_stats_rows")(B_, H_, W_, ldy)
    rpb = L.raw("vmtl_conv2d_stats_block")(B_, H_, W_, ldy)
    assert (rows, rpb) == (2, 64)

    def launch():
        y, st = Bf.out(B_, H_, W_, ldy), Bf.out(rows, 2, ldy)
        L.callk("vmtl_conv2d_fwd", x=xd, wp=wd, bias=bd, y=y, stats=st, act=1, shuffle=0, stream=None, **geo)
        return y, st

    old, new = _both_routes(vmtl_env, launch)
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]), "statistics launch differs between the routes"
    o = _clean("stats launch", y=new[0], stats=new[1])
    assert_close(o["y"][..., :Nw], (ref + bias.double()).clamp_min(0), what="stats launch y")
    yf = o["y"].reshape(M, ldy)
    for t in range(rows):  # (mean, M2) of the row block, from the output the kernel itself stored
        blk = yf[t * rpb:(t + 1) * rpb]
        mean = blk.mean(0)
        assert_close(o["stats"][t, 0], mean, what="stats mean", atol=1e-6)
        assert_close(o["stats"][t, 1], ((blk - mean) ** 2).sum(0), what="stats M2", atol=1e-5)
    Bf.p.close()


def test_igemm_fused_batchnorm_backward_epilogue_is_unchanged(dev, vmtl_env):
    L = _lib()
    Bf = _Bufs(dev)
    vmtl_env("VMTL_FORCE_TILE", TILE)
    KH, Cs, Nw = 3, 36, 150
    x, wp, ref = _conv_problem(KH, Cs, Nw, 91)
    geo = _geo(KH, Cs, Nw)
    ldy, M = geo["ldy"], B_ * H_ * W_
    g = torch.Generator().manual_seed(92)
    ez = dict(ez_x=torch.randn(M, ldy, generator=g), ez_mean=torch.randn(ldy, generator=g),
              ez_invstd=torch.randn(ldy, generator=g).abs() + 0.5, ez_gamma=torch.randn(ldy, generator=g),
              ez_beta=torch.randn(ldy, generator=g))
    xd, wd = Bf.put(x), Bf.put(wp)
    ezd = {k: Bf.put(v) for k, v in ez.items()}
    rows = L.raw("vmtl_conv2d_stats_rows")(B_, H_, W_, ldy)

    def launch():
        y, st = Bf.out(M, ldy), Bf.out(rows, 2, ldy)
        L.callk("vmtl_conv2d_bnbwd", x=xd, wp=wd, y=y, stats=st, ez_act=1, stream=None, **ezd, **geo)
        return y, st

    old, new = _both_routes(vmtl_env, launch)
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]), "bnbwd launch differs between the routes"
    o = _clean("bnbwd launch", dz=new[0], stats=new[1])
    acc = torch.cat([ref.reshape(M, Nw), torch.zeros(M, ldy - Nw, dtype=torch.float64)], 1)
    xh = (ez["ez_x"].double() - ez["ez_mean"].double()) * ez["ez_invstd"].double()
    z = ez["ez_gamma"].double() * xh + ez["ez_beta"].double()
    dz = acc * (z > 0)
    dz[:, Nw:] = 0.0
    far = z.abs() > 1e-5  # an element whose pre-activation rounds onto the other side of the kink is not an error
    assert_close(torch.where(far, o["dz"], dz)[:, :Nw], dz[:, :Nw], what="bnbwd dz")
    for t in range(rows):
        blk, xb = o["dz"][t * 64:(t + 1) * 64], xh[t * 64:(t + 1) * 64]
        assert_close(o["stats"][t, 0, :Nw], blk.sum(0)[:Nw], what="bnbwd sum dz", atol=1e-5)
        assert_close(o["stats"][t, 1, :Nw], (blk * xb).sum(0)[:Nw], what="bnbwd sum dz*xhat", atol=1e-5)
    Bf.p.close()


@pytest.mark.parametrize("slices", [2, 3])
def test_igemm_split_k_slices_keep_their_k_range(dev, vmtl_env, slices):
    """49 chunks (3x3 over 172 channels) in 2 slices (25 + 24) and 3 slices (17 + 17 + 15): a chunk past the slice end
    lies inside the K range of the next slice and must not be multiplied"""
    L = _lib()
    Bf = _Bufs(dev)
    vmtl_env("VMTL_FORCE_TILE", TILE)
    KH, Cs, Nw = 3, 172, 150
    x, wp, ref = _conv_problem(KH, Cs, Nw, 55 + slices)
    geo = _geo(KH, Cs, Nw)
    ldy = geo["ldy"]
    vmtl_env("VMTL_KSPLIT_BLOCKS", 4 * slices)  # the tile grid is 2 x 2 workgroups
    assert L.raw("vmtl_conv2d_ksplit")(B_, H_, W_, ldy, KH * KH * Cs) == slices
    xd, wd = Bf.put(x), Bf.put(wp)
    vmtl_env("VMTL_IG_PIPE", 1)
    _expect_depth(L, Cs, 0, _cdiv(49, slices), 4 * slices, 0, 2)

    def launch():
        y, ws = Bf.out(B_, H_, W_, ldy), Bf.out(slices, B_, H_, W_, ldy)
        L.callk("vmtl_conv2d_fwd_ws", x=xd, wp=wd, bias=None, y=y, ws=ws, stream=None, **geo)
        return y, ws

    old, new = _both_routes(vmtl_env, launch)
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]), "split-K launch differs between the routes"
    o = _clean(f"split-K {slices}", y=new[0], ws=new[1])
    assert_close(o["y"][..., :Nw], ref, what=f"split-K {slices} slices")
    Bf.p.close()


# ---------------------------------------------------------------------------------------------- weight gradient
def _route(L, Bn, H, W, Cs, Ho, Wo, Nw, KH, stride, pad):
    r = L.raw("vmtl_conv2d_wgrad_route")(Bn, H, W, Cs, Ho, Wo, Nw, KH, KH, stride, pad, FP32)
    return r & 3, (r >> 2) & 1, (r >> 3) & 7, r >> 6


def _wg_case(L, Bf, vmtl_env, switch, Bn, Ho, Wo, KH, stride, pad, Cs, Nw, splits, seed, what, new_route, old_route):
    """one layer through the old route (switch = 0) and the new one; the new slabs against fp64"""
    H, W = (Ho - 1) * stride + KH - 2 * pad, (Wo - 1) * stride + KH - 2 * pad
    M, ldy, Ktot = Bn * Ho * Wo, _c4(Nw), KH * KH * Cs
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Bn, H, W, Cs, generator=g)
    dy = torch.randn(M, ldy, generator=g)
    dy[:, Nw:] = 0.0
    xd, dyd = Bf.put(x), Bf.put(dy)
    vmtl_env("VMTL_FORCE_WG_SPLITS", splits)
    sp = L.raw("vmtl_conv2d_wgrad_splits")(M, Nw, Ktot)
    slabs = {}
    for on in (0, 1):
        vmtl_env(switch, on)
        assert _route(L, Bn, H, W, Cs, Ho, Wo, Nw, KH, stride, pad) == (new_route if on else old_route), (what, on)
        slabs[on] = Bf.out(sp, Nw, Ktot)
        L.callk("vmtl_conv2d_wgrad", x=xd, dy=dyd, slabs=slabs[on], splits=sp, B=Bn, H=H, W=W, Cs=Cs, Ho=Ho, Wo=Wo,
                ldy=ldy, Nw=Nw, KH=KH, KW=KH, stride=stride, pad=pad, stream=None)
    torch.cuda.synchronize()
    assert torch.equal(slabs[0], slabs[1]), f"{what}: slabs differ between {switch}=0 and =1"
    o = _clean(what, slabs=slabs[1])
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (Nw, Cs, KH, KH),
                                      dy[:, :Nw].double().view(Bn, Ho, Wo, Nw).permute(0, 3, 1, 2), stride=stride, padding=pad)
    assert_close(o["slabs"].sum(0), ref.permute(0, 2, 3, 1).reshape(Nw, Ktot), what=what)
    return sp


@pytest.mark.parametrize("rows", [128, 144])
@pytest.mark.parametrize("Cs", [8, 16])  # Ktot = 72: one ragged kk tile; 144: two
def test_wgrad_tall_tiles_two_chunks_equal_one_chunk_and_fp64(dev, vmtl_env, rows, Cs):
    L = _lib()
    Bf = _Bufs(dev)
    vmtl_env("VMTL_FORCE_WG_ROWS", rows)
    vmtl_env("VMTL_WG_MIN_STEPS", 1)         # lets VMTL_FORCE_WG_SPLITS cut slices shorter than four chunks
    vmtl_env("VMTL_WG_PIPE_MIN_CHUNKS", 1)   # and lets those reach the peeled loop
    vmtl_env("VMTL_WG_PIPE_TALL", 3)
    for Nw in (130, 150):
        for splits, chunks in ((8, 1), (4, 2), (3, 3), (2, 4), (1, 8)):  # B = 2, 4 x 32: eight chunks; 3 slices: 3 + 3 + 2
            sp = _wg_case(L, Bf, vmtl_env, "VMTL_WG_PIPE", 2, 4, 32, 3, 1, 1, Cs, Nw, splits, 1000 * rows + 10 * Nw + splits,
                          f"wgrad {rows} rows Cs={Cs} Nw={Nw} slices of {chunks} chunk(s)", (1, 1, 2, rows), (1, 0, 1, rows))
            assert sp == splits
    Bf.p.close()


RG_MAPS = [(8, 4), (4, 8), (2, 16), (8, 16)]  # (Ho, Wo): 8, 4, 2, 2 output rows per chunk
RG_GEOM = {"3x3": (3, 1, 1), "4x4s2": (4, 2, 1)}  # the second on a 2Ho x 2Wo input


@pytest.mark.parametrize("pipe", [0, 1], ids=["guarded", "peeled"])
@pytest.mark.parametrize("kind", list(RG_GEOM))
@pytest.mark.parametrize("Ho,Wo", RG_MAPS)
def test_wgrad_row_group_loader_equals_general_loader_and_fp64(dev, vmtl_env, Ho, Wo, kind, pipe):
    L = _lib()
    Bf = _Bufs(dev)
    KH, stride, pad = RG_GEOM[kind]
    vmtl_env("VMTL_WG_MIN_STEPS", 1)
    vmtl_env("VMTL_WG_PIPE_MIN_CHUNKS", 1)
    vmtl_env("VMTL_WG_PIPE_TALL", 3)
    vmtl_env("VMTL_WG_ROWGROUP", 1)
    vmtl_env("VMTL_WG_PIPE", pipe)
    Bn = 3
    chunks = Bn * Ho * Wo // 32  # 3 (one per image) or 12 (four per image)
    for rows, Nw in ((144, 150),):  # the 144-row tile: the only one with a row-group instantiation
        vmtl_env("VMTL_FORCE_WG_ROWS", rows)
        new = (2, 1, 2, rows) if pipe else (2, 0, 1, rows)
        # (images, slices).  One chunk per image: one slice, and 2 + 1 chunks (a last slice shorter than the others).  Four
        # chunks per image: one slice, 4 slices of 3 chunks (they end inside an image), 3 of 4, and five images in
        # 7 + 7 + 6 chunks (a shorter last slice, every slice ending inside an image)
        for bn, splits in ((Bn, 1), (Bn, 2)) if chunks == 3 else ((Bn, 1), (Bn, 4), (Bn, 3), (5, 3)):
            _wg_case(L, Bf, vmtl_env, "VMTL_WG_FAST", bn, Ho, Wo, KH, stride, pad, 8, Nw, splits, 7 * Ho + Wo + splits + bn,
                     f"wgrad row groups {kind} {Ho}x{Wo} B={bn} rows={rows} splits={splits}", new, (0, 0, 1, rows))
    Bf.p.close()


def test_wgrad_odd_row_count_stays_on_the_general_loader(dev, vmtl_env):
    """(3, 16): a chunk of two rows would straddle two images"""
    L = _lib()
    Bf = _Bufs(dev)
    vmtl_env("VMTL_FORCE_WG_ROWS", 144)
    for kind, (KH, stride, pad) in RG_GEOM.items():
        _wg_case(L, Bf, vmtl_env, "VMTL_WG_FAST", 2, 3, 16, KH, stride, pad, 8, 150, 0, 5, f"wgrad {kind} 3x16", (0, 0, 1, 144),
                 (0, 0, 1, 144))
    Bf.p.close()
