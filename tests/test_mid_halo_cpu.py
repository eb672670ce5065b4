"""Host-side contract of the mid-width halo-tile conv (vmtl_conv3x3_halo, no GPU needed): the shape guard, the statistics
geometry, the routing rule (ops.conv_plan) and the argument checks that return before any launch."""
from vision_mtl_amd import ops
from vision_mtl_amd._lib import lib


def test_mid_halo_guard():
    sup = lib().raw("vmtl_conv3x3_halo_supported")
    for cs in (64, 68):
        for ldy, nw in ((16, 16), (32, 32), (64, 64), (68, 67), (68, 68), (68, 65), (64, 61)):
            assert sup(32, 64, 128, cs, ldy, nw) == 1, (cs, ldy, nw)
    assert sup(32, 64, 128, 36, 68, 67) == 0 and sup(32, 64, 128, 72, 68, 67) == 0  # input width
    assert sup(32, 64, 128, 68, 36, 33) == 0 and sup(32, 64, 128, 68, 48, 48) == 0  # output width
    assert sup(32, 64, 128, 68, 68, 64) == 0  # ldy must be round_up(Nw, 4)
    assert sup(0, 64, 128, 68, 68, 67) == 0
    assert sup(512, 256, 256, 68, 68, 67) == 0  # x over 2 GiB: 32-bit offsets in the kernel


def test_mid_halo_statistics_geometry():
    rows, blk = lib().raw("vmtl_conv3x3_halo_stat_rows"), lib().raw("vmtl_conv3x3_halo_stat_block")
    assert rows(32, 64, 128) == 32 * 16 * 4 and blk(32, 64, 128) == 128  # one row per 4 x 32 tile
    assert rows(16, 128, 128) * 128 == 16 * 128 * 128
    assert rows(1, 6, 32) == 0 and rows(1, 8, 48) == 0  # partial tiles: no statistics
    assert blk(1, 6, 32) == 0


def test_mid_halo_argument_checks():
    f = lib().raw("vmtl_conv3x3_halo")
    none5 = (None,) * 5
    # (x, pa, pc, act_in, a_out, wp, bias, y, stats, ep_mode, ez_x, ez_mean, ez_invstd, ez_gamma, ez_beta, ez_act,
    #  B, H, W, Cs, ldy, Nw, Cout, stream)
    assert f(None, None, None, 0, None, 1, None, 1, None, 0, *none5, 0, 1, 4, 32, 68, 68, 67, 67, None) == -1  # null x
    assert f(1, 1, None, 0, None, 1, None, 1, None, 0, *none5, 0, 1, 4, 32, 68, 68, 67, 67, None) == -1  # pa without pc
    assert f(1, None, None, 0, 1, 1, None, 1, None, 0, *none5, 0, 1, 4, 32, 68, 68, 67, 67, None) == -1  # a_out without pa
    assert f(1, 1, 1, 2, None, 1, None, 1, None, 0, *none5, 0, 1, 4, 32, 68, 68, 67, 67, None) == -1  # prologue act
    assert f(1, None, None, 0, None, 1, None, 1, 1, 1, *none5, 0, 1, 6, 32, 68, 68, 67, 67, None) == -1  # partial tiles
    assert f(1, None, None, 0, None, 1, None, 1, 1, 1, *none5, 0, 1, 4, 48, 68, 68, 67, 67, None) == -1  # partial tiles
    assert f(1, None, None, 0, None, 1, None, 1, None, 1, *none5, 0, 1, 4, 32, 68, 68, 67, 67, None) == -1  # no stats
    assert f(1, None, None, 0, None, 1, None, 1, 1, 2, *none5, 0, 1, 4, 32, 68, 68, 67, 67, None) == -1  # ep 2 operands
    assert f(1, None, None, 0, None, 1, None, 1, None, 0, *none5, 0, 1, 4, 32, 36, 36, 33, 33, None) == -3  # not instantiated
    assert f(1, None, None, 0, None, 1, None, 1, None, 0, *none5, 0, 1, 4, 32, 68, 48, 48, 48, None) == -3


def test_mid_halo_route_and_statistics_geometry_follow_each_other(monkeypatch):
    def plan(B, H, W, Cs, ldy, KH=3, KW=3, stride=1, pad=1, prec=0, epilogue=None):
        Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        return ops.conv_plan(B, H, W, Cs, Ho, Wo, ldy, KH, KW, stride, pad, prec=prec, epilogue=epilogue)

    # the bs-32 `basic` block-3 layers (68 -> 67 and 68 -> 16 at 64 x 128) and MTAN's 64 -> 64 at 128 x 128
    assert plan(32, 64, 128, 68, 68, epilogue="stats").route == "mid_halo"
    assert plan(32, 64, 128, 68, 16).route == "mid_halo"
    assert plan(16, 128, 128, 64, 64, epilogue="stats").route == "mid_halo"
    assert plan(32, 64, 128, 68, 68, epilogue="stats")[2:] == (2048, 128)
    assert plan(32, 64, 128, 68, 68, prec=1).route != "mid_halo"  # bf16 stays on the implicit GEMM
    assert plan(32, 64, 128, 68, 68, stride=2).route != "mid_halo"
    assert plan(32, 64, 128, 68, 68, KH=1, KW=1, pad=0).route != "mid_halo"
    assert plan(2, 64, 64, 68, 68).route != "mid_halo"  # too few pixels
    assert plan(32, 66, 128, 68, 68, epilogue="stats").route != "mid_halo"  # partial tiles
    igemm = (lib().raw("vmtl_conv2d_stats_rows")(32, 64, 128, 68), lib().raw("vmtl_conv2d_stats_block")(32, 64, 128, 68))
    monkeypatch.setattr(ops, "_MID_HALO", False)  # VMTL_MID_HALO=0
    assert plan(32, 64, 128, 68, 68, epilogue="stats").route != "mid_halo"
    assert plan(32, 64, 128, 68, 68, epilogue="stats")[2:] == igemm


def test_split_k_drops_the_epilogue_before_the_route_is_chosen(monkeypatch):
    """A launch that would split K loses its statistics / fused BatchNorm-backward epilogue first; its route is chosen
    after that, so a narrow layer that lost them still runs on the narrow halo-tile kernel (without an epilogue)."""
    # a real split: the tile-starved 130 -> 70 layer at 2 x 12 x 12 (decoder block 0 at small batch)
    p = ops.conv_plan(2, 12, 12, 132, 12, 12, 72, 3, 3, 1, 1, epilogue="stats")
    assert p.route == "ksplit" and p.ksplit > 1 and p.stats_rows == p.rpb == 0
    # no real shape both splits K (that needs a contraction of 32 K-steps of 32: over 113 input channels of a 3x3) and
    # fits the narrow halo-tile kernel (at most 36), so the split is stubbed on the 32 -> 16 layer at 65536 pixels
    narrow = (16, 64, 64, 32, 64, 64, 16, 3, 3, 1, 1)
    for ep in ("stats", "bnbwd"):
        p = ops.conv_plan(*narrow, epilogue=ep)
        assert p.route == "small" and p.ksplit == 1 and p.stats_rows * p.rpb == 16 * 64 * 64
    monkeypatch.setitem(lib()._fn, "vmtl_conv2d_ksplit", lambda *a: 2)
    for ep in (None, "stats", "bnbwd"):
        assert ops.conv_plan(*narrow, epilogue=ep) == ops.ConvPlan("small", 2, 0, 0)
    assert ops.conv_plan(16, 64, 64, 68, 64, 64, 68, 3, 3, 1, 1, epilogue="stats") == ops.ConvPlan("ksplit", 2, 0, 0)
