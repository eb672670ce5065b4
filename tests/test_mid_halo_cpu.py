"""Host-side contract of the mid-width halo-tile conv (vmtl_conv3x3_halo, no GPU needed): the shape guard, the statistics
geometry, the routing rule and the argument checks that return before any launch."""
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
    # the bs-32 `basic` block-3 layers (68 -> 67 and 68 -> 16 at 64 x 128) and MTAN's 64 -> 64 at 128 x 128
    assert ops._mid_halo_route(32, 64, 128, 68, 68, 3, 3, 1, 1, with_stats=True, prec=0)
    assert ops._mid_halo_route(32, 64, 128, 68, 16, 3, 3, 1, 1, prec=0)
    assert ops._mid_halo_route(16, 128, 128, 64, 64, 3, 3, 1, 1, with_stats=True, prec=0)
    assert ops.conv_stats_geometry(32, 64, 128, 68, 68, 3, 3, 1, 1) == (2048, 128)
    assert not ops._mid_halo_route(32, 64, 128, 68, 68, 3, 3, 1, 1, prec=1)  # bf16 stays on the implicit GEMM
    assert not ops._mid_halo_route(32, 64, 128, 68, 68, 3, 3, 2, 1, prec=0)
    assert not ops._mid_halo_route(32, 64, 128, 68, 68, 1, 1, 1, 0, prec=0)
    assert not ops._mid_halo_route(2, 64, 64, 68, 68, 3, 3, 1, 1, prec=0)  # too few pixels
    assert not ops._mid_halo_route(32, 66, 128, 68, 68, 3, 3, 1, 1, with_stats=True, prec=0)  # partial tiles
    igemm = (lib().raw("vmtl_conv2d_stats_rows")(32, 64, 128, 68), lib().raw("vmtl_conv2d_stats_block")(32, 64, 128, 68))
    monkeypatch.setattr(ops, "_MID_HALO", False)  # VMTL_MID_HALO=0
    assert not ops._mid_halo_route(32, 64, 128, 68, 68, 3, 3, 1, 1, with_stats=True, prec=0)
    assert ops.conv_stats_geometry(32, 64, 128, 68, 68, 3, 3, 1, 1) == igemm
