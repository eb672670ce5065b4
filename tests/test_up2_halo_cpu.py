"""Host-side contract of the UP2 halo-tile kernel (no GPU needed): the shape guard, the statistics geometry and the
argument checks that return before any launch."""
from vision_mtl_amd._lib import lib


def test_up2_halo_guard_and_geometry():
    L = lib()
    sup = L.raw("vmtl_conv2d_up2_halo_supported")
    assert sup(32, 64, 128, 68, 0, 36, 33) == 1 and sup(32, 32, 64, 136, 16, 68, 67) == 1
    assert sup(32, 64, 128, 68, 0, 36, 32) == 0 and sup(32, 32, 64, 136, 0, 68, 67) == 0 and sup(2, 8, 8, 40, 8, 36, 33) == 0
    assert sup(4096, 256, 256, 68, 0, 36, 33) == 0  # over 2 GiB: 32-bit offsets in the kernel
    rows, blk = L.raw("vmtl_conv2d_up2_halo_stat_rows"), L.raw("vmtl_conv2d_up2_halo_stat_block")
    assert blk(68, 0, 36, 33) == 256 and blk(136, 16, 68, 67) == 128  # 2*TM x 32 full-resolution pixels per tile
    assert rows(32, 64, 128, 68, 0, 36, 33) * 256 == 4 * 32 * 64 * 128
    assert rows(32, 32, 64, 136, 16, 68, 67) * 128 == 4 * 32 * 32 * 64
    assert rows(1, 7, 32, 68, 0, 36, 33) == 0 and rows(1, 4, 20, 136, 16, 68, 67) == 0  # partial tiles: no statistics


def test_up2_halo_argument_checks():
    f = lib().raw("vmtl_conv2d_up2_halo")
    assert f(None, None, None, None, None, 1, 4, 16, 68, 0, 36, 33, None) == -1  # null operands
    assert f(1, 1, 1, 1, None, 1, 4, 16, 68, 0, 36, 33, None) == -1  # skip given without skip channels
    assert f(1, None, 1, 1, None, 1, 4, 16, 72, 0, 36, 33, None) == -3  # not instantiated
    assert f(1, None, 1, 1, 1, 1, 3, 16, 68, 0, 36, 33, None) == -1  # statistics on partial tiles


def test_up2_statistics_geometry_follows_the_route():
    from vision_mtl_amd import ops

    assert ops.up2_plan(32, 64, 128, 68, 0, 36, 33, 0, True) == ops.ConvPlan("up2_halo", 1, 4096, 256)
    bm = lib().raw("vmtl_conv2d_up2_stats_block")(32, 64, 128, 36)
    assert ops.up2_plan(32, 64, 128, 68, 0, 36, 33, 1, True)[2:] == (4 * 32 * 64 * 128 // bm, bm)  # bf16: implicit GEMM
    assert ops.up2_plan(32, 64, 128, 68, 0, 36, 33, 0, False)[2:] == (0, 0)
