"""Host-side routing of the two-chunk prefetch (csrc/conv_igemm.hip PF = 2, csrc/conv_wgrad.hip PD = 2 on the tall tiles)
and of the weight gradient's row-group loader, through the library's two routing queries.  No GPU: plain host functions."""
import pytest

FP32, BF16 = 0, 1
TILE_64x144 = 11
MIN_CHUNKS = 4   # VMTL_IG_PIPE_MIN_CHUNKS' default: the peel alone is three chunks
MAX_GRID = 512   # two workgroups per CU


def _L():
    from vision_mtl_amd._lib import lib

    return lib()


def _depth(*a):
    return _L().raw("vmtl_conv2d_pipe_depth")(*a)  # (tile, Cs, C2s, nk, workgroups, up2, precision)


def _route(B, Ho, Wo, Nw, Cs=8, KH=3, stride=1, pad=1, prec=FP32):
    """(loader, peeled, PD, rows) of the weight gradient of a KHxKH conv with this OUTPUT map"""
    H, W = (Ho - 1) * stride + KH - 2 * pad, (Wo - 1) * stride + KH - 2 * pad
    r = _L().raw("vmtl_conv2d_wgrad_route")(B, H, W, Cs, Ho, Wo, Nw, KH, KH, stride, pad, prec)
    assert r >= 0
    return r & 3, (r >> 2) & 1, (r >> 3) & 7, r >> 6


def _depth_rule(tile, Cs, C2s, nk, grid, up2, prec, up2_on):
    ok = (prec == FP32 and tile == TILE_64x144 and Cs >= 32 and (not up2 or (up2_on and (C2s == 0 or C2s >= 32)))
          and nk >= MIN_CHUNKS and grid <= MAX_GRID)
    return 2 if ok else 1


@pytest.mark.parametrize("up2_on", [0, 1])
def test_depth_2_is_the_64x144_tile_with_wide_segments_long_k_and_a_small_grid(vmtl_env, up2_on):
    """the UP2 class is left off by default (it measured slower); VMTL_IG_PIPE_UP2=1 switches it on"""
    if up2_on:
        vmtl_env("VMTL_IG_PIPE_UP2", "1")
    for tile in range(16):
        for Cs in (4, 8, 28, 32, 36, 272, 1072):
            for C2s in (0, 4, 28, 32, 136):
                for nk in (1, 3, 4, 5, 76):
                    for grid in (1, 256, 512, 513, 4096):
                        for up2 in (0, 1):
                            for prec in (FP32, BF16):
                                a = (tile, Cs, C2s, nk, grid, up2, prec)
                                assert _depth(*a) == _depth_rule(*a, up2_on), a


def test_headline_decoder_blocks_0_and_1_take_depth_2(vmtl_env):
    """bs 32, 128x256: block 0 (540 channels, 8x16, split-K 2 -> 512 workgroups) and block 1 (270 channels, 16x32: 512
    workgroups) run the 64x144 tile; a plain 3x3 over 540 channels is 152 chunks, the UP2 form of block 1 gathers 540 + 40"""
    assert _depth(TILE_64x144, 540, 0, 76, 512, 0, FP32) == 2
    assert _depth(TILE_64x144, 272, 0, 77, 512, 0, FP32) == 2
    assert _depth(TILE_64x144, 540, 40, 79, 512, 1, FP32) == 1   # the UP2 class: off by default
    vmtl_env("VMTL_IG_PIPE_UP2", "1")
    assert _depth(TILE_64x144, 540, 40, 79, 512, 1, FP32) == 2
    assert _depth(TILE_64x144, 540, 16, 72, 512, 1, FP32) == 1   # a 16-channel skip: the straight-line K walk does not hold


def test_ig_pipe_switch_restores_the_one_chunk_loop(vmtl_env):
    vmtl_env("VMTL_IG_PIPE_UP2", "1")
    vmtl_env("VMTL_IG_PIPE", "0")
    for up2 in (0, 1):
        assert _depth(TILE_64x144, 540, 0, 76, 512, up2, FP32) == 1
    vmtl_env("VMTL_IG_PIPE", "1")
    for up2 in (0, 1):
        assert _depth(TILE_64x144, 540, 0, 76, 512, up2, FP32) == 2
    vmtl_env("VMTL_IG_PIPE_UP2", "0")
    assert _depth(TILE_64x144, 540, 0, 76, 512, 0, FP32) == 2
    assert _depth(TILE_64x144, 540, 0, 76, 512, 1, FP32) == 1
    vmtl_env("VMTL_IG_PIPE_MIN_CHUNKS", "1")
    assert _depth(TILE_64x144, 32, 0, 1, 4, 0, FP32) == 2


# (Ho, Wo) -> loader: 1 = whole output rows (Wo % 32 == 0), 2 = row group (Wo divides 32, Ho a multiple of 32 / Wo)
MAPS = {(4, 32): 1, (3, 64): 1, (8, 4): 2, (4, 8): 2, (2, 16): 2, (8, 16): 2, (16, 1): 0, (32, 1): 2, (16, 2): 2,
        (3, 16): 0, (7, 8): 0, (8, 12): 0, (8, 24): 0, (10, 20): 0, (8, 48): 0}


@pytest.mark.parametrize("rows,Nw", [(144, 150), (144, 540)])
def test_row_group_loader_on_the_144_row_tile(vmtl_env, rows, Nw):
    if Nw == 150:
        vmtl_env("VMTL_FORCE_WG_ROWS", rows)  # 150 rows would take two 80-row tiles
    for (Ho, Wo), want in MAPS.items():
        for KH, stride, pad in ((3, 1, 1), (4, 2, 1)):
            loader, _, _, r = _route(2, Ho, Wo, Nw, KH=KH, stride=stride, pad=pad)
            assert (loader, r) == (want, rows), (Ho, Wo, KH)
        assert _route(2, Ho, Wo, Nw, prec=BF16)[0] == (want if want == 1 else 0), (Ho, Wo)  # the bf16 tiles: no row groups
    vmtl_env("VMTL_WG_ROWGROUP", "0")
    for (Ho, Wo), want in MAPS.items():
        assert _route(2, Ho, Wo, Nw)[0] == (want if want == 1 else 0), (Ho, Wo)
    vmtl_env("VMTL_WG_ROWGROUP", "1")
    vmtl_env("VMTL_WG_FAST", "0")
    for (Ho, Wo) in MAPS:
        assert _route(2, Ho, Wo, Nw) == (0, 0, 1, rows), (Ho, Wo)


def test_other_tiles_keep_the_general_loader_on_narrow_maps():
    for Nw in (16, 20, 33, 48, 64, 67, 80, 128):  # 128: the 128-row tile has no row-group instantiation either
        for (Ho, Wo), want in MAPS.items():
            assert _route(2, Ho, Wo, Nw)[0] == (want if want == 1 else 0), (Nw, Ho, Wo)


def test_a_pointwise_conv_is_one_flat_row():
    for Ho, Wo in ((8, 4), (3, 16), (5, 32)):
        if (2 * Ho * Wo) % 32 == 0:
            assert _route(2, Ho, Wo, 150, Cs=40, KH=1, pad=0)[0] == 1, (Ho, Wo)


def test_tall_tiles_take_two_chunks_from_the_measured_slice_length(vmtl_env):
    vmtl_env("VMTL_WG_MIN_STEPS", "1")
    vmtl_env("VMTL_WG_PIPE_MIN_CHUNKS", "4")
    for rows, Nw in ((144, 150), (128, 128)):
        vmtl_env("VMTL_FORCE_WG_ROWS", rows)
        for splits, chunks in ((8, 1), (4, 2), (3, 3), (2, 4), (1, 8)):  # M = 256: eight chunks
            vmtl_env("VMTL_FORCE_WG_SPLITS", splits)
            for (Ho, Wo), loader in (((4, 32), 1), ((8, 16), 2 if rows == 144 else 0)):
                want = (loader, 1, 2, rows) if chunks >= 4 and loader else (loader, 0, 1, rows)
                assert _route(2, Ho, Wo, Nw) == want, (rows, chunks, Ho, Wo)
            assert _route(2, 4, 32, Nw, prec=BF16) == (1, 0, 1, rows)      # bf16: the registers are not there
            assert _route(2, 8, 20, Nw) == (0, 0, 1, rows)                 # the general loader keeps its guards
    vmtl_env("VMTL_FORCE_WG_SPLITS", 1)
    vmtl_env("VMTL_WG_PIPE", "0")
    for rows, Nw in ((144, 150), (128, 128)):
        vmtl_env("VMTL_FORCE_WG_ROWS", rows)
        assert _route(2, 4, 32, Nw) == (1, 0, 1, rows)
        assert _route(2, 8, 16, Nw) == (2 if rows == 144 else 0, 0, 1, rows)
    vmtl_env("VMTL_WG_PIPE", "1")
    for mask, on in ((0, ()), (1, (144,)), (2, (128,)), (3, (128, 144))):
        vmtl_env("VMTL_WG_PIPE_TALL", mask)
        for rows, Nw in ((144, 150), (128, 128)):
            vmtl_env("VMTL_FORCE_WG_ROWS", rows)
            assert _route(2, 4, 32, Nw)[1:3] == ((1, 2) if rows in on else (0, 1)), (mask, rows)


def test_measured_minimum_slice_lengths(vmtl_env):
    """the 144-row tile takes two chunks from 4-chunk slices, the 128-row tile from 6 (the measured crossovers)"""
    vmtl_env("VMTL_WG_MIN_STEPS", "1")
    for rows, Nw, first in ((144, 150, 4), (128, 128, 6)):
        vmtl_env("VMTL_FORCE_WG_ROWS", rows)
        for splits, chunks in ((8, 3), (6, 4), (5, 5), (4, 6), (3, 8)):  # M = 768: 24 chunks
            vmtl_env("VMTL_FORCE_WG_SPLITS", splits)
            assert _route(6, 4, 32, Nw) == ((1, 1, 2, rows) if chunks >= first else (1, 0, 1, rows)), (rows, chunks)


def test_narrow_tiles_route_as_before(vmtl_env):
    """PD = 3 tiles: the peeled loop with the scalar-chunk loader; PD = 2 (48 / 64 rows) and 68 / 80 rows: guarded"""
    for Nw, rows, pd, peeled in ((16, 16, 3, 1), (20, 20, 3, 1), (32, 32, 3, 1), (33, 36, 3, 1), (48, 48, 2, 0), (64, 64, 2, 0),
                                 (67, 68, 1, 0), (80, 80, 1, 0)):
        assert _route(2, 16, 32, Nw) == (1, peeled, pd, rows), Nw
        assert _route(2, 10, 20, Nw) == (0, 0, pd, rows), Nw
    vmtl_env("VMTL_WG_PIPE", "0")
    for Nw in (16, 20, 32, 33):
        assert _route(2, 16, 32, Nw)[1] == 0


def test_bad_arguments():
    assert _L().raw("vmtl_conv2d_wgrad_route")(0, 4, 4, 8, 4, 4, 8, 3, 3, 1, 1, FP32) == -1
    assert _L().raw("vmtl_conv2d_wgrad_route")(1, 4, 4, 8, 4, 4, 8, 3, 3, 1, 1, 7) == -1
