"""Host side of the strip-walking weight gradient (csrc/conv_wgrad_small.hip): which layers it takes and how many slabs it
asks for.  No GPU: the three queries are plain host functions of the library."""
import pytest


def _q():
    from vision_mtl_amd._lib import lib

    L = lib()
    return (L.raw("vmtl_conv3x3_wgrad_small_supported"), L.raw("vmtl_conv3x3_wgrad_small_slabs"),
            L.raw("vmtl_conv3x3_wgrad_small_slabs_for"))


def _routed():
    from vision_mtl_amd._lib import lib

    return lib().raw("vmtl_conv3x3_wgrad_small_supported_p")  # (Cs, ldy, W, pixels, precision)


def _narrow_rule(Cs, ldy, W):
    """supported() before the tail rows and the 80-float pixels"""
    return (4 <= Cs <= 36 and Cs % 4 == 0 and 4 <= ldy <= 36 and ldy % 4 == 0 and not (Cs > 32 and ldy > 32)
            and W >= 32 and W % 32 == 0)


# the headline's (basic, 128x256, bs 32) four layers of DESIGN.md section 9: (Cs, ldy, W) -> on the strip kernel (now, before)
HEADLINE = {"blk4.conv2 33->33": ((36, 36, 256), 1, 0),
            "heads 33->20": ((36, 20, 256), 1, 1),
            "blk3.conv1 skip half 16->67": ((16, 68, 128), 1, 0),
            "blk3.conv2 67->67": ((68, 68, 128), 1, 0)}


@pytest.mark.parametrize("W", [32, 64, 256])
def test_slabs_for_equals_slabs_on_every_narrow_pair(W):
    _, slabs, slabs_for = _q()
    for B, H in ((1, 1), (1, 5), (2, 9), (3, 70), (16, 256), (32, 128), (64, 33)):
        old = slabs(B, H, W)
        assert old > 0
        for Cs in range(4, 37, 4):
            for ldy in range(4, 37, 4):
                for Nw in {1, ldy - 3, ldy}:
                    assert slabs_for(B, H, W, Cs, ldy, Nw) == old, (B, H, W, Cs, ldy, Nw)


def test_slabs_for_runs_fewer_segments_on_a_wide_layer_and_rejects_nonsense():
    _, slabs, slabs_for = _q()
    assert 0 < slabs_for(32, 64, 128, 68, 68, 67) < slabs(32, 64, 128)
    assert 0 < slabs_for(32, 64, 128, 16, 68, 67) < slabs(32, 64, 128)
    for bad in ((0, 8, 32, 16, 16, 16), (1, 0, 32, 16, 16, 16), (1, 8, 48, 16, 16, 16), (1, 8, 16, 16, 16, 16),
                (1, 8, 32, 0, 16, 16), (1, 8, 32, 16, 0, 1), (1, 8, 32, 16, 16, 0)):
        assert slabs_for(*bad) == 0, bad


def test_every_shape_accepted_before_is_still_accepted(vmtl_env):
    supported, _, _ = _q()
    for wide in ("1", "0"):
        vmtl_env("VMTL_WGRAD_SMALL_WIDE", wide)
        for W in (32, 64, 96, 256, 1024):
            for Cs in range(4, 37, 4):
                for ldy in range(4, 37, 4):
                    if _narrow_rule(Cs, ldy, W):
                        assert supported(Cs, ldy, W) == 1, (wide, Cs, ldy, W)


def test_refused_shapes(vmtl_env):
    supported, _, _ = _q()
    for wide in ("1", "0"):
        vmtl_env("VMTL_WGRAD_SMALL_WIDE", wide)
        for W in (0, 16, 31, 33, 48, 80, 250):  # not a multiple of the 32-pixel strip
            for Cs, ldy in ((16, 16), (36, 36), (68, 68), (16, 68)):
                assert supported(Cs, ldy, W) == 0, (wide, Cs, ldy, W)
        for Cs, ldy in ((0, 16), (16, 0), (3, 16), (16, 3), (33, 33), (18, 16), (16, 38), (67, 67), (66, 16),   # not quads
                        (72, 16), (16, 72), (72, 72), (136, 136), (68, 136), (1072, 540)):                   # above 68
            assert supported(Cs, ldy, 64) == 0, (wide, Cs, ldy)


def test_headline_layers_resolve_to_the_routes_of_the_design_table(vmtl_env):
    supported, _, _ = _q()
    routed = _routed()
    for name, ((Cs, ldy, W), now, before) in HEADLINE.items():
        pixels = 32 * (W // 2) * W  # bs 32, 128x256 and 64x128
        assert routed(Cs, ldy, W, pixels, 0) == now, name
        assert supported(Cs, ldy, W) == now, name
    vmtl_env("VMTL_WGRAD_SMALL_WIDE", "0")
    for name, ((Cs, ldy, W), now, before) in HEADLINE.items():
        assert routed(Cs, ldy, W, 32 * (W // 2) * W, 0) == supported(Cs, ldy, W) == before, name
        assert before == int(_narrow_rule(Cs, ldy, W)), name


def test_wide_switch_restores_the_narrow_rule_everywhere(vmtl_env):
    supported, _, _ = _q()
    vmtl_env("VMTL_WGRAD_SMALL_WIDE", "0")
    for W in (32, 48, 128):
        for Cs in range(0, 81, 4):
            for ldy in range(0, 81, 4):
                assert supported(Cs, ldy, W) == int(_narrow_rule(Cs, ldy, W)), (Cs, ldy, W)
    vmtl_env("VMTL_WGRAD_SMALL", "0")  # the general kernel everywhere
    vmtl_env("VMTL_WGRAD_SMALL_WIDE", "1")
    for Cs, ldy in ((16, 16), (36, 36), (68, 68)):
        assert supported(Cs, ldy, 64) == 0


def _routes(monkeypatch, shape, Nw, prec):
    """The launches ops._wgrad issues for a (B, H, W, Cs, ldy) 3x3 layer, recorded instead of run (CPU tensors)."""
    import torch

    from vision_mtl_amd import ops

    B, H, W, Cs, ldy = shape
    seen = []
    monkeypatch.setattr(ops, "_k", lambda name, _flop=None, _xflop=None, **kw: seen.append((name, kw)))
    x, dy = torch.zeros(B, H, W, Cs), torch.zeros(B, H, W, ldy)
    slabs, ns = ops._wgrad(x, dy, ops.ConvGeom.of(x.shape, ldy, 3, 3, 1, 1), Nw=Nw, flop=1.0, prec=prec)
    assert len(seen) == 1 and slabs.shape == (ns, Nw, 9 * Cs)
    return seen[0][0], seen[0][1], ns


# (B, H, W, Cs, ldy), Nw: the headline's four layers and MTAN's 64 -> 64, at the 65,536 pixels from which the classes added
# last are routed to the strip kernel
ROUTED = [((1, 256, 256, 36, 36), 33), ((1, 256, 256, 36, 20), 20), ((1, 256, 256, 16, 68), 67), ((1, 256, 256, 68, 68), 67),
          ((1, 256, 256, 64, 64), 64)]


@pytest.mark.parametrize("shape,Nw", ROUTED)
def test_fp32_weight_gradients_take_the_strip_kernel_with_this_layers_slab_count(monkeypatch, vmtl_env, shape, Nw):
    _, _, slabs_for = _q()
    name, kw, ns = _routes(monkeypatch, shape, Nw, 0)
    B, H, W, Cs, ldy = shape
    assert name == "vmtl_conv3x3_wgrad_small"
    assert ns == kw["nslabs"] == slabs_for(B, H, W, Cs, ldy, Nw)
    vmtl_env("VMTL_WGRAD_SMALL_WIDE", "0")
    name, _, _ = _routes(monkeypatch, shape, Nw, 0)
    assert name == ("vmtl_conv3x3_wgrad_small" if _narrow_rule(Cs, ldy, W) else "vmtl_conv2d_wgrad")


@pytest.mark.parametrize("shape,Nw", ROUTED)
def test_small_maps_stay_where_they_were(monkeypatch, vmtl_env, shape, Nw):
    """Below 65,536 pixels (never measured; the wide geometry has fewer workgroups than CUs) the classes added last stay on
    the dense kernel; VMTL_WS_WIDE_MIN_PIXELS moves the bound (the GPU tests run those classes at a few thousand pixels)."""
    B, H, W, Cs, ldy = shape
    small = (B, H // 2, W, Cs, ldy)
    name, _, _ = _routes(monkeypatch, small, Nw, 0)
    assert name == ("vmtl_conv3x3_wgrad_small" if _narrow_rule(Cs, ldy, W) else "vmtl_conv2d_wgrad")
    vmtl_env("VMTL_WS_WIDE_MIN_PIXELS", "1")
    assert _routes(monkeypatch, small, Nw, 0)[0] == "vmtl_conv3x3_wgrad_small"
    assert _routes(monkeypatch, (1, 8, 32, Cs, ldy), Nw, 0)[0] == "vmtl_conv3x3_wgrad_small"


@pytest.mark.parametrize("shape,Nw", ROUTED)
def test_bf16_weight_gradients_stay_where_they_were(monkeypatch, vmtl_env, shape, Nw):
    """The strip kernel is fp32.  In a bf16 mode it keeps the layers it had (bf16 on conv_wgrad_kernel measured slower
    there); the classes the tail rows and 80-float pixels opened were measured against the fp32 dense kernel only, so
    their bf16 launches stay on vmtl_conv2d_wgrad_p - at every size."""
    supported, _, _ = _q()
    routed = _routed()
    B, H, W, Cs, ldy = shape
    for min_pixels in (None, "1"):
        if min_pixels:
            vmtl_env("VMTL_WS_WIDE_MIN_PIXELS", min_pixels)
        name, kw, _ = _routes(monkeypatch, shape, Nw, 1)
        if _narrow_rule(Cs, ldy, W):
            assert name == "vmtl_conv3x3_wgrad_small" and routed(Cs, ldy, W, B * H * W, 1) == 1
        else:
            assert name == "vmtl_conv2d_wgrad_p" and kw["precision"] == 1 and routed(Cs, ldy, W, B * H * W, 1) == 0
        assert routed(Cs, ldy, W, B * H * W, 0) == supported(Cs, ldy, W) == 1


def test_routing_at_bf16_is_the_narrow_rule():
    routed = _routed()
    for W in (32, 48, 128):
        for Cs in range(0, 81, 4):
            for ldy in range(0, 81, 4):
                for pixels in (1, 1 << 16, 1 << 24):
                    assert routed(Cs, ldy, W, pixels, 1) == int(_narrow_rule(Cs, ldy, W)), (Cs, ldy, W, pixels)
                assert routed(Cs, ldy, W, (1 << 16) - 1, 0) == int(_narrow_rule(Cs, ldy, W)), (Cs, ldy, W)
