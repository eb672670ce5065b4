"""The user-selectable convolution precision without a GPU: the C ABI surface of the *_p entry points, the Python switch
(vision_mtl_amd.precision) and argument checking that happens before any launch."""
import ctypes

import pytest

P_ENTRY_POINTS = ["vmtl_conv2d_fwd_p", "vmtl_conv2d_fwd_ws_p", "vmtl_conv2d_bnbwd_p", "vmtl_conv2d_up2_fwd_p",
                  "vmtl_conv2d_up2_fwd_ws_p", "vmtl_conv2d_wgrad_p", "vmtl_conv1x1_cat_wgrad_p"]


def test_p_entry_points_declared_and_exported():
    from vision_mtl_amd._lib import HEADER, lib, parse_header

    protos = parse_header()
    L = lib()
    for name in P_ENTRY_POINTS:
        assert name in protos, f"{name} not declared in {HEADER}"
        legacy = protos[name[:-2]]
        _, argtypes, argnames = protos[name]
        # the namesake's arguments, plus `int precision` just before the stream
        assert argnames == legacy[2][:-1] + ["precision", "stream"], name
        assert argtypes[-2] is ctypes.c_int
        assert L.raw(name) is not None
    text = HEADER.read_text()
    assert "#define VMTL_PREC_FP32 0" in text and "#define VMTL_PREC_BF16 1" in text
    assert not any(n.startswith("VMTL_PREC") for n in protos)


def test_default_and_switching():
    import vision_mtl_amd as v

    assert v.get_conv_precision() == "fp32"
    with v.conv_precision("bf16"):
        assert v.get_conv_precision() == "bf16"
        with v.conv_precision("fp32"):
            assert v.get_conv_precision() == "fp32"
        assert v.get_conv_precision() == "bf16"
    assert v.get_conv_precision() == "fp32"
    v.set_conv_precision("bf16")
    try:
        assert v.get_conv_precision() == "bf16"
    finally:
        v.set_conv_precision("fp32")


def test_unknown_mode_raises():
    import vision_mtl_amd as v

    for bad in ("fp16", "tf32", "high", None, 1):
        with pytest.raises(ValueError):
            v.set_conv_precision(bad)
        with pytest.raises(ValueError):
            with v.conv_precision(bad):
                pass
    assert v.get_conv_precision() == "fp32"


def test_matmul_precision_is_not_consulted():
    import torch

    import vision_mtl_amd as v

    before = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("high")
        assert v.get_conv_precision() == "fp32"
    finally:
        torch.set_float32_matmul_precision(before)


def test_unknown_precision_value_returns_minus_one():
    """precision is checked first: a valid geometry with null pointers and precision 7 is refused before any launch"""
    from vision_mtl_amd._lib import lib

    L = lib()
    geo = (1, 8, 8, 8, 8, 8, 8, 8, 8, 3, 3, 1, 1)  # B H W Cs Ho Wo ldy Nw Cout KH KW stride pad
    assert L.raw("vmtl_conv2d_fwd_p")(None, None, None, None, None, *geo, 0, 0, 7, None) == -1
    assert L.raw("vmtl_conv2d_fwd_ws_p")(None, None, None, None, None, *geo, 7, None) == -1
    assert L.raw("vmtl_conv2d_bnbwd_p")(None, None, None, None, None, None, None, None, None, 0, *geo, 7, None) == -1
    assert L.raw("vmtl_conv2d_up2_fwd_p")(None, None, None, None, None, 1, 4, 4, 8, 8, 8, 8, 7, None) == -1
    assert L.raw("vmtl_conv2d_up2_fwd_ws_p")(None, None, None, None, None, 1, 4, 4, 8, 8, 8, 8, 7, None) == -1
    assert L.raw("vmtl_conv2d_wgrad_p")(None, None, None, 1, 1, 8, 8, 8, 8, 8, 8, 8, 3, 3, 1, 1, 7, None) == -1
    assert L.raw("vmtl_conv1x1_cat_wgrad_p")(None, 8, None, 8, None, None, 1, 64, 8, 8, 7, None) == -1
    for prec in (-1, 2, 7):
        assert L.raw("vmtl_conv2d_fwd_p")(None, None, None, None, None, *geo, 0, 0, prec, None) == -1


def test_fp32_calls_keep_legacy_names(monkeypatch):
    """fp32 mode launches the legacy entry points with their legacy keywords (bench.py sorts launches by name);
    only bf16 launches the _p variants"""
    from vision_mtl_amd import ops

    calls = []
    monkeypatch.setattr(ops, "_k", lambda name, _flop=None, _xflop=None, **kw: calls.append((name, sorted(kw))))
    ops._kp("vmtl_conv2d_wgrad", 0, _flop=1.0, x=1, dy=2)
    ops._kp("vmtl_conv2d_wgrad", 1, _flop=1.0, x=1, dy=2)
    assert calls == [("vmtl_conv2d_wgrad", ["dy", "x"]), ("vmtl_conv2d_wgrad_p", ["dy", "precision", "x"])]
