"""The "bf16_pw" precision mode without a GPU: the C ABI surface of the pointwise *_p entry points, the Python switch
(vision_mtl_amd.precision: a third mode that is routing only - the C ABI keeps two precision values) and the argument
checking that happens before any launch."""
import ctypes

import pytest

PW_P_ENTRY_POINTS = ["vmtl_conv1x1_fwd_p", "vmtl_conv1x1_cat_fwd_p", "vmtl_conv1x1_cat_dgrad_p", "vmtl_conv1x1_bn_fwd_p",
                     "vmtl_conv1x1_bn_res_fwd_p", "vmtl_conv1x1_bnbwd_p", "vmtl_conv1x1_bnbwd_add_p"]


def test_pw_p_entry_points_declared_and_exported():
    from vision_mtl_amd._lib import HEADER, lib, parse_header

    protos = parse_header()
    L = lib()
    for name in PW_P_ENTRY_POINTS:
        assert name in protos, f"{name} not declared in {HEADER}"
        legacy = protos[name[:-2]]
        _, argtypes, argnames = protos[name]
        # the namesake's arguments, plus `int precision` just before the stream
        assert argnames == legacy[2][:-1] + ["precision", "stream"], name
        assert argtypes[-2] is ctypes.c_int
        assert L.raw(name) is not None
    # the statistics geometry takes no precision
    for name in ("vmtl_conv1x1_stats_block", "vmtl_conv1x1_stats_rows"):
        assert protos[name][2] == ["M", "ldy", "Ks", "variant"] and name + "_p" not in protos
    text = HEADER.read_text()
    assert "#define VMTL_PREC_FP32 0" in text and "#define VMTL_PREC_BF16 1" in text
    assert text.count("#define VMTL_PREC_") == 2  # "bf16_pw" is not a third C value


@pytest.mark.parametrize("prec", [-1, 2, 7])
def test_unknown_precision_value_returns_minus_one(prec):
    """precision is checked first: a valid geometry with null pointers is refused with -1 before any launch"""
    from vision_mtl_amd._lib import lib

    raw = lib().raw
    M, Ks, ldy, Nw, Cout = 64, 16, 8, 8, 8
    N = None
    assert raw("vmtl_conv1x1_fwd_p")(N, N, N, N, N, M, Ks, ldy, Nw, Cout, prec, N) == -1
    assert raw("vmtl_conv1x1_cat_fwd_p")(N, 8, N, 8, N, N, N, N, M, ldy, Nw, Cout, prec, N) == -1
    assert raw("vmtl_conv1x1_cat_dgrad_p")(N, N, N, 8, N, 8, 7, M, Ks, prec, N) == -1
    assert raw("vmtl_conv1x1_bn_fwd_p")(N, N, N, 1, N, N, N, N, N, M, Ks, ldy, Nw, Cout, prec, N) == -1
    assert raw("vmtl_conv1x1_bn_res_fwd_p")(N, N, N, 0, N, N, N, N, N, N, M, Ks, ldy, Nw, Cout, prec, N) == -1
    assert raw("vmtl_conv1x1_bnbwd_p")(N, N, N, N, N, N, N, N, N, 1, M, Ks, ldy, Nw, Cout, prec, N) == -1
    assert raw("vmtl_conv1x1_bnbwd_add_p")(N, N, N, N, N, N, N, N, N, N, 0, M, Ks, ldy, Nw, Cout, prec, N) == -1


def test_bf16_pw_switches_nests_and_restores():
    import vision_mtl_amd as v

    assert v.get_conv_precision() == "fp32"
    with v.conv_precision("bf16_pw"):
        assert v.get_conv_precision() == "bf16_pw"
        with v.conv_precision("bf16"):
            assert v.get_conv_precision() == "bf16"
            with v.conv_precision("bf16_pw"):
                assert v.get_conv_precision() == "bf16_pw"
            assert v.get_conv_precision() == "bf16"
        with v.conv_precision("fp32"):
            assert v.get_conv_precision() == "fp32"
        assert v.get_conv_precision() == "bf16_pw"
    assert v.get_conv_precision() == "fp32"
    v.set_conv_precision("bf16_pw")
    try:
        assert v.get_conv_precision() == "bf16_pw"
        with pytest.raises(ValueError):
            v.set_conv_precision("bf16_pointwise")
        assert v.get_conv_precision() == "bf16_pw"
    finally:
        v.set_conv_precision("fp32")
    with pytest.raises(RuntimeError):
        with v.conv_precision("bf16_pw"):
            raise RuntimeError("restored on the way out")
    assert v.get_conv_precision() == "fp32"


def test_precision_codes_per_mode():
    import vision_mtl_amd as v
    from vision_mtl_amd.precision import conv_prec_code, pw_prec_code

    assert (conv_prec_code(), pw_prec_code()) == (0, 0)  # the default is still fp32
    for mode, codes in (("fp32", (0, 0)), ("bf16", (1, 0)), ("bf16_pw", (1, 1))):
        with v.conv_precision(mode):
            assert (conv_prec_code(), pw_prec_code()) == codes, mode
    assert (conv_prec_code(), pw_prec_code()) == (0, 0)


def test_pointwise_launches_keep_legacy_names_in_fp32(monkeypatch):
    """a pointwise launch issued with code 0 (the "fp32" and "bf16" modes) uses the legacy entry point and keywords
    (bench.py and tools/step_table.py sort launches by name); code 1 ("bf16_pw") the _p variant plus `precision`"""
    from vision_mtl_amd import ops

    calls = []
    monkeypatch.setattr(ops, "_k", lambda name, _flop=None, _xflop=None, **kw: calls.append((name, dict(kw))))
    kw = dict(x=1, wp=2, bias=None, y=3, stats=None, M=64, Ks=16, ldy=8, Nw=8, Cout=8)
    for name in ("vmtl_conv1x1_fwd", "vmtl_conv1x1_bn_fwd", "vmtl_conv1x1_cat_dgrad"):
        calls.clear()
        ops._kp(name, 0, _flop=1.0, **kw)
        ops._kp(name, 1, _flop=1.0, **kw)
        assert calls == [(name, kw), (name + "_p", dict(kw, precision=1))]


def test_conv_launch_routes_the_pointwise_precision(monkeypatch):
    """ops._conv_launch on the "pw" route issues vmtl_conv1x1_fwd under the POINTWISE code, whatever the convolution code"""
    from vision_mtl_amd import ops

    calls = []
    monkeypatch.setattr(ops, "_k", lambda name, _flop=None, _xflop=None, **kw: calls.append((name, kw.get("precision"))))
    plan = ops.ConvPlan("pw", 1, 0, 0)
    geo = ops.ConvGeom(2, 6, 9, 16, 6, 9, 12, 1, 1, 1, 0)  # B H W Cs Ho Wo ldy KH KW stride pad
    for prec, pw_prec, want in ((0, 0, ("vmtl_conv1x1_fwd", None)), (1, 0, ("vmtl_conv1x1_fwd", None)),
                                (1, 1, ("vmtl_conv1x1_fwd_p", 1))):
        calls.clear()
        ops._conv_launch(None, None, None, None, geo, Cout=10, Nw=10, prec=prec, plan=plan, pw_prec=pw_prec)
        assert calls == [want], (prec, pw_prec)
