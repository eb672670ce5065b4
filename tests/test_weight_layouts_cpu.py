"""ops.Layout / ops.ConvGeom against the literal integers the autograd nodes of ops.py wrote out by hand before these
types existed.  The literals are data: each is the ten-tuple (R1, R0, T, C, Cs, sr1, sr0, st, sc, flip) or the positional
geometry run of the named node, for the shapes below.  No GPU, no library: pure integer arithmetic."""
import pytest


def _ops():
    from vision_mtl_amd import ops
    return ops


# Cin not a multiple of 4; a 1x1 and a 3x3 kernel
COUT, CIN, CS, LDY = 19, 67, 68, 20


@pytest.mark.parametrize("KK", [1, 9])
def test_dense_layouts(KK):
    L = _ops().Layout
    # _Conv2d.forward / _BNActConv.forward (KK = 9) / _BNActPw.forward (KK = 1): packs.get(weight, "fwd", ...)
    assert L.fwd(COUT, CIN, KK, CS) == (1, COUT, KK, CIN, CS, 0, CIN * KK, 1, KK, 0)
    # _Conv2d.backward / _BNActConv.backward / _BNActPw.backward: packs.get(weight, "dgrad", ...)
    assert L.dgrad(COUT, CIN, KK, LDY) == (1, CIN, KK, COUT, LDY, 0, KK, 1, CIN * KK, 1)


def test_dense_layouts_literal_numbers():
    L = _ops().Layout
    assert L.fwd(19, 67, 9, 68) == (1, 19, 9, 67, 68, 0, 603, 1, 9, 0)
    assert L.dgrad(19, 67, 9, 20) == (1, 67, 9, 19, 20, 0, 9, 1, 603, 1)
    assert L.fwd(19, 67, 1, 68) == (1, 19, 1, 67, 68, 0, 67, 1, 1, 0)  # _BNActPw: (1, Cout, 1, Cin, Cs, 0, Cin, 1, 1, 0)
    assert L.dgrad(19, 67, 1, 20) == (1, 67, 1, 19, 20, 0, 1, 1, 67, 1)  # _BNActPw: (1, Cin, 1, Cout, ldy, 0, 1, 1, Cin, 1)


def test_layout_is_a_plain_tuple_to_its_consumers():
    import struct

    L = _ops().Layout
    lay = L.fwd(COUT, CIN, 9, CS)
    lit = (1, COUT, 9, CIN, CS, 0, CIN * 9, 1, 9, 0)
    assert hash(lay) == hash(lit) and {lit: 1}[lay] == 1  # _PackCache keys
    assert (0, "fwd", lay, 0) == (0, "fwd", lit, 0)
    R1, R0, T, C, Cs, sr1, sr0, st, sc, flip = lay  # _build_table / pack(src, *params)
    assert struct.pack("<qqqqiiiiii", sr1, sr0, st, sc, R1, R0, T, C, Cs, flip) == struct.pack(
        "<qqqqiiiiii", *lit[5:9], *lit[:5], lit[9])
    assert (lay.R1, lay.R0, lay.T, lay.C, lay.Cs, lay.sr1, lay.sr0, lay.st, lay.sc, lay.flip) == lit


def test_conv1x1_cat_layouts():
    L = _ops().Layout
    Cout, Ca, Cb = 19, 64, 35
    Cin, Ks, ldy = Ca + Cb, Ca + 36, 20
    assert L.fwd(Cout, Cin, 1, Ks) == (1, Cout, 1, Cin, Ks, 0, Cin, 1, 1, 0)  # _Conv1x1Cat.forward, and its unpack
    assert L.dgrad(Cout, Cin, 1, ldy) == (1, Cin, 1, Cout, ldy, 0, 1, 1, Cin, 1)  # _Conv1x1Cat.backward


def test_conv_transpose_layouts():
    L = _ops().Layout
    Cin, Cout = 64, 32
    Cs, ldy = 64, 32
    assert L.ct_fwd(Cin, Cout, Cs) == (4, Cout, 1, Cin, Cs, 1, 4, 0, Cout * 4, 0)  # _ConvT2x2.forward "ct_fwd"
    assert L.ct_fwd(64, 32, 64) == (4, 32, 1, 64, 64, 1, 4, 0, 128, 0)
    # _ConvT2x2.backward "ct_bwd", and the unpack of its weight gradient (1, Cin, 4, Cout, ldy, 0, Cout * 4, 1, 4)
    assert L.ct_bwd(Cin, Cout, ldy) == (1, Cin, 4, Cout, ldy, 0, Cout * 4, 1, 4, 0)
    assert L.ct_bwd(64, 32, 32) == (1, 64, 4, 32, 32, 0, 128, 1, 4, 0)


def test_depthwise_and_vector_layouts():
    L = _ops().Layout
    C, K, Cs = 72, 5, 72
    assert L.dw(C, K, Cs) == (1, 1, K * K, C, Cs, 0, 0, 1, K * K, 0)  # _DwConv.forward / _BNActDw.forward "dw"
    assert L.dw(72, 5, 72) == (1, 1, 25, 72, 72, 0, 0, 1, 25, 0)
    assert L.dw(18, 3, 20) == (1, 1, 9, 18, 20, 0, 0, 1, 9, 0)
    # _DecoderTail.forward "heads_bias"; _copy_vec's R1=1, R0=1, T=1, C=n, Cs=n, sr1=0, sr0=0, st=0, sc=1, flip=0
    assert L.vec(19) == (1, 1, 1, 19, 19, 0, 0, 0, 1, 0)
    assert L.vec(1) == (1, 1, 1, 1, 1, 0, 0, 0, 1, 0)


def test_up2_skip_slice_layouts():
    """the skip channels [C0, Cin) of an UP2 conv's (Cout, Cin, 3, 3) weight, read with offset = C0 * 9"""
    L = _ops().Layout
    Cout, Cin, C0 = 19, 67 + 24, 24
    C1, C1s, ldy = Cin - C0, 68, 20
    # _up2_dskip: packs.get(weight, "up2_dskip", ..., offset=C0 * 9)
    assert L.dgrad(Cout, C1, 9, ldy, Cw=Cin) == (1, C1, 9, Cout, ldy, 0, 9, 1, Cin * 9, 1)
    # _up2_wgrad: unpack(slabs, None, 1, Cout, 9, C1, C1s, 0, Cin * 9, 1, 9, out=dw.view(-1)[C0 * 9:])
    assert L.fwd(Cout, C1, 9, C1s, Cw=Cin) == (1, Cout, 9, C1, C1s, 0, Cin * 9, 1, 9, 0)
    assert L.fwd(19, 67, 9, 68, Cw=91) == (1, 19, 9, 67, 68, 0, 819, 1, 9, 0)


def test_head_group_and_squeeze_excite_layouts():
    L = _ops().Layout
    Ca, Cb, C2, ldy2 = 19, 1, 16, 16
    ldyh = 20
    # _DecoderTail.forward "heads_fwd" (per head, rows of the group operand are 9 * ldy2 wide) and its two unpacks
    assert L.fwd(Ca, C2, 9, ldy2) == (1, Ca, 9, C2, ldy2, 0, C2 * 9, 1, 9, 0)
    assert L.fwd(Cb, C2, 9, ldy2) == (1, Cb, 9, C2, ldy2, 0, C2 * 9, 1, 9, 0)
    # _DecoderTail.backward pack_heads_dgrad: pack(w, 1, C2, 9, Ca, ldyh, 0, 9, 1, C2 * 9, flip=1)
    assert L.dgrad(Ca, C2, 9, ldyh) == (1, C2, 9, Ca, ldyh, 0, 9, 1, C2 * 9, 1)
    # _DualHead: pack(wa, 1, Ca, KK, Cin, Cs, 0, Cin * KK, 1, KK) / pack(wa, 1, Cin, KK, Ca, ldy, 0, KK, 1, Cin * KK, flip=1)
    Cin, Cs, KK = 67, 68, 9
    assert L.fwd(Ca, Cin, KK, Cs) == (1, Ca, KK, Cin, Cs, 0, Cin * KK, 1, KK, 0)
    assert L.dgrad(Ca, Cin, KK, ldyh) == (1, Cin, KK, Ca, ldyh, 0, KK, 1, Cin * KK, 1)
    # _SqueezeExcite.backward: the (C, R, 1, 1) expand and (R, C, 1, 1) reduce weights, transposed
    C, R, Cs, Rs = 72, 24, 72, 24
    assert L.dgrad(C, R, 1, Cs) == (1, R, 1, C, Cs, 0, 1, 1, R, 1)
    assert L.dgrad(R, C, 1, Rs) == (1, C, 1, R, Rs, 0, 1, 1, C, 1)


def test_conv_geom():
    G = _ops().ConvGeom
    g = G(2, 12, 20, 68, 12, 20, 20, 3, 3, 1, 1)
    assert g.M == 2 * 12 * 20
    # _Conv2d.backward: _conv_launch(dy, wd, None, dx, B, Ho, Wo, ldy, H, W, Cs, Cin, Cin, KH, KW, 1, KH - 1 - pad, ...)
    assert g.dgrad() == (2, 12, 20, 20, 12, 20, 68, 3, 3, 1, 1)
    # 1x1 / pad 0
    g1 = G(2, 12, 20, 68, 12, 20, 20, 1, 1, 1, 0)
    assert g1.dgrad() == (2, 12, 20, 20, 12, 20, 68, 1, 1, 1, 0)
    # a non-square 3x3 with pad 0 ("valid"): the data gradient pads by K - 1
    g2 = G(3, 9, 14, 16, 7, 12, 8, 3, 3, 1, 0)
    assert g2.M == 3 * 7 * 12
    assert g2.dgrad() == (3, 7, 12, 8, 9, 14, 16, 3, 3, 1, 2)
    assert g2.dgrad().M == 3 * 9 * 14
    with pytest.raises(AssertionError):  # a strided conv has no stride-1 data-gradient geometry
        G(2, 12, 20, 68, 6, 10, 20, 3, 3, 2, 1).dgrad()
    # the output extent conv2d / _Conv2d.forward computed: (H + 2 * pad - K) // stride + 1
    assert G.of((2, 12, 20, 68), 20, 3, 3, 1, 1) == g
    assert G.of((2, 13, 21, 4), 64, 7, 7, 2, 3) == (2, 13, 21, 4, 7, 11, 64, 7, 7, 2, 3)
    assert G.of((3, 9, 14, 16), 8, 3, 3) == g2
    # conv_plan(**geo) of the parent's _BNActConv.backward: the field names are conv_plan's parameter names, in order
    assert tuple(g._asdict()) == ("B", "H", "W", "Cs", "Ho", "Wo", "ldy", "KH", "KW", "stride", "pad")
