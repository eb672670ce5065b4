"""Host-side contract of the split-K entry points of the implicit-GEMM convolutions (no GPU needed): the arguments are
validated before the K split is decided, so a bad extent is answered with a status and never reaches the split's
division by the tile count.  Pointers are dummy non-null values; every call returns before any launch."""
import pytest

from vision_mtl_amd._lib import lib

ERR_ARG = -1

# 1 x 8 x 8 x 128 -> 64, 3x3 / s1 / p1: Ktot = 1152 = 36 K steps, so the split is reached (it starts at 32)
#        B  H  W  Cs   Ho Wo ldy Nw  Cout KH KW stride pad
PLAIN = (1, 8, 8, 128, 8, 8, 64, 64, 64, 3, 3, 1, 1)
# 1 x 6 x 8 low-res pixels, 240 + 40 -> 70: Ktot = 4 * 240 + 9 * 40 = 1320 = 42 K steps
#      B  H2 W2 C0s  C1s ldy Cout
UP2 = (1, 6, 8, 240, 40, 72, 70)


def _with(base, names, **kw):
    a = dict(zip(names, base))
    a.update(kw)
    return tuple(a[n] for n in names)


def _plain(**kw):
    return _with(PLAIN, ("B", "H", "W", "Cs", "Ho", "Wo", "ldy", "Nw", "Cout", "KH", "KW", "stride", "pad"), **kw)


def _up2(**kw):
    return _with(UP2, ("B", "H2", "W2", "C0s", "C1s", "ldy", "Cout"), **kw)


def test_base_shapes_reach_the_split():
    assert lib().raw("vmtl_conv2d_ksplit")(1, 8, 8, 64, 1152) > 1
    assert lib().raw("vmtl_conv2d_up2_ksplit")(1, 6, 8, 72, 1320) > 1


@pytest.mark.parametrize("name,args", [
    ("vmtl_conv2d_ksplit", (0, 8, 8, 64, 1152)),  # B = 0
    ("vmtl_conv2d_ksplit", (1, 0, 8, 64, 1152)),  # Ho = 0
    ("vmtl_conv2d_ksplit", (1, 8, 8, 64, 0)),  # Ktot = 0
    ("vmtl_conv2d_ksplit", (-1, 8, 8, 64, 1152)),
    ("vmtl_conv2d_up2_ksplit", (0, 6, 8, 72, 1320)),
    ("vmtl_conv2d_up2_ksplit", (1, 0, 8, 72, 1320)),
    ("vmtl_conv2d_up2_ksplit", (1, 6, 8, 72, 0)),
    ("vmtl_conv2d_up2_ksplit", (1, 6, -8, 72, 1320)),
])
def test_ksplit_of_an_empty_shape_is_no_split(name, args):
    assert lib().raw(name)(*args) == 1


# (case, pointer overrides, geometry overrides); x, wp, bias, y, ws are the pointers
PLAIN_BAD = [
    ("B = 0", {}, dict(B=0)),
    ("null x", dict(x=None), {}),
    ("Cs % 4 != 0", {}, dict(Cs=130)),
    ("Nw > ldy", {}, dict(Nw=65)),
    ("output extent against H / pad / K / stride", {}, dict(Ho=7)),
    ("output extent against W / pad / K / stride", {}, dict(Wo=9)),
    ("B * Ho * Wo over 2^31 - 1", {}, dict(B=40000, H=256, W=256, Ho=256, Wo=256)),
    ("Ho = 0", {}, dict(H=0, Ho=0)),
]


@pytest.mark.parametrize("case,ptrs,geo", PLAIN_BAD, ids=[c[0] for c in PLAIN_BAD])
def test_plain_split_k_entry_points_validate_before_the_split(case, ptrs, geo):
    p = dict(x=1, wp=1, bias=None, y=1, ws=1)
    p.update(ptrs)
    ptr = (p["x"], p["wp"], p["bias"], p["y"], p["ws"])
    assert lib().raw("vmtl_conv2d_fwd_ws")(*ptr, *_plain(**geo), None) == ERR_ARG
    for prec in (0, 1):
        assert lib().raw("vmtl_conv2d_fwd_ws_p")(*ptr, *_plain(**geo), prec, None) == ERR_ARG


# The UP2 entry points take no output extent (it is twice the low-res one by construction): the contradiction they can
# be given is a skip tensor that disagrees with its channel count.  Cout is their Nw.
UP2_BAD = [
    ("B = 0", {}, dict(B=0)),
    ("null xl", dict(xl=None), {}),
    ("C0s % 4 != 0", {}, dict(C0s=242)),
    ("Nw > ldy", {}, dict(Cout=73)),
    ("skip against C1s", dict(skip=None), {}),
    ("B * H2 * W2 * 4 over 2^31 - 1", {}, dict(B=40000, H2=128, W2=128)),
    ("H2 = 0", {}, dict(H2=0)),
    ("ldy % 4 != 0", {}, dict(ldy=74)),
]


@pytest.mark.parametrize("case,ptrs,geo", UP2_BAD, ids=[c[0] for c in UP2_BAD])
def test_up2_split_k_entry_points_validate_before_the_split(case, ptrs, geo):
    p = dict(xl=1, skip=1, wp_eff=1, y=1, ws=1)
    p.update(ptrs)
    ptr = (p["xl"], p["skip"], p["wp_eff"], p["y"], p["ws"])
    assert lib().raw("vmtl_conv2d_up2_fwd_ws")(*ptr, *_up2(**geo), None) == ERR_ARG
    for prec in (0, 1):
        assert lib().raw("vmtl_conv2d_up2_fwd_ws_p")(*ptr, *_up2(**geo), prec, None) == ERR_ARG


def test_precision_is_checked_before_everything_else():
    """precision = 2 is refused even where every other argument is one that crashed the split (B = 0) or is null."""
    none5 = (None,) * 5
    for prec in (2, -1):
        assert lib().raw("vmtl_conv2d_fwd_ws_p")(*none5, *_plain(B=0), prec, None) == ERR_ARG
        assert lib().raw("vmtl_conv2d_up2_fwd_ws_p")(*none5, *_up2(B=0), prec, None) == ERR_ARG
        assert lib().raw("vmtl_conv2d_fwd_ws_p")(1, 1, None, 1, 1, *PLAIN, prec, None) == ERR_ARG
        assert lib().raw("vmtl_conv2d_up2_fwd_ws_p")(1, 1, 1, 1, 1, *UP2, prec, None) == ERR_ARG
