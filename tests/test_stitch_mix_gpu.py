"""-m gpu: the full cross-stitch mix kernels (csrc/stitch_mix.hip) through ops.stitch_mix and
CrossStitchLayer(mixing="full") against the fp64 einsum on the CPU, both weight layouts in every case.

Shapes are the smallest that reach each code path (M = B*H*W rows, Cs = ceil4(C)):
  C=6 / C=1            padded lanes (Cs 8 / 4)
  C=20                 no padding
  C=1028, M=30         more than one 256-quad column panel
  M=33                 a partly filled split of the reduction blocks (3 blocks of 11 rows); M=65: 5 blocks of 13
  B=2, 96x96 (M=18432) the reduction-block count capped at 1024
Bars: y and dx within 1e-6 of the reference's max magnitude (a two-term fp32 sum); dw within max(1e-5, 4 x the error of
the same sums done in fp32 by torch on the CPU) of max |dw|."""
import pytest
import torch

from tests.util import ceil4, from_dev_nhwc, to_dev_nhwc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 5, 6), (1, 3, 5, 1), (1, 3, 11, 20), (1, 5, 13, 6), (1, 5, 6, 1028), (2, 96, 96, 20)]
JUNK = 37.5


def _eq(cw, back=False):
    if back:
        return "abc,ancij->bncij" if cw else "ab,ancij->bncij"
    return "abc,bncij->ancij" if cw else "ab,bncij->ancij"


def _dw(dy, x, cw, dtype):
    """block (a,b) of the weight gradient: sum over batch and pixels (and channels, layer-wise) of dy_a * x_b"""
    return torch.einsum("ancij,bncij->abc" if cw else "ancij,bncij->ab", dy.to(dtype), x.to(dtype))


_CASES = {}


def _case(shape, cw):
    """inputs and the fp64 reference of one case, computed once per session and never modified"""
    key = (shape, cw)
    if key not in _CASES:
        B, H, W, C = shape
        g = torch.Generator().manual_seed(1000 + 7 * C + H * W + int(cw))
        x = torch.randn(2, B, C, H, W, generator=g)
        dy = torch.randn(2, B, C, H, W, generator=g)
        w = torch.rand((2, 2, C) if cw else (2, 2), generator=g)
        ref = dict(y=torch.einsum(_eq(cw), w.double(), x.double()), dx=torch.einsum(_eq(cw, True), w.double(), dy.double()),
                   dw=_dw(dy, x, cw, torch.float64))
        mag = float(ref["dw"].abs().max())
        err32 = float((_dw(dy, x, cw, torch.float32).double() - ref["dw"]).abs().max()) / mag
        ref["dw_bar"] = max(1e-5, 4.0 * err32)
        _CASES[key] = (x, dy, w, ref)
    return _CASES[key]


def _run(dev, x, dy, w, C, x_grad=True, w_grad=True, junk=None):
    """ops.stitch_mix forward + backward on padded NHWC tensors; junk: value written into the padded lanes of x and dy"""
    from vision_mtl_amd import ops

    xs = [to_dev_nhwc(x[t], dev) for t in range(2)]
    gs = [to_dev_nhwc(dy[t], dev) for t in range(2)]
    if junk is not None:
        for t in xs + gs:
            t[..., C:] = junk
    xs = [t.requires_grad_(x_grad) for t in xs]
    wd = w.to(dev).requires_grad_(w_grad)
    y0, y1 = ops.stitch_mix(xs[0], xs[1], wd, C)
    torch.autograd.backward([y0, y1], gs)
    torch.cuda.synchronize()
    return dict(y=(y0.detach(), y1.detach()), dx=tuple(t.grad for t in xs), dw=wd.grad)


def _assert_within(got, ref, tol, what):
    err, mag = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max-abs error {err:.3e}, magnitude {mag:.3e}, bar {tol:.1e} of it")
    assert err <= tol * mag, f"{what}: max-abs error {err:.3e} vs magnitude {mag:.3e} (bar {tol:.1e})"


def _nchw(pair, C):
    return torch.stack([from_dev_nhwc(t, C) for t in pair])


@pytest.mark.parametrize("cw", [True, False], ids=["channel_wise", "layer_wise"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_backward_match_fp64_einsum(dev, shape, cw):
    x, dy, w, ref = _case(shape, cw)
    C = shape[3]
    out = _run(dev, x, dy, w, C)
    _assert_within(_nchw(out["y"], C), ref["y"], 1e-6, "y")
    _assert_within(_nchw(out["dx"], C), ref["dx"], 1e-6, "dx")
    assert out["dw"].shape == w.shape
    _assert_within(out["dw"], ref["dw"], ref["dw_bar"], "dw")
    dw = out["dw"].cpu()
    assert float(dw[0, 1].abs().max()) > 0 and float(dw[1, 0].abs().max()) > 0, "off-diagonal blocks must get a gradient"
    for t in out["y"] + out["dx"]:
        assert bool((t[..., C:] == 0).all()), "padded lanes must be zero"


@pytest.mark.parametrize("cw", [True, False], ids=["channel_wise", "layer_wise"])
@pytest.mark.parametrize("shape", [(1, 3, 5, 6), (1, 3, 5, 1), (1, 3, 11, 17)], ids=lambda s: "x".join(map(str, s)))
def test_padded_lanes_are_written_as_zeros_and_ignored(dev, shape, cw):
    x, dy, w, ref = _case(shape, cw)
    C = shape[3]
    assert ceil4(C) > C
    clean, junk = _run(dev, x, dy, w, C), _run(dev, x, dy, w, C, junk=JUNK)
    for k in ("y", "dx"):
        for a, b in zip(clean[k], junk[k]):
            assert bool((b[..., C:] == 0).all()), f"{k}: junk in the padded input lanes reached the output"
            assert torch.equal(a, b), k
    assert torch.equal(clean["dw"], junk["dw"]), "dw must not depend on the padded lanes"
    _assert_within(junk["dw"], ref["dw"], ref["dw_bar"], "dw")


@pytest.mark.parametrize("cw", [True, False], ids=["channel_wise", "layer_wise"])
@pytest.mark.parametrize("shape", [(1, 3, 11, 6), (1, 5, 6, 1028), (2, 96, 96, 20)], ids=lambda s: "x".join(map(str, s)))
def test_zero_off_diagonal_equals_the_diagonal_path(dev, shape, cw):
    from vision_mtl_amd import ops

    x, dy, w, ref = _case(shape, cw)
    C = shape[3]
    w = w.clone()
    w[0, 1] = 0.0
    w[1, 0] = 0.0
    mix = _run(dev, x, dy, w, C)
    wd = w.to(dev).requires_grad_(True)
    dw_ref = _dw(dy, x, cw, torch.float64)
    for t in range(2):
        xt = to_dev_nhwc(x[t], dev).requires_grad_(True)
        y = ops.stitch(xt, wd, t, C)
        y.backward(to_dev_nhwc(dy[t], dev))
        assert torch.equal(mix["y"][t], y.detach()), f"y of task {t}"
        assert torch.equal(mix["dx"][t], xt.grad), f"dx of task {t}"
    mag = float(dw_ref.abs().max())
    for t in range(2):
        err = float((mix["dw"][t, t].double() - wd.grad[t, t].double()).abs().max())
        assert err <= ref["dw_bar"] * mag, f"dw block ({t},{t}): {err:.3e} vs magnitude {mag:.3e}"
    assert float(wd.grad[0, 1].abs().max()) == 0.0  # the diagonal path leaves these at zero, the mix does not
    assert float(mix["dw"][0, 1].abs().max()) > 0.0


@pytest.mark.parametrize("cw", [True, False], ids=["channel_wise", "layer_wise"])
def test_selective_backward(dev, cw):
    shape = (1, 3, 11, 6)
    x, dy, w, ref = _case(shape, cw)
    C = shape[3]
    frozen = _run(dev, x, dy, w, C, w_grad=False)
    assert frozen["dw"] is None
    _assert_within(_nchw(frozen["dx"], C), ref["dx"], 1e-6, "dx with frozen weights")
    for t in frozen["dx"]:
        assert bool((t[..., C:] == 0).all())
    only_w = _run(dev, x, dy, w, C, x_grad=False)
    assert only_w["dx"] == (None, None)
    _assert_within(only_w["dw"], ref["dw"], ref["dw_bar"], "dw with inputs that need no gradient")
    both = _run(dev, x, dy, w, C)
    assert torch.equal(both["dw"], only_w["dw"]) and all(torch.equal(a, b) for a, b in zip(both["dx"], frozen["dx"]))


@pytest.mark.parametrize("cw", [True, False], ids=["channel_wise", "layer_wise"])
def test_backward_is_reproducible(dev, cw):
    shape = (2, 96, 96, 20)
    x, dy, w, _ = _case(shape, cw)
    a, b = _run(dev, x, dy, w, shape[3]), _run(dev, x, dy, w, shape[3])
    assert torch.equal(a["dw"], b["dw"])
    assert all(torch.equal(p, q) for p, q in zip(a["dx"], b["dx"]))


def test_entry_points_reject_bad_arguments(dev):
    """aliasing, Cs % 4 != 0 and C > Cs return VMTL_ERR_ARG (-1) before anything is launched"""
    from vision_mtl_amd._lib import lib

    M, C, Cs = 8, 6, 8
    t = [torch.full((M, Cs), 3.0, device=dev) for _ in range(6)]
    w = torch.rand(2, 2, C, device=dev)
    dw = torch.full((2, 2, C), 5.0, device=dev)
    partial = torch.empty(4 * lib().raw("vmtl_reduce_rows")(M) + 4, Cs, device=dev)
    p = [v.data_ptr() for v in t]
    fwd, bwd = lib().raw("vmtl_stitch_mix"), lib().raw("vmtl_stitch_mix_bwd")
    assert fwd(p[0], p[1], w.data_ptr(), p[0], p[2], M, C, Cs, 1, 0) == -1  # y0 aliases x0
    assert fwd(p[0], p[1], w.data_ptr(), p[2], p[1], M, C, Cs, 1, 0) == -1  # y1 aliases x1
    assert fwd(p[0], p[1], w.data_ptr(), p[2], p[2], M, C, Cs, 1, 0) == -1  # y0 aliases y1
    assert fwd(p[0], p[1], w.data_ptr(), p[2], p[3], M, C, 6, 1, 0) == -1  # Cs = 6
    assert fwd(p[0], p[1], w.data_ptr(), p[2], p[3], M, Cs + 1, Cs, 1, 0) == -1  # C > Cs
    assert fwd(p[0], p[1], w.data_ptr(), p[2], p[3], 0, C, Cs, 1, 0) == -1  # M = 0
    assert fwd(p[0], p[1], None, p[2], p[3], M, C, Cs, 1, 0) == -1
    args = (w.data_ptr(), p[4], p[5], partial.data_ptr(), dw.data_ptr())
    assert bwd(p[0], p[1], p[2], p[3], w.data_ptr(), p[2], p[5], partial.data_ptr(), dw.data_ptr(), M, C, Cs, 1, 0) == -1
    assert bwd(p[0], p[1], p[2], p[3], w.data_ptr(), p[4], None, partial.data_ptr(), dw.data_ptr(), M, C, Cs, 1, 0) == -1
    assert bwd(p[0], p[1], p[2], p[3], *args, M, C, 6, 1, 0) == -1
    assert bwd(p[0], p[1], p[2], p[3], *args, M, Cs + 1, Cs, 1, 0) == -1
    assert bwd(p[0], p[1], p[2], p[3], *args, 0, C, Cs, 1, 0) == -1
    assert bwd(p[0], p[1], p[2], p[3], w.data_ptr(), p[4], p[5], None, dw.data_ptr(), M, C, Cs, 1, 0) == -1
    torch.cuda.synchronize()
    assert all(bool((v == 3.0).all()) for v in t) and bool((dw == 5.0).all()), "a rejected call wrote something"


@pytest.mark.parametrize("cw", [True, False], ids=["channel_wise", "layer_wise"])
def test_cross_stitch_layer_full_forward_equals_einsum(dev, cw):
    from vision_mtl_amd.models.cross_stitch_model import CrossStitchLayer

    shape = (1, 3, 11, 6)
    x, dy, w, ref = _case(shape, cw)
    C = shape[3]
    layer = CrossStitchLayer(2, C if cw else None, mixing="full").to(dev)
    with torch.no_grad():
        layer.weights.copy_(w.to(dev))
    xd = x.to(dev).requires_grad_(True)
    y = layer(xd)
    assert y.shape == x.shape
    y.backward(dy.to(dev))
    _assert_within(y.detach(), ref["y"], 1e-6, "layer y")
    _assert_within(xd.grad, ref["dx"], 1e-6, "layer dx")
    _assert_within(layer.weights.grad, ref["dw"], ref["dw_bar"], "layer dw")
