"""-m gpu: the squeeze-excite node on its one-launch-per-direction route (vmtl_se_gate_fwd / vmtl_se_gate_bwd /
vmtl_se_wgrad) against the torch-CPU fp32 formula of timm SqueezeExcite that test_squeeze_excite_fused uses, at the
shapes where the one-workgroup-per-image kernels can go wrong where the batch-sized GEMMs could not: one image, one
pixel, channel counts that are no multiple of 4 (scalar weight loads), fewer pixels than row lanes, the row limit, the
largest weights, production maps, odd HW.  Tolerance: tests/util.assert_close at its default 1e-4 of the reference's
magnitude."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_close, ceil4, from_dev_nhwc, to_dev_nhwc

pytestmark = pytest.mark.gpu

# (B, C, R, H, W)
CASES = [
    (1, 18, 7, 1, 1),       # one image, one pixel, C and R not multiples of 4
    (2, 72, 24, 3, 5),      # HW smaller than the row lanes of the reduction
    (64, 40, 10, 2, 2),     # the row limit
    (3, 960, 240, 4, 8),    # the largest weights
    (2, 672, 168, 8, 16),   # production maps at a small batch
    (2, 120, 32, 16, 32),
    (5, 120, 32, 9, 7),     # odd HW
]
NAMES = ["w_reduce", "b_reduce", "w_expand", "b_expand"]


def _ops():
    from vision_mtl_amd import ops

    return ops


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Inputs and the torch-CPU fp32 result of one case: (x, wr, br, we, be, gy), y, [dx, dwr, dbr, dwe, dbe]."""
    B, C, R, H, W = case
    g = torch.Generator().manual_seed(29)
    x = torch.randn(B, C, H, W, generator=g)
    wr, br = torch.randn(R, C, 1, 1, generator=g) / C ** 0.5, torch.randn(R, generator=g) * 0.5
    we, be = torch.randn(C, R, 1, 1, generator=g) * (2.0 / R ** 0.5), torch.randn(C, generator=g)
    ref = [t.clone().requires_grad_(True) for t in (x, wr, br, we, be)]
    s = F.conv2d(F.relu(F.conv2d(ref[0].mean((2, 3), keepdim=True), ref[1], ref[2])), ref[3], ref[4])
    yr = ref[0] * F.hardsigmoid(s)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)
    return (x, wr, br, we, be, gy), yr.detach(), [t.grad for t in ref]


def _run(dev, case, x_grad=True):
    """The node on the device: y, dx (None without x_grad), the four parameter gradients."""
    ops = _ops()
    (x, wr, br, we, be, gy), _, _ = _reference(case)
    xd = to_dev_nhwc(x, dev).requires_grad_(x_grad)
    d = [t.to(dev).requires_grad_(True) for t in (wr, br, we, be)]
    y = ops.squeeze_excite(xd, d[0], d[1], d[2], d[3])
    y.backward(to_dev_nhwc(gy, dev))
    return y.detach(), xd.grad, [t.grad for t in d]


def _check(dev, case, x_grad=True):
    C = case[1]
    _, yr, gr = _reference(case)
    y, dx, dp = _run(dev, case, x_grad)
    assert_close(from_dev_nhwc(y, C), yr, what="se fwd")
    if ceil4(C) > C:
        assert y[..., C:].abs().max().item() == 0.0
    if x_grad:
        assert_close(from_dev_nhwc(dx, C), gr[0], what="se dx")
        if ceil4(C) > C:
            assert dx[..., C:].abs().max().item() == 0.0
    else:
        assert dx is None
    for i, name in enumerate(NAMES):
        assert_close(dp[i].cpu(), gr[i + 1], what=f"se d{name}")


def _route(case):
    """vmtl_se_gate_supported: bit 0 - fused backward and weight gradient, bit 1 - fused forward."""
    from vision_mtl_amd._lib import lib

    return lib().raw("vmtl_se_gate_supported")(case[0], case[1], case[2])


# "default": the route production takes (the forward gate of large weights stays on the batch-sized GEMMs);
# "everywhere": VMTL_SE_FUSED=2, every case on all three new kernels
ROUTES = ["default", "everywhere"]


def _set_route(vmtl_env, route, case):
    if route == "everywhere":
        vmtl_env("VMTL_SE_FUSED", 2)
        assert _route(case) == 3
    else:
        assert _route(case) & 1


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", CASES)
def test_se_gate_matches_torch(dev, vmtl_env, case, route):
    """y and all five gradients; pad columns of y and dx exactly zero."""
    _set_route(vmtl_env, route, case)
    _check(dev, case)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", CASES)
def test_se_gate_without_input_grad(dev, vmtl_env, case, route):
    """x.requires_grad = False: no dx, the parameter gradients (which need dg and dh) still match."""
    _set_route(vmtl_env, route, case)
    _check(dev, case, x_grad=False)


@pytest.mark.parametrize("case", [(5, 120, 32, 9, 7), (3, 960, 240, 4, 8), (1, 18, 7, 1, 1)])
def test_se_gate_is_deterministic(dev, vmtl_env, case):
    _set_route(vmtl_env, "everywhere", case)
    a, b = _run(dev, case), _run(dev, case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for ga, gb in zip(a[2], b[2]):
        assert torch.equal(ga, gb)


def test_se_old_route(dev, vmtl_env):
    """VMTL_SE_FUSED=0: the earlier launch sequence of the same build, held to the same comparison."""
    case = (5, 120, 32, 9, 7)
    vmtl_env("VMTL_SE_FUSED", 0)
    assert _route(case) == 0
    names = _launches(dev, case)
    assert names["fwd"] == ["vmtl_hw_reduce", "vmtl_fc_fwd", "vmtl_fc_fwd", "vmtl_channel_scale_add"]
    _check(dev, case)
    _check(dev, case, x_grad=False)


def _launches(dev, case):
    """Entry points of one forward + backward of the node, by phase (ops._k wrapped as tests/production.py does)."""
    ops = _ops()
    (x, wr, br, we, be, gy), _, _ = _reference(case)
    xd = to_dev_nhwc(x, dev).requires_grad_(True)
    d = [t.to(dev).requires_grad_(True) for t in (wr, br, we, be)]
    gyd = to_dev_nhwc(gy, dev)
    names = {"fwd": [], "bwd": []}
    phase = ["fwd"]
    orig_k = ops._k

    def _k(name, _flop=None, _xflop=None, **kw):
        names[phase[0]].append(name)
        return orig_k(name, _flop=_flop, _xflop=_xflop, **kw)

    ops._k = _k
    try:
        y = ops.squeeze_excite(xd, d[0], d[1], d[2], d[3])
        phase[0] = "bwd"
        y.backward(gyd)
    finally:
        ops._k = orig_k
    return names


def test_se_gate_launch_count(dev):
    """On a shape whose forward gate is fused too (every shape is under VMTL_SE_FUSED=2): two forward launches (gate,
    scale); two main-stream backward launches (gate gradient, scale) besides the one weight-gradient launch that goes
    to the side stream when the gradients have arena slots."""
    case = (2, 120, 32, 16, 32)
    assert _route(case) == 3
    names = _launches(dev, case)
    assert names["fwd"] == ["vmtl_se_gate_fwd", "vmtl_channel_scale_add"]
    side = [n for n in names["bwd"] if n == "vmtl_se_wgrad"]
    main = [n for n in names["bwd"] if n != "vmtl_se_wgrad"]
    assert len(side) == 1
    assert main == ["vmtl_se_gate_bwd", "vmtl_channel_scale_add"]
