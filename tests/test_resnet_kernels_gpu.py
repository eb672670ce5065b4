"""-m gpu: the three ResNet kernels of csrc/resnet.hip against torch fp64 on the CPU - the phase-decomposed data gradient of
a stride-2 dense conv, BatchNorm + ReLU + MaxPool2d(3, 2, 1) (fused and plain), and the residual close
act(BN_a(z) + r) with an identity or a downsample shortcut."""
import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_close, from_dev_nhwc, to_dev_nhwc

pytestmark = pytest.mark.gpu


def _nhwc_leaf(x_nchw, dev):
    return to_dev_nhwc(x_nchw, dev).detach().requires_grad_(True)


# ----------------------------------------------------------------------------- stride-2 data gradient
@pytest.mark.parametrize("K,pad", [(3, 1), (1, 0), (7, 3)])
@pytest.mark.parametrize("H,W", [(12, 16), (13, 9), (1, 5)])
@pytest.mark.parametrize("Cin,Cout", [(5, 7), (3, 64)])
def test_conv2d_stride2_input_grad(dev, K, pad, H, W, Cin, Cout):
    """ops.conv2d(stride=2) with x.requires_grad: dx equals torch's (fp64) input gradient; pixels no window covers are 0."""
    from vision_mtl_amd import ops

    g = torch.Generator().manual_seed(K * 100 + H * 10 + W + Cin)
    B = 2
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) / (Cin * K * K) ** 0.5
    Ho, Wo = (H + 2 * pad - K) // 2 + 1, (W + 2 * pad - K) // 2 + 1
    dy = torch.randn(B, Cout, Ho, Wo, generator=g)
    xd = _nhwc_leaf(x, dev)
    y = ops.conv2d(xd, w.to(dev), None, 2, pad)
    assert y.shape == (B, Ho, Wo, ops.ceil4(Cout))
    y.backward(to_dev_nhwc(dy, dev))
    x64 = x.double().requires_grad_(True)
    F.conv2d(x64, w.double(), None, 2, pad).backward(dy.double())
    dx = xd.grad.cpu()
    assert_close(from_dev_nhwc(dx, Cin), x64.grad, tol=1e-5, what=f"dx K={K} pad={pad} {H}x{W}")
    assert float(dx[..., Cin:].abs().max() if dx.shape[-1] > Cin else 0.0) == 0.0, "pad channels must stay 0"
    if K == 1:  # odd rows / columns receive nothing: exact zeros
        assert float(dx[:, 1::2].abs().max() if H > 1 else 0.0) == 0.0
        assert float(dx[:, :, 1::2].abs().max()) == 0.0


def test_conv2d_stride2_input_grad_bf16(dev):
    """bf16 operands: the data gradient runs under the precision its forward recorded, checked against fp64 on
    bf16-rounded dy and weights."""
    from vision_mtl_amd import conv_precision, ops

    g = torch.Generator().manual_seed(3)
    B, Cin, Cout, H, W = 2, 6, 10, 15, 14
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / 7.0
    dy = torch.randn(B, Cout, 8, 7, generator=g)
    xd = _nhwc_leaf(x, dev)
    with conv_precision("bf16"):
        y = ops.conv2d(xd, w.to(dev), None, 2, 1)
    y.backward(to_dev_nhwc(dy, dev))  # outside the scope: the recorded precision holds
    rb = lambda t: t.to(torch.bfloat16).double()
    x64 = x.double().requires_grad_(True)
    F.conv2d(x64, rb(w), None, 2, 1).backward(rb(dy))
    assert_close(from_dev_nhwc(xd.grad.cpu(), Cin), x64.grad, tol=1e-5, what="bf16 dx")


def test_conv2d_stride2_unsupported_pad_raises(dev):
    from vision_mtl_amd import ops

    xd = _nhwc_leaf(torch.randn(1, 4, 9, 9), dev)
    y = ops.conv2d(xd, torch.randn(4, 4, 5, 5, device=dev), None, 2, 2)  # 5x5 / pad 2: phases need two pads
    with pytest.raises(NotImplementedError):
        y.sum().backward()


# ----------------------------------------------------------------------------- BatchNorm + ReLU + MaxPool2d(3, 2, 1)
def _bn(C, dev, seed, training):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(C, generator=g))
        bn.bias.copy_(0.2 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    ref = {k: v.clone() for k, v in bn.state_dict().items()}
    return bn.to(dev).train(training), ref


def _ref_bn(x64, ref, training):
    rm, rv = ref["running_mean"].double().clone(), ref["running_var"].double().clone()
    gam = ref["weight"].double().clone().requires_grad_(True)
    bet = ref["bias"].double().clone().requires_grad_(True)
    y = F.batch_norm(x64, rm, rv, gam, bet, training, 0.1, 1e-5)
    return y, gam, bet, rm, rv


def _check_bn_state(bn, rm, rv, ref, training, what):
    assert_close(bn.running_mean.cpu(), rm.float(), tol=1e-5, what=f"{what} running_mean")
    assert_close(bn.running_var.cpu(), rv.float(), tol=1e-5, what=f"{what} running_var")
    assert int(bn.num_batches_tracked) == int(ref["num_batches_tracked"]) + (1 if training else 0)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("H,W", [(16, 12), (15, 11), (2, 3)])
@pytest.mark.parametrize("fused", [True, False])
def test_bn_relu_maxpool3(dev, training, H, W, fused, monkeypatch):
    from vision_mtl_amd import ops

    monkeypatch.setattr(ops, "FUSE_STEM_POOL", fused)
    B, C = 3, 6
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(B, C, H, W, generator=g)
    ga = torch.randn(B, C, H, W, generator=g)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gp = torch.randn(B, C, Ho, Wo, generator=g)
    bn, ref = _bn(C, dev, 7, training)
    xd = _nhwc_leaf(x, dev)
    a, p = ops.bn_act_pool3(xd, bn, C, ops.ACT_RELU)
    assert a.shape == (B, H, W, 8) and p.shape == (B, Ho, Wo, 8)
    ((a * to_dev_nhwc(ga, dev)).sum() + (p * to_dev_nhwc(gp, dev)).sum()).backward()
    x64 = x.double().requires_grad_(True)
    z, gam, bet, rm, rv = _ref_bn(x64, ref, training)
    a64 = F.relu(z)
    p64 = F.max_pool2d(a64, 3, 2, 1)
    ((a64 * ga.double()).sum() + (p64 * gp.double()).sum()).backward()
    assert_close(from_dev_nhwc(a.detach().cpu(), C), a64.detach(), tol=1e-5, what="activation")
    assert_close(from_dev_nhwc(p.detach().cpu(), C), p64.detach(), tol=1e-5, what="pool")
    assert float(p.detach()[..., C:].abs().max()) == 0.0 and float(a.detach()[..., C:].abs().max()) == 0.0
    assert_close(from_dev_nhwc(xd.grad.cpu(), C), x64.grad, tol=1e-4, what="dx")
    assert_close(bn.weight.grad.cpu(), gam.grad, tol=1e-4, what="dgamma")
    assert_close(bn.bias.grad.cpu(), bet.grad, tol=1e-4, what="dbeta")
    _check_bn_state(bn, rm, rv, ref, training, "pool")


@pytest.mark.parametrize("H,W", [(9, 10), (4, 4)])
def test_plain_maxpool3_ties_and_nan(dev, H, W):
    """The plain node on integer data (many ties) with a NaN: values and the routing of the gradient follow torch's CPU
    max_pool2d (first maximum in window order wins, NaN wins)."""
    from vision_mtl_amd import ops

    g = torch.Generator().manual_seed(H + W)
    B, C = 2, 5
    x = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
    x[0, 1, 2, 3] = float("nan")
    gp = torch.randn(B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=g)
    xd = _nhwc_leaf(x, dev)
    p = ops.maxpool3s2(xd, C)
    (p * to_dev_nhwc(gp, dev)).sum().backward()
    xc = x.clone().requires_grad_(True)
    pc = F.max_pool2d(xc, 3, 2, 1)
    (pc * gp).sum().backward()
    assert torch.equal(torch.isnan(from_dev_nhwc(p.detach().cpu(), C)), torch.isnan(pc.detach()))
    assert torch.equal(torch.nan_to_num(from_dev_nhwc(p.detach().cpu(), C)), torch.nan_to_num(pc.detach()))
    assert_close(from_dev_nhwc(xd.grad.cpu(), C), xc.grad, tol=1e-6, what="routed gradient")


# ----------------------------------------------------------------------------- residual close
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("downsample", [False, True])
def test_bn_add_act(dev, training, downsample):
    from vision_mtl_amd import ops

    B, C, H, W = 2, 10, 7, 9
    g = torch.Generator().manual_seed(int(training) * 2 + int(downsample))
    z = torch.randn(B, C, H, W, generator=g)
    r = torch.randn(B, C, H, W, generator=g)
    dy = torch.randn(B, C, H, W, generator=g)
    bn, ref = _bn(C, dev, 11, training)
    bnd, refd = _bn(C, dev, 12, training)
    zd, rd = _nhwc_leaf(z, dev), _nhwc_leaf(r, dev)
    if downsample:
        y = ops.bn_add_act(zd, None, 0, bn, C, ops.ACT_RELU, zd=rd, bn_d=bnd)
    else:
        y = ops.bn_add_act(zd, None, 0, bn, C, ops.ACT_RELU, res=rd)
    y.backward(to_dev_nhwc(dy, dev))
    z64, r64 = z.double().requires_grad_(True), r.double().requires_grad_(True)
    za, gam, bet, rm, rv = _ref_bn(z64, ref, training)
    if downsample:
        rr, gamd, betd, rmd, rvd = _ref_bn(r64, refd, training)
    else:
        rr = r64
    y64 = F.relu(za + rr)
    y64.backward(dy.double())
    assert_close(from_dev_nhwc(y.detach().cpu(), C), y64.detach(), tol=1e-5, what="y")
    assert float(y.detach()[..., C:].abs().max()) == 0.0
    assert_close(from_dev_nhwc(zd.grad.cpu(), C), z64.grad, tol=1e-4, what="dz")
    assert_close(from_dev_nhwc(rd.grad.cpu(), C), r64.grad, tol=1e-4, what="dres / dzd")
    assert_close(bn.weight.grad.cpu(), gam.grad, tol=1e-4, what="dgamma")
    assert_close(bn.bias.grad.cpu(), bet.grad, tol=1e-4, what="dbeta")
    _check_bn_state(bn, rm, rv, ref, training, "bn_a")
    if downsample:
        assert_close(bnd.weight.grad.cpu(), gamd.grad, tol=1e-4, what="dgamma_d")
        assert_close(bnd.bias.grad.cpu(), betd.grad, tol=1e-4, what="dbeta_d")
        _check_bn_state(bnd, rmd, rvd, refd, training, "bn_d")


def test_bn_add_act_eval_table(dev):
    """Eval mode inside ops.eval_bn_table: the statistics come from the table, the result equals the launch-per-layer
    path's bit for bit."""
    from vision_mtl_amd import ops

    B, C, H, W = 2, 12, 5, 6
    g = torch.Generator().manual_seed(9)
    z, r = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    bn, _ = _bn(C, dev, 4, False)
    bnd, _ = _bn(C, dev, 5, False)
    holder = torch.nn.ModuleList([bn, bnd]).eval()
    zd, rd = to_dev_nhwc(z, dev), to_dev_nhwc(r, dev)
    y0 = ops.bn_add_act(zd, None, 0, bn, C, ops.ACT_RELU, zd=rd, bn_d=bnd)
    with ops.eval_bn_table(holder) as t:
        assert t is not None
        y1 = ops.bn_add_act(zd, None, 0, bn, C, ops.ACT_RELU, zd=rd, bn_d=bnd)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
