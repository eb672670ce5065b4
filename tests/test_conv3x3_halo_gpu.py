"""-m gpu: the halo-tile 3x3 kernel for the 64/68-channel layers (csrc/conv3x3_halo.hip, vmtl_conv3x3_halo) against plain
PyTorch fp32 on the CPU: every epilogue mode with and without the prologue, the statistics rows, ops.bn_act_conv on the
new route, the routing of the bs-32 `basic` step and the end-to-end gradients of `basic` and `mtan` with the route forced
on at small shapes.  Tolerance 1e-4 of the reference's max magnitude (BASELINE.json north_star), as test_conv_small_gpu.py."""
import argparse
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_close, assert_grads_tight, ceil4, from_dev_nhwc, identity_activations, to_dev_nhwc

pytestmark = pytest.mark.gpu


def _pack_fwd(ops, w, dev):
    Cout, Cin = w.shape[:2]
    return ops.pack(w.to(dev), 1, Cout, 9, Cin, ceil4(Cin), 0, Cin * 9, 1, 9)


def _halo(ops, x, wp, y, Cs, ldy, Nw, Cout, **kw):
    B, H, W, _ = x.shape
    ops._mid_halo(x, wp, y, B, H, W, Cs, ldy, Nw, Cout, 0.0, **kw)


# B, Cin, Cout, H, W: 64 -> 64, 68 -> 67 (67 logical channels in 68), 68 -> 16, 64 -> 32, and a 68-row operand
HALO_CASES = [(2, 64, 64, 8, 64), (2, 67, 67, 12, 32), (1, 67, 16, 8, 64), (2, 64, 32, 4, 96), (1, 68, 68, 8, 32)]


def _per_tile(t, B, H, W):  # (B,C,H,W) -> (tiles, C, 128) in the kernel's tile order (image, tile row, tile column)
    return t.view(B, -1, H // 4, 4, W // 32, 32).permute(0, 2, 4, 1, 3, 5).reshape(-1, t.shape[1], 128)


@pytest.mark.parametrize("case", HALO_CASES + [(1, 67, 67, 7, 45), (1, 64, 32, 5, 40)])  # the last two: partial tiles
def test_conv3x3_halo_plain_and_prologue(dev, case):
    from vision_mtl_amd import ops

    B, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    bias = torch.randn(Cout, generator=g)
    Cs, ldy = ceil4(Cin), ceil4(Cout)
    xd, wp = to_dev_nhwc(x, dev), _pack_fwd(ops, w, dev)
    y = torch.full((B, H, W, ldy), float("nan"), device=dev)
    _halo(ops, xd, wp, y, Cs, ldy, Cout, Cout, bias=bias.to(dev))
    assert_close(from_dev_nhwc(y, Cout), F.conv2d(x, w, bias, padding=1), what="halo conv plain")
    assert float(y[..., Cout:].abs().sum()) == 0.0, "pad channels must be zero"
    # prologue relu(a*x + c), transformed input written back
    pa, pc = torch.randn(Cin, generator=g), torch.randn(Cin, generator=g)
    pad = lambda v: torch.cat([v, torch.zeros(Cs - Cin)]).to(dev)
    a_out = torch.full_like(xd, float("nan"))
    y.fill_(float("nan"))
    _halo(ops, xd, wp, y, Cs, ldy, Cout, Cout, pa=pad(pa), pc=pad(pc), act_in=ops.ACT_RELU, a_out=a_out)
    a_ref = F.relu(x * pa.view(1, -1, 1, 1) + pc.view(1, -1, 1, 1))
    assert_close(from_dev_nhwc(a_out, Cin), a_ref, what="halo conv a_out")
    assert float(a_out[..., Cin:].abs().sum()) == 0.0
    assert_close(from_dev_nhwc(y, Cout), F.conv2d(a_ref, w, None, padding=1), what="halo conv prologue")


@pytest.mark.parametrize("prologue", [False, True])
@pytest.mark.parametrize("case", HALO_CASES)
def test_conv3x3_halo_epilogues(dev, case, prologue):
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib

    B, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(18)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    Cs, ldy = ceil4(Cin), ceil4(Cout)
    xd, wp = to_dev_nhwc(x, dev), _pack_fwd(ops, w, dev)
    pro = {}
    xin = x
    if prologue:  # BatchNorm-apply as the prologue, no activation
        pa, pc = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g)
        pad = lambda v: torch.cat([v, torch.zeros(Cs - Cin)]).to(dev)
        pro = dict(pa=pad(pa), pc=pad(pc))
        xin = x * pa.view(1, -1, 1, 1) + pc.view(1, -1, 1, 1)
    yr = F.conv2d(xin, w, None, padding=1)
    tiles = lib().raw("vmtl_conv3x3_halo_stat_rows")(B, H, W)
    assert tiles == B * (H // 4) * (W // 32) and lib().raw("vmtl_conv3x3_halo_stat_block")(B, H, W) == 128
    # mode 1: per-tile (mean, M2)
    y = torch.full((B, H, W, ldy), float("nan"), device=dev)
    stats = torch.full((tiles, 2, ldy), float("nan"), device=dev)
    _halo(ops, xd, wp, y, Cs, ldy, Cout, Cout, stats=stats, ep_mode=1, **pro)
    assert_close(from_dev_nhwc(y, Cout), yr, what="mode 1 values")
    pt = _per_tile(yr, B, H, W).double()
    assert_close(stats[:, 0, :Cout].cpu(), pt.mean(-1), tol=1e-5, atol=1e-6, what="tile mean")
    assert_close(stats[:, 1, :Cout].cpu(), ((pt - pt.mean(-1, keepdim=True)) ** 2).sum(-1), tol=1e-4, what="tile M2")
    assert float(stats[:, :, Cout:].abs().sum()) == 0.0
    # mode 2: dz = conv * relu'(gamma * xhat + beta), per-tile (sum dz, sum dz*xhat)
    xz = torch.randn(B, Cout, H, W, generator=g)
    mean, invstd = torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5
    gamma, beta = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g) * 0.3
    v = lambda t: t.view(1, -1, 1, 1)
    xhat = (xz - v(mean)) * v(invstd)
    dz_ref = yr * ((v(gamma) * xhat + v(beta)) > 0).float()
    padc = lambda t: torch.cat([t, torch.zeros(ldy - Cout)]).to(dev)
    y.fill_(float("nan"))
    _halo(ops, xd, wp, y, Cs, ldy, Cout, Cout, stats=stats, ep_mode=2,
          ez=(to_dev_nhwc(xz, dev), padc(mean), padc(invstd), gamma.to(dev), beta.to(dev), ops.ACT_RELU), **pro)
    assert_close(from_dev_nhwc(y, Cout), dz_ref, what="mode 2 dz")
    assert float(y[..., Cout:].abs().sum()) == 0.0
    scale = float(_per_tile(dz_ref.abs(), B, H, W).sum(-1).max())
    assert_close(stats[:, 0, :Cout].cpu(), _per_tile(dz_ref, B, H, W).double().sum(-1), tol=1e-5, atol=1e-5 * scale,
                 what="sum dz")
    assert_close(stats[:, 1, :Cout].cpu(), _per_tile(dz_ref * xhat, B, H, W).double().sum(-1), tol=1e-5,
                 atol=1e-5 * scale, what="sum dz*xhat")


@pytest.fixture
def forced_route(monkeypatch):
    """the route on at any pixel count (the default keeps small launches on the implicit GEMM)"""
    from vision_mtl_amd import ops

    monkeypatch.setattr(ops, "_MID_HALO", True)
    monkeypatch.setattr(ops, "_MID_HALO_MIN_ROWS", 0)


# B, C (channels of x = conv input), Cout, H, W
BNCONV_CASES = [(2, 67, 67, 8, 64), (2, 64, 64, 8, 32), (1, 67, 16, 4, 64)]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("case", BNCONV_CASES)
def test_bn_act_conv_on_the_halo_route_matches_torch(dev, forced_route, case, training):
    from vision_mtl_amd import ops

    B, C, Cout, H, W = case
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3
    bn = torch.nn.BatchNorm2d(C)
    bn.weight.data = torch.rand(C, generator=g) + 0.5
    bn.bias.data = torch.randn(C, generator=g) * 0.2
    bn.running_mean.data = torch.randn(C, generator=g) * 0.1
    bn.running_var.data = torch.rand(C, generator=g) + 0.5
    bn.train(training)
    bnd = copy.deepcopy(bn).to(dev)
    w = torch.randn(Cout, C, 3, 3, generator=g) / (C * 9) ** 0.5
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv2d(F.relu(bn(xr)), wr, None, padding=1)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy)

    xd = to_dev_nhwc(x, dev).requires_grad_(True)
    wd = w.to(dev).requires_grad_(True)
    ops._RECORD = []
    try:
        y, stats, rpb = ops.bn_act_conv(xd, None, 0, bnd, C, ops.ACT_RELU, wd, want_stats=True)
        assert_close(from_dev_nhwc(y, Cout), yr.detach(), what="bn_act_conv fwd")
        assert rpb == 128 and stats.shape[0] == B * (H // 4) * (W // 32)
        mean = stats.cpu().double()[:, 0, :Cout].mean(0)
        assert_close(mean, yr.detach().double().mean((0, 2, 3)), tol=1e-5, atol=1e-6, what="output stats mean")
        y.backward(to_dev_nhwc(gy, dev))
        halo = [kw["ep_mode"] for name, kw, _, _ in ops._RECORD if name == "vmtl_conv3x3_halo"]
    finally:
        ops._RECORD = None
    # forward with the BatchNorm prologue; the fused data gradient too when dy has 64 / 68 channels
    assert halo == ([1, 2] if Cout >= 64 else [1]), halo
    assert_close(from_dev_nhwc(xd.grad, C), xr.grad, tol=2e-4, what="bn_act_conv dx")
    assert_close(wd.grad.cpu(), wr.grad, tol=2e-4, what="bn_act_conv dw")
    assert_close(bnd.weight.grad.cpu(), bn.weight.grad, tol=2e-4, what="bn_act_conv dgamma")
    assert_close(bnd.bias.grad.cpu(), bn.bias.grad, tol=2e-4, what="bn_act_conv dbeta")
    assert_close(bnd.running_mean.cpu(), bn.running_mean, tol=1e-5, what="running_mean")
    assert_close(bnd.running_var.cpu(), bn.running_var, tol=1e-5, what="running_var")
    assert int(bnd.num_batches_tracked) == int(bn.num_batches_tracked)


def _recorded_basic_step(dev, B, H, W):
    from oracle.losses import synthetic_batch
    from vision_mtl_amd import ops
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import build_model

    torch.manual_seed(3)
    model = build_model(argparse.Namespace(model_name="basic", backbone_weights=None), argparse.Namespace(num_classes=19))
    module = MTLModule(model.to(dev).train(), num_classes=19, device=str(dev))
    batch = {k: v.to(dev) for k, v in synthetic_batch(B, H, W, 19, seed=3).items()}
    ops._RECORD = []
    try:
        loss = module.training_step(batch, 0)
        loss.backward()
        rec = list(ops._RECORD)
    finally:
        ops._RECORD = None
    torch.cuda.synchronize()
    return rec


def test_basic_step_routes_the_mid_width_convs(dev, monkeypatch):
    from vision_mtl_amd import ops

    rec = _recorded_basic_step(dev, 32, 128, 256)
    halo = sorted((kw["Cs"], kw["ldy"], kw["ep_mode"], kw["pa"] is not None)
                  for name, kw, _, _ in rec if name == "vmtl_conv3x3_halo")
    # block 3: conv2 forward (BatchNorm prologue + statistics), its fused data gradient, conv1's skip data gradient
    assert halo == [(68, 16, 0, False), (68, 68, 1, True), (68, 68, 2, False)], halo
    monkeypatch.setattr(ops, "_MID_HALO", False)  # VMTL_MID_HALO=0
    rec = _recorded_basic_step(dev, 2, 128, 256)
    assert not any(name == "vmtl_conv3x3_halo" for name, _, _, _ in rec)


@pytest.mark.parametrize("kind,shape,C", [("basic", (2, 128, 128), 19), ("mtan", (2, 32, 32), 14)])
def test_gradients_with_the_route_forced_on(dev, forced_route, kind, shape, C):
    """End-to-end parameter gradients with every 64/68-channel 3x3 conv on the halo kernel, against the fp64 oracle, in
    the identity-activation variant of tests/test_tight_grads_gpu.py (no ReLU-mask flips: a tight bar)."""
    from oracle.losses import step_losses, synthetic_batch
    from vision_mtl_amd import ops
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import build_model

    torch.manual_seed(11)
    model = build_model(argparse.Namespace(model_name=kind, backbone_weights=None), argparse.Namespace(num_classes=C))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1 and p.numel() > 1 and float(p.detach().abs().max()) in (0.0, 1.0):
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    B, H, W = shape
    batch = synthetic_batch(B, H, W, C, seed=11, masked=0.1)

    def oracle(dtype):
        sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
        leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
        img = batch["img"].to(dtype)
        if kind == "basic":
            from oracle.unet_mobilenetv3 import basic_forward

            raw = basic_forward(sd, img, True)
        else:
            from oracle.mtan import mtan_forward

            raw = mtan_forward(sd, img, ["depth", "segm"], 4, True)
        losses = step_losses(raw, batch["mask"], batch["depth"].to(dtype))
        losses["loss"].backward()
        return losses["loss"].detach(), {k: v.grad for k, v in leaves.items()}

    with identity_activations():
        loss64, g64 = oracle(torch.float64)
        _, g32 = oracle(torch.float32)
        model = model.to(dev).train()
        module = MTLModule(model, num_classes=C, device=str(dev))
        ops._RECORD = []
        try:
            loss = module.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
            loss.backward()
            n_halo = sum(1 for name, _, _, _ in ops._RECORD if name == "vmtl_conv3x3_halo")
        finally:
            ops._RECORD = None
        torch.cuda.synchronize()
    assert n_halo > 0, "the route was not taken"
    assert_close(loss.detach().cpu(), loss64.float(), tol=1e-4, what=f"{kind} loss (identity activations)")
    hip = {k: p.grad.cpu() for k, p in model.named_parameters() if p.grad is not None}
    g32 = {k: v for k, v in g32.items() if v is not None}
    eh, ec, k = assert_grads_tight(hip, g64, g32)
    print(f"{kind} ({n_halo} halo launches): worst gradient error {eh:.2e} of its magnitude at {k} (fp32 CPU: {ec:.2e})")
