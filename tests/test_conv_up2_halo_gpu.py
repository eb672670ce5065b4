"""-m gpu: the halo-tile kernel for the narrow UP2 decoder convs (csrc/conv_up2_halo.hip, vmtl_conv2d_up2_halo) against
plain PyTorch on the CPU (nearest-x2 upsample, concat, 3x3 conv in float64), its BatchNorm partial rows, and the routing
of ops.up2_conv / ops.bn_act_conv(up2=True) to it."""
import argparse

import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_close, ceil4, from_dev_nhwc, to_dev_nhwc

pytestmark = pytest.mark.gpu


def _ref(x, sk, w):
    up = F.interpolate(x.double(), scale_factor=2, mode="nearest")
    return F.conv2d(torch.cat([up, sk.double()], 1) if sk is not None else up, w.double(), None, padding=1)


def _operands(dev, B, C0, C1, H2, W2, Cout, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C0, H2, W2, generator=g)
    sk = torch.randn(B, C1, 2 * H2, 2 * W2, generator=g) if C1 else None
    w = torch.randn(Cout, C0 + C1, 3, 3, generator=g) / ((C0 + C1) * 9) ** 0.5
    return x, sk, w


def _launch(dev, x, sk, w, with_stats):
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib

    L = lib()
    B, C0, H2, W2 = x.shape
    C1 = 0 if sk is None else sk.shape[1]
    Cout = w.shape[0]
    C0s, C1s, ldy = ceil4(C0), ceil4(C1), ceil4(Cout)
    xd = to_dev_nhwc(x, dev)
    skd = to_dev_nhwc(sk, dev) if C1 else None
    wp = torch.empty(4, Cout, 4 * C0s + 9 * C1s, device=dev)
    ops._k("vmtl_pack_up2_fwd", w=w.to(dev).contiguous(), dst=wp, Cout=Cout, C0=C0, C0s=C0s, C1=C1, C1s=C1s)
    y = torch.full((B, 2 * H2, 2 * W2, ldy), float("nan"), device=dev)
    rows = L.raw("vmtl_conv2d_up2_halo_stat_rows")(B, H2, W2, C0s, C1s, ldy, Cout)
    stats = torch.full((rows, 2, ldy), float("nan"), device=dev) if with_stats and rows else None
    L.callk("vmtl_conv2d_up2_halo", xl=xd, skip=skd, wp_eff=wp, y=y, stats=stats, B=B, H2=H2, W2=W2, C0s=C0s, C1s=C1s,
            ldy=ldy, Cout=Cout, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y, stats, L.raw("vmtl_conv2d_up2_halo_stat_block")(C0s, C1s, ldy, Cout)


# B, C0, C1, H2, W2, Cout: the two `basic` decoder shapes at reduced batch, then partial tiles at the right / bottom border
CASES = [(2, 67, 0, 64, 128, 33), (2, 135, 16, 32, 64, 67), (1, 67, 0, 7, 20, 33), (1, 135, 16, 5, 40, 67),
         (3, 67, 0, 2, 3, 33), (1, 135, 16, 1, 1, 67)]


@pytest.mark.parametrize("case", CASES)
def test_up2_halo_matches_torch(dev, case):
    B, C0, C1, H2, W2, Cout = case
    x, sk, w = _operands(dev, B, C0, C1, H2, W2, Cout)
    y, _, _ = _launch(dev, x, sk, w, with_stats=False)
    assert_close(from_dev_nhwc(y, Cout), _ref(x, sk, w), tol=1e-5, what=f"up2 halo {case}")
    assert y[..., Cout:].abs().max().item() == 0.0  # storage channels stay zero


@pytest.mark.parametrize("case", CASES[:2] + [(1, 67, 0, 8, 32, 33), (1, 135, 16, 4, 16, 67)])
def test_up2_halo_statistics_rows(dev, case):
    """The per-tile (mean, M2) rows, merged as equal-sized blocks of the reported row block, give the output's
    per-channel mean and (biased) variance."""
    B, C0, C1, H2, W2, Cout = case
    x, sk, w = _operands(dev, B, C0, C1, H2, W2, Cout, seed=9)
    y, stats, rpb = _launch(dev, x, sk, w, with_stats=True)
    assert stats is not None and stats.shape[0] * rpb == 4 * B * H2 * W2
    st = stats.double().cpu()
    mean = st[:, 0].mean(0)
    var = (st[:, 1] + rpb * (st[:, 0] - mean) ** 2).sum(0) / (4 * B * H2 * W2)
    yo = _ref(x, sk, w)
    assert_close(mean[:Cout], yo.mean((0, 2, 3)), tol=1e-5, atol=1e-6, what="up2 halo stats mean")
    assert_close(var[:Cout], yo.var((0, 2, 3), unbiased=False), tol=1e-4, what="up2 halo stats var")
    assert_close(from_dev_nhwc(y, Cout), yo, tol=1e-5, what="up2 halo y (stats launch)")


def test_up2_halo_rejects_what_it_does_not_cover(dev):
    from vision_mtl_amd._lib import lib

    L = lib()
    # statistics need whole tiles; other channel counts are not instantiated
    assert L.raw("vmtl_conv2d_up2_halo_stat_rows")(1, 7, 20, 68, 0, 36, 33) == 0
    assert L.raw("vmtl_conv2d_up2_halo_supported")(2, 8, 16, 72, 0, 36, 33) == 0
    assert L.raw("vmtl_conv2d_up2_halo_supported")(2, 8, 16, 68, 0, 36, 34) == 0
    xl = torch.zeros(2, 8, 16, 72, device=dev)
    wp = torch.zeros(4, 33, 4 * 72, device=dev)
    y = torch.zeros(2, 16, 32, 36, device=dev)
    rc = L.raw("vmtl_conv2d_up2_halo")(xl.data_ptr(), None, wp.data_ptr(), y.data_ptr(), None, 2, 8, 16, 72, 0, 36, 33, None)
    assert rc == -3


def test_up2_shape_outside_the_guard_takes_the_implicit_gemm(dev):
    from vision_mtl_amd import ops

    x, sk, w = _operands(dev, 2, 71, 0, 8, 16, 33)
    ops._RECORD = []
    try:
        y, _ = ops.up2_conv(to_dev_nhwc(x, dev), 71, None, w.to(dev), want_stats=True)
        names = [r[0] for r in ops._RECORD]
    finally:
        ops._RECORD = None
    assert "vmtl_conv2d_up2_fwd" in names and "vmtl_conv2d_up2_halo" not in names
    assert_close(from_dev_nhwc(y, 33), _ref(x, sk, w), tol=1e-5, what="up2 igemm")


def _recorded_up2(dev, precision):
    import vision_mtl_amd
    from oracle.losses import synthetic_batch
    from vision_mtl_amd import ops
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import build_model

    torch.manual_seed(3)
    model = build_model(argparse.Namespace(model_name="basic", backbone_weights=None), argparse.Namespace(num_classes=19))
    module = MTLModule(model.to(dev).train(), num_classes=19, device=str(dev))
    batch = {k: v.to(dev) for k, v in synthetic_batch(2, 128, 256, 19, seed=3).items()}
    ops._RECORD = []
    try:
        with vision_mtl_amd.conv_precision(precision):
            loss = module.training_step(batch, 0)
            loss.backward()
        rec = list(ops._RECORD)
    finally:
        ops._RECORD = None
    torch.cuda.synchronize()
    return [(name, kw["C0s"], kw["C1s"]) for name, kw, _, _ in rec if "H2" in kw]


def test_basic_step_routes_the_narrow_up2_convs(dev):
    halo = {(c0, c1) for name, c0, c1 in _recorded_up2(dev, "fp32") if name == "vmtl_conv2d_up2_halo"}
    assert halo == {(68, 0), (136, 16)}  # decoder blocks 4 (67 -> 33) and 3 (135 + 16 -> 67)
    assert all(name != "vmtl_conv2d_up2_halo" for name, _, _ in _recorded_up2(dev, "bf16"))
