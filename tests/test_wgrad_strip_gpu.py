"""-m gpu: the strip-walking weight gradient (csrc/conv_wgrad_small.hip) on the shapes its tail rows (1-4 output channels past
the last 16-row MFMA tile, on the vector ALU) and its 80-float LDS pixels (40-68 channels on a side) added, at the smallest
sizes at which each new path can go wrong (VMTL_WS_WIDE_MIN_PIXELS=1: a training step sends those classes to the strip
kernel from 65,536 pixels only).  Every case runs ops.conv2d backward on three routes - the default routing, the same
with many short bands (VMTL_WS_TARGET=4096: every halo row and every ragged last band), and conv_wgrad_kernel
(VMTL_WGRAD_SMALL=0) - on poisoned, guard-banded op buffers, against the fp64 CPU weight gradient under the bar of
test_kernels_gpu.test_conv3x3_wgrad_small (1e-4 of the reference's magnitude)."""
import pytest
import torch
import torch.nn.functional as F

from tests import poison
from tests.util import assert_close, ceil4, to_dev_nhwc

pytestmark = pytest.mark.gpu

CASES = [(1, 33, 5, 32, 33),    # one strip, one live tail row, 21 kk tiles
         (2, 36, 9, 64, 35),    # three live tail rows, two strips
         (1, 33, 70, 96, 20),   # one MFMA tile + 4 tail rows, several bands with a ragged last one
         (2, 13, 6, 32, 17),    # one live tail row on one MFMA tile
         (2, 16, 9, 64, 67),    # wide dY, 64 + 3
         (1, 24, 5, 32, 40),    # wide dY, narrow end
         (1, 67, 7, 32, 67),    # wide x and dY, 39 kk tiles
         (2, 64, 6, 64, 64),    # wide x and dY, no tail
         (1, 40, 5, 32, 1),     # wide x, a single output row
         (1, 64, 20, 32, 33)]   # wide x (eight waves) against a narrow dY with one tail row; three bands, the last ragged


def _lib():
    from vision_mtl_amd._lib import lib

    return lib()


@pytest.mark.parametrize("case", CASES)
def test_wgrad_strip_routes_against_fp64(dev, case, vmtl_env):
    from vision_mtl_amd import ops

    B, Cin, H, W, Cout = case
    Cs, ldy = ceil4(Cin), ceil4(Cout)
    if not _lib().raw("vmtl_conv3x3_wgrad_small_supported")(Cs, ldy, W):
        pytest.skip(f"Cs {Cs}, ldy {ldy}: this class did not beat conv_wgrad_kernel and stays off the strip kernel (DESIGN.md)")
    vmtl_env("VMTL_WS_WIDE_MIN_PIXELS", "1")  # a training step routes the classes added last from 65,536 pixels; here: always
    g = torch.Generator().manual_seed(2468)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    gy = torch.randn(B, Cout, H, W, generator=g)
    w64 = w.double().requires_grad_(True)
    F.conv2d(x.double(), w64, None, padding=1).backward(gy.double())
    got = {}
    for mode, target in (("strip", None), ("strip_bands", 4096), ("general", None)):
        vmtl_env("VMTL_WGRAD_SMALL", "0" if mode == "general" else "1")
        if target:
            vmtl_env("VMTL_WS_TARGET", str(target))
        with poison.patched("guard"):
            wd = w.to(dev).requires_grad_(True)
            y = ops.conv2d(to_dev_nhwc(x, dev), wd, None, stride=1, pad=1)
            y.backward(to_dev_nhwc(gy, dev))
            got[mode] = wd.grad.cpu()
    for mode, v in got.items():
        print(f"{case} {mode}: max-abs error {(v.double() - w64.grad).abs().max().item():.3e} of {w64.grad.abs().max().item():.3e}")
    for mode, v in got.items():
        assert_close(v, w64.grad, what=f"wgrad {mode} {case}")
    assert not torch.equal(got["strip"], got["general"])  # two kernels (two summation orders) really ran


@pytest.mark.parametrize("shape", [(2, 16, 64, 16, 16, 16),     # narrow: the count of vmtl_conv3x3_wgrad_small_slabs
                                   (2, 128, 1024, 40, 4, 1),    # wide x: 4 bands per strip where a narrow layer has 16
                                   (2, 128, 1024, 16, 40, 40)]) # wide dY: 8 bands per strip against 16
def test_wgrad_strip_rejects_a_wrong_slab_count(dev, shape):
    """The entry point checks nslabs against the geometry of THIS layer's widths: a wide layer runs fewer segments, and
    the count of a narrow layer of the same extent is refused for it."""
    L = _lib()
    B, H, W, Cs, ldy, Nw = shape
    ns = L.raw("vmtl_conv3x3_wgrad_small_slabs_for")(B, H, W, Cs, ldy, Nw)
    narrow = L.raw("vmtl_conv3x3_wgrad_small_slabs")(B, H, W)
    assert ns > 0
    wrong = [ns + 1, ns - 1, 0]
    if max(Cs, ldy) > 36:
        assert narrow > ns, "the shape must be one where the two queries differ"
        wrong.append(narrow)
    else:
        assert narrow == ns
    x = torch.zeros(B, H, W, Cs, device=dev)
    dy = torch.zeros(B, H, W, ldy, device=dev)
    slabs = torch.zeros(max(ns, narrow) + 1, Nw, 9 * Cs, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    fn = L.raw("vmtl_conv3x3_wgrad_small")
    for n in wrong:
        assert fn(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), n, B, H, W, Cs, ldy, Nw, st) == -1, n  # VMTL_ERR_ARG
    assert fn(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), ns, B, H, W, Cs, ldy, Nw, st) == 0
    torch.cuda.synchronize()
