"""-m gpu: the depth loss with multi-scale gradient matching (csrc/depth_grad.hip) through the C ABI (vmtl_depth_grad_fwd /
vmtl_depth_grad_bwd) and through the node (ops.depth_loss, losses.GradientMatchingLoss / SILogGradLoss), every launch
under poison.patched("guard") and launch_guard.patched().

What is decided and what is rounded are checked apart.  The device's `resid` is checked per pixel against fp64
log pred - log target within 2^-19 * max(1, |log pred|, |log target|) (the bound tests/test_ohem_kernels_gpu.py derives for
one logf pair and a subtraction: 16 fp32 ulps at the logs' magnitude), exactly 0 at invalid pixels, and the counts N_k
exactly.  Loss, terms and gradient are then compared with the fp64 oracle evaluated WITH THE DEVICE'S SIGNS
(depth_grad_oracle.reference(signs_from=resid)): loss within 1e-5 relative, gradient within 1e-4 of its magnitude (the
bounds of tests/test_loss_ignore_gpu.py for SILog), and every pair whose device sign differs from the fp64 sign must have
|dR_fp64| within the two ends' residual bounds - a flip is legitimate only inside the rounding band.  Against the pure
fp64 oracle, signs included, only on the inputs built with a margin (|dR| >= 2^-10 at steps 1..8, asserted first); scales
5 and 6 are covered by the signs_from path only (every small case at 4, 5 and 6 scales), since that period-16 field ties
at step 16."""
import contextlib
import functools
import math

import pytest
import torch

from tests import depth_grad_oracle as O, launch_guard, poison
from tests.util import assert_close

pytestmark = pytest.mark.gpu

GOUT = O.GOUT
SMALL = sorted(n for n in O.CASES if not n.startswith(("cap", "long")))
WEIGHTS = ((1.0, 0.5), (0.0, 1.0))


def _ops():
    from vision_mtl_amd import ops

    return ops


def _bits(x):
    return x.contiguous().view(torch.int32)


@contextlib.contextmanager
def _guarded():
    with poison.patched("guard") as p, launch_guard.patched():
        yield p


def _abi(dev, pred, target, mask, scales, sw, gw, min_depth=O.MIN_DEPTH, gout=GOUT):
    """vmtl_depth_grad_fwd + vmtl_depth_grad_bwd on device tensors [B][H][W]; resid and dpred start out as the poison
    sentinel, so a pixel the kernels skip shows.  Everything comes back as written, on the device."""
    ops = _ops()
    from vision_mtl_amd._lib import lib

    B, H, W = pred.shape
    loss, terms, stats = ops._empty((), pred), ops._empty((2,), pred), ops._empty((3,), pred)
    resid, d = ops._empty((B, H, W), pred), ops._empty((B, H, W), pred)
    _bits(resid).fill_(poison.SENTINEL)
    _bits(d).fill_(poison.SENTINEL)
    counts = torch.full((scales,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(lib().raw("vmtl_depth_grad_workspace_bytes")(B, H, W, scales) // 8, dtype=torch.float64, device=dev)
    geom = dict(B=B, H=H, W=W, scales=scales, silog_weight=sw, grad_weight=gw)
    ops._k("vmtl_depth_grad_fwd", pred=pred, target=target, mask=mask, min_depth=min_depth, loss=loss, terms=terms,
           stats=stats, counts=counts, resid=resid, workspace=ws, **geom)
    g = torch.tensor(gout, device=dev)
    ops._k("vmtl_depth_grad_bwd", pred=pred, target=target, mask=mask, min_depth=min_depth, resid=resid, stats=stats,
           counts=counts, grad_out=g, dpred=d, **geom)
    return dict(loss=loss, terms=terms, stats=stats, counts=counts, resid=resid, grad=d)


def _dev_case(c, dev):
    return c["pred"].to(dev), c["target"].to(dev)


@functools.lru_cache(maxsize=None)
def _bound(name):
    c = O.case(name)
    return O.resid_bound(c["pred"], c["target"], c["valid"])


def _check_resid_and_counts(c, out, scales):
    valid, resid = c["valid"], out["resid"].cpu()
    assert not poison.is_sentinel(resid).any() and not poison.is_sentinel(out["grad"].cpu()).any()
    assert bool((_bits(resid[~valid]) == 0).all())
    err = (resid.double() - O.resid64(c["pred"], c["target"], valid)).abs()
    bound = _bound(c["name"])
    assert bool((err[valid] <= bound[valid]).all()), f"resid error {float((err[valid] / bound[valid]).max()):.3f} of its bound"
    want = [int(valid[:, ::1 << k, ::1 << k].sum()) for k in range(scales)]
    assert out["counts"].cpu().tolist() == want
    return float((err[valid] / bound[valid]).max()) if valid.any() else 0.0


def _check_against_device_signs(c, out, scales, sw, gw):
    """loss, terms and gradient against the fp64 oracle that takes each pair's sign from the device's resid"""
    valid = c["valid"]
    r = O.reference(c["pred"], c["target"], valid, scales, sw, gw, signs_from=out["resid"].cpu())
    loss, terms, grad = float(out["loss"]), out["terms"].cpu(), out["grad"].cpu()
    assert bool((_bits(grad[~valid]) == 0).all())  # +0.0f bit for bit
    flips, bound = r["flips"], _bound(c["name"]).flatten()
    assert bool((flips["absdr"] <= bound[flips["i"]] + bound[flips["j"]]).all()), "a sign flipped outside the rounding band"
    if sw != 0 and int(valid.sum()) < 2:
        assert math.isnan(loss) and math.isnan(float(terms[0]))
        return r
    assert abs(loss - float(r["loss"])) <= 1e-5 * abs(float(r["loss"])), (loss, float(r["loss"]))
    assert abs(float(terms[0]) - float(r["silog"])) <= 1e-5 * abs(float(r["silog"]))
    assert abs(float(terms[1]) - float(r["lgrad"])) <= 1e-5 * abs(float(r["lgrad"]))
    assert not torch.isnan(grad).any()
    assert_close(grad, r["grad"], tol=1e-4, what="depth loss gradient")
    return r


@pytest.mark.parametrize("scales", [4, 5, 6])
@pytest.mark.parametrize("name", SMALL)
def test_resid_counts_and_arithmetic_with_the_device_signs(dev, name, scales):
    c = O.case(name)
    pred, target = _dev_case(c, dev)
    with _guarded():
        for sw, gw in WEIGHTS:
            out = _abi(dev, pred, target, None, scales, sw, gw)
            worst = _check_resid_and_counts(c, out, scales)
            r = _check_against_device_signs(c, out, scales, sw, gw)
            print(f"{name}, scales {scales}, weights ({sw}, {gw}): loss {float(out['loss']):.8g} (fp64 {float(r['loss']):.8g}), "
                  f"N_k {out['counts'].tolist()}, resid error {worst:.3f} of its bound, flips {r['flips']['absdr'].numel()}")


def test_above_the_partial_count_cap(dev):
    """5x512x512 = 1280 blocks' worth of pixels on the 1024 blocks of 1024 pixels the forward is capped at (and 5120
    on the 4096 blocks of 256 pixels of the backward)"""
    c = O.case("cap-holes")
    pred, target = _dev_case(c, dev)
    with _guarded():
        out = _abi(dev, pred, target, None, 4, 1.0, 0.5)
        _check_resid_and_counts(c, out, 4)
        _check_against_device_signs(c, out, 4, 1.0, 0.5)


def test_a_row_too_long_for_int_offsets_takes_the_64_bit_index_kernels(dev):
    """W > 2^24: 32 * W, the farthest neighbour's offset, is no longer kept in an int, so the long long instantiations
    run (1x1x(2^24+8): one row, no y pairs).  Indices past 2^31 need buffers of 8 GiB and are not exercised."""
    c = O.case("long-holes")
    assert c["shape"][2] > 1 << 24
    pred, target = _dev_case(c, dev)
    with _guarded():
        out = _abi(dev, pred, target, None, 3, 1.0, 0.5)
        _check_resid_and_counts(c, out, 3)
        _check_against_device_signs(c, out, 3, 1.0, 0.5)


@pytest.mark.parametrize("name", ["odd-checker", "edge-checker", "seams-checker"])
def test_checkerboard_has_no_pair_at_step_one_and_all_at_step_two(dev, name):
    c = O.case(name)
    pred, target = _dev_case(c, dev)
    B, H, W = c["shape"]
    with _guarded():
        one = _abi(dev, pred, target, None, 1, 0.0, 1.0)
        two = _abi(dev, pred, target, None, 2, 0.0, 1.0)
    assert int(_bits(one["loss"])) == 0 and bool((_bits(one["grad"]) == 0).all())
    assert two["counts"].tolist() == [int(c["valid"].sum()), B * ((H + 1) // 2) * ((W + 1) // 2)]
    assert float(two["loss"]) > 0 and float(two["terms"][1]) == float(two["loss"])


@pytest.mark.parametrize("name", ["odd-dead", "seams-dead"])
def test_wholly_invalid_batch_with_the_term_alone_is_exactly_zero(dev, name):
    c = O.case(name)
    pred, target = _dev_case(c, dev)
    with _guarded():
        out = _abi(dev, pred, target, None, 4, 0.0, 1.0)
        masked = _abi(dev, pred, torch.full_like(target, 0.3), torch.zeros(c["shape"], dtype=torch.uint8, device=dev), 4, 0.0, 1.0)
    for o in (out, masked):
        assert int(_bits(o["loss"])) == 0
        assert bool((_bits(o["grad"]) == 0).all()) and bool((_bits(o["resid"]) == 0).all())
        assert o["counts"].tolist() == [0, 0, 0, 0]
        assert not torch.isnan(o["terms"]).any() and not torch.isnan(o["stats"]).any()


@pytest.mark.parametrize("name", ["odd-holes", "seams-deadimage", "wide-holes"])
def test_mask_dtypes_and_min_depth_agree_bit_for_bit(dev, name):
    c = O.case(name)
    pred, target = _dev_case(c, dev)
    ops = _ops()
    vb = c["valid"].to(dev)
    with _guarded():
        plain = _abi(dev, pred, target, None, 4, 1.0, 0.5)
        u8 = _abi(dev, pred, target, vb.to(torch.uint8), 4, 1.0, 0.5)
        nodes = []
        for mask in (None, vb, vb.to(torch.uint8)):
            p = pred.clone().requires_grad_(True)
            loss = ops.depth_loss(p.unsqueeze(3), target.unsqueeze(3), mask=None if mask is None else mask.unsqueeze(3))
            (loss * GOUT).backward()
            nodes.append((loss.detach(), p.grad))
    for k in ("loss", "terms", "stats", "counts", "resid", "grad"):
        assert torch.equal(plain[k].view(torch.int32), u8[k].view(torch.int32)), k
    for loss, grad in nodes:
        assert torch.equal(_bits(loss), _bits(plain["loss"])) and torch.equal(_bits(grad), _bits(plain["grad"]))
    # a mask takes the place of min_depth: with every target above it, the mask alone decides
    with _guarded():
        full_t = torch.where(vb, target, torch.full_like(target, 0.2))
        m = _abi(dev, pred, full_t, vb.to(torch.uint8), 4, 1.0, 0.5)
    assert torch.equal(_bits(m["loss"]), _bits(plain["loss"])) and torch.equal(_bits(m["grad"]), _bits(plain["grad"]))


@pytest.mark.parametrize("scales", [1, 4])
@pytest.mark.parametrize("name", O.MARGIN_CASES)
def test_against_the_pure_fp64_oracle_signs_included(dev, name, scales):
    c = O.case(name)
    valid = c["valid"]
    m = O.margin(c["pred"], c["target"], valid, O.MARGIN_SCALES)
    need = 2 * float(_bound(name).max())
    assert m > 0.99 * O.MARGIN and m > 10 * need, f"{name}: margin {m:.3e}, rounding band {need:.3e}"
    pred, target = _dev_case(c, dev)
    with _guarded():
        for sw, gw in WEIGHTS:
            out = _abi(dev, pred, target, None, scales, sw, gw)
            _check_resid_and_counts(c, out, scales)
            dev_signs = _check_against_device_signs(c, out, scales, sw, gw)
            assert dev_signs["flips"]["absdr"].numel() == 0
            if sw != 0 and int(valid.sum()) < 2:
                continue
            r = O.reference(c["pred"], c["target"], valid, scales, sw, gw)
            assert abs(float(out["loss"]) - float(r["loss"])) <= 1e-5 * abs(float(r["loss"]))
            assert_close(out["grad"].cpu(), r["grad"], tol=1e-4, what="gradient against the pure fp64 oracle")


def test_term_alone_is_finite_with_fewer_than_two_valid_pixels_and_silog_is_nan(dev):
    ops = _ops()
    one_p, one_t = torch.full((1, 1, 1), 0.4, device=dev), torch.full((1, 1, 1), 0.2, device=dev)
    p = torch.full((1, 6, 9), 0.4, device=dev)
    t = torch.zeros(1, 6, 9, device=dev)
    t[0, 2, 4] = 0.2  # a single valid pixel
    with _guarded():
        for pp, tt in ((one_p, one_t), (p, t)):
            out = _abi(dev, pp, tt, None, 4, 0.0, 1.0)
            assert int(_bits(out["loss"])) == 0 and bool((_bits(out["grad"]) == 0).all())
            assert not torch.isnan(out["terms"]).any() and not torch.isnan(out["stats"]).any()
            assert out["counts"][0].item() == 1
            on = _abi(dev, pp, tt, None, 4, 1.0, 0.5)
            assert math.isnan(float(on["loss"])) and math.isnan(float(on["terms"][0])) and float(on["terms"][1]) == 0.0
            assert math.isnan(float(ops.silog(pp, tt)))  # as the SILog node


def test_non_positive_prediction_on_a_valid_pixel_is_nan_or_inf_and_on_an_invalid_one_is_not_seen(dev):
    c = O.case("seams-holes")
    pred, target = _dev_case(c, dev)
    valid = c["valid"]
    iv = (~valid).flatten().nonzero()[7].item()
    pair = torch.zeros_like(valid)
    pair[:, :, :-1] = valid[:, :, :-1] & valid[:, :, 1:]  # a valid pixel with a valid right neighbour: it is in a pair
    vv = pair.flatten().nonzero()[11].item()
    with _guarded():
        base = _abi(dev, pred, target, None, 4, 1.0, 0.5)
        for bad in (-0.25, 0.0):
            p = pred.clone()
            p.view(-1)[iv] = bad
            same = _abi(dev, p, target, None, 4, 1.0, 0.5)
            for k in ("loss", "terms", "resid", "grad"):
                assert torch.equal(_bits(same[k]), _bits(base[k])), (bad, k)
        p = pred.clone()
        p.view(-1)[vv] = -0.25
        for sw, gw in WEIGHTS:
            assert math.isnan(float(_abi(dev, p, target, None, 4, sw, gw)["loss"]))
        # pred == 0: R = -inf.  SILog's mean and variance turn NaN; the term alone sums |R' - (-inf)| = +inf (eager torch too)
        p.view(-1)[vv] = 0.0
        assert math.isnan(float(_abi(dev, p, target, None, 4, 1.0, 0.5)["loss"]))
        alone = _abi(dev, p, target, None, 4, 0.0, 1.0)
        assert float(alone["loss"]) == math.inf and float(alone["resid"].view(-1)[vv]) == -math.inf
        r = O.reference(p.cpu(), c["target"], valid, 4, 0.0, 1.0)
        assert float(r["loss"]) == math.inf


@pytest.mark.parametrize("name", ["wide-holes", "cap-holes"])
def test_two_runs_agree_bit_for_bit(dev, name):
    c = O.case(name)
    pred, target = _dev_case(c, dev)
    with _guarded():
        a = _abi(dev, pred, target, None, 4, 1.0, 0.5)
        b = _abi(dev, pred, target, None, 4, 1.0, 0.5)
    for k in ("loss", "terms", "stats", "counts", "resid", "grad"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


@pytest.mark.parametrize("name", ["odd-holes", "seams-holes"])
def test_node_returns_the_abi_bits_in_every_layout_and_honours_grad_out(dev, name):
    from vision_mtl_amd.losses import GradientMatchingLoss, SILogGradLoss

    ops = _ops()
    c = O.case(name)
    pred, target = _dev_case(c, dev)
    B, H, W = c["shape"]
    with _guarded():
        abi = _abi(dev, pred, target, None, 3, 1.0, 0.25)
        for shape in ((B, H, W, 1), (B, 1, H, W), (B, H, W)):
            p = pred.clone().view(shape).requires_grad_(True)
            loss = ops.depth_loss(p, target.view(shape), grad_weight=0.25, scales=3)
            assert loss.shape == () and loss.is_cuda
            (loss * GOUT).backward()
            assert p.grad.shape == p.shape
            assert torch.equal(_bits(loss.detach()), _bits(abi["loss"]))
            assert torch.equal(_bits(p.grad.view(B, H, W)), _bits(abi["grad"]))
        # grad_out against fp64 (not by bits: 0.37 * g and g are rounded apart)
        r = O.reference(c["pred"], c["target"], c["valid"], 3, 1.0, 0.25, signs_from=abi["resid"].cpu(), gout=GOUT)
        unit = O.reference(c["pred"], c["target"], c["valid"], 3, 1.0, 0.25, signs_from=abi["resid"].cpu(), gout=1.0)
        assert_close(abi["grad"].cpu(), r["grad"], tol=1e-4, what="gradient under grad_out = 0.37")
        assert_close(r["grad"], GOUT * unit["grad"], tol=1e-12, what="the oracle's own grad_out")
        p1 = pred.clone().requires_grad_(True)
        ops.depth_loss(p1, target, grad_weight=0.25, scales=3).backward()
        assert_close(p1.grad.cpu(), unit["grad"], tol=1e-4, what="gradient under grad_out = 1")
        # the two criteria are the op with their weights
        p2, p3 = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
        both = SILogGradLoss(grad_weight=0.25, scales=3)(p2.unsqueeze(3), target.unsqueeze(3))
        assert torch.equal(_bits(both.detach()), _bits(abi["loss"]))
        term = GradientMatchingLoss(scales=3)(p3, target)
        alone = _abi(dev, pred, target, None, 3, 0.0, 1.0, gout=1.0)
        term.backward()
        assert torch.equal(_bits(term.detach()), _bits(alone["loss"])) and torch.equal(_bits(p3.grad), _bits(alone["grad"]))
        assert abs(float(term.detach()) - float(abi["terms"][1])) <= 1e-6 * float(term.detach())


@pytest.mark.parametrize("name", ["odd-holes", "seams-deadimage", "wide-holes"])
def test_the_silog_part_is_the_silog_node(dev, name):
    ops = _ops()
    c = O.case(name)
    pred, target = _dev_case(c, dev)
    with _guarded():
        out = _abi(dev, pred, target, None, 4, 1.0, 0.5)
        ref = ops.silog(pred, target)
    assert abs(float(out["terms"][0]) - float(ref)) <= 1e-5 * abs(float(ref)), (float(out["terms"][0]), float(ref))
