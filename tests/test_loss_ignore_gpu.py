"""-m gpu: the weighted / ignoring cross entropy (vmtl_ce_fwd_ex / vmtl_ce_bwd_ex through ops.cross_entropy(weight=,
ignore_index=)), SILog with an explicit mask (vmtl_silog_*_mask) and the metrics with an ignore index
(vmtl_confusion_matrix_ex / vmtl_segm_metrics_ex).

References: torch.nn.functional.cross_entropy on the CPU in fp64; reference losses.py:29-36 restated in fp64; the metric
definitions restated in numpy.  Tolerances are those of the unweighted tests of the same kernels (the same arithmetic
with one more multiply): |loss - ref| < 1e-5 as tests/test_surface_gpu.py::test_cross_entropy_with_argmax_matches_
separate_ops, gradient 1e-5 of its magnitude as tests/test_kernels_gpu.py::test_cross_entropy, SILog 1e-5 (loss) / 1e-4
(gradient) as test_silog_l1_sigmoid there, derived metrics 1e-6 as test_segm_metrics_match_definitions."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import poison
from tests.util import assert_close

pytestmark = pytest.mark.gpu

IGN = 255
GOUT = 1.7  # the loss is scaled before backward: grad_output is not 1
# name: (C, B, H, W).  a: ragged last wave; b, c: the rows kernel at ld = 16 / 20; d: ld = 24 != 4*ceil(C/4), the wide-ld
# NHWC kernel; e: past the 32 logits the register forms hold; f: P = 526 683 > 2048 * 256, the grid-stride loop and block cap;
# g, h, i, j: Q = ceil(C/4) = 3, 6, 7, 8 at C % 4 != 0 (the rows kernel), the cases of the Q switches that a, b, c leave out
CASES = {"a": (3, 2, 5, 13), "b": (14, 2, 5, 13), "c": (19, 2, 5, 13), "d": (20, 2, 5, 13), "e": (33, 2, 5, 13),
         "f": (3, 3, 419, 419), "g": (9, 2, 5, 13), "h": (22, 2, 5, 13), "i": (26, 2, 5, 13), "j": (30, 2, 5, 13)}
COMBOS = ("ignore", "weight", "both")


def _ops():
    from vision_mtl_amd import ops

    return ops


def _ceil4(c):
    return (c + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def _case(name, combo):
    """Inputs on the CPU and the fp64 reference (loss, gradient of GOUT * loss), computed once per (case, combination)."""
    C, B, H, W = CASES[name]
    g = torch.Generator().manual_seed(1000 + 17 * sorted(CASES).index(name) + COMBOS.index(combo))
    z = torch.randn(B, C, H, W, generator=g) * 3
    z[:, 0] = z[:, min(2, C - 1)]  # ties: the first maximum wins
    t = torch.randint(0, C, (B, H, W), generator=g)
    ign = IGN if combo != "weight" else None
    if ign is not None:
        t[torch.rand(B, H, W, generator=g) < 0.3] = ign
    w = 0.1 + 1.9 * torch.rand(C, generator=g) if combo != "ignore" else None
    zr = z.double().requires_grad_(True)
    lr = F.cross_entropy(zr, t, weight=None if w is None else w.double(), ignore_index=-100 if ign is None else ign)
    (lr * GOUT).backward()
    return dict(C=C, shape=(B, H, W), z=z, t=t, w=w, ign=ign, loss=lr.detach(), grad=zr.grad)


def _dev_inputs(c, dev):
    return c["z"].to(dev), c["t"].to(dev), None if c["w"] is None else c["w"].to(dev)


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_argmax_and_backward_match_torch(dev, name, combo):
    """Forward, fused-argmax forward and the backward the node runs (NHWC rows of ceil4(C+1) floats: the rows kernel for
    a, b, c, f, g, h, i, j; the wide-ld kernel for d and e) against torch in fp64; the argmax at every pixel, ignored
    ones included; ignored rows bitwise 0.0; no NaN anywhere."""
    ops = _ops()
    c = _case(name, combo)
    z, t, w = _dev_inputs(c, dev)
    z1, z2 = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    l1 = ops.cross_entropy(z1, t, weight=w, ignore_index=c["ign"])
    l2, pred = ops.cross_entropy_with_argmax(z2, t, weight=w, ignore_index=c["ign"])
    ref = c["loss"].item()
    print(f"{name}/{combo}: loss {l1.item():.8g} (torch fp64 {ref:.8g})")
    assert abs(l1.item() - ref) < 1e-5
    assert torch.equal(l1, l2)
    assert torch.equal(pred, ops.argmax_channels(z))
    assert torch.equal(pred.cpu(), c["z"].argmax(dim=1))
    (l1 * GOUT).backward()
    (l2 * GOUT).backward()
    assert torch.equal(z1.grad, z2.grad)
    gd = z1.grad.cpu()
    print(f"{name}/{combo}: gradient max-abs error {float((gd.double() - c['grad']).abs().max()):.3e} of "
          f"{float(c['grad'].abs().max()):.3e}")
    assert not torch.isnan(gd).any()
    assert_close(gd, c["grad"], tol=1e-5, what="weighted / ignoring CE gradient")
    if c["ign"] is not None:
        rows = gd.permute(0, 2, 3, 1)[c["t"] == c["ign"]]
        assert rows.numel() > 0 and bool((_bits(rows) == 0).all())  # +0.0 bit for bit


class _Probe(torch.autograd.Function):
    """Identity whose backward records the gradient it is handed, as a head's data-gradient node receives it."""
    seen = None

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        _Probe.seen = (dy.stride(), tuple(dy.shape), getattr(dy, "_vmtl_nhwc", None))
        return dy


@pytest.mark.parametrize("name", ["c", "d"])
def test_gradient_hand_off_is_the_nhwc_view(dev, name):
    """The node returns the (B,C,H,W) view of [B][H][W][ceil4(C+1)] storage with _vmtl_nhwc set, as _CrossEntropy.backward
    does: the consumer (ops.decoder_tail) takes the storage without a relayout."""
    ops = _ops()
    c = _case(name, "both")
    C, (B, H, W) = c["C"], c["shape"]
    z, t, w = _dev_inputs(c, dev)
    ld = _ceil4(C + 1)
    for fused in (False, True):
        zd = z.clone().requires_grad_(True)
        f = ops.cross_entropy_with_argmax if fused else ops.cross_entropy
        out = f(_Probe.apply(zd), t, weight=w, ignore_index=IGN)
        _Probe.seen = None
        (out[0] if fused else out).backward()
        stride, shape, st = _Probe.seen
        assert shape == (B, C, H, W) and stride == (H * W * ld, 1, W * ld, ld)
        assert st is not None and tuple(st.shape) == (B, H, W, ld)
        if C % 4:  # rows of exactly ceil4(C) floats: the pad lane is zero, as the unweighted rows kernel leaves it
            assert bool((_bits(st[..., C:]) == 0).all())


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_c_abi_layouts_write_the_lanes_the_unweighted_kernels_write(dev, name):
    """vmtl_ce_bwd_ex called directly in the three layouts - NHWC rows of exactly ceil4(C) floats, NHWC with a wider ld,
    plain NCHW strides - on sentinel-filled buffers: the values match torch, and the set of written elements is the one
    vmtl_ce_bwd_strided writes (ops.decoder_tail owns the lanes beyond)."""
    ops = _ops()
    from vision_mtl_amd._lib import lib

    c = _case(name, "both")
    C, (B, H, W) = c["C"], c["shape"]
    HW, P = H * W, B * H * W
    z, t, w = _dev_inputs(c, dev)
    loss, stats = torch.empty((), device=dev), torch.empty(2, device=dev)
    ws = torch.empty(lib().raw("vmtl_ce_ex_workspace_bytes")(P) // 8, dtype=torch.float64, device=dev)
    ops._k("vmtl_ce_fwd_ex", logits=z, target=t, weight=w, ignore_index=IGN, loss=loss, stats=stats, workspace=ws,
           argmax=None, B=B, HW=HW, C=C, sb=C * HW, sc=HW, sp=1)
    valid = c["t"] != IGN
    den = float(c["w"][c["t"][valid]].double().sum())
    assert abs(stats[0].item() - den) <= 1e-6 * den
    assert abs(stats[1].item() / stats[0].item() - c["loss"].item()) < 1e-5
    gout = torch.tensor(GOUT, device=dev)
    lds = [_ceil4(C), _ceil4(C) + 4, _ceil4(C) + 8]
    layouts = [("nhwc", ld, (B, H, W, ld), (HW * ld, 1, ld)) for ld in lds] + [("nchw", 0, (B, C, H, W), (C * HW, HW, 1))]
    for kind, ld, shape, (dsb, dsc, dsp) in layouts:
        bufs = []
        for ex in (True, False):
            d = torch.empty(shape, device=dev)
            _bits(d).fill_(poison.SENTINEL)
            kw = dict(logits=z, target=t, grad_out=gout, dlogits=d, B=B, HW=HW, C=C, sb=C * HW, sc=HW, sp=1, dsb=dsb,
                      dsc=dsc, dsp=dsp)
            if ex:
                ops._k("vmtl_ce_bwd_ex", weight=w, ignore_index=IGN, stats=stats, **kw)
            else:
                ops._k("vmtl_ce_bwd_strided", **kw)
            bufs.append(d)
        dex, dun = bufs
        assert torch.equal(poison.is_sentinel(dex), poison.is_sentinel(dun)), f"{kind} ld={ld}: other lanes written"
        got = (dex[..., :C].permute(0, 3, 1, 2) if kind == "nhwc" else dex).cpu()
        assert not torch.isnan(got).any()
        assert_close(got, c["grad"], tol=1e-5, what=f"{kind} ld={ld}")
        rows = got.permute(0, 2, 3, 1)[~valid]
        assert bool((_bits(rows) == 0).all())
        if kind == "nhwc":
            pad = dex[..., C:_ceil4(C)]
            assert pad.numel() == 0 or bool((_bits(pad) == 0).all())  # the pad lanes of a row are zeros, as unweighted


def test_ignore_index_inside_the_class_range(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    C = 14
    z = torch.randn(2, C, 5, 13, generator=g) * 3
    t = torch.randint(0, C, (2, 5, 13), generator=g)
    w = 0.1 + 1.9 * torch.rand(C, generator=g)
    assert int((t == 2).sum()) > 0
    for wt in (None, w):
        zr = z.double().requires_grad_(True)
        lr = F.cross_entropy(zr, t, weight=None if wt is None else wt.double(), ignore_index=2)
        lr.backward()
        zd = z.to(dev).requires_grad_(True)
        l = ops.cross_entropy(zd, t.to(dev), weight=None if wt is None else wt.to(dev), ignore_index=2)
        l.backward()
        assert abs(l.item() - lr.item()) < 1e-5
        assert_close(zd.grad.cpu(), zr.grad, tol=1e-5, what="CE gradient, ignore_index = class 2")
        assert bool((_bits(zd.grad.cpu().permute(0, 2, 3, 1)[t == 2]) == 0).all())


@pytest.mark.parametrize("C", [14, 33])
def test_out_of_range_targets_are_nan_not_silent(dev, C):
    """A target outside [0, C) that is NOT the ignore index is NaN in the loss and in its gradient row (never a silent 0,
    and never an index into the weight table); a batch in which every pixel is ignored is NaN (0/0), as torch."""
    ops = _ops()
    g = torch.Generator().manual_seed(C)
    z = torch.randn(2, C, 5, 13, generator=g).to(dev)
    t = torch.randint(0, C, (2, 5, 13), generator=g).to(dev)
    t[1, 2, 3] = IGN
    w = (0.1 + 1.9 * torch.rand(C, generator=g)).to(dev)
    for bad in (C, -1):
        for wt in (None, w):
            tb = t.clone()
            tb[0, 1, 2] = bad
            zd = z.clone().requires_grad_(True)
            loss, pred = ops.cross_entropy_with_argmax(zd, tb, weight=wt, ignore_index=IGN)
            assert torch.isnan(loss)
            assert torch.equal(pred, ops.argmax_channels(z))
            loss.backward()
            assert torch.isnan(zd.grad[0, :, 1, 2]).all()
            assert bool((_bits(zd.grad[1, :, 2, 3]) == 0).all())
    zd = z.clone().requires_grad_(True)
    loss = ops.cross_entropy(zd, torch.full_like(t, IGN), weight=w, ignore_index=IGN)
    assert torch.isnan(loss)
    loss.backward()
    assert bool((_bits(zd.grad) == 0).all())  # ignored pixels: 0.0f, not 0 * inf


def test_defaults_take_the_unweighted_path(dev):
    ops = _ops()
    from vision_mtl_amd.losses import CrossEntropyLoss

    c = _case("c", "weight")
    z, t, _ = _dev_inputs(c, dev)
    names, orig = [], ops._k

    def rec(name, *a, **kw):
        names.append(name)
        return orig(name, *a, **kw)

    z1, z2 = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    ops._k = rec
    try:
        crit = CrossEntropyLoss()
        l1 = crit(z1, t)
        l1.backward()
        lp, pred = crit.forward_with_predictions(z, t)
    finally:
        ops._k = orig
    assert names == ["vmtl_ce_fwd", "vmtl_ce_bwd_strided", "vmtl_ce_fwd_argmax"]
    l2 = ops.cross_entropy(z2, t)
    l2.backward()
    assert torch.equal(l1, l2) and torch.equal(lp, l2) and torch.equal(z1.grad, z2.grad)
    assert torch.equal(pred, ops.argmax_channels(z))
    # weight = ones and nothing ignored: the unweighted loss, within the tolerance
    z3 = z.clone().requires_grad_(True)
    l3 = ops.cross_entropy(z3, t, weight=torch.ones(c["C"], device=dev))
    l3.backward()
    assert abs(l3.item() - l2.item()) < 1e-5
    assert_close(z3.grad, z2.grad, tol=1e-5, what="weight = ones")


@pytest.mark.parametrize("name", ["c", "f"])
def test_two_runs_are_bit_identical(dev, name):
    ops = _ops()
    c = _case(name, "both")
    z, t, w = _dev_inputs(c, dev)
    runs = []
    for _ in range(2):
        zd = z.clone().requires_grad_(True)
        l = ops.cross_entropy(zd, t, weight=w, ignore_index=IGN)
        l.backward()
        runs.append((l.detach().clone(), zd.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_argument_checks(dev):
    ops = _ops()
    z = torch.randn(1, 5, 4, 4, device=dev)
    t = torch.zeros(1, 4, 4, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="weight"):
        ops.cross_entropy(z, t, weight=torch.ones(4, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cross_entropy(z, t, weight=torch.ones(5))
    with pytest.raises(TypeError):
        ops.cross_entropy(z, t, weight=torch.ones(5, device=dev, dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.cross_entropy(z, t, ignore_index=2.5)
    w = torch.ones(5, device=dev, requires_grad=True)
    zd = z.clone().requires_grad_(True)
    ops.cross_entropy(zd, t, weight=w).backward()
    assert w.grad is None and zd.grad is not None  # the weight receives no gradient


# ------------------------------------------------------------------------------------------------ SILog with a mask
def _silog_ref(pred, target, mask):
    """reference losses.py:29-36 in fp64"""
    p = pred.double().requires_grad_(True)
    g = torch.log(p[mask]) - torch.log(target.double()[mask])
    loss = 10 * torch.sqrt(torch.var(g) + 0.15 * torch.pow(torch.mean(g), 2))
    loss.backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize("P", [130, 4 * 1024 * 1024 + 3])  # the second: above the 1024 blocks x 1024 pixels of sl_blocks
def test_silog_with_mask(dev, P):
    ops = _ops()
    g = torch.Generator().manual_seed(P % 1000)
    shape = (2, 5, 13, 1) if P == 130 else (P,)
    pred = 0.05 + 0.9 * torch.rand(shape, generator=g)
    target = 0.002 + 0.498 * torch.rand(shape, generator=g)
    target[torch.rand(shape, generator=g) < 0.1] = 5e-4  # below min_depth, some of them inside the mask
    mask = torch.rand(shape, generator=g) < 0.7
    lr, gr = _silog_ref(pred, target, mask)
    for m in (mask, mask.to(torch.uint8)):
        pd = pred.to(dev).requires_grad_(True)
        l = ops.silog(pd, target.to(dev), 1e-3, mask=m.to(dev))
        l.backward()
        assert abs(l.item() - lr.item()) <= 1e-5 * abs(lr.item())
        assert_close(pd.grad.cpu(), gr, tol=1e-4, what="masked silog grad")
        assert bool((_bits(pd.grad.cpu()[~mask]) == 0).all())
    # the mask the unmasked node applies itself: the same bits
    own = target > 1e-3
    p1, p2 = pred.to(dev).requires_grad_(True), pred.to(dev).requires_grad_(True)
    l1 = ops.silog(p1, target.to(dev), 1e-3)
    l2 = ops.silog(p2, target.to(dev), 123.0, mask=own.to(dev))  # min_depth is not applied with a mask
    l1.backward()
    l2.backward()
    assert torch.equal(l1, l2) and torch.equal(p1.grad, p2.grad)


def test_silog_mask_misuse_and_loss_class(dev):
    ops = _ops()
    from vision_mtl_amd.losses import SILogLoss

    pred = (0.05 + 0.9 * torch.rand(2, 5, 13, 1)).to(dev)
    target = (0.002 + 0.498 * torch.rand(2, 5, 13, 1)).to(dev)
    with pytest.raises(ValueError, match="mask"):
        ops.silog(pred, target, 1e-3, mask=torch.ones(2, 5, 13, dtype=torch.bool, device=dev))
    with pytest.raises(TypeError):
        ops.silog(pred, target, 1e-3, mask=torch.ones(2, 5, 13, 1, device=dev))
    mask = torch.rand(2, 5, 13, 1, device=dev) < 0.6
    assert torch.equal(SILogLoss()(pred, target, mask=mask), ops.silog(pred, target, 1e-3, mask=mask))
    with pytest.raises(NotImplementedError):  # spatially mismatched pred / target: still no silent resample
        SILogLoss()(pred, target[:, :, :6], mask=mask)


# ------------------------------------------------------------------------------------------------ metrics
def _metrics_np(pred, target, C, ign, beta=1.0):
    """The definitions of csrc/metrics.hip with an ignore index: pixels whose target equals it are dropped; a class in
    [0, C) is left out of the Jaccard class mean; accuracy over the valid pixels; F-beta support-weighted."""
    pred, target = pred.reshape(-1), target.reshape(-1)
    keep = target != ign
    cm = np.bincount(target[keep] * C + pred[keep], minlength=C * C).reshape(C, C)
    tp = np.diag(cm).astype(np.float64)
    row, col = cm.sum(1).astype(np.float64), cm.sum(0).astype(np.float64)
    fn, fp = row - tp, col - tp
    acc = tp.sum() / cm.sum()
    uni = tp + fp + fn
    j = np.where(uni > 0, tp / np.maximum(uni, 1), 0.0)
    jac = np.mean([j[c] for c in range(C) if c != ign])
    b2 = beta * beta
    den = (1 + b2) * tp + b2 * fn + fp
    f = np.where(den > 0, (1 + b2) * tp / np.maximum(den, 1), 0.0)
    return cm, acc, jac, (f * row).sum() / row.sum()


@pytest.mark.parametrize("ign", [255, 3])
@pytest.mark.parametrize("C", [14, 19])
def test_metrics_with_ignore_index(dev, C, ign):
    from vision_mtl_amd import metrics as M

    g = torch.Generator().manual_seed(10 * C + ign)
    shape = (3, 40, 56)
    target = torch.randint(0, C - 2, shape, generator=g)  # C-2: a false positive only; C-1: absent from both
    pred = torch.where(torch.rand(shape, generator=g) < 0.6, target, torch.randint(0, C - 1, shape, generator=g))
    target[torch.rand(shape, generator=g) < 0.3] = ign  # an in-range ignore class keeps its own (fewer) pixels as well
    assert int((pred == ign).sum()) > 0 or ign >= C  # predictions of the ignored class on valid pixels count
    cm_ref, acc, jac, fb = _metrics_np(pred.numpy(), target.numpy(), C, ign)
    assert cm_ref[C - 1].sum() == 0 and cm_ref[:, C - 1].sum() == 0 and cm_ref[C - 2].sum() == 0
    cm = M.confusion_matrix(pred.to(dev), target.to(dev), C, ignore_index=ign)
    assert np.array_equal(cm.cpu().numpy().astype(np.int64), cm_ref)  # integer counts: exact
    for cls, ref in ((M.Accuracy, acc), (M.JaccardIndex, jac), (M.FBetaScore, fb)):
        got = float(cls(C, ignore_index=ign)(pred.to(dev), target.to(dev)))
        assert abs(got - ref) <= 1e-6, (cls.__name__, got, ref)
    if ign >= C:  # the existing entry point drops an out-of-range label as "not a class": the same counts
        assert torch.equal(M.confusion_matrix(pred.to(dev), target.to(dev), C), cm)


# ------------------------------------------------------------------------------------------------ poisoned buffers
@pytest.mark.parametrize("C", [19, 20])
def test_ce_nodes_on_poisoned_guard_banded_buffers(dev, C):
    ops = _ops()
    c = _case("c" if C == 19 else "d", "both")
    z, t, w = _dev_inputs(c, dev)
    with poison.patched("guard") as p:
        z1, z2 = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
        l1 = ops.cross_entropy(z1, t, weight=w, ignore_index=IGN)
        l2, pred = ops.cross_entropy_with_argmax(z2, t, weight=w, ignore_index=IGN)
        (l1 * GOUT).backward()
        (l2 * GOUT).backward()
        assert p.count >= 6  # loss, stats and the gradient storage of both nodes came from ops._empty
    for l, zd in ((l1, z1), (l2, z2)):
        assert not poison.is_sentinel(l.reshape(1)).any() and not poison.is_sentinel(zd.grad).any()
        assert abs(l.item() - c["loss"].item()) < 1e-5
        assert_close(zd.grad.cpu(), c["grad"], tol=1e-5, what="CE gradient on guarded buffers")
    assert torch.equal(pred.cpu(), c["z"].argmax(dim=1))


def test_masked_silog_on_poisoned_guard_banded_buffers(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    pred = 0.05 + 0.9 * torch.rand(2, 5, 13, 1, generator=g)
    target = 0.002 + 0.498 * torch.rand(2, 5, 13, 1, generator=g)
    mask = torch.rand(2, 5, 13, 1, generator=g) < 0.7
    lr, gr = _silog_ref(pred, target, mask)
    with poison.patched("guard") as p:
        pd = pred.to(dev).requires_grad_(True)
        l = ops.silog(pd, target.to(dev), 1e-3, mask=mask.to(dev))
        l.backward()
        assert p.count >= 3
    assert not poison.is_sentinel(l.reshape(1)).any() and not poison.is_sentinel(pd.grad).any()
    assert abs(l.item() - lr.item()) <= 1e-5 * abs(lr.item())
    assert_close(pd.grad.cpu(), gr, tol=1e-4, what="masked silog grad on guarded buffers")
