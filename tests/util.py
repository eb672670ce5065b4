"""Test-only helpers: move tensors between the reference's NCHW layout (CPU, torch fp32 = the
oracle side) and the library's padded NHWC layout (GPU side)."""
import torch


def ceil4(c):
    return (c + 3) // 4 * 4


def to_dev_nhwc(x_nchw, dev):
    B, C, H, W = x_nchw.shape
    out = torch.zeros(B, H, W, ceil4(C), dtype=torch.float32)
    out[..., :C] = x_nchw.permute(0, 2, 3, 1)
    return out.to(dev)


def from_dev_nhwc(y, C):
    return y[..., :C].permute(0, 3, 1, 2).contiguous().cpu()


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def assert_close(a, b, tol=1e-4, what="", atol=0.0):
    """max|a-b| <= tol * max|b| + atol.  atol is for quantities that are analytically zero (e.g. the
    gradient of a conv bias that feeds a train-mode BatchNorm), where both sides are rounding noise."""
    a, b = a.double(), b.double()
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= tol * ref + atol, f"{what}: max-abs error {err:.3e} vs reference magnitude {ref:.3e} (tol {tol}, atol {atol})"


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def assert_grads_as_good_as_fp32_cpu(named_hip, g64, g32, floor=5e-2, whole_floor=5e-3, factor=4.0):
    """End-to-end gradient bar for the deep ReLU + train-mode-BatchNorm networks.

    Measured on the MI355X (tools/diag_*.py): every kernel is accurate to 1e-4..1e-6 in
    isolation and every in-network layer backward is BIT-IDENTICAL to its isolated recomputation, yet
    end-to-end gradients of two fp32 implementations differ by ~1e-3 (rel-L2): a pre-activation that is
    ~0 gets a different ReLU mask in one element out of ~5e5, which changes the gradient by O(|g|) in a
    3x3xC neighbourhood and spreads further down.  The fp32 CPU oracle shows the same effect against an
    fp64 run of itself (basic: 3e-3..6e-3).  Hence: per tensor, rel-L2 error vs the fp64 gradient
    <= max(floor, factor x the fp32 CPU oracle's own error); whole gradient <= max(whole_floor, 2 x)."""
    num = den = num32 = 0.0
    worst = (0.0, 0.0, "")
    gmax = max(float(v.abs().max()) for v in g64.values())
    for k, g in named_hip.items():
        ref = g64[k]
        if float(ref.abs().max()) <= 1e-6 * gmax:  # analytically-zero gradients (bias in front of a BatchNorm)
            assert float(g.abs().max()) <= 1e-5 * gmax, f"{k}: expected a (numerically) zero gradient"
            continue
        eh, ec = rel_l2(g, ref), rel_l2(g32[k], ref)
        assert eh <= max(floor, factor * ec), f"grad {k}: rel-L2 error {eh:.2e} (fp32 CPU oracle: {ec:.2e})"
        if eh > worst[0]:
            worst = (eh, ec, k)
        num += float((g.double() - ref.double()).pow(2).sum())
        num32 += float((g32[k].double() - ref.double()).pow(2).sum())
        den += float(ref.double().pow(2).sum())
    tot, tot32 = (num / den) ** 0.5, (num32 / den) ** 0.5
    assert tot <= max(whole_floor, 2.0 * tot32), f"whole-gradient rel-L2 error {tot:.2e} (fp32 CPU oracle: {tot32:.2e})"
    print(f"gradient bar: worst tensor {worst[2]} rel-L2 {worst[0]:.2e} (fp32 CPU oracle {worst[1]:.2e}); whole gradient "
          f"{tot:.2e} (fp32 CPU oracle {tot32:.2e})")
    return tot, tot32


import contextlib


@contextlib.contextmanager
def identity_activations():
    """TEST-ONLY: every ReLU / hardswish / hard-sigmoid of BOTH sides becomes the identity (sigmoid is smooth and stays),
    train-mode BatchNorm kept - a network in which no pre-activation can land on the other side of a kink in one of two
    fp32 implementations, so end-to-end gradients can be held to a TIGHT bar (kernel / indexing errors are no longer
    hidden behind the ReLU-mask-flip noise that justifies assert_grads_as_good_as_fp32_cpu's floors).
    HIP side: the activation codes handed to the C ABI are rewritten in a wrapper around ops._k (nothing in the product
    changes); oracle side: torch.nn.functional.relu / hardswish / hardsigmoid (and the oracle's own lookup table)."""
    import torch.nn.functional as F

    import oracle.unet_mobilenetv3 as ou
    from vision_mtl_amd import ops

    ident = lambda x, *a, **k: x
    saved_f = {n: getattr(F, n) for n in ("relu", "hardswish", "hardsigmoid")}
    saved_tbl = dict(ou._ACT)
    kinked = (ops.ACT_RELU, ops.ACT_HSWISH, ops.ACT_HSIGMOID)
    orig_k = ops._k

    def _k(name, _flop=None, _xflop=None, **kw):
        for key, v in kw.items():
            if (key == "act" or key.endswith("_act") or key.startswith("act")) and isinstance(v, int) and v in kinked:
                kw[key] = ops.ACT_NONE
        return orig_k(name, _flop=_flop, _xflop=_xflop, **kw)

    try:
        for n in saved_f:
            setattr(F, n, ident)
        for key in ou._ACT:
            ou._ACT[key] = ident
        ops._k = _k
        yield
    finally:
        ops._k = orig_k
        ou._ACT.update(saved_tbl)
        for n, f in saved_f.items():
            setattr(F, n, f)


def assert_grads_tight(named_hip, g64, g32, tol=1e-4, factor=4.0):
    """Every parameter gradient within max(tol, factor x the fp32 CPU oracle's own error) of the fp64 gradient, both
    measured as max-abs error over the tensor's max magnitude.  Returns the worst (hip, cpu32) errors."""
    worst = (0.0, 0.0, "")
    gmax = max(float(v.abs().max()) for v in g64.values() if v is not None)
    for k, g in named_hip.items():
        if g64.get(k) is None:  # a parameter the step never uses (CSNet holds stitch layers for non-stitch sites)
            assert float(g.abs().max()) == 0.0, f"{k}: the oracle has no gradient here, the HIP path a non-zero one"
            continue
        ref = g64[k].double()
        mag = float(ref.abs().max())
        if mag <= 1e-6 * gmax:
            assert float(g.abs().max()) <= 1e-5 * gmax, f"{k}: expected a (numerically) zero gradient"
            continue
        eh = float((g.double() - ref).abs().max()) / mag
        ec = float((g32[k].double() - ref).abs().max()) / mag
        assert eh <= max(tol, factor * ec), f"grad {k}: max-abs error {eh:.2e} of its magnitude (fp32 CPU oracle: {ec:.2e})"
        if eh > worst[0]:
            worst = (eh, ec, k)
    return worst


def nontrivial_bn_affine(model, seed=5, scale=0.1):
    """BatchNorm affine parameters (1-D, all 0 or all 1 at construction) moved off their initial values, in place."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1 and p.numel() > 1 and float(p.detach().abs().max()) in (0.0, 1.0):
                p.add_(torch.randn(p.shape, generator=g) * scale)


def worst_of_runs(g64, runs):
    """per tensor, the run (dict of gradients) whose max-abs error against the fp64 gradient is largest"""
    err = lambda g, k: float((g[k].double() - g64[k].double()).abs().max())
    return {k: max(runs, key=lambda g: err(g, k))[k] for k, v in g64.items() if v is not None}


def _metrics_cpu(pred, target, C, beta=1.0):
    """torchmetrics 0.7.3 definitions (package not installable offline: restated from its documentation).
    Accuracy(average="micro"), JaccardIndex(num_classes=C) = mean over classes of tp/(tp+fp+fn) with absent_score 0,
    FBetaScore(average="weighted", mdmc_average="global") = support-weighted mean of the per-class F-beta."""
    pred, target = pred.reshape(-1), target.reshape(-1)
    cm = torch.zeros(C, C, dtype=torch.int64)
    cm.index_put_((target, pred), torch.ones_like(target), accumulate=True)
    tp = cm.diag().double()
    fn, fp = cm.sum(1).double() - tp, cm.sum(0).double() - tp
    acc = tp.sum() / cm.sum()
    union = tp + fp + fn
    jac = torch.where(union > 0, tp / union.clamp_min(1), torch.zeros_like(tp)).mean()
    den = (1 + beta ** 2) * tp + beta ** 2 * fn + fp
    f = torch.where(den > 0, (1 + beta ** 2) * tp / den.clamp_min(1), torch.zeros_like(tp))
    support = cm.sum(1).double()
    return cm, float(acc), float(jac), float((f * support).sum() / support.sum())
