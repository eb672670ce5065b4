"""-m "not gpu": the host side of the depth loss with multi-scale gradient matching - the test oracle itself (against a
plain-loop restatement and against central finite differences), the margin of the margin-built cases, the three C-ABI
entry points (declared, exported, arguments checked before a device is touched), argument validation of ops.depth_loss,
the two criteria and the module / init_model arguments (the default module keeps its hparams, children and state-dict
keys)."""
import argparse
import math

import pytest
import torch

from tests import depth_grad_oracle as O

ENTRY_POINTS = {
    "vmtl_depth_grad_workspace_bytes": ["B", "H", "W", "scales"],
    "vmtl_depth_grad_fwd": ["pred", "target", "mask", "min_depth", "B", "H", "W", "scales", "silog_weight", "grad_weight",
                            "loss", "terms", "stats", "counts", "resid", "workspace", "stream"],
    "vmtl_depth_grad_bwd": ["pred", "target", "mask", "min_depth", "resid", "stats", "counts", "grad_out", "B", "H", "W",
                            "scales", "silog_weight", "grad_weight", "dpred", "stream"],
}
DEFAULT_HPARAMS = {"num_classes", "optim_dict", "lr", "device", "loss_segm_weight", "loss_depth_weight",
                   "segm_ignore_index", "segm_class_weights"}


def _loops(pred, target, valid, scales):
    """L_grad and the N_k by plain loops over pixels, in Python floats: independent of the oracle's slicing"""
    B, H, W = pred.shape
    R = [[[math.log(float(pred[b, y, x])) - math.log(float(target[b, y, x])) if valid[b, y, x] else None
           for x in range(W)] for y in range(H)] for b in range(B)]
    total, counts = 0.0, []
    for k in range(scales):
        s, n, acc = 1 << k, 0, 0.0
        for b in range(B):
            for y in range(0, H, s):
                for x in range(0, W, s):
                    if R[b][y][x] is None:
                        continue
                    n += 1
                    if x + s < W and R[b][y][x + s] is not None:
                        acc += abs(R[b][y][x + s] - R[b][y][x])
                    if y + s < H and R[b][y + s][x] is not None:
                        acc += abs(R[b][y + s][x] - R[b][y][x])
        counts.append(n)
        if n:
            total += acc / n
    return total, counts


@pytest.mark.parametrize("name", ["odd-holes", "odd-checker", "odd-deadimage", "odd-holes-margin"])
def test_oracle_agrees_with_plain_loops(name):
    c = O.case(name)
    assert c["shape"] == (2, 5, 13)
    for scales in (1, 3, 4, 6):
        r = O.reference(c["pred"], c["target"], c["valid"], scales, silog_weight=0.0, grad_weight=1.0)
        total, counts = _loops(c["pred"], c["target"], c["valid"], scales)
        assert r["counts"] == counts
        assert abs(float(r["loss"]) - total) <= 1e-12 * max(1.0, total)
        assert float(r["silog"]) == 0.0 and float(r["lgrad"]) == float(r["loss"])
        assert bool((r["grad"][~c["valid"]] == 0).all())
    if "checker" in name:  # no valid pair at step 1; every pair of the step-2 grid (all on one colour) is valid
        r1 = O.reference(c["pred"], c["target"], c["valid"], 1, silog_weight=0.0, grad_weight=1.0)
        assert float(r1["loss"]) == 0.0 and float(r1["grad"].abs().max()) == 0.0
        assert O.reference(c["pred"], c["target"], c["valid"], 2)["counts"][1] == 2 * 3 * 7


def test_oracle_composes_silog_and_the_term_and_takes_device_signs():
    c = O.case("odd-holes")
    pred, target, valid = c["pred"], c["target"], c["valid"]
    both = O.reference(pred, target, valid, 4, silog_weight=1.0, grad_weight=0.5)
    term = O.reference(pred, target, valid, 4, silog_weight=0.0, grad_weight=1.0)
    g = O.resid64(pred, target, valid)[valid]
    silog = 10 * torch.sqrt(torch.var(g) + 0.15 * torch.mean(g) ** 2)
    assert abs(float(both["silog"]) - float(silog)) < 1e-12
    assert abs(float(both["loss"]) - (float(silog) + 0.5 * float(term["loss"]))) < 1e-12
    # its own residual rounded to fp32 as `signs_from`: the margin of random data is far above fp32 rounding, so no flip
    same = O.reference(pred, target, valid, 4, signs_from=both["resid"].float())
    assert same["flips"]["absdr"].numel() == 0 and float(same["loss"]) == float(both["loss"])
    assert torch.equal(same["grad"], both["grad"])
    # an all-equal device residual decides every pair as a tie: the term and its gradient vanish, every pair is reported
    tie = O.reference(pred, target, valid, 4, silog_weight=0.0, grad_weight=1.0, signs_from=torch.zeros_like(pred))
    assert float(tie["loss"]) == 0.0 and float(tie["grad"].abs().max()) == 0.0
    assert tie["flips"]["absdr"].numel() > 0 and float(tie["flips"]["absdr"].min()) > 0
    # negated: every pair flips, the term changes sign
    neg = O.reference(pred, target, valid, 4, silog_weight=0.0, grad_weight=1.0, signs_from=-both["resid"].float())
    assert abs(float(neg["loss"]) + float(term["loss"])) < 1e-12
    assert neg["flips"]["absdr"].numel() == tie["flips"]["absdr"].numel()


@pytest.mark.parametrize("sw,gw", [(1.0, 0.5), (0.0, 1.0)])
def test_oracle_gradient_matches_central_differences(sw, gw):
    c = O.case("odd-holes")
    pred, target, valid = c["pred"].double(), c["target"], c["valid"]
    r = O.reference(pred, target, valid, 4, silog_weight=sw, grad_weight=gw, gout=1.0)
    h = 1e-7  # far below the smallest |dR| of this case, so no |.| changes branch
    assert O.margin(c["pred"], target, valid, 4) > 1e-4
    f = lambda p: float(O.reference(p, target, valid, 4, silog_weight=sw, grad_weight=gw, gout=1.0)["loss"])
    gen = torch.Generator().manual_seed(0)
    for flat in torch.randperm(pred.numel(), generator=gen)[:24].tolist():
        up, dn = pred.clone(), pred.clone()
        up.view(-1)[flat] += h
        dn.view(-1)[flat] -= h
        fd = (f(up) - f(dn)) / (2 * h)
        an = float(r["grad"].view(-1)[flat])
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (flat, fd, an)
        if not bool(valid.view(-1)[flat]):
            assert an == 0.0 and fd == 0.0


@pytest.mark.parametrize("name", O.MARGIN_CASES)
def test_margin_built_cases_keep_their_margin(name):
    c = O.case(name)
    m = O.margin(c["pred"], c["target"], c["valid"], O.MARGIN_SCALES)
    # a device sign can differ from the fp64 sign only where |dR| is within the two ends' residual bounds
    need = 2 * float(O.resid_bound(c["pred"], c["target"], c["valid"]).max())
    assert m > 0.99 * O.MARGIN and m > 10 * need, (m, need)  # 2^-10 less the rounding of pred to fp32
    vp = c["pred"][c["valid"]]
    assert vp.numel() == 0 or (float(vp.min()) > 0.04 and float(vp.max()) < 0.74)
    if c["valid"].numel() >= 65:
        counts = O.reference(c["pred"], c["target"], c["valid"], O.MARGIN_SCALES)["counts"]
        assert all(n > 0 for n in counts), counts


def test_entry_points_are_declared_exported_and_check_their_arguments():
    from vision_mtl_amd._lib import HEADER, lib, parse_header

    protos = parse_header(HEADER)
    l = lib()
    for name, args in ENTRY_POINTS.items():
        assert name in protos, f"{name} is not declared in vmtl.h"
        assert protos[name][2] == args
        assert hasattr(l._dll, name), f"{name} declared in vmtl.h but not exported"
    # three SILog doubles and an (S_k, N_k) pair per scale, per block of 1024 pixels, at most 1024 blocks
    f = l.raw("vmtl_depth_grad_workspace_bytes")
    assert f(1, 1, 1, 1) == 8 * 5 and f(1, 1, 1, 6) == 8 * 15 and f(1, 32, 32, 4) == 8 * 11
    assert f(1, 32, 33, 4) == 2 * 8 * 11 and f(4, 512, 512, 4) == f(64, 1024, 1024, 4) == 1024 * 8 * 11
    assert f(1, 1, 1, 0) == 0 and f(1, 1, 1, 7) == 0 and f(0, 1, 1, 1) == 0
    # pointers, geometry, scales and the weights are validated before the first launch (only the thread's last HIP error
    # is cleared before that: VMTL_ENTER)
    fwd, bwd = l.raw("vmtl_depth_grad_fwd"), l.raw("vmtl_depth_grad_bwd")
    assert fwd(None, None, None, 1e-3, 1, 1, 1, 4, 1.0, 0.5, None, None, None, None, None, None, None) == -1
    assert bwd(None, None, None, 1e-3, None, None, None, None, 1, 1, 1, 4, 1.0, 0.5, None, None) == -1
    p = 8  # any non-null address: nothing is launched, so nothing dereferences it
    for scales in (0, 7, -1):
        assert fwd(p, p, None, 1e-3, 1, 1, 1, scales, 1.0, 0.5, p, p, p, p, p, p, None) == -1
        assert bwd(p, p, None, 1e-3, p, p, p, p, 1, 1, 1, scales, 1.0, 0.5, p, None) == -1
    for bad in (-1.0, math.nan, math.inf):
        assert fwd(p, p, None, 1e-3, 1, 1, 1, 4, bad, 0.5, p, p, p, p, p, p, None) == -1
        assert fwd(p, p, None, 1e-3, 1, 1, 1, 4, 1.0, bad, p, p, p, p, p, p, None) == -1
        assert bwd(p, p, None, 1e-3, p, p, p, p, 1, 1, 1, 4, 1.0, bad, p, None) == -1
    assert fwd(p, p, None, 1e-3, 1, 0, 1, 4, 1.0, 0.5, p, p, p, p, p, p, None) == -1


def test_op_refuses_cpu_tensors_and_bad_arguments():
    from vision_mtl_amd import ops
    from vision_mtl_amd.losses import GradientMatchingLoss, SILogGradLoss

    pred, target = torch.full((1, 4, 4, 1), 0.5), torch.full((1, 4, 4, 1), 0.25)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_loss(pred, target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_loss(pred, target, mask=torch.ones(1, 4, 4, 1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GradientMatchingLoss()(pred, target)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SILogGradLoss()(pred, target)
    for bad in (0, 7, -1):
        with pytest.raises(ValueError, match="scales"):
            ops.depth_loss(pred, target, scales=bad)
    for bad in (2.0, "4", True):
        with pytest.raises(TypeError, match="scales"):
            ops.depth_loss(pred, target, scales=bad)
    for name in ("grad_weight", "silog_weight"):
        for bad in (-0.5, math.nan, math.inf):
            with pytest.raises(ValueError, match=name):
                ops.depth_loss(pred, target, **{name: bad})
        with pytest.raises(TypeError, match=name):
            ops.depth_loss(pred, target, **{name: "1"})
    with pytest.raises(ValueError, match="pred must be"):
        ops.depth_loss(torch.zeros(4, 4), torch.zeros(4, 4))
    with pytest.raises(ValueError, match="pred must be"):
        ops.depth_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))
    with pytest.raises(ValueError, match="same number of elements"):
        ops.depth_loss(pred, torch.zeros(1, 4, 5, 1))
    with pytest.raises(TypeError, match="mask"):
        ops.depth_loss(pred, target, mask=torch.ones(1, 4, 4, 1))
    with pytest.raises(ValueError, match="mask shape"):
        ops.depth_loss(pred, target, mask=torch.ones(1, 4, 4, dtype=torch.bool))


def test_criteria_arguments_and_shape_errors():
    from vision_mtl_amd.losses import GradientMatchingLoss, SILogGradLoss, SILogLoss

    term, both = GradientMatchingLoss(), SILogGradLoss()
    assert (term.scales, term.min_depth) == (4, 1e-3)
    assert (both.grad_weight, both.scales, both.min_depth) == (0.5, 4, 1e-3)
    for crit in (term, both, SILogGradLoss(grad_weight=2, scales=6), GradientMatchingLoss(scales=1)):
        assert list(crit.state_dict()) == [] and list(crit.parameters()) == [] and list(crit.buffers()) == []
    for cls in (GradientMatchingLoss, SILogGradLoss):
        for bad in (0, 7):
            with pytest.raises(ValueError, match="scales"):
                cls(scales=bad)
        with pytest.raises(TypeError, match="scales"):
            cls(scales=2.0)
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="grad_weight"):
            SILogGradLoss(grad_weight=bad)
    with pytest.raises(TypeError, match="grad_weight"):
        SILogGradLoss(grad_weight="0.5")
    # SILogLoss.forward's shape errors
    for crit in (both, SILogLoss()):
        with pytest.raises(IndexError):
            crit(torch.zeros(4), torch.zeros(4))
        with pytest.raises(NotImplementedError):
            crit(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 8, 8))
        with pytest.raises(ValueError, match="shape mismatch"):
            crit(torch.zeros(2, 1, 4, 4), torch.zeros(1, 1, 4, 4))
        with pytest.raises(ValueError, match="shape mismatch"):
            crit(torch.zeros(1, 4, 4, 1), torch.zeros(1, 1, 4, 1), interpolate=False)


def test_default_module_is_unchanged_and_init_model_reads_the_arguments():
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.losses import SILogGradLoss, SILogLoss
    from vision_mtl_amd.utils.pipeline_utils import init_model

    cfg = argparse.Namespace(num_classes=5)
    plain = init_model(argparse.Namespace(model_name="mtan"), cfg)
    assert set(plain.hparams) == DEFAULT_HPARAMS
    assert type(plain.depth_criterion) is SILogLoss
    assert [n for n, _ in plain.named_children()] == ["model", "segm_criterion", "depth_criterion"]
    module = init_model(argparse.Namespace(model_name="mtan", depth_grad_weight=0.5, depth_grad_scales=3), cfg)
    assert set(module.hparams) == DEFAULT_HPARAMS | {"depth_grad_weight", "depth_grad_scales"}
    assert module.hparams["depth_grad_weight"] == 0.5 and module.hparams["depth_grad_scales"] == 3
    assert type(module.depth_criterion) is SILogGradLoss
    assert (module.depth_criterion.grad_weight, module.depth_criterion.scales) == (0.5, 3)
    assert [n for n, _ in module.named_children()] == ["model", "segm_criterion", "depth_criterion"]
    assert list(module.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in module.named_parameters()] == [n for n, _ in plain.named_parameters()]
    plain.load_state_dict(module.state_dict())  # strict: no missing / unexpected key
    dflt = MTLModule(torch.nn.Linear(1, 1), num_classes=5, depth_grad_weight=1)
    assert dflt.hparams["depth_grad_scales"] == 4 and dflt.depth_criterion.scales == 4
    only_scales = MTLModule(torch.nn.Linear(1, 1), num_classes=5, depth_grad_scales=2)  # the weight turns the term on
    assert set(only_scales.hparams) == DEFAULT_HPARAMS and type(only_scales.depth_criterion) is SILogLoss
    for bad in (0.0, -0.5, math.nan, math.inf, "0.5", True):
        with pytest.raises(ValueError, match="depth_grad_weight"):
            MTLModule(torch.nn.Linear(1, 1), num_classes=5, depth_grad_weight=bad)
    for bad in (0, 7, 2.0, True):
        with pytest.raises(ValueError, match="depth_grad_scales"):
            MTLModule(torch.nn.Linear(1, 1), num_classes=5, depth_grad_weight=0.5, depth_grad_scales=bad)
