"""-m "not gpu": the host side of the Dice / Jaccard / Tversky region term of the segmentation loss - the oracle checked
against the textbook Dice and Jaccard forms and its closed-form gradient coefficients against autograd, the three C-ABI
entry points (declared, exported, arguments checked before a device is touched), every argument error of ops, losses and
MTLModule on CPU inputs, and the module / init_model arguments (the default module keeps its hparams and criterion)."""
import argparse
import math

import pytest
import torch
import torch.nn.functional as F

from tests import region_oracle as R

ENTRY_POINTS = {
    "vmtl_ce_region_workspace_bytes": ["P", "C"],
    "vmtl_ce_region_fwd": ["logits", "target", "weight", "ignore_index", "alpha", "beta", "smooth", "ce_weight",
                           "region_weight", "loss", "terms", "stats", "coef", "counts", "workspace", "argmax", "B", "HW",
                           "C", "sb", "sc", "sp", "stream"],
    "vmtl_ce_region_bwd": ["logits", "target", "weight", "ignore_index", "stats", "coef", "grad_out", "ce_weight",
                           "region_weight", "dlogits", "B", "HW", "C", "sb", "sc", "sp", "dsb", "dsc", "dsp", "stream"],
}
DEFAULT_HPARAMS = {"num_classes", "optim_dict", "lr", "device", "loss_segm_weight", "loss_depth_weight",
                   "segm_ignore_index", "segm_class_weights"}
REGION_HPARAMS = {"segm_region_weight", "segm_region_alpha", "segm_region_beta", "segm_region_smooth"}


# ------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", R.SMALL + R.VARIANTS)
def test_oracle_is_dice_and_jaccard(name):
    c = R.case(name)
    C = c["C"]
    p = F.softmax(c["z"].double(), dim=1)
    TP, S, N = R.sums(p, c["t"], c["valid"], C)
    present = N > 0
    assert int(N.sum()) == c["V"]
    dice = (1.0 - 2.0 * TP / (S + N))[present].sum() / C
    jacc = (1.0 - TP / (S + N - TP))[present].sum() / C
    assert abs(float(R.region_term(p, c["t"], c["valid"], 0.5, 0.5, 0.0)[0]) - float(dice)) < 1e-14
    assert abs(float(R.region_term(p, c["t"], c["valid"], 1.0, 1.0, 0.0)[0]) - float(jacc)) < 1e-14
    if name in R.VARIANTS:  # class 7 is gone from the valid labels, in c_void_only although the label map holds it
        assert int(N[7]) == 0 and int(present.sum()) == C - 1
        assert (name == "c_void_only") == bool((c["t"] == 7).any())
    # the bound the GPU tests lean on: no present class is ill-conditioned
    for al, be, sm in R.SETTINGS:
        D = R.region_term(p, c["t"], c["valid"], al, be, sm)[2]
        assert float(D[present].min()) >= 1.2, (name, al, be, sm, float(D[present].min()))


@pytest.mark.parametrize("setting", R.SETTINGS)
@pytest.mark.parametrize("name", R.SMALL + R.VARIANTS)
def test_closed_form_coefficients_match_autograd(name, setting):
    al, be, sm = setting
    c = R.case(name)
    C, t, valid = c["C"], c["t"], c["valid"]
    p = F.softmax(c["z"].double(), dim=1).requires_grad_(True)
    R.region_term(p, t, valid, al, be, sm)[0].backward()
    a, b = R.coefficients(p.detach(), t, valid, al, be, sm)
    onehot = F.one_hot(t.clamp(0, C - 1), C).permute(0, 3, 1, 2).double()
    want = (b.view(1, C, 1, 1) + a.view(1, C, 1, 1) * onehot) * valid.unsqueeze(1)
    assert float((p.grad - want).abs().max()) <= 1e-11
    absent = R.sums(p.detach(), t, valid, C)[2] == 0
    assert bool((a[absent] == 0).all()) and bool((b[absent] == 0).all())
    # and through the softmax: dz = p (g - sum_k p_k g_k), against autograd on the logits
    r = R.reference(c["z"], t, al, be, sm, None, c["ign"], ce_weight=0.0)
    pd = p.detach()
    dz = R.GOUT * pd * (want - (pd * want).sum(dim=1, keepdim=True))
    assert float((r["grad"] - dz).abs().max()) <= 1e-11


def test_oracle_conventions_all_void_and_term_alone():
    c = R.case("a")
    t = torch.full_like(c["t"], R.IGN)
    r = R.reference(c["z"], t, ce_weight=0.0)
    assert float(r["loss"]) == 0.0 and not r["grad"].any() and not r["coef"].any()
    r = R.reference(c["z"], t, ce_weight=1.0)
    assert math.isnan(float(r["loss"])) and float(r["region"]) == 0.0
    both = R.reference(c["z"], c["t"], 0.3, 0.7, 1.0, c["w"], R.IGN, ce_weight=0.5, region_weight=2.0)
    assert abs(float(both["loss"]) - (0.5 * float(both["ce"]) + 2.0 * float(both["region"]))) < 1e-14


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_exported_and_check_their_arguments():
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import HEADER, lib, parse_header

    protos = parse_header(HEADER)
    l = lib()
    for name, args in ENTRY_POINTS.items():
        assert name in protos, f"{name} is not declared in vmtl.h"
        assert protos[name][2] == args
        assert hasattr(l._dll, name), f"{name} declared in vmtl.h but not exported"
    assert "#define VMTL_CE_REGION_MAX_CLASSES 32" in HEADER.read_text() and ops.CE_REGION_MAX_CLASSES == 32
    # host-only: one row of 3C + 4 eight-byte columns per block of 512 pixels, at most 512 blocks
    f = l.raw("vmtl_ce_region_workspace_bytes")
    assert f(1, 19) == f(512, 19) == 8 * 61 and f(513, 19) == 2 * 8 * 61
    assert f(512 * 512, 3) == f(1 << 30, 3) == 512 * 8 * 13
    assert f(130, 1) == f(130, 33) == f(0, 19) == 0
    # arguments are validated before anything else: no device is touched.  A pointer that is never followed stands in.
    fwd, bwd = l.raw("vmtl_ce_region_fwd"), l.raw("vmtl_ce_region_bwd")
    one = 8

    def call_fwd(C=19, alpha=0.5, beta=0.5, smooth=0.0, cw=1.0, rw=1.0, ptr=one):
        return fwd(ptr, ptr, None, 255, alpha, beta, smooth, cw, rw, ptr, ptr, ptr, ptr, ptr, ptr, None, 1, 1, C, 1, 1, 1,
                   None)

    assert call_fwd(ptr=None) == -1
    for kw in (dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=math.nan), dict(alpha=math.inf), dict(beta=0.0),
               dict(beta=math.inf), dict(smooth=-0.5), dict(smooth=math.nan), dict(cw=-1.0), dict(cw=math.inf),
               dict(rw=0.0), dict(rw=-2.0), dict(rw=math.nan)):
        assert call_fwd(**kw) == -1, kw
    for C in (1, 33, 64):
        assert call_fwd(C=C) == -3, C  # unsupported, without a launch
    assert bwd(None, None, None, 255, None, None, None, 1.0, 1.0, None, 1, 1, 19, 1, 1, 1, 1, 1, 1, None) == -1
    assert bwd(one, one, None, 255, one, one, one, 1.0, 0.0, one, 1, 1, 19, 1, 1, 1, 1, 1, 1, None) == -1
    assert bwd(one, one, None, 255, one, one, one, 1.0, 1.0, one, 1, 1, 33, 1, 1, 1, 1, 1, 1, None) == -3


# ------------------------------------------------------------------------------------------------------ arguments
def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from vision_mtl_amd import ops

    z, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64)
    for f in (ops.segm_region_loss, ops.segm_region_loss_with_argmax):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(z, t)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(z, t, 0.5, 0.3, 0.7, 1.0, weight=torch.ones(3), ignore_index=255, ce_weight=0.0)
        for name, bad in (("region_weight", 0.0), ("region_weight", -1.0), ("region_weight", math.inf),
                          ("alpha", 0.0), ("alpha", math.nan), ("beta", -0.5), ("beta", math.inf),
                          ("smooth", -1e-3), ("smooth", math.nan), ("ce_weight", -1.0), ("ce_weight", math.inf)):
            with pytest.raises(ValueError, match=name):
                f(z, t, **{name: bad})
        for name in ("region_weight", "alpha", "beta", "smooth", "ce_weight"):
            for bad in ("1", True, None, torch.ones(())):
                with pytest.raises(TypeError, match=name):
                    f(z, t, **{name: bad})
        with pytest.raises(TypeError, match="ignore_index"):
            f(z, t, ignore_index=1.5)
        for C in (1, 33):
            with pytest.raises(ValueError, match="2 to 32 classes"):
                f(torch.zeros(1, C, 2, 2), t)
        with pytest.raises(ValueError, match="B,C,H,W"):
            f(torch.zeros(3, 2, 2), t)
    assert ops.region_loss_number(0, "smooth") == 0.0 and ops.region_loss_number(2, "alpha", positive=True) == 2.0


def test_loss_modules_arguments():
    from vision_mtl_amd.losses import CrossEntropyLoss, DiceLoss, JaccardLoss, TverskyLoss

    z, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64)
    plain = CrossEntropyLoss()
    assert plain.region_weight is None
    crit = CrossEntropyLoss(weight=[0.5, 1.0, 2.0], ignore_index=255, region_weight=0.5, region_alpha=0.3,
                            region_beta=0.7, region_smooth=1)
    assert crit.region_weight == 0.5 and crit.region == (0.3, 0.7, 1.0) and list(crit.state_dict()) == []
    assert CrossEntropyLoss(region_weight=2).region == (0.5, 0.5, 0.0)
    for kw in (dict(ohem_min_kept=10), dict(ohem_min_kept=10, ohem_thresh=0.7)):
        with pytest.raises(ValueError, match="does not combine"):
            CrossEntropyLoss(region_weight=0.5, **kw)
    for kw in (dict(region_weight=0.0), dict(region_weight=-1.0), dict(region_weight=math.nan),
               dict(region_weight=1.0, region_alpha=0.0), dict(region_weight=1.0, region_beta=math.inf),
               dict(region_weight=1.0, region_smooth=-1.0)):
        with pytest.raises(ValueError):
            CrossEntropyLoss(**kw)
    for kw in (dict(region_weight="1"), dict(region_weight=True), dict(region_weight=1.0, region_alpha="a"),
               dict(region_weight=1.0, region_smooth=None)):
        with pytest.raises(TypeError):
            CrossEntropyLoss(**kw)
    for f in (crit, crit.forward_with_predictions):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(z, t)
    tv = TverskyLoss(0.3, 0.7, 1.0, ignore_index=255)
    assert (tv.alpha, tv.beta, tv.smooth, tv.ignore_index) == (0.3, 0.7, 1.0, 255)
    d, j = DiceLoss(), JaccardLoss(smooth=1.0, ignore_index=0)
    assert (d.alpha, d.beta, d.smooth, d.ignore_index) == (0.5, 0.5, 0.0, None)
    assert (j.alpha, j.beta, j.smooth, j.ignore_index) == (1.0, 1.0, 1.0, 0)
    for m in (tv, d, j):
        assert list(m.state_dict()) == [] and list(m.parameters()) == []
        for f in (m, m.forward_with_predictions):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                f(z, t)
    for bad in (dict(alpha=0.0), dict(beta=-1.0), dict(smooth=-1.0), dict(alpha=math.nan)):
        with pytest.raises(ValueError):
            TverskyLoss(**bad)
    with pytest.raises(ValueError):
        DiceLoss(smooth=math.inf)
    for bad in (dict(alpha="x"), dict(smooth=True), dict(ignore_index=1.5), dict(ignore_index=True)):
        with pytest.raises(TypeError):
            TverskyLoss(**bad)


def test_default_module_is_unchanged_and_init_model_reads_the_arguments():
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.losses import CrossEntropyLoss
    from vision_mtl_amd.utils.pipeline_utils import init_model

    cfg = argparse.Namespace(num_classes=5)
    plain = init_model(argparse.Namespace(model_name="mtan"), cfg)
    assert set(plain.hparams) == DEFAULT_HPARAMS
    assert type(plain.segm_criterion) is CrossEntropyLoss and plain.segm_criterion.region_weight is None
    assert plain.segm_criterion.ohem_min_kept is None and plain.segm_criterion.ignore_index is None
    assert [n for n, _ in plain.named_children()] == ["model", "segm_criterion", "depth_criterion"]
    w = (0.5, 1.0, 1.5, 2.0, 0.25)
    module = init_model(argparse.Namespace(model_name="mtan", segm_ignore_index=255, segm_class_weights=w,
                                           segm_region_weight=0.5, segm_region_alpha=0.3, segm_region_beta=0.7,
                                           segm_region_smooth=1.0), cfg)
    assert set(module.hparams) == DEFAULT_HPARAMS | REGION_HPARAMS
    assert [module.hparams[k] for k in sorted(REGION_HPARAMS)] == [0.3, 0.7, 1.0, 0.5]
    assert list(module.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in module.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert [n for n, _ in module.named_children()] == ["model", "segm_criterion", "depth_criterion"]
    crit = module.segm_criterion
    assert (crit.region_weight, crit.region, crit.ignore_index) == (0.5, (0.3, 0.7, 1.0), 255)
    assert crit.weight.tolist() == list(w) and not hasattr(module, "segm_train_criterion")
    dice = init_model(argparse.Namespace(model_name="mtan", segm_region_weight=1), cfg)
    assert dice.segm_criterion.region == (0.5, 0.5, 0.0) and dice.hparams["segm_region_weight"] == 1.0
    lin = torch.nn.Linear(1, 1)
    for kw in (dict(segm_ohem_min_kept=8), dict(segm_ohem_min_kept=8, segm_ohem_thresh=0.7)):
        with pytest.raises(ValueError, match="does not combine"):
            MTLModule(lin, num_classes=5, segm_region_weight=0.5, **kw)
    for kw in (dict(segm_region_weight=0.0), dict(segm_region_weight=math.nan),
               dict(segm_region_weight=1.0, segm_region_alpha=0.0), dict(segm_region_weight=1.0, segm_region_beta=-1.0),
               dict(segm_region_weight=1.0, segm_region_smooth=math.inf)):
        with pytest.raises(ValueError):
            MTLModule(lin, num_classes=5, **kw)
    for kw in (dict(segm_region_weight="0.5"), dict(segm_region_weight=True),
               dict(segm_region_weight=1.0, segm_region_alpha=None)):
        with pytest.raises(TypeError):
            MTLModule(lin, num_classes=5, **kw)
    for C in (1, 33):
        with pytest.raises(ValueError, match="2 to 32 classes"):
            MTLModule(lin, num_classes=C, segm_region_weight=0.5)
    # the other arguments are not looked at while the option is unset
    assert set(MTLModule(lin, num_classes=40, segm_region_alpha=0.3).hparams) == DEFAULT_HPARAMS
