"""-m "not gpu": the host side of online hard example mining in the segmentation cross entropy - the three C-ABI entry
points (declared, exported, pointer-checked before a device is touched), constructor and op argument validation, the
module / init_model arguments (the default module keeps its hparams and state-dict keys), and the test oracle itself
against an independent torch.topk formulation."""
import argparse
import math

import pytest
import torch

from tests import ohem_oracle as O

ENTRY_POINTS = {
    "vmtl_ce_ohem_workspace_bytes": ["P"],
    "vmtl_ce_ohem_fwd": ["logits", "target", "weight", "ignore_index", "nll_thresh", "min_kept_total", "loss", "stats",
                         "counts", "nll", "workspace", "argmax", "B", "HW", "C", "sb", "sc", "sp", "stream"],
    "vmtl_ce_ohem_bwd": ["logits", "target", "weight", "ignore_index", "stats", "nll", "grad_out", "dlogits", "B", "HW",
                         "C", "sb", "sc", "sp", "dsb", "dsc", "dsp", "stream"],
}
DEFAULT_HPARAMS = {"num_classes", "optim_dict", "lr", "device", "loss_segm_weight", "loss_depth_weight",
                   "segm_ignore_index", "segm_class_weights"}


def test_entry_points_are_declared_exported_and_check_their_pointers():
    from vision_mtl_amd._lib import HEADER, lib, parse_header

    protos = parse_header(HEADER)
    l = lib()
    for name, args in ENTRY_POINTS.items():
        assert name in protos, f"{name} is not declared in vmtl.h"
        assert protos[name][2] == args
        assert hasattr(l._dll, name), f"{name} declared in vmtl.h but not exported"
    # host-only: the cleared head (8 counters' worth of bytes, 2048 + 2048 + 1024 32-bit bins) and three doubles per
    # block of the sum pass, at most 2048 blocks of 256 pixels
    f = l.raw("vmtl_ce_ohem_workspace_bytes")
    head = 64 + 4 * (2048 + 2048 + 1024)
    assert f(1) == head + 24 and f(130) == head + 24 and f(257) == head + 48
    assert f(2048 * 256) == f(1 << 30) == head + 3 * 2048 * 8
    assert all(f(p) % 8 == 0 for p in (1, 130, 257, 526683, 1 << 30))
    # pointers (and the two host constants) are validated before anything else: no device is touched
    fwd, bwd = l.raw("vmtl_ce_ohem_fwd"), l.raw("vmtl_ce_ohem_bwd")
    assert fwd(None, None, None, 255, 0.5, 1, None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, None) == -1
    assert bwd(None, None, None, 255, None, None, None, None, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1


def test_cross_entropy_loss_arguments():
    from vision_mtl_amd.losses import CrossEntropyLoss

    plain = CrossEntropyLoss()
    assert plain.ohem_min_kept is None and plain.ohem_thresh is None
    crit = CrossEntropyLoss(weight=[0.5, 1.0, 2.0], ignore_index=255, ohem_min_kept=100, ohem_thresh=0.7)
    assert crit.ohem_min_kept == 100 and crit.ohem_thresh == 0.7 and crit.ignore_index == 255
    assert list(crit.state_dict()) == []
    assert CrossEntropyLoss(ohem_min_kept=1).ohem_thresh is None  # pure top-K
    assert CrossEntropyLoss(ohem_min_kept=1, ohem_thresh=1.0).ohem_thresh == 1.0
    with pytest.raises(ValueError, match="ohem_min_kept"):
        CrossEntropyLoss(ohem_thresh=0.7)  # a threshold alone does not turn mining on
    for bad in (0, -3):
        with pytest.raises(ValueError):
            CrossEntropyLoss(ohem_min_kept=bad)
    for bad in (2.0, "100", True):
        with pytest.raises(TypeError):
            CrossEntropyLoss(ohem_min_kept=bad)
    for bad in (0.0, -0.1, 1.5, math.nan, math.inf):
        with pytest.raises(ValueError):
            CrossEntropyLoss(ohem_min_kept=10, ohem_thresh=bad)
    with pytest.raises(TypeError):
        CrossEntropyLoss(ohem_min_kept=10, ohem_thresh="0.7")


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from vision_mtl_amd import ops

    z, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64)
    for f in (ops.cross_entropy_ohem, ops.cross_entropy_ohem_with_argmax):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(z, t, 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(z, t, 2, thresh=0.7, weight=torch.ones(3), ignore_index=255)
        with pytest.raises(ValueError, match="min_kept"):
            f(z, t, 0)
        with pytest.raises(TypeError, match="min_kept"):
            f(z, t, 2.0)
        with pytest.raises(ValueError, match="thresh"):
            f(z, t, 2, thresh=0.0)
        with pytest.raises(ValueError, match="thresh"):
            f(z, t, 2, thresh=math.nan)
        with pytest.raises(TypeError):
            f(z, t, 2, ignore_index=1.5)
    assert ops.ohem_tau(None) == math.inf and ops.ohem_tau(0.7) == -math.log(0.7)
    assert math.copysign(1.0, ops.ohem_tau(1.0)) == 1.0 and ops.ohem_tau(1.0) == 0.0  # +0.0, not -0.0
    from vision_mtl_amd.losses import CrossEntropyLoss

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CrossEntropyLoss(ohem_min_kept=2)(z, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CrossEntropyLoss(ohem_min_kept=2, ohem_thresh=0.5).forward_with_predictions(z, t)


def test_default_module_is_unchanged_and_init_model_reads_the_arguments():
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import init_model

    cfg = argparse.Namespace(num_classes=5)
    plain = init_model(argparse.Namespace(model_name="mtan"), cfg)
    assert set(plain.hparams) == DEFAULT_HPARAMS
    assert not hasattr(plain, "segm_train_criterion")
    assert plain.segm_criterion.ohem_min_kept is None
    assert [n for n, _ in plain.named_children()] == ["model", "segm_criterion", "depth_criterion"]
    w = (0.5, 1.0, 1.5, 2.0, 0.25)
    module = init_model(argparse.Namespace(model_name="mtan", segm_ignore_index=255, segm_class_weights=w,
                                           segm_ohem_min_kept=256, segm_ohem_thresh=0.7), cfg)
    assert set(module.hparams) == DEFAULT_HPARAMS | {"segm_ohem_min_kept", "segm_ohem_thresh"}
    assert module.hparams["segm_ohem_min_kept"] == 256 and module.hparams["segm_ohem_thresh"] == 0.7
    assert list(module.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in module.named_parameters()] == [n for n, _ in plain.named_parameters()]
    mined, unmined = module.segm_train_criterion, module.segm_criterion
    assert (mined.ohem_min_kept, mined.ohem_thresh, mined.ignore_index) == (256, 0.7, 255)
    assert mined.weight.tolist() == list(w)
    # the criterion of validation, test and predict: the same weights and ignore index, no mining
    assert (unmined.ohem_min_kept, unmined.ignore_index, unmined.weight.tolist()) == (None, 255, list(w))
    top_k = MTLModule(torch.nn.Linear(1, 1), num_classes=5, segm_ohem_min_kept=8)
    assert top_k.hparams["segm_ohem_thresh"] is None and top_k.segm_train_criterion.ohem_thresh is None
    with pytest.raises(ValueError, match="ohem_min_kept"):
        MTLModule(torch.nn.Linear(1, 1), num_classes=5, segm_ohem_thresh=0.7)
    with pytest.raises(ValueError):
        MTLModule(torch.nn.Linear(1, 1), num_classes=5, segm_ohem_min_kept=0)
    with pytest.raises(TypeError):
        MTLModule(torch.nn.Linear(1, 1), num_classes=5, segm_ohem_min_kept=2.5)


def _topk_formulation(nll, valid, K, tau):
    """Independent of ohem_oracle: the K hardest valid pixels by torch.topk, their smallest nll as kappa, and membership
    spelled as (nll >= cut) over valid pixels; no NaN in these inputs."""
    flat = torch.where(valid, nll, torch.full_like(nll, -1.0)).flatten()
    K = min(K, int(valid.sum()))
    kappa = torch.topk(flat, K).values.min() if K > 0 else torch.tensor(math.inf, dtype=nll.dtype)
    cut = min(float(kappa), tau)
    return cut, valid & (nll >= cut)


@pytest.mark.parametrize("name", O.SMALL)
def test_oracle_agrees_with_a_topk_formulation(name):
    c = O.case(name)
    nll32 = c["nll"].float()
    for total in O.kept_totals(c["V"]):
        for thresh in O.THRESHOLDS:
            tau = O.tau_of(thresh)
            for w in (None, c["w"]):
                r = O.reference(c["z"], c["t"], total, thresh, w, O.IGN)
                cut, kept = _topk_formulation(c["nll"], c["valid"], total, tau)
                assert float(r["cut"]) == cut and torch.equal(r["kept"], kept)
                assert int(kept.sum()) >= min(total, c["V"])
                wt = torch.ones_like(c["nll"]) if w is None else w.double()[c["t"].clamp(0, c["C"] - 1)]
                assert abs(float(r["loss"]) - float((wt * c["nll"])[kept].sum() / wt[kept].sum())) < 1e-12
                rows = r["grad"].permute(0, 2, 3, 1)
                assert bool((rows[~kept] == 0).all()) and bool((rows[kept].abs().amax(dim=1) > 0).all())
            tau32 = float(torch.tensor(tau, dtype=torch.float32))
            cut32, kept32 = O.select(nll32, c["valid"], total, tau32)
            ref_cut, ref_kept = _topk_formulation(nll32, c["valid"], total, tau32)
            assert float(cut32) == ref_cut and torch.equal(kept32, ref_kept)


def test_oracle_conventions_nan_ties_and_empty():
    nan = math.nan
    nll = torch.tensor([0.5, nan, 2.0, 2.0, 0.1, 7.0], dtype=torch.float32)
    valid = torch.tensor([True, True, True, True, True, False])
    cut, kept = O.select(nll, valid, 1, math.inf)  # K = 1: the NaN pixel is the hardest, kappa is NaN, cut = tau
    assert float(cut) == math.inf and kept.tolist() == [False, True, False, False, False, False]
    cut, kept = O.select(nll, valid, 2, math.inf)  # rank 2 is one of the tied 2.0s: both stay
    assert float(cut) == 2.0 and kept.tolist() == [False, True, True, True, False, False]
    cut, kept = O.select(nll, valid, 2, 0.3)       # tau below kappa: everything not below tau
    assert abs(float(cut) - 0.3) < 1e-7 and kept.tolist() == [True, True, True, True, False, False]
    cut, kept = O.select(nll, torch.zeros(6, dtype=torch.bool), 3, 0.3)  # V = 0: K = 0, cut = tau, nothing kept
    assert abs(float(cut) - 0.3) < 1e-7 and not kept.any()
    assert O.margin(nll.double(), valid, 2, math.inf) == 0.0  # a tie at the cut: no margin
