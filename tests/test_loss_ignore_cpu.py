"""-m "not gpu": the host side of the weighted / ignoring segmentation loss - constructor and argument validation, the
non-persistent weight buffer, init_model reading the two attributes, prepare_sample(void_label=), and the header /
ctypes prototypes of the new entry points (the pattern of tests/test_abi.py)."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

NEW_ENTRY_POINTS = {
    "vmtl_ce_ex_workspace_bytes": ["P"],
    "vmtl_ce_fwd_ex": ["logits", "target", "weight", "ignore_index", "loss", "stats", "workspace", "argmax", "B", "HW",
                       "C", "sb", "sc", "sp", "stream"],
    "vmtl_ce_bwd_ex": ["logits", "target", "weight", "ignore_index", "stats", "grad_out", "dlogits", "B", "HW", "C", "sb",
                       "sc", "sp", "dsb", "dsc", "dsp", "stream"],
    "vmtl_silog_fwd_mask": ["pred", "target", "mask", "loss", "stats", "workspace", "P", "stream"],
    "vmtl_silog_bwd_mask": ["pred", "target", "mask", "stats", "grad_out", "dpred", "P", "stream"],
    "vmtl_confusion_matrix_ex": ["pred", "target", "cm", "P", "C", "ignore_index", "stream"],
    "vmtl_segm_metrics_ex": ["cm", "C", "beta", "ignore_index", "out", "stream"],
}


def test_new_entry_points_are_declared_and_exported():
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import HEADER, lib, parse_header

    protos = parse_header(HEADER)
    l = lib()
    for name, args in NEW_ENTRY_POINTS.items():
        assert name in protos, f"{name} is not declared in vmtl.h"
        restype, argtypes, argnames = protos[name]
        assert argnames == args
        assert hasattr(l._dll, name), f"{name} declared in vmtl.h but not exported"
        if "ignore_index" in args:  # a long long: the "nothing to ignore" value must fit
            assert argtypes[args.index("ignore_index")] is ctypes.c_longlong
    assert ops.NO_IGNORE == -(1 << 63) == ctypes.c_longlong(ops.NO_IGNORE).value
    assert "#define VMTL_NO_IGNORE (-0x7fffffffffffffffLL - 1)" in HEADER.read_text()
    # host-only: the (numerator, denominator) partials of at most 2048 blocks, 8-byte granules
    f = l.raw("vmtl_ce_ex_workspace_bytes")
    assert f(1) == 16 and f(130) == 16 and f(257) == 32 and f(1 << 30) == 2 * 2048 * 8
    # the launching entry points validate their pointers before anything else: no device is touched
    assert l.raw("vmtl_ce_fwd_ex")(None, None, None, 255, None, None, None, None, 1, 1, 1, 1, 1, 1, None) == -1
    assert l.raw("vmtl_ce_bwd_ex")(None, None, None, 255, None, None, None, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1
    assert l.raw("vmtl_silog_fwd_mask")(None, None, None, None, None, None, 1, None) == -1
    assert l.raw("vmtl_silog_bwd_mask")(None, None, None, None, None, None, 1, None) == -1
    assert l.raw("vmtl_confusion_matrix_ex")(None, None, None, 1, 1, 255, None) == -1
    assert l.raw("vmtl_segm_metrics_ex")(None, 1, 1.0, 255, None, None) == -1


def test_cross_entropy_loss_arguments():
    from vision_mtl_amd.losses import CrossEntropyLoss

    plain = CrossEntropyLoss()
    assert plain.weight is None and plain.ignore_index is None  # None, not torch's -100: nothing is ignored
    assert list(plain.state_dict()) == []
    w = [0.5, 1.0, 2.0]
    crit = CrossEntropyLoss(weight=w, ignore_index=255)
    assert crit.ignore_index == 255 and crit.weight.dtype == torch.float32 and crit.weight.tolist() == w
    assert list(crit.state_dict()) == []  # persistent=False: checkpoints keep the reference's keys
    assert "weight" in dict(crit.named_buffers())  # ... but .to(device) moves it
    assert crit.to(torch.float64).weight.dtype == torch.float64
    src = torch.tensor(w)
    crit = CrossEntropyLoss(weight=src)
    src[0] = 9.0
    assert crit.weight[0].item() == 0.5  # the criterion owns a copy
    with pytest.raises(ValueError):
        CrossEntropyLoss(weight=torch.ones(2, 3))
    with pytest.raises(ValueError):
        CrossEntropyLoss(weight=[])
    for bad in (2.0, "255", True):
        with pytest.raises(TypeError):
            CrossEntropyLoss(ignore_index=bad)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from vision_mtl_amd import ops

    z, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cross_entropy(z, t, ignore_index=255)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cross_entropy_with_argmax(z, t, weight=torch.ones(3))
    with pytest.raises(TypeError):
        ops.cross_entropy(z, t, ignore_index=1.5)
    p = torch.full((1, 2, 2, 1), 0.5)
    with pytest.raises(ValueError, match="mask"):
        ops.silog(p, p, 1e-3, mask=torch.ones(1, 2, 2, dtype=torch.bool))
    with pytest.raises(TypeError, match="mask"):
        ops.silog(p, p, 1e-3, mask=torch.ones(1, 2, 2, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.silog(p, p, 1e-3, mask=torch.ones(1, 2, 2, 1, dtype=torch.bool))


def test_module_and_init_model_read_the_new_arguments():
    from vision_mtl_amd import metrics as M
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import init_model

    cfg = argparse.Namespace(num_classes=5)
    plain = init_model(argparse.Namespace(model_name="mtan"), cfg)
    assert plain.segm_criterion.weight is None and plain.segm_criterion.ignore_index is None
    assert plain.hparams["segm_ignore_index"] is None and plain.hparams["segm_class_weights"] is None
    assert all(m.ignore_index is None for k, m in plain.metrics.items() if k != "mae")
    w = (0.5, 1.0, 1.5, 2.0, 0.25)
    module = init_model(argparse.Namespace(model_name="mtan", segm_ignore_index=255, segm_class_weights=w), cfg)
    assert module.segm_criterion.ignore_index == 255 and module.segm_criterion.weight.tolist() == list(w)
    assert module.hparams["segm_ignore_index"] == 255 and module.hparams["segm_class_weights"] == list(w)
    assert module.segm_ignore_index == 255
    assert all(m.ignore_index == 255 for k, m in module.metrics.items() if k != "mae")
    assert list(module.state_dict()) == list(plain.state_dict())
    with pytest.raises(ValueError, match="segm_class_weights"):
        MTLModule(torch.nn.Linear(1, 1), num_classes=5, segm_class_weights=[1.0, 2.0])
    for cls in (M.Accuracy, M.JaccardIndex, M.FBetaScore):
        assert cls(5).ignore_index is None and cls(5, ignore_index=None).ignore_index is None
        assert cls(5, ignore_index=3).ignore_index == 3


def test_prepare_sample_void_label():
    from vision_mtl_amd.data import prepare_sample

    raw = {"img": np.zeros((4, 6, 3), np.float32), "mask": np.array([[-1, 0, 1, 2, -1, 3]] * 4),
           "depth": np.full((4, 6), 0.5, np.float32)}
    ref = prepare_sample(raw, num_classes=19)["mask"]
    assert ref[0].tolist() == [18, 0, 1, 2, 18, 3]  # the reference's rule (cityscapes.py:42) stays the default
    got = prepare_sample(raw, num_classes=19, void_label=255)["mask"]
    assert got.dtype == torch.int64 and got[0].tolist() == [255, 0, 1, 2, 255, 3]
    assert raw["mask"][0, 0] == -1  # the caller's array is left alone
    with pytest.raises(ValueError, match="void_label"):
        prepare_sample(raw, num_classes=14, dataset="nyuv2", void_label=255)


def test_silog_loss_keeps_refusing_mismatched_sizes():
    from vision_mtl_amd.losses import SILogLoss

    p, t = torch.full((1, 4, 4, 1), 0.5), torch.full((1, 4, 3, 1), 0.5)
    with pytest.raises(NotImplementedError):
        SILogLoss()(p, t, mask=torch.ones(1, 4, 3, 1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a mask no longer raises NotImplementedError
        SILogLoss()(p, p, mask=torch.ones(1, 4, 4, 1, dtype=torch.bool))
