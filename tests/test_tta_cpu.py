"""-m "not gpu": the host side of test-time augmentation and output-size predictions - the view table of
inference.PredictAugment against the oracle's, argument validation, the three ops' refusal of CPU tensors, the three
C-ABI entry points (declared, exported, arguments checked before a device is touched), the default module (attribute
None, hparams, children and state-dict keys as they were), init_model's arguments, the tie-band condition of the cases
the GPU tests use, and the strength of the comparator those tests use (it must fail on planted defects)."""
import argparse
import math

import pytest
import torch

from tests import tta_oracle as O

DEFAULT_HPARAMS = {"num_classes", "optim_dict", "lr", "device", "loss_segm_weight", "loss_depth_weight",
                   "segm_ignore_index", "segm_class_weights"}


def _aug(**kw):
    from vision_mtl_amd.inference import PredictAugment

    return PredictAugment(**kw)


@pytest.mark.parametrize("hw, scales, flip, multiple", [
    ((128, 256), (0.75, 1.0, 1.25), True, 32),
    ((256, 256), (0.5, 1.0, 1.5, 2.0), False, 32),
    ((32, 64), (0.4,), False, 32),          # the clamp to size_multiple
    ((128, 256), (1.0, 1.01), True, 32),    # de-duplication
    ((36, 52), (0.5, 1.0, 1.5), True, 4),   # another stride
])
def test_view_table_is_the_oracles(hw, scales, flip, multiple):
    got = _aug(scales=scales, flip=flip, size_multiple=multiple).views(*hw)
    assert got == O.view_table(*hw, scales, flip, multiple)
    assert len({v[:3] for v in got}) == len(got)


def test_view_table_examples():
    six = _aug(scales=(0.75, 1.0, 1.25), flip=True).views(128, 256)
    assert [v[:3] for v in six] == [(96, 192, False), (96, 192, True), (128, 256, False), (128, 256, True),
                                    (160, 320, False), (160, 320, True)]
    assert _aug(scales=(0.4,)).views(32, 64) == [(32, 32, False, 0.4)]
    assert _aug(scales=(1.0, 1.01), flip=True).views(128, 256) == [(128, 256, False, 1.0), (128, 256, True, 1.0)]
    assert _aug().views(128, 256) == [(128, 256, False, 1.0)]
    assert _aug().out_size(128, 256) == (128, 256) and _aug(output_size=(1024, 2048)).out_size(128, 256) == (1024, 2048)


def test_validation():
    for bad in ((), (1.0, math.nan), (math.inf,), (0.0,), (-1.0, 1.0), 1.0):
        with pytest.raises(ValueError, match="scales"):
            _aug(scales=bad)
    for bad in ("mean", "PROB", None, 0):
        with pytest.raises(ValueError, match="merge"):
            _aug(merge=bad)
    for bad in ((0, 4), (4,), (4, 4, 4), (4.0, 4), (-1, 4), 4, "44", (True, 4)):
        with pytest.raises(ValueError, match="output_size"):
            _aug(output_size=bad)
    for bad in (0, -32, 32.0, True):
        with pytest.raises(ValueError, match="size_multiple"):
            _aug(size_multiple=bad)


def test_more_than_32_classes_is_refused():
    from vision_mtl_amd import ops

    assert ops.TTA_MAX_CLASSES == 32

    class Wide(torch.nn.Module):
        def forward(self, x):
            B, _, H, W = x.shape
            return {"segm": torch.zeros(B, 33, H, W), "depth": torch.zeros(B, 1, H, W)}

    with pytest.raises(ValueError, match="32 classes"):
        _aug(size_multiple=1)(Wide(), torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match="merge"):  # the ops check the mode themselves
        ops.tta_finish(torch.zeros(1, 2, 4, 4), None, 1.0, merge="mean")


def test_no_cpu_fallback():
    from vision_mtl_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tta_view(torch.zeros(1, 3, 8, 8), (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tta_view(torch.zeros(1, 8, 8, 3), (4, 4), flip=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tta_accumulate(torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tta_finish(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _aug(scales=(0.5,), size_multiple=4)(torch.nn.Identity(), torch.zeros(1, 3, 8, 8))  # its first launch: the view


def test_entry_points_check_their_arguments_before_any_launch():
    from vision_mtl_amd._lib import lib

    l = lib()
    for name in ("vmtl_tta_view", "vmtl_tta_accumulate", "vmtl_tta_finish"):
        assert name in l.protos
    p = 4096  # a dummy, aligned address: every call below must return before it is used
    view, acc, fin = l.raw("vmtl_tta_view"), l.raw("vmtl_tta_accumulate"), l.raw("vmtl_tta_finish")
    assert view(None, 4, p, 1, 4, 4, 4, 4, 0, None) == -1
    assert view(p, 5, p, 1, 4, 4, 4, 4, 0, None) == -1          # ld
    assert view(p, 4, p + 4, 1, 4, 4, 4, 4, 0, None) == -1      # out not 16-byte aligned
    assert view(p + 4, 4, p, 1, 4, 4, 4, 4, 0, None) == -1      # ld 4 input not 16-byte aligned
    assert view(p, 3, p, 1, 4, 4, 0, 4, 0, None) == -1
    assert acc(p, None, p, None, 1, 33, 4, 4, 4, 4, 0, 1.0, 1.0, 0, 1, None) == -3
    assert acc(p, None, p, None, 1, 0, 4, 4, 4, 4, 0, 1.0, 1.0, 1, 1, None) == -3
    assert acc(p, p, p, None, 1, 5, 4, 4, 4, 4, 0, 1.0, 1.0, 0, 1, None) == -1   # the depth pair is null together
    assert acc(p, None, p, p, 1, 5, 4, 4, 4, 4, 0, 1.0, 1.0, 0, 1, None) == -1
    assert acc(p, None, p, None, 1, 5, 4, 4, 4, 4, 0, 1.0, 1.0, 2, 1, None) == -1  # mode
    assert fin(p, None, 1.0, p, None, None, 1, 33, 4, 4, 4, 4, 0, None) == -3
    assert fin(p, None, 1.0, p, None, None, 1, 0, 4, 4, 4, 4, 1, None) == -3
    assert fin(p, p, 1.0, p, None, None, 1, 5, 4, 4, 4, 4, 0, None) == -1
    assert fin(p, None, 0.0, p, None, None, 1, 5, 4, 4, 4, 4, 0, None) == -1
    assert fin(p, None, 1.0, p, None, None, 1, 5, 4, 4, 4, 4, 7, None) == -1
    assert fin(p, None, 1.0, None, None, None, 1, 5, 4, 4, 4, 4, 0, None) == -1


def test_default_module_is_unchanged_and_init_model_reads_the_arguments():
    from vision_mtl_amd.inference import PredictAugment
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import init_model

    cfg = argparse.Namespace(num_classes=5)
    plain = init_model(argparse.Namespace(model_name="mtan"), cfg)
    assert plain.predict_augment is None
    assert set(plain.hparams) == DEFAULT_HPARAMS
    assert [n for n, _ in plain.named_children()] == ["model", "segm_criterion", "depth_criterion"]
    assert MTLModule(torch.nn.Linear(1, 1), num_classes=5).predict_augment is None
    module = init_model(argparse.Namespace(model_name="mtan", predict_scales=(0.5, 1.0), predict_flip=True,
                                           predict_output_size=[64, 128], predict_merge="logit"), cfg)
    pa = module.predict_augment
    assert isinstance(pa, PredictAugment)
    assert (pa.scales, pa.flip, pa.output_size, pa.merge) == ((0.5, 1.0), True, (64, 128), "logit")
    assert (pa.size_multiple, pa.compensate_depth, pa.return_confidence) == (32, False, False)
    assert set(module.hparams) == DEFAULT_HPARAMS
    assert [n for n, _ in module.named_children()] == ["model", "segm_criterion", "depth_criterion"]
    assert list(module.state_dict()) == list(plain.state_dict())
    plain.load_state_dict(module.state_dict())  # strict: no missing / unexpected key
    only_flip = init_model(argparse.Namespace(model_name="mtan", predict_flip=True), cfg).predict_augment
    assert (only_flip.scales, only_flip.flip, only_flip.output_size, only_flip.merge) == ((1.0,), True, None, "prob")
    with pytest.raises(ValueError, match="merge"):
        init_model(argparse.Namespace(model_name="mtan", predict_merge="mean"), cfg)


def test_targets_of_the_wrong_size_are_refused_before_any_launch():
    from vision_mtl_amd.lit_module import MTLModule

    module = MTLModule(torch.nn.Linear(1, 1), num_classes=5)
    module.predict_augment = _aug(output_size=(8, 8), size_multiple=4)
    batch = {"img": torch.zeros(2, 3, 4, 4), "mask": torch.zeros(2, 4, 4, dtype=torch.int64), "depth": torch.zeros(2, 4, 4, 1)}
    with pytest.raises(ValueError, match="predict_augment"):
        module.predict_step(batch)


# ---- the oracle itself, and the conditions the GPU tests rest on
def test_oracle_flip_and_identity_conventions():
    c = O.case("c19")
    z, d, _, _ = c["views"][0]
    H, W = c["base"]
    a, ad = O.merge_view(z, d, (H, W), False, "logit")
    assert torch.equal(a, z.double()) and torch.equal(ad, torch.sigmoid(d.double())[:, 0])
    af, adf = O.merge_view(torch.flip(z, [3]), torch.flip(d, [3]), (H, W), True, "logit")
    assert torch.equal(af, a) and torch.equal(adf, ad)
    p, _ = O.merge_view(z, None, (H, W), False, "prob", weight=2.0)
    assert float((p.sum(1) - 2.0).abs().max()) < 1e-12
    img = torch.rand(2, 3, 7, 13, generator=torch.Generator().manual_seed(3))
    assert torch.equal(O.view_image(img, (7, 13), True), torch.flip(img.double(), [3]))
    # a hand-checked pixel: 2 -> 4 upsampling, src = (x + 0.5) / 2 - 0.5 clamped at 0 -> 0, .25, .75, 1 (clamped)
    row = torch.tensor([[[[0.0, 4.0]]]])
    assert O.interp(row, (1, 4)).flatten().tolist() == [0.0, 1.0, 3.0, 4.0]


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_tie_band_condition(name, mode):
    """a condition on the inputs, checked here so that the GPU test cannot hide a failure in its exemptions: the fp32
    restatement agrees with the fp64 arg-max everywhere outside the tie band, and the band is at most 1 % of the pixels"""
    r64, r32 = O.reference(name, mode), O.reference(name, mode, torch.float32)
    band = O.tie_band(r32, r64)
    frac = float(band.double().mean())
    print(f"{name} {mode}: tie band {100 * frac:.4f} % of {band.numel()} pixels, map bar {O.bar(r32['map'], r64['map']):.3e}")
    assert frac <= O.BAND_MAX
    assert bool((r32["segm"] == r64["segm"])[~band].all())
    got = {k: r32[k] for k in ("segm", "depth", "confidence")}
    O.compare(got, r32, r64, what=f"{name} {mode} fp32 restatement")  # the fp32 side is within its own bar by definition


def _defect(name, mode, kind):
    """the fp32 restatement with one planted defect, finished as the device would"""
    c = O.case(name)
    views, inv = c["views"], 1.0 / len(c["views"])
    if kind == "flip not undone":
        acc, acc_d = O.merge(views, c["base"], mode, torch.float32, undo_flip=False)
    elif kind == "view dropped":
        acc, acc_d = O.merge(views[:-1], c["base"], mode, torch.float32)
    else:
        acc, acc_d = O.merge(views, c["base"], mode, torch.float32)
        if kind == "shifted by one pixel":
            acc, acc_d = torch.roll(acc, 1, 3), torch.roll(acc_d, 1, 2)
        elif kind == "channel scaled":
            acc = acc.clone()
            acc[:, min(1, c["C"] - 1)] *= 1.0 + 1e-3
        else:
            raise AssertionError(kind)
    r = O.finish(acc, acc_d, inv, c["out"], mode, torch.float32)
    return {k: r[k] for k in ("segm", "depth", "confidence")}


@pytest.mark.parametrize("kind", ["shifted by one pixel", "flip not undone", "view dropped", "channel scaled"])
@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_comparator_fails_on_a_planted_defect(name, mode, kind):
    r64, r32 = O.reference(name, mode), O.reference(name, mode, torch.float32)
    with pytest.raises(AssertionError):
        O.compare(_defect(name, mode, kind), r32, r64, what=kind)
