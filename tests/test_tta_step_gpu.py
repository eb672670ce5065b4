"""-m gpu: inference.PredictAugment through MTLModule.predict_step and GraphedEval(stage="predict"), on the tiny MTAN of
tests/golden/mtan_tiny.pt (2x32x48, C = 5, stride 16) and on `basic` at 2x32x64, C = 5 (stride 32), both in eval mode.

The merge is isolated from the model's own rounding: the per-view logits are the DEVICE's (module.model on ops.tta_view of
the batch, copied to the host) and the fp64 oracle merges those, so what is compared is views + merge + finish.  Bars and
the tie band as in tests/test_tta_kernels_gpu.py (tests/tta_oracle.py: 4 x the fp32 CPU restatement's own error, floored
at 2^-22 of the maximum; an arg-max is exempt where the fp64 top-2 margin is below 2 x the bar, at most 1 % of the pixels)."""
import argparse
import gc
import math
import os

import pytest
import torch

from tests import tta_oracle as O
from tests.util import _metrics_cpu

pytestmark = pytest.mark.gpu

C = 5
G = os.path.join(os.path.dirname(__file__), "golden")
MODELS = ["mtan", "basic"]
STRIDE = {"mtan": 16, "basic": 32}
SIZE = {"mtan": (32, 48), "basic": (32, 64)}


@pytest.fixture(autouse=True)
def _collect_models():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _module(dev, name, **kw):
    from vision_mtl_amd.lit_module import MTLModule

    if name == "mtan":
        from vision_mtl_amd.models.mtan_model import MTANMiniUnet

        fx = torch.load(os.path.join(G, "mtan_tiny.pt"), weights_only=False)
        c = fx["cfg"]
        assert c["C"] == C
        model = MTANMiniUnet(3, dict(fx["tasks"]), c["hidden"], c["first"], c["levels"])
        model.load_state_dict(fx["state_dict"])
    else:
        from vision_mtl_amd.utils.pipeline_utils import build_model

        torch.manual_seed(0)
        model = build_model(argparse.Namespace(model_name="basic", backbone_weights=None), argparse.Namespace(num_classes=C))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # running buffers away from their init values: eval mode then matters
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    return MTLModule(model.to(dev), num_classes=C, device=str(dev), **kw).eval()


def _aug(name, **kw):
    from vision_mtl_amd.inference import PredictAugment

    return PredictAugment(size_multiple=STRIDE[name], **kw)


def _batch(name, dev, seed=100, size=None, targets=True, ignore=None):
    from vision_mtl_amd.data import synthetic_batch

    H, W = SIZE[name]
    b = synthetic_batch(2, H, W, C, seed=seed, masked=0.1)
    if size is not None and targets:  # targets at the output size
        t = synthetic_batch(2, size[0], size[1], C, seed=seed + 1, masked=0.1)
        b["mask"], b["depth"] = t["mask"], t["depth"]
    if ignore is not None:
        g = torch.Generator().manual_seed(seed + 2)
        b["mask"][torch.rand(b["mask"].shape, generator=g) < 0.2] = ignore
    if not targets:
        b = {"img": b["img"]}
    return {k: v.to(dev) for k, v in b.items()}


def _bits(x):
    return x.contiguous().view(torch.int32)


def _bn_state(model):
    return {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}


@pytest.mark.parametrize("name", MODELS)
def test_identity_reproduces_the_plain_step_with_no_view_launch(dev, name, monkeypatch):
    from vision_mtl_amd import ops

    module = _module(dev, name)
    batch = _batch(name, dev, targets=False)
    with torch.no_grad():
        plain = module.predict_step(batch)
    module.predict_augment = _aug(name, scales=(1.0,), flip=False, merge="logit")
    names, orig = [], ops._k

    def rec(entry, /, *a, **kw):
        names.append(entry)
        return orig(entry, *a, **kw)

    monkeypatch.setattr(ops, "_k", rec)
    got = module.predict_step(batch)  # runs under no_grad by itself
    monkeypatch.setattr(ops, "_k", orig)
    assert set(got) == {"segm", "depth"} and got["depth"].shape == plain["depth"].shape and not got["depth"].requires_grad
    assert torch.equal(got["segm"], plain["segm"])
    assert torch.equal(_bits(got["depth"]), _bits(plain["depth"]))
    assert "vmtl_tta_view" not in names
    assert names.count("vmtl_tta_accumulate") == 1 and names.count("vmtl_tta_finish") == 1


@pytest.mark.parametrize("kw", [dict(flip=True, merge="prob"),
                                dict(scales=(0.5, 1.0, 1.5), flip=True, merge="logit", output_size="2x"),
                                dict(scales=(0.5, 1.0, 1.5), flip=True, merge="prob", output_size="2x", compensate_depth=True)],
                         ids=["flip", "scales-flip-2x-logit", "scales-flip-2x-prob-gain"])
@pytest.mark.parametrize("name", MODELS)
def test_composed_merge_against_fp64(dev, name, kw):
    from vision_mtl_amd import ops

    H, W = SIZE[name]
    kw = dict(kw)
    if kw.get("output_size") == "2x":
        kw["output_size"] = (2 * H, 2 * W)
    module = _module(dev, name)
    aug = module.predict_augment = _aug(name, return_confidence=True, **kw)
    batch = _batch(name, dev, targets=False)
    table = aug.views(H, W)
    assert len(table) == (2 if "scales" not in kw else 6) and table == O.view_table(H, W, aug.scales, aug.flip, STRIDE[name])
    got = {k: v.cpu() for k, v in module.predict_step(batch).items()}
    assert set(got) == {"segm", "depth", "confidence"} and got["depth"].shape == (2, *aug.out_size(H, W), 1)
    got["depth"] = got["depth"][..., 0]
    views = []
    with torch.no_grad():
        for h, w, flip, s in table:
            view = batch["img"] if (h, w, flip) == (H, W, False) else ops.tta_view(batch["img"], (h, w), flip)
            out = module.model(view)
            assert tuple(out["segm"].shape) == (2, C, h, w) and tuple(out["depth"].shape) == (2, 1, h, w)
            views.append((out["segm"].cpu(), out["depth"].cpu(), flip, s))
    ref = {}
    for dt in (torch.float64, torch.float32):
        acc, acc_d = O.merge(views, (H, W), aug.merge, dt, compensate_depth=aug.compensate_depth)
        ref[dt] = O.finish(acc, acc_d, 1.0 / len(views), aug.out_size(H, W), aug.merge, dt)
    sh = O.compare(got, ref[torch.float32], ref[torch.float64], what=f"{name} {kw}")
    print(f"{name} {kw}: {len(views)} views, depth {sh['depth']:.3f}, confidence {sh['confidence']:.3f} of their bars; tie band "
          f"{100 * sh['band']:.3f} %")


@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("name", MODELS)
def test_targets_at_output_size_metrics_and_nan_loss(dev, name, ignore, monkeypatch):
    from vision_mtl_amd import metrics as M

    H, W = SIZE[name]
    size = (2 * H, 2 * W)
    module = _module(dev, name, segm_ignore_index=ignore)
    module.predict_augment = _aug(name, scales=(0.5, 1.0), flip=True, output_size=size)
    batch = _batch(name, dev, size=size, ignore=ignore)
    cms, orig = [], M.confusion_matrix

    def rec(*a, **k):
        cms.append(orig(*a, **k))
        return cms[-1]

    monkeypatch.setattr(M, "confusion_matrix", rec)
    out = module.predict_step(batch)
    monkeypatch.setattr(M, "confusion_matrix", orig)
    so = module.step_outputs["predict"]
    assert all(len(v) == 1 for v in so.values()) and len(cms) == 1
    assert math.isnan(float(so["loss"][0]))
    segm, mask = out["segm"].cpu(), batch["mask"].cpu()
    valid = torch.ones_like(mask, dtype=torch.bool) if ignore is None else mask != ignore
    assert ignore is None or 0 < int((~valid).sum()) < valid.numel()
    cm, acc, jac, fb = _metrics_cpu(segm[valid], mask[valid], C)
    assert torch.equal(cms[0].cpu().long(), cm)  # the count behind the step's metrics, exactly
    assert int(cm.sum()) == int(valid.sum())
    assert abs(float(so["accuracy"][0]) - acc) <= 1e-6 and abs(float(so["jaccard_index"][0]) - jac) <= 1e-6
    assert abs(float(so["fbeta_score"][0]) - fb) <= 1e-6
    mae = float((out["depth"].cpu().double() - batch["depth"].cpu().double()).abs().mean())
    assert abs(float(so["mae"][0]) - mae) <= 1e-6
    # targets at the training resolution are the wrong size for this object
    with pytest.raises(ValueError, match="predict_augment"):
        module.predict_step(_batch(name, dev, ignore=ignore))
    assert all(len(v) == 1 for v in so.values())


@pytest.mark.parametrize("name", MODELS)
def test_graphed_predict_replays_bit_identical_to_eager(dev, name):
    from vision_mtl_amd.graphed import GraphedEval

    H, W = SIZE[name]
    size = (2 * H, 2 * W)
    module = _module(dev, name)
    module.predict_augment = _aug(name, scales=(0.5, 1.0, 1.5), flip=True, output_size=size, return_confidence=True)
    module.step_outputs["predict"]["loss"].append(torch.tensor(1.5, device=dev))
    before_bn = _bn_state(module.model)
    before_so = {s: {k: list(v) for k, v in d.items()} for s, d in module.step_outputs.items()}
    geval = GraphedEval(module, _batch(name, dev, seed=7, size=size), stage="predict")
    torch.cuda.synchronize()
    assert geval.predict_augment is module.predict_augment
    for k, v in _bn_state(module.model).items():
        assert torch.equal(v, before_bn[k]), k
    for s, d in module.step_outputs.items():
        assert {k: len(v) for k, v in d.items()} == {k: len(v) for k, v in before_so[s].items()}
        assert all(a is b for k in d for a, b in zip(d[k], before_so[s][k]))
    batches = [_batch(name, dev, seed=100 + i, size=size) for i in range(2)]
    got = [geval(b) for b in batches]
    so_g = {k: [x.clone() for x in v[-2:]] for k, v in module.step_outputs["predict"].items()}
    ref = [module.predict_step(b) for b in batches]
    so_e = {k: [x.clone() for x in v[-2:]] for k, v in module.step_outputs["predict"].items()}
    for a, b in zip(got, ref):
        assert set(a) == set(b) == {"segm", "depth", "confidence"}
        assert torch.equal(a["segm"], b["segm"])
        assert torch.equal(_bits(a["depth"]), _bits(b["depth"])) and torch.equal(_bits(a["confidence"]), _bits(b["confidence"]))
    assert not torch.equal(got[0]["depth"], got[1]["depth"])
    for k in so_g:
        for x, y in zip(so_g[k], so_e[k]):
            assert torch.equal(x.float(), y.float()) or (x.isnan().all() and y.isnan().all()), k
    # another object than the one captured: refused
    captured = module.predict_augment
    module.predict_augment = _aug(name, flip=True)
    with pytest.raises(ValueError, match="predict_augment"):
        geval(batches[0])
    module.predict_augment = None
    with pytest.raises(ValueError, match="predict_augment"):
        geval(batches[0])
    module.predict_augment = captured
    again = geval(batches[0])
    assert torch.equal(again["segm"], got[0]["segm"]) and torch.equal(_bits(again["depth"]), _bits(got[0]["depth"]))


@pytest.mark.parametrize("name", MODELS)
def test_other_steps_ignore_the_attribute(dev, name):
    module = _module(dev, name)
    batch = _batch(name, dev)
    H, W = SIZE[name]

    start = {k: v.clone() for k, v in module.model.state_dict().items()}

    def losses():
        module.model.load_state_dict(start)  # the train-mode steps move the running buffers the eval-mode ones read
        module.train()
        with torch.no_grad():
            out = [module.training_step(batch), module.validation_step(batch), module.test_step(batch)]
        module.eval()
        with torch.no_grad():
            out += [module.validation_step(batch), module.test_step(batch)]
        return [x.detach().clone() for x in out]

    plain = losses()
    module.predict_augment = _aug(name, scales=(0.5, 1.0, 1.5), flip=True, output_size=(2 * H, 2 * W))
    with_obj = losses()
    for a, b in zip(plain, with_obj):
        assert torch.equal(_bits(a), _bits(b))
