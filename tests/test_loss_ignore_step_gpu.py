"""-m gpu: MTLModule(segm_ignore_index=, segm_class_weights=) through the whole step - eager, GraphedStep and
GraphedEval - on `basic` (2x3x32x64, C = 19) and on the `mtan` configuration of tests/golden/mtan_tiny.pt, with about
20 % void pixels (label 255) in the masks.

The loss is checked against loss_segm_weight * F.cross_entropy(weight, ignore_index) + loss_depth_weight * SILog, both
evaluated on the CPU in fp64 from the logits / depth predictions of the SAME step (captured at calc_losses), with the
kernels' own tolerances (tests/test_loss_ignore_gpu.py: 1e-5 absolute for the cross entropy, 1e-5 relative for SILog).
Captured steps are compared with the eager step bit for bit, as tests/test_graphed_eval_gpu.py compares them (the graph
runs the same deterministic forward kernels on the same inputs); the parameter gradients of the training step with the
bound of tests/test_train_loop_gpu.py::assert_close_ (their weight-gradient sums are not order-fixed)."""
import argparse
import gc
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
IGN = 255
W_SEGM, W_DEPTH = 0.7, 1.3
NAMES = ("basic", "mtan")


@pytest.fixture(autouse=True)
def _collect_models():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _setup(name):
    """(model factory, C, (B, H, W)); every call of the factory gives the same weights"""
    if name == "basic":
        from vision_mtl_amd.utils.pipeline_utils import build_model

        C, shape = 19, (2, 32, 64)

        def make():
            torch.manual_seed(3)
            return build_model(argparse.Namespace(model_name="basic", backbone_weights=None),
                               argparse.Namespace(num_classes=C))
    else:
        from vision_mtl_amd.models.mtan_model import MTANMiniUnet

        fx = torch.load(os.path.join(G, "mtan_tiny.pt"), weights_only=False)
        C, cfg = fx["cfg"]["C"], fx["cfg"]
        B, _, H, W = fx["batch"]["img"].shape
        shape = (B, H, W)

        def make():
            m = MTANMiniUnet(3, dict(fx["tasks"]), cfg["hidden"], cfg["first"], cfg["levels"])
            m.load_state_dict(fx["state_dict"])
            return m
    return make, C, shape


def _weights(C):
    return (0.1 + 1.9 * torch.rand(C, generator=torch.Generator().manual_seed(C))).tolist()


def _module(make, C, dev, **kw):
    from vision_mtl_amd.lit_module import MTLModule

    return MTLModule(make().to(dev).train(), num_classes=C, device=str(dev), loss_segm_weight=W_SEGM,
                     loss_depth_weight=W_DEPTH, segm_ignore_index=IGN, segm_class_weights=_weights(C), **kw)


def _batch(C, shape, seed):
    from vision_mtl_amd.data import synthetic_batch

    B, H, W = shape
    b = synthetic_batch(B, H, W, C, seed=seed, masked=0.1)
    g = torch.Generator().manual_seed(seed + 1)
    b["mask"][torch.rand(B, H, W, generator=g) < 0.2] = IGN
    return b


def _dev(b, dev):
    return {k: v.to(dev) for k, v in b.items()}


def _so(module, stage):
    return {k: [v.clone() for v in vals] for k, vals in module.step_outputs[stage].items()}


def _assert_so_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert len(a[k]) == len(b[k]) and len(a[k]) > 0, k
        for x, y in zip(a[k], b[k]):
            assert torch.isfinite(x).all(), (k, x)
            assert torch.equal(x.float(), y.float()), (k, x, y)


def _silog_fp64(pred, target, min_depth=1e-3):
    pred, target = pred.double(), target.double()
    m = target > min_depth
    g = torch.log(pred[m]) - torch.log(target[m])
    return 10 * torch.sqrt(torch.var(g) + 0.15 * torch.pow(torch.mean(g), 2))  # reference losses.py:29-36


@pytest.mark.parametrize("name", NAMES)
def test_step_loss_is_the_weighted_ignoring_sum_and_gradients_are_finite(dev, name):
    from vision_mtl_amd import metrics as M

    make, C, shape = _setup(name)
    module = _module(make, C, dev)
    assert module.hparams["segm_ignore_index"] == IGN and len(module.hparams["segm_class_weights"]) == C
    batch = _batch(C, shape, seed=21)
    seen, orig = {}, module.calc_losses

    def calc(gt_mask, gt_depth, out):
        r = orig(gt_mask, gt_depth, out)
        seen.update(out=dict(out), losses=r)
        return r

    module.calc_losses = calc
    loss = module.training_step(_dev(batch, dev), 0)
    loss.backward()
    torch.cuda.synchronize()
    out = seen["out"]
    ce = F.cross_entropy(out["segm_logits"].detach().cpu().double(), batch["mask"],
                         weight=torch.tensor(_weights(C), dtype=torch.float32).double(), ignore_index=IGN)
    sl = _silog_fp64(out["depth_predictions"].detach().cpu(), batch["depth"])
    ref = W_SEGM * ce + W_DEPTH * sl
    print(f"{name}: loss {loss.item():.8g}, CPU fp64 {ref.item():.8g} (CE {ce.item():.6g}, SILog {sl.item():.6g})")
    assert abs(seen["losses"]["loss_segm"].item() - ce.item()) < 1e-5
    assert abs(loss.item() - ref.item()) <= W_SEGM * 1e-5 + W_DEPTH * 1e-5 * abs(sl.item())
    grads = [p.grad for p in module.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    # the step's metrics leave the void pixels out: the confusion matrix of its own predictions, void excluded
    pred = out["segm_predictions"]
    assert torch.equal(pred, out["segm_logits"].detach().argmax(dim=1))
    valid = batch["mask"] != IGN
    acc = float((pred.cpu()[valid] == batch["mask"][valid]).double().mean())
    assert abs(float(module.step_outputs["train"]["accuracy"][-1]) - acc) <= 1e-6
    cm = M.confusion_matrix(pred, batch["mask"].to(dev), C, ignore_index=IGN)
    assert int(cm.sum()) == int(valid.sum())
    for k in ("jaccard_index", "fbeta_score", "mae"):
        assert bool(torch.isfinite(module.step_outputs["train"][k][-1]))


@pytest.mark.parametrize("name", NAMES)
def test_graphed_step_replay_equals_the_eager_step(dev, name):
    from vision_mtl_amd import dp
    from vision_mtl_amd.graphed import GraphedStep

    make, C, shape = _setup(name)
    batch, example = _batch(C, shape, seed=31), _batch(C, shape, seed=30)
    sd0 = {k: v.clone() for k, v in make().state_dict().items()}

    def run(graphed):
        module = _module(make, C, dev)
        arena = dp.FlatArena(module.model)
        if graphed:
            gstep = GraphedStep(module, example, arena=arena)
            module.model.load_state_dict(sd0)  # undo the BatchNorm-buffer drift of the warm-up / rehearsal steps
            dp.ops.packs.invalidate()
            loss = gstep(batch)
        else:
            arena.rebind_grads()
            loss = module.training_step(_dev(batch, dev), 0)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), arena.flat_grad.clone(), _so(module, "train")

    le, ge, soe = run(False)
    lg, gg, sog = run(True)
    assert torch.isfinite(le) and torch.equal(lg.float(), le.float()), (float(lg), float(le))
    _assert_so_equal(sog, soe)
    assert bool(torch.isfinite(gg).all())
    err, mag = float((gg.double() - ge.double()).abs().max()), float(ge.double().abs().max())
    assert err <= 1e-5 * mag + 1e-8, f"replayed gradients: {err:.3e} vs magnitude {mag:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_graphed_eval_replay_equals_the_eager_validation_step(dev, name):
    from vision_mtl_amd.graphed import GraphedEval

    make, C, shape = _setup(name)
    batches = [_batch(C, shape, seed=41 + i) for i in range(2)]
    me, mg = _module(make, C, dev), _module(make, C, dev)
    geval = GraphedEval(mg, _batch(C, shape, seed=40), stage="val")
    lg = [geval(b) for b in batches]
    with torch.no_grad():
        le = [me.validation_step(_dev(b, dev)) for b in batches]
    for a, b in zip(lg, le):
        assert torch.isfinite(b) and torch.equal(a.float(), b.float()), (float(a), float(b))
    _assert_so_equal(_so(mg, "val"), _so(me, "val"))


def test_state_dict_keys_do_not_change(dev):
    from vision_mtl_amd.lit_module import MTLModule

    make, C, _ = _setup("mtan")
    plain = MTLModule(make().to(dev), num_classes=C, device=str(dev))
    new = _module(make, C, dev)
    assert list(new.state_dict().keys()) == list(plain.state_dict().keys())
    assert new.segm_criterion.weight.device.type == "cuda"  # the weights joined the model on its device
    plain.load_state_dict(new.state_dict())  # strict: no missing / unexpected key
