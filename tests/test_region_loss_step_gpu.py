"""-m gpu: MTLModule(segm_region_weight=, segm_region_alpha=, ...) through the whole step - eager, GraphedStep and
GraphedEval - on `basic` (3x3x64x96, C = 19) and on the `mtan` configuration of tests/golden/mtan_tiny.pt, in the pattern
of tests/test_depth_grad_step_gpu.py / tests/test_ohem_step_gpu.py: region weight 0.5 with (alpha, beta, smooth) =
(0.3, 0.7, 1.0), about 20 % void pixels (label 255), class weights on, static loss weights 0.7 / 1.3.

The step's loss_segm is compared bit for bit with the stand-alone node on the logits captured at calc_losses and with the
fp64 oracle (tests/region_oracle.py) within the kernels' 1e-5; the gradient must reach the head as the node's NHWC
storage (the backward records exactly the relayout launches of a plain cross-entropy step).  Parameter gradients are
compared with the CPU oracle model + the oracle's composition of the loss in fp64 under the bar of
tests/test_depth_grad_step_gpu.py (tests/util.py::assert_grads_as_good_as_fp32_cpu).  A captured step replayed on
three batches is compared with the eager loop bit for bit: losses, step outputs and the flat gradient."""
import argparse
import gc
import os

import pytest
import torch

from tests import region_oracle as R
from tests.util import assert_grads_as_good_as_fp32_cpu

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
IGN = 255
W_SEGM, W_DEPTH = 0.7, 1.3
REGION = dict(segm_region_weight=0.5, segm_region_alpha=0.3, segm_region_beta=0.7, segm_region_smooth=1.0)
SETTING = (0.3, 0.7, 1.0)
NAMES = ("basic", "mtan")


@pytest.fixture(autouse=True)
def _collect_models():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _setup(name):
    """(model factory, CPU oracle forward(sd, img), C, (B, H, W)); every call of the factory gives the same weights"""
    if name == "basic":
        from oracle.unet_mobilenetv3 import basic_forward
        from vision_mtl_amd.utils.pipeline_utils import build_model

        C, shape = 19, (3, 64, 96)

        def make():
            torch.manual_seed(3)
            return build_model(argparse.Namespace(model_name="basic", backbone_weights=None),
                               argparse.Namespace(num_classes=C))

        forward = lambda sd, img: basic_forward(sd, img, True)
    else:
        from oracle.mtan import mtan_forward
        from vision_mtl_amd.models.mtan_model import MTANMiniUnet

        fx = torch.load(os.path.join(G, "mtan_tiny.pt"), weights_only=False)
        C, cfg = fx["cfg"]["C"], fx["cfg"]
        B, _, H, W = fx["batch"]["img"].shape
        shape = (B, H, W)

        def make():
            m = MTANMiniUnet(3, dict(fx["tasks"]), cfg["hidden"], cfg["first"], cfg["levels"])
            m.load_state_dict(fx["state_dict"])
            return m

        forward = lambda sd, img: mtan_forward(sd, img, list(dict(fx["tasks"])), cfg["levels"], training=True)
    return make, forward, C, shape


def _weights(C):
    return (0.1 + 1.9 * torch.rand(C, generator=torch.Generator().manual_seed(C))).tolist()


def _module(make, C, dev, term=True, **kw):
    from vision_mtl_amd.lit_module import MTLModule

    if term:
        kw.update(REGION)
    return MTLModule(make().to(dev).train(), num_classes=C, device=str(dev), loss_segm_weight=W_SEGM,
                     loss_depth_weight=W_DEPTH, segm_ignore_index=IGN, segm_class_weights=_weights(C), **kw)


def _batch(C, shape, seed, void=0.2, drop=0):
    """`drop`: the labels of the last `drop` classes become class 0, so those classes are absent from the batch"""
    from vision_mtl_amd.data import synthetic_batch

    B, H, W = shape
    b = synthetic_batch(B, H, W, C, seed=seed, masked=0.1)
    b["mask"][b["mask"] >= C - drop] = 0
    g = torch.Generator().manual_seed(seed + 1)
    b["mask"][torch.rand(B, H, W, generator=g) < void] = IGN
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


def _capture_calc_losses(module):
    seen, orig = {}, module.calc_losses

    def calc(gt_mask, gt_depth, out):
        r = orig(gt_mask, gt_depth, out)
        seen.update(out=dict(out), losses=r)
        return r

    module.calc_losses = calc
    return seen


def _recorded(fn):
    """([(entry point, its integer arguments)], fn())"""
    from vision_mtl_amd import ops

    launches, orig_k = [], ops._k

    def rec(kname, *a, **kw):
        launches.append((kname, {k: v for k, v in kw.items() if isinstance(v, int)}))
        return orig_k(kname, *a, **kw)

    ops._k = rec
    try:
        out = fn()
    finally:
        ops._k = orig_k
    return launches, out


def _train(module, batch, dev):
    def step():
        loss = module.training_step(_dev(batch, dev), 0)
        loss.backward()
        return loss

    launches, loss = _recorded(step)
    torch.cuda.synchronize()
    return launches, loss


def _relayouts(launches):
    return [(n, kw) for n, kw in launches if n in ("vmtl_nchw_to_nhwc", "vmtl_nhwc_to_nchw")]


@pytest.mark.parametrize("name", NAMES)
def test_training_step_matches_the_node_the_fp64_oracle_and_the_oracle_model(dev, name):

    from vision_mtl_amd import ops

    make, forward, C, shape = _setup(name)
    module = _module(make, C, dev)
    assert {k: module.hparams[k] for k in REGION} == REGION
    assert module.segm_criterion.weight.device.type == "cuda"
    batch = _batch(C, shape, seed=21)
    sd0 = {k: v.clone() for k, v in make().state_dict().items()}
    seen = _capture_calc_losses(module)
    launches, loss = _train(module, batch, dev)
    names = [n for n, _ in launches]
    assert names.count("vmtl_ce_region_fwd") == 1 and names.count("vmtl_ce_region_bwd") == 1
    assert not any(n.startswith("vmtl_ce_") and "region" not in n for n in names)
    # ---- the gradient reaches the head as the node's NHWC storage: the relayout launches of a plain step, no more
    plain = _module(make, C, dev, term=False)
    ops.packs.invalidate()
    plain_launches, _ = _train(plain, batch, dev)
    assert "vmtl_ce_bwd_ex" in [n for n, _ in plain_launches]
    assert _relayouts(launches) == _relayouts(plain_launches)
    assert not any(kw.get("C") == C for n, kw in _relayouts(launches) if n == "vmtl_nchw_to_nhwc")
    # ---- the stand-alone node on the logits of this step, and the fp64 oracle
    logits = seen["out"]["segm_logits"].detach()
    loss_segm = seen["losses"]["loss_segm"].detach()
    w = torch.tensor(_weights(C), dtype=torch.float32)
    alone, pred = ops.segm_region_loss_with_argmax(logits, batch["mask"].to(dev), 0.5, *SETTING, weight=w.to(dev),
                                                   ignore_index=IGN)
    assert torch.equal(alone.view(torch.int32), loss_segm.view(torch.int32))
    assert torch.equal(pred, seen["out"]["segm_predictions"]) and torch.equal(pred, logits.argmax(dim=1))
    r = R.reference(logits.cpu(), batch["mask"], *SETTING, w, IGN, 1.0, 0.5)
    print(f"{name}: loss_segm {float(loss_segm):.8g}, fp64 oracle {float(r['loss']):.8g} (CE {float(r['ce']):.6g}, "
          f"L_region {float(r['region']):.6g}), present classes {int((r['N'] > 0).sum())} of {C}")
    assert abs(float(loss_segm) - float(r["loss"])) < 1e-5
    assert float(r["region"]) > 0

    # ---- every parameter gradient against the CPU oracle model + the oracle's composition, fp64 (fp32: the yardstick)
    def cpu(dtype):
        from oracle.losses import silog

        sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
        leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
        out = forward(sd, batch["img"].to(dtype))
        ls = R.compose(out["segm"], batch["mask"], *SETTING, w, IGN, 1.0, 0.5)["loss"]
        ld = silog(torch.sigmoid(out["depth"]).permute(0, 2, 3, 1), batch["depth"].to(dtype), interpolate=False)
        (W_SEGM * ls + W_DEPTH * ld).backward()
        return {k: v.grad for k, v in leaves.items()}, float(W_SEGM * ls + W_DEPTH * ld)

    (g64, l64), (g32, _) = cpu(torch.float64), cpu(torch.float32)
    print(f"{name}: step loss {float(loss.detach()):.8g}, CPU oracle model fp64 {l64:.8g}")
    hip = {k: q.grad.cpu() for k, q in module.model.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in hip.values())
    assert_grads_as_good_as_fp32_cpu(hip, g64, g32)


@pytest.mark.parametrize("name", NAMES)
def test_validation_test_and_predict_report_the_combined_loss(dev, name):
    from vision_mtl_amd import ops

    make, _, C, shape = _setup(name)
    module = _module(make, C, dev)
    batch = _batch(C, shape, seed=51)
    w = torch.tensor(_weights(C), dtype=torch.float32, device=dev)
    for stage in ("val", "test", "predict"):
        seen = _capture_calc_losses(module)
        step = {"val": module.validation_step, "test": module.test_step, "predict": module.predict_step}[stage]

        def run():
            with torch.no_grad():
                step(_dev(batch, dev), 0)

        launches, _ = _recorded(run)
        names = [n for n, _ in launches]
        assert names.count("vmtl_ce_region_fwd") == 1 and "vmtl_ce_fwd_ex" not in names
        logits = seen["out"]["segm_logits"].detach()
        alone = ops.segm_region_loss(logits, batch["mask"].to(dev), 0.5, *SETTING, weight=w, ignore_index=IGN)
        ce = ops.cross_entropy(logits, batch["mask"].to(dev), weight=w, ignore_index=IGN)
        loss_segm = seen["losses"]["loss_segm"]
        assert torch.equal(alone.view(torch.int32), loss_segm.view(torch.int32))
        assert float(loss_segm) > float(ce) and bool(torch.isfinite(module.step_outputs[stage]["loss"][-1]))
        module.calc_losses = type(module).calc_losses.__get__(module)


@pytest.mark.parametrize("name", NAMES)
def test_graphed_step_replays_equal_the_eager_loop(dev, name):
    """Three batches with different void shares and different sets of present classes: V, every N_c and the mask of
    present classes move between replays and stay on the device."""
    from vision_mtl_amd import dp
    from vision_mtl_amd.graphed import GraphedStep

    make, _, C, shape = _setup(name)
    batches = [_batch(C, shape, seed=31 + i, void=v, drop=d) for i, (v, d) in enumerate(((0.2, 0), (0.6, 1), (0.9, C // 2)))]
    example = _batch(C, shape, seed=30)
    assert len({int((b["mask"] != IGN).sum()) for b in batches}) == 3
    present = [frozenset(b["mask"][b["mask"] != IGN].unique().tolist()) for b in batches]
    assert len(set(present)) == 3 and len(present[2]) < len(present[0]) <= C
    sd0 = {k: v.clone() for k, v in make().state_dict().items()}

    def run(graphed):
        module = _module(make, C, dev)
        arena = dp.FlatArena(module.model)
        if graphed:
            gstep = GraphedStep(module, example, arena=arena)
            dp.ops.packs.invalidate()
        else:
            arena.rebind_grads()
        losses, grads = [], []
        for b in batches:  # every step from the same weights and BatchNorm buffers: no optimizer in between
            module.model.load_state_dict(sd0)
            dp.ops.packs.invalidate()
            arena.flat_grad.zero_()
            arena.rebind_grads()
            loss = gstep(b) if graphed else module.training_step(_dev(b, dev), 0)
            loss.backward()
            torch.cuda.synchronize()
            losses.append(loss.detach().clone())
            grads.append(arena.flat_grad.clone())
        so = _so(module, "train")
        return losses, grads, {k: v[-len(batches):] for k, v in so.items()}

    le, ge, soe = run(False)
    lg, gg, sog = run(True)
    assert len({float(x) for x in le}) == 3
    for a, b in zip(lg, le):
        assert torch.isfinite(b) and torch.equal(a.float(), b.float()), (float(a), float(b))
    _assert_so_equal(sog, soe)
    for a, b in zip(gg, ge):
        assert bool(torch.isfinite(a).all())
        err, mag = float((a.double() - b.double()).abs().max()), float(b.double().abs().max())
        assert torch.equal(a, b), f"replayed gradients: {err:.3e} vs magnitude {mag:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_graphed_eval_equals_the_eager_validation_step(dev, name):
    from vision_mtl_amd.graphed import GraphedEval

    make, _, C, shape = _setup(name)
    batches = [_batch(C, shape, seed=41 + i, void=v, drop=d) for i, (v, d) in enumerate(((0.2, 0), (0.6, 3), (0.9, 0)))]
    me, mg = _module(make, C, dev), _module(make, C, dev)
    geval = GraphedEval(mg, _batch(C, shape, seed=40), stage="val")
    lg = [geval(b) for b in batches]
    with torch.no_grad():
        le = [me.validation_step(_dev(b, dev)) for b in batches]
    for a, b in zip(lg, le):
        assert torch.isfinite(b) and torch.equal(a.float(), b.float()), (float(a), float(b))
    _assert_so_equal(_so(mg, "val"), _so(me, "val"))
    plain = _module(make, C, dev, term=False)
    with torch.no_grad():
        lp = [plain.validation_step(_dev(b, dev)) for b in batches]
    assert all(float(a) > float(b) for a, b in zip(le, lp))  # the validation loss includes the term


@pytest.mark.parametrize("name", NAMES)
def test_option_unset_is_the_step_it_was(dev, name):
    """A module given the other three arguments but no segm_region_weight against one built without any of them: the
    plain launches, the same bits in the loss, the step outputs and every parameter gradient."""
    from vision_mtl_amd import dp
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.losses import CrossEntropyLoss

    make, _, C, shape = _setup(name)
    batch = _batch(C, shape, seed=61)
    out = []
    for unset in (False, True):
        kw = dict(segm_region_weight=None, segm_region_alpha=0.3, segm_region_beta=0.7, segm_region_smooth=1.0) if unset else {}
        module = MTLModule(make().to(dev).train(), num_classes=C, device=str(dev), loss_segm_weight=W_SEGM,
                           loss_depth_weight=W_DEPTH, **kw)
        assert type(module.segm_criterion) is CrossEntropyLoss and module.segm_criterion.region_weight is None
        assert not any(k.startswith("segm_region") for k in module.hparams)
        dp.ops.packs.invalidate()
        plain_batch = dict(batch, mask=batch["mask"].clamp(0, C - 1))  # no ignore index here: every label is a class
        launches, loss = _train(module, plain_batch, dev)
        names = [n for n, _ in launches]
        assert names.count("vmtl_ce_fwd_argmax") == 1 and names.count("vmtl_ce_bwd_strided") == 1
        assert not any("region" in n for n in names)
        grads = {k: p.grad.clone() for k, p in module.model.named_parameters()}
        # the loss launches (the weight-pack launches of a step depend on what the pack cache already holds)
        loss_launches = [n for n in names if "silog" in n or n.startswith("vmtl_ce_") or n == "vmtl_add_losses"]
        out.append((loss_launches, loss.detach().clone(), _so(module, "train"), grads))
    assert out[0][0] == out[1][0] and len(out[0][0]) >= 4
    assert torch.isfinite(out[0][1]) and torch.equal(out[0][1], out[1][1])
    _assert_so_equal(out[0][2], out[1][2])
    worst = max(float((out[0][3][k].double() - out[1][3][k].double()).abs().max()) for k in out[0][3])
    print(f"{name}: largest parameter-gradient difference between the two modules {worst:.3e}")
    assert all(torch.equal(out[0][3][k], out[1][3][k]) for k in out[0][3])
