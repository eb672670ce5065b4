"""-m gpu: MTLModule(segm_ohem_min_kept=, segm_ohem_thresh=) through the whole step - eager, GraphedStep and GraphedEval -
on `basic` (2x3x32x64, C = 19) and on the `mtan` configuration of tests/golden/mtan_tiny.pt, in the pattern of
tests/test_loss_ignore_step_gpu.py: min_kept = 256 per image, thresh 0.7 (an untrained network puts every pixel above
tau, so tau is the cut) and 1e-3 (nothing reaches tau, so the K-th largest nll is the cut), about 20 % void pixels
(label 255), class weights on.

The training step's loss_segm is compared bit for bit with the stand-alone op on the logits captured at calc_losses, and
with the fp64 oracle (tests/ohem_oracle.py) within the kernels' 1e-5 - after asserting that the fp64 nll of those logits
keeps its margin around the cut, so that membership cannot differ.  Validation, test and predict report the un-mined
loss, bit-equal to a module built without the two arguments.  Captured steps are compared with eager ones as
tests/test_loss_ignore_step_gpu.py compares them."""
import argparse
import gc
import os

import pytest
import torch

from tests import ohem_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
IGN = 255
W_SEGM, W_DEPTH = 0.7, 1.3
NAMES = ("basic", "mtan")
MIN_KEPT = 256
THRESHOLDS = (0.7, 1e-3)
# the batch seed of the eager test, per (model, thresh): the margin precondition below has to hold on the logits the
# model produces for that batch.  Seed 21 (the seed of tests/test_loss_ignore_step_gpu.py) does, with two orders of
# magnitude to spare: margins 1.6e-3 (basic) and 1.9e-3 (mtan) against 1.7e-5 and 9.3e-6 needed.
SEED ={("basic", 0.7): 21, ("basic", 1e-3): 21, ("mtan", 0.7): 21, ("mtan", 1e-3): 21}


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


def _module(make, C, dev, thresh=None, mining=True):
    from vision_mtl_amd.lit_module import MTLModule

    kw = dict(segm_ohem_min_kept=MIN_KEPT, segm_ohem_thresh=thresh) if mining else {}
    return MTLModule(make().to(dev).train(), num_classes=C, device=str(dev), loss_segm_weight=W_SEGM,
                     loss_depth_weight=W_DEPTH, segm_ignore_index=IGN, segm_class_weights=_weights(C), **kw)


def _batch(C, shape, seed, void=0.2):
    from vision_mtl_amd.data import synthetic_batch

    B, H, W = shape
    b = synthetic_batch(B, H, W, C, seed=seed, masked=0.1)
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


@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_training_step_mines_and_matches_the_op_and_the_fp64_oracle(dev, name, thresh):
    from vision_mtl_amd import ops

    make, C, shape = _setup(name)
    module = _module(make, C, dev, thresh)
    assert module.hparams["segm_ohem_min_kept"] == MIN_KEPT and module.hparams["segm_ohem_thresh"] == thresh
    assert module.segm_train_criterion.weight.device.type == "cuda"
    batch = _batch(C, shape, seed=SEED[name, thresh])
    seen = _capture_calc_losses(module)
    names, orig_k = [], ops._k

    def rec(kname, *a, **kw):
        names.append(kname)
        return orig_k(kname, *a, **kw)

    ops._k = rec
    try:
        loss = module.training_step(_dev(batch, dev), 0)
        loss.backward()
    finally:
        ops._k = orig_k
    torch.cuda.synchronize()
    assert names.count("vmtl_ce_ohem_fwd") == 1 and names.count("vmtl_ce_ohem_bwd") == 1
    assert "vmtl_ce_fwd_ex" not in names and "vmtl_ce_bwd_ex" not in names
    logits = seen["out"]["segm_logits"].detach()
    loss_segm = seen["losses"]["loss_segm"].detach()
    w = torch.tensor(_weights(C), dtype=torch.float32)
    alone, pred = ops.cross_entropy_ohem_with_argmax(logits, batch["mask"].to(dev), MIN_KEPT, thresh=thresh,
                                                     weight=w.to(dev), ignore_index=IGN)
    assert torch.equal(alone.view(torch.int32), loss_segm.view(torch.int32))
    assert torch.equal(pred, seen["out"]["segm_predictions"]) and torch.equal(pred, logits.argmax(dim=1))
    # the fp64 oracle on the same logits; first: its nll stays clear of both decisions by twice the kernels' nll bound
    z = logits.cpu()
    total = MIN_KEPT * shape[0]
    nll, valid = O.nll64(z, batch["mask"], IGN)
    need = 2 * 2.0 ** -19 * max(1.0, float(z.abs().max()))
    m = O.margin(nll, valid, total, O.tau_of(thresh))
    print(f"{name}, thresh {thresh}, seed {SEED[name, thresh]}: margin {m:.3e} (needs {need:.3e}), V {int(valid.sum())}")
    assert m > need
    r = O.reference(z, batch["mask"], total, thresh, w, IGN)
    print(f"{name}, thresh {thresh}: loss_segm {float(loss_segm):.8g}, fp64 oracle {float(r['loss']):.8g}, cut "
          f"{float(r['cut']):.6g}, kept {int(r['kept'].sum())}")
    assert abs(float(loss_segm) - float(r["loss"])) < 1e-5
    if thresh == 0.7:   # tau governs: an untrained network is nowhere 70 % sure
        assert float(r["cut"]) == O.tau_of(thresh)
    else:               # kappa governs: fewer than K pixels are below a probability of 1e-3
        assert float(r["cut"]) < O.tau_of(thresh) and int(r["kept"].sum()) == total < int(valid.sum())
    grads = [p.grad for p in module.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)


@pytest.mark.parametrize("name", NAMES)
def test_validation_test_and_predict_report_the_unmined_loss(dev, name):
    from vision_mtl_amd import ops

    make, C, shape = _setup(name)
    mined, plain = _module(make, C, dev, 1e-3), _module(make, C, dev, mining=False)
    batch = _batch(C, shape, seed=51)
    names, orig_k = [], ops._k

    def rec(kname, *a, **kw):
        names.append(kname)
        return orig_k(kname, *a, **kw)

    for stage in ("val", "test", "predict"):
        out = []
        for module in (mined, plain):
            module.model.load_state_dict(make().state_dict())
            ops.packs.invalidate()
            step = {"val": module.validation_step, "test": module.test_step, "predict": module.predict_step}[stage]
            ops._k = rec
            try:
                with torch.no_grad():
                    step(_dev(batch, dev), 0)
            finally:
                ops._k = orig_k
            out.append(_so(module, stage))
        assert not any("ohem" in n for n in names) and "vmtl_ce_fwd_ex" in names
        _assert_so_equal(out[0], out[1])
    # ... while the training step of the same module does mine
    names.clear()
    ops._k = rec
    try:
        mined.training_step(_dev(batch, dev), 0)
    finally:
        ops._k = orig_k
    assert "vmtl_ce_ohem_fwd" in names and mined._mining is False


@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_graphed_step_replays_equal_the_eager_loop(dev, name, thresh):
    """Three changing batches with different void shares, so that V, K's clamp and the cut all move between replays:
    K and tau are host constants of the capture, everything else stays on the device."""
    from vision_mtl_amd import dp
    from vision_mtl_amd.graphed import GraphedStep

    make, C, shape = _setup(name)
    batches = [_batch(C, shape, seed=31 + i, void=v) for i, v in enumerate((0.2, 0.6, 0.9))]
    example = _batch(C, shape, seed=30)
    assert len({int((b["mask"] != IGN).sum()) for b in batches}) == 3
    assert int((batches[2]["mask"] != IGN).sum()) < MIN_KEPT * shape[0]  # the last batch clamps K to V
    sd0 = {k: v.clone() for k, v in make().state_dict().items()}

    def run(graphed):
        module = _module(make, C, dev, thresh)
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
        assert err <= 1e-5 * mag + 1e-8, f"replayed gradients: {err:.3e} vs magnitude {mag:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_graphed_eval_equals_the_eager_validation_step(dev, name):
    from vision_mtl_amd.graphed import GraphedEval

    make, C, shape = _setup(name)
    batches = [_batch(C, shape, seed=41 + i) for i in range(2)]
    me, mg = _module(make, C, dev, 0.7), _module(make, C, dev, 0.7)
    geval = GraphedEval(mg, _batch(C, shape, seed=40), stage="val")
    lg = [geval(b) for b in batches]
    with torch.no_grad():
        le = [me.validation_step(_dev(b, dev)) for b in batches]
    for a, b in zip(lg, le):
        assert torch.isfinite(b) and torch.equal(a.float(), b.float()), (float(a), float(b))
    _assert_so_equal(_so(mg, "val"), _so(me, "val"))
    plain = _module(make, C, dev, mining=False)
    with torch.no_grad():
        lp = [plain.validation_step(_dev(b, dev)) for b in batches]
    for a, b in zip(le, lp):
        assert torch.equal(a.float(), b.float())
