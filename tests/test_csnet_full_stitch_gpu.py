"""-m gpu: CSNet(stitch_mixing="full") - every stitch site mixes the two task networks with the whole (2,2[,C]) matrix -
against the straight-line CPU oracle (oracle/cross_stitch.py) whose module-level `_stitch` is replaced, for the test
only, by the full-mix einsum below.  2x64x64, 19 classes, both stitch layouts: one train-mode step, the tight gradient
bar of tests/test_tight_grads_gpu.py (identity activations, non-trivial BatchNorm affine parameters, worst fp32 oracle
over a fixed set of thread counts), eval mode, gradients written into FlatArena slots (side stream off / on, hipGraph
replay), GraphedStep and GraphedEval."""
import argparse

import pytest
import torch

from tests.util import assert_close, assert_grads_tight, identity_activations, nontrivial_bn_affine, worst_of_runs

pytestmark = pytest.mark.gpu
NC, SHAPE = 19, (2, 64, 64)
LAYOUTS = pytest.mark.parametrize("channel_wise", [True, False], ids=["channel_wise", "layer_wise"])
ENC_SITE = "cross_stitch_layers.0_encoder_model_blocks_1.weights"


def _full_stitch(sd, name, feats, tasks):
    """the cross-stitch unit: y_a = sum_b w[a,b,(c)] * x_b"""
    w = sd[f"cross_stitch_layers.{name}.weights"]
    x = torch.stack([feats[t] for t in tasks])
    y = torch.einsum("abc,bncij->ancij" if w.dim() == 3 else "ab,bncij->ancij", w, x)
    return {t: y[a] for a, t in enumerate(tasks)}


@pytest.fixture
def full_oracle(monkeypatch):
    import oracle.cross_stitch as oc

    monkeypatch.setattr(oc, "_stitch", _full_stitch)
    return oc.csnet_forward


def _build(channel_wise, seed=11, mixing="full"):
    from vision_mtl_amd.utils.pipeline_utils import build_model

    torch.manual_seed(seed)
    return build_model(argparse.Namespace(model_name="csnet", backbone_weights=None, channel_wise_stitching=channel_wise,
                                          cross_stitch_mixing=mixing), argparse.Namespace(num_classes=NC))


def _batch(seed=11):
    from oracle.losses import synthetic_batch

    return synthetic_batch(*SHAPE, NC, seed=seed, masked=0.1)


def _oracle_step(forward, sd0, batch, dtype, training=True):
    """one step of the patched oracle: outputs, loss, gradients by name, and the state dict it moved (running buffers)"""
    from oracle.losses import step_losses

    sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    out = forward(sd, batch["img"].to(dtype), ["depth", "segm"], training)
    loss = step_losses(out, batch["mask"], batch["depth"].to(dtype))["loss"]
    loss.backward()
    return ({t: o.detach() for t, o in out.items()}, loss.detach(), {k: v.grad for k, v in leaves.items()},
            {k: v.detach() for k, v in sd.items()})


_STEP = {}


def _step_reference(forward, channel_wise):
    """the fp64 train-mode step of the patched oracle from seed 11, computed once per layout and left unchanged"""
    if channel_wise not in _STEP:
        sd0 = {k: v.clone() for k, v in _build(channel_wise).state_dict().items()}
        _STEP[channel_wise] = (sd0,) + _oracle_step(forward, sd0, _batch(), torch.float64)
    return _STEP[channel_wise]


@LAYOUTS
def test_train_step_matches_patched_oracle(dev, full_oracle, channel_wise):
    from vision_mtl_amd.lit_module import MTLModule

    sd0, out64, loss64, g64, sd_after = _step_reference(full_oracle, channel_wise)
    batch = _batch()
    model = _build(channel_wise)
    model.load_state_dict(sd0)
    model = model.to(dev).train()
    module = MTLModule(model, num_classes=NC, device=str(dev))
    dbatch = {k: v.to(dev) for k, v in batch.items()}
    out = model(dbatch["img"])
    assert list(out.keys()) == ["depth", "segm"]
    for t in out:
        assert_close(out[t].detach().cpu(), out64[t], tol=1e-4, what=f"full-mix csnet out {t}")
    model.load_state_dict(sd0)  # the running buffers move once, as the oracle's
    loss = module.training_step(dbatch, 0)
    loss.backward()
    torch.cuda.synchronize()
    assert_close(loss.detach().cpu(), loss64, tol=1e-4, what="full-mix csnet loss")
    sd = model.state_dict()
    n_running = 0
    for k, v in sd_after.items():
        if "running" in k:
            assert_close(sd[k].cpu(), v, tol=1e-4, what=k)
            n_running += 1
        elif "num_batches" in k:
            assert int(sd[k]) == int(v), k
    assert n_running > 0
    n_none = 0
    for k, p in model.named_parameters():
        if g64[k] is None:  # encoder-block BatchNorm parameters never run in the leaf walk
            assert p.grad is None, f"{k} should not receive a gradient"
            n_none += 1
        else:
            assert p.grad is not None, f"no gradient for {k}"
    assert n_none > 0
    # the off-diagonal stitch weights now take part: non-zero gradients at an encoder site, as in the oracle
    w = dict(model.named_parameters())[ENC_SITE].grad.cpu()
    assert float(w[0, 1].abs().max()) > 0.0 and float(w[1, 0].abs().max()) > 0.0
    assert float(g64[ENC_SITE][0, 1].abs().max()) > 0.0


@LAYOUTS
def test_every_gradient_is_tight_without_mask_flips(dev, full_oracle, channel_wise):
    from vision_mtl_amd.lit_module import MTLModule

    model = _build(channel_wise)
    nontrivial_bn_affine(model)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    batch = _batch()
    with identity_activations():
        threads = torch.get_num_threads()
        try:
            _, loss64, g64, _ = _oracle_step(full_oracle, sd0, batch, torch.float64)
            runs = []
            for n in (1, 2, 4, 8, 16):  # the bar is the fp32 oracle's worst error over a fixed set of thread counts
                torch.set_num_threads(n)
                runs.append(_oracle_step(full_oracle, sd0, batch, torch.float32)[2])
        finally:
            torch.set_num_threads(threads)
        g32 = worst_of_runs(g64, runs)
        model = model.to(dev).train()
        module = MTLModule(model, num_classes=NC, device=str(dev))
        loss = module.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
        loss.backward()
        torch.cuda.synchronize()
    assert_close(loss.detach().cpu(), loss64.float(), tol=1e-4, what="full-mix csnet loss (identity activations)")
    hip = {k: p.grad.cpu() for k, p in model.named_parameters() if p.grad is not None}
    missing = [k for k, p in model.named_parameters() if p.grad is None and g64.get(k) is not None
               and float(g64[k].abs().max()) > 0]
    assert not missing, f"no gradient for {missing[:5]}"
    stitch = [k for k in hip if k.startswith("cross_stitch_layers.")]
    assert len(stitch) == 11
    eh, ec, k = assert_grads_tight(hip, g64, g32)
    print(f"full-mix csnet: worst gradient error {eh:.2e} of its magnitude at {k} (fp32 CPU oracle there: {ec:.2e})")
    # decoder-site stitch gradients are analytically ~0 here (a train-mode BatchNorm follows the conv): the encoder
    # site is where the off-diagonal entries must show
    off = hip[ENC_SITE]
    mag = float(g64[ENC_SITE].abs().max())
    assert float(off[0, 1].abs().max()) > 1e-2 * mag and float(off[1, 0].abs().max()) > 1e-2 * mag


@LAYOUTS
def test_eval_forward_matches_patched_oracle(dev, full_oracle, channel_wise):
    sd0, _, _, _, sd_after = _step_reference(full_oracle, channel_wise)
    batch = _batch(seed=12)
    with torch.no_grad():
        ref = full_oracle({k: v.clone() for k, v in sd_after.items()}, batch["img"].double(), ["depth", "segm"], False)
    model = _build(channel_wise)
    model.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in sd_after.items()})
    model = model.to(dev).eval()
    with torch.no_grad():
        out = model(batch["img"].to(dev))
    for t in ("depth", "segm"):
        assert_close(out[t].cpu(), ref[t], tol=1e-4, what=f"full-mix csnet eval out {t}")
    after = model.state_dict()
    for k, v in sd_after.items():
        if "running" in k:
            assert torch.equal(after[k].cpu(), v.float()), f"eval moved {k}"
    # the diagnostics hook keeps working: same outputs, one record per task after every merge / up / decoder conv
    model.debug_acts = []
    with torch.no_grad():
        again = model(batch["img"].to(dev))
    recorded, model.debug_acts = model.debug_acts, None
    assert all(torch.equal(again[t], out[t]) for t in out)
    n_ops = sum(op in ("merge", "up", "conv_bn_relu") for op, _ in model._program)
    assert n_ops == 15 and len(recorded) == 2 * n_ops
    assert {r[2] for r in recorded} == {"depth", "segm"} and all(torch.isfinite(r[3]).all() for r in recorded)


@LAYOUTS
def test_arena_slots_side_stream_and_graph(dev, channel_wise):
    """as tests/test_arena_gpu.py; the used stitch parameters are written whole by the mix backward, so the whole
    gradient buffer is poisoned with NaN (but for the structurally-zero bias slots the arena keeps)"""
    from vision_mtl_amd import dp, ops
    from vision_mtl_amd.lit_module import MTLModule

    model = _build(channel_wise, seed=5).to(dev).train()
    module = MTLModule(model, num_classes=NC, device=str(dev))
    batch = {k: v.to(dev) for k, v in _batch(seed=3).items()}
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}

    def step():
        model.load_state_dict(sd0)  # same BatchNorm running buffers every time
        ops.packs.invalidate()
        loss = module.training_step(batch, 0)
        loss.backward()
        return loss.detach().clone()

    loss_ref = step()
    params = [p for p in model.parameters() if p.requires_grad]
    used = [p.grad is not None for p in params]  # encoder-block BatchNorm parameters never run in the leaf walk
    assert all(p.grad is not None for p in model.cross_stitch_layers.parameters())
    ref = [p.grad.clone() if u else torch.zeros_like(p) for p, u in zip(params, used)]
    for p in model.parameters():
        p.grad = None

    arena = dp.FlatArena(model)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    flat_ref = torch.cat([g.reshape(-1) for g in ref])
    live = torch.cat([torch.full((p.numel(),), u, dtype=torch.bool) for p, u in zip(params, used)]).to(dev)

    def same(flat):  # slots of parameters the step never touches keep whatever they held
        return torch.equal(flat[live], flat_ref[live])
    was = ops.side.enabled
    try:
        for enabled in (False, True):
            ops.side.enabled = enabled
            arena.flat_grad.fill_(float("nan"))  # every live slot must be overwritten, not accumulated into
            arena.slots_clobbered()  # written behind the arena's back: structurally-zero slots get re-zeroed
            loss = step()
            torch.cuda.synchronize()
            assert ops.side.pending is None
            assert torch.equal(loss, loss_ref)
            assert same(arena.flat_grad), f"side stream {enabled}: slot gradients differ"
        ops.side.enabled = True
        step()  # warm: packed-operand table, side stream exist before capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss = step()
        for _ in range(2):
            arena.flat_grad.fill_(float("nan"))
            for p in arena.params:  # slots the arena KNOWS to be zero are not rewritten by the captured step
                if id(p) in arena._zero_bias:
                    p._vmtl_gslot.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_loss, loss_ref)
            assert same(arena.flat_grad), "hipGraph replay: slot gradients differ"
        assert ops.side.pending is None
    finally:
        ops.side.enabled = was


@LAYOUTS
def test_graphed_step_matches_eager_on_changing_batches(dev, channel_wise):
    from vision_mtl_amd import dp, ops
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.lit_module import MTLModule

    batches = [_batch(seed=100 + i) for i in range(2)]
    sd0 = {k: v.clone() for k, v in _build(channel_wise).state_dict().items()}

    def run(graphed):
        model = _build(channel_wise).to(dev).train()
        module = MTLModule(model, num_classes=NC, device=str(dev))
        arena = dp.FlatArena(model)
        opt = dp.ArenaAdam(arena, lr=1e-3)  # the fused Adam launch over the flat buffers
        if graphed:
            gstep = GraphedStep(module, _batch(seed=99), arena=arena)
        model.load_state_dict(sd0)  # undo the BatchNorm-buffer drift of the warm-up / rehearsal steps
        ops.packs.invalidate()
        losses = []
        for b in batches:
            opt.zero_grad()
            if graphed:
                loss = gstep(b)
            else:
                arena.rebind_grads()
                loss = module.training_step({k: v.to(dev) for k, v in b.items()}, 0)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    le, sde = run(False)
    lg, sdg = run(True)
    assert le[1] != le[0]
    for k, (a, b) in enumerate(zip(lg, le)):
        assert abs(a - b) <= 1e-5 * abs(b), f"step {k}: replayed loss {a} vs eager {b}"
    for k in sde:
        if sde[k].is_floating_point():
            err, mag = float((sdg[k].double() - sde[k].double()).abs().max()), float(sde[k].double().abs().max())
            assert err <= 1e-5 * mag + 1e-8, f"{k}: {err:.3e} vs magnitude {mag:.3e}"
    stitch = [k for k in sde if k.startswith("cross_stitch_layers.")]
    assert any(not torch.equal(sde[k][0, 1], sd0[k][0, 1]) for k in stitch), "the off-diagonal stitch weights did not train"


@LAYOUTS
def test_graphed_eval_matches_eager_eval(dev, channel_wise):
    from vision_mtl_amd.graphed import GraphedEval
    from vision_mtl_amd.lit_module import MTLModule

    model = _build(channel_wise).to(dev).eval()
    module = MTLModule(model, num_classes=NC, device=str(dev))
    module.eval()
    batches = [{"img": _batch(seed=200 + i)["img"]} for i in range(2)]
    gpred = GraphedEval(module, {"img": _batch(seed=7)["img"]}, stage="predict")
    got = [gpred(b) for b in batches]
    with torch.no_grad():
        ref = [module.predict_step({"img": b["img"].to(dev)}) for b in batches]
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a["segm"], b["segm"]), f"batch {k}: segm"
        assert torch.equal(a["depth"], b["depth"]), f"batch {k}: depth"
    assert not torch.equal(got[0]["depth"], got[1]["depth"])
