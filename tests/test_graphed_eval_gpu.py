"""-m gpu: forward-only captured steps (vision_mtl_amd.graphed.GraphedEval) and the batched eval-mode BatchNorm statistics
(vmtl_bn_eval_stats_batch through ops.eval_bn_table).  Replays are compared BITWISE with the eager steps: the graph runs
the same kernels on the same inputs in the same order, and every forward kernel here is deterministic (the per-channel
reductions are two-stage with a fixed merge order; the metrics count integers)."""
import argparse
import gc
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 19
B, H, W = 2, 64, 64
MODELS = [("basic", None), ("csnet", True), ("csnet", False), ("mtan", None)]


@pytest.fixture(autouse=True)
def _collect_models():
    """A FlatArena and its parameters reference each other: collect the models of a test when it ends, so that no later
    test finds their packed-operand entries still alive (ops.packs re-packs every live model's weights each step)."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _module(dev, name, cw=None, seed=0):
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.utils.pipeline_utils import build_model

    torch.manual_seed(seed)
    ns = argparse.Namespace(model_name=name, backbone_weights=None)
    if cw is not None:
        ns.channel_wise_stitching = cw
    model = build_model(ns, argparse.Namespace(num_classes=C))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # running buffers / affine parameters away from their init values: eval mode then matters
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(0.2 * torch.randn(n, generator=g))
                m.running_var.copy_(0.5 + torch.rand(n, generator=g))
                m.weight.copy_(1.0 + 0.1 * torch.randn(n, generator=g))
                m.bias.copy_(0.1 * torch.randn(n, generator=g))
    return MTLModule(model.to(dev), num_classes=C, device=str(dev))


def _batches(n, seed=100, targets=True):
    from vision_mtl_amd.data import synthetic_batch

    out = [synthetic_batch(B, H, W, C, seed=seed + i, masked=0.1) for i in range(n)]
    return out if targets else [{"img": b["img"]} for b in out]


def _dev(b, dev):
    return {k: v.to(dev) for k, v in b.items()}


def _so(module, stage, start):
    return {k: [v.clone() for v in vals[start:]] for k, vals in module.step_outputs[stage].items()}


def _assert_so_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert len(a[k]) == len(b[k]), k
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x.float(), y.float()) or (x.isnan().all() and y.isnan().all()), (k, x, y)


def _bn_state(model):
    return {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}


# ---- 1. kernel
def test_batched_eval_stats_bitwise_equal_to_per_layer_kernels(dev):
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib

    g = torch.Generator().manual_seed(5)
    Cs_all = [1, 3, 16, 19, 67, 960]
    size = lib().raw("vmtl_bn_eval_desc_bytes")()
    SENT, TAIL = -7.0, 8
    recs, ref, got, keep = [], [], [], []
    for i in range(40):
        Cn = Cs_all[i % len(Cs_all)]
        Cs = ops.ceil4(Cn) + 4 * int(torch.randint(0, 3, (1,), generator=g))
        rm = torch.randn(Cn, generator=g).to(dev)
        rv = (0.01 + torch.rand(Cn, generator=g)).to(dev)
        gamma = torch.randn(Cn, generator=g).to(dev) if i % 3 else None
        beta = torch.randn(Cn, generator=g).to(dev) if i % 4 else None
        coef = i % 2 == 0
        outs = [torch.full((4, Cs + TAIL), SENT, device=dev) for _ in range(2)]
        keep += [rm, rv, gamma, beta]  # the table holds raw addresses: keep the inputs alive until the launch
        ptr = lambda t: 0 if t is None else t.data_ptr()
        o = outs[1]
        recs.append(struct.pack(ops._EvalBNTable.DESC, rm.data_ptr(), rv.data_ptr(), ptr(gamma), ptr(beta),
                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr() if coef else 0,
                                o[3].data_ptr() if coef else 0, Cn, Cs, 1e-5, 0).ljust(size, b"\0"))
        r = outs[0]
        if coef:
            ops._k("vmtl_bn_eval_stats_coef", running_mean=rm, running_var=rv, C=Cn, Cs=Cs, eps=1e-5, save_mean=r[0],
                   save_invstd=r[1], gamma=gamma, beta=beta, coef_a=r[2], coef_c=r[3])
        else:
            ops._k("vmtl_bn_eval_stats", running_mean=rm, running_var=rv, C=Cn, Cs=Cs, eps=1e-5, save_mean=r[0],
                   save_invstd=r[1])
        ref.append(r)
        got.append(o)
    descs = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(dev)
    ops._k("vmtl_bn_eval_stats_batch", descs=descs, n=len(recs), max_cs=max(o.shape[1] - TAIL for o in got))
    torch.cuda.synchronize()
    for i, (r, o) in enumerate(zip(ref, got)):
        assert torch.equal(r, o), f"entry {i}"
        assert bool((o[:, -TAIL:] == SENT).all()), f"entry {i}: wrote past Cs"
        Cs = o.shape[1] - TAIL
        Cn = Cs_all[i % len(Cs_all)]
        assert bool((o[:2, Cn:Cs] == 0).all())


# ---- 2. predict parity
@pytest.mark.parametrize("name,cw", MODELS)
@pytest.mark.parametrize("targets", [True, False])
def test_predict_replay_bitwise_equal_to_eager(dev, name, cw, targets):
    from vision_mtl_amd.graphed import GraphedEval

    module = _module(dev, name, cw)
    module.eval()
    batches = _batches(3, targets=targets)
    geval = GraphedEval(module, _batches(1, seed=7, targets=targets)[0], stage="predict")
    assert geval._table is not None
    start = len(module.step_outputs["predict"]["loss"])
    got = [geval(b) for b in batches]
    so_g = _so(module, "predict", start)
    start = len(module.step_outputs["predict"]["loss"])
    with torch.no_grad():
        ref = [module.predict_step(_dev(b, dev)) for b in batches]
    so_e = _so(module, "predict", start)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a["segm"], b["segm"]), f"batch {k}: segm"
        assert torch.equal(a["depth"], b["depth"]), f"batch {k}: depth"
    assert not torch.equal(got[0]["depth"], got[1]["depth"])
    _assert_so_equal(so_g, so_e)
    assert len(so_g["loss"]) == (3 if targets else 0)


# ---- 3. validation parity (train mode under no_grad: batch statistics, running buffers move)
@pytest.mark.parametrize("name,cw", [("basic", None), ("csnet", True), ("mtan", None)])
def test_validation_replay_bitwise_equal_to_eager(dev, name, cw):
    from vision_mtl_amd.graphed import GraphedEval

    batches = _batches(3)
    me, mg = _module(dev, name, cw), _module(dev, name, cw)
    me.train(), mg.train()
    geval = GraphedEval(mg, _batches(1, seed=7)[0], stage="val")
    lg = [geval(b) for b in batches]
    with torch.no_grad():
        le = [me.validation_step(_dev(b, dev)) for b in batches]
    for k, (a, b) in enumerate(zip(lg, le)):
        assert torch.equal(a, b), f"batch {k}: loss {float(a)} vs {float(b)}"
    _assert_so_equal(_so(mg, "val", 0), _so(me, "val", 0))
    se, sg = _bn_state(me.model), _bn_state(mg.model)
    for k in se:
        assert torch.equal(sg[k], se[k]), k


# ---- 4. no side effects
@pytest.mark.parametrize("stage,train", [("val", True), ("predict", False)])
def test_construction_and_replay_have_no_side_effects(dev, stage, train):
    from vision_mtl_amd import dp
    from vision_mtl_amd.graphed import GraphedEval

    module = _module(dev, "basic")
    module.train(train)
    arena = dp.FlatArena(module.model)
    arena.flat_grad.copy_(torch.randn(arena.flat_grad.numel(), generator=torch.Generator().manual_seed(3)))
    for k in module.step_outputs["val"]:
        module.step_outputs["val"][k].append(torch.tensor(1.5, device=dev))
    before_bn = _bn_state(module.model)
    before_so = {s: _so(module, s, 0) for s in module.step_outputs}
    before_grad = arena.flat_grad.clone()
    grads = [p.grad for p in module.parameters()]
    geval = GraphedEval(module, _batches(1, seed=7)[0], stage=stage)
    torch.cuda.synchronize()
    after = _bn_state(module.model)
    for k in before_bn:
        assert torch.equal(after[k], before_bn[k]), k
    for s in before_so:
        _assert_so_equal(_so(module, s, 0), before_so[s])
    assert torch.equal(arena.flat_grad, before_grad)
    assert all(a is b for a, b in zip(grads, [p.grad for p in module.parameters()]))
    geval(_batches(1)[0])
    torch.cuda.synchronize()
    assert torch.equal(arena.flat_grad, before_grad)


# ---- 5. interleaved with training
def test_eval_replay_sees_weights_after_optimizer_steps(dev):
    from vision_mtl_amd import dp
    from vision_mtl_amd.graphed import GraphedEval, GraphedStep

    module = _module(dev, "basic")
    arena = dp.FlatArena(module.model)
    opt = dp.ArenaAdam(arena, lr=1e-3)
    module.train()
    gstep = GraphedStep(module, _batches(1, seed=7)[0], arena=arena)
    module.eval()
    gpred = GraphedEval(module, _batches(1, seed=8, targets=False)[0], stage="predict")
    train_b, pb = _batches(2, seed=200), _batches(1, seed=300, targets=False)[0]
    outs = []
    for tb in train_b:
        module.train()
        opt.zero_grad()
        gstep(tb).backward()
        opt.step()
        module.eval()
        out = gpred(pb)
        with torch.no_grad():
            ref = module.predict_step(_dev(pb, dev))
        assert torch.equal(out["segm"], ref["segm"]) and torch.equal(out["depth"], ref["depth"])
        outs.append(out["depth"])
    assert not torch.equal(outs[0], outs[1])  # same batch, new weights and running buffers


# ---- 6. one launch for every eval-mode BatchNorm
@pytest.mark.parametrize("name", ["basic", "mtan"])
def test_captured_predict_step_issues_one_eval_stats_launch(dev, name, monkeypatch):
    from vision_mtl_amd import ops
    from vision_mtl_amd.graphed import GraphedEval

    module = _module(dev, name)
    module.eval()
    example = _batches(1, seed=7, targets=False)[0]

    def count(bn_table):
        names = []
        orig = ops._k

        def rec(name, *a, **kw):
            if torch.cuda.is_current_stream_capturing():
                names.append(name)
            return orig(name, *a, **kw)

        monkeypatch.setattr(ops, "_k", rec)
        try:
            GraphedEval(module, example, stage="predict", bn_table=bn_table)
        finally:
            monkeypatch.setattr(ops, "_k", orig)
        return names

    with_t, without = count(True), count(False)
    per_layer = ("vmtl_bn_eval_stats", "vmtl_bn_eval_stats_coef")
    assert with_t.count("vmtl_bn_eval_stats_batch") == 1 and with_t[0] == "vmtl_bn_eval_stats_batch"
    assert sum(with_t.count(n) for n in per_layer) == 0
    assert without.count("vmtl_bn_eval_stats_batch") == 0
    nbn = sum(without.count(n) for n in per_layer)
    assert nbn > 1 and len(without) - len(with_t) == nbn - 1


# ---- 7. misuse
def test_misuse(dev):
    from vision_mtl_amd import ops
    from vision_mtl_amd._lib import lib
    from vision_mtl_amd.graphed import GraphedEval

    f = lib().raw("vmtl_bn_eval_stats_batch")
    s = torch.cuda.current_stream().cuda_stream
    table = torch.zeros(lib().raw("vmtl_bn_eval_desc_bytes")(), dtype=torch.uint8, device=dev)
    assert f(None, 1, 4, s) == -1
    assert f(table.data_ptr(), 0, 4, s) == -1
    assert f(table.data_ptr(), 1, 6, s) == -1

    module = _module(dev, "basic")
    module.eval()
    gpred = GraphedEval(module, _batches(1, seed=7, targets=False)[0], stage="predict")
    from vision_mtl_amd.data import synthetic_batch

    with pytest.raises(ValueError, match="shape"):
        gpred({"img": synthetic_batch(B + 1, H, W, C)["img"]})
    module.train()
    with pytest.raises(ValueError, match="training"):
        gpred(_batches(1, targets=False)[0])
    module.eval()
    b1, b2 = _batches(2, targets=False)
    o1 = gpred(b1)
    keep = {k: v.clone() for k, v in o1.items()}
    o2 = gpred(b2)
    assert torch.equal(o1["segm"], keep["segm"]) and torch.equal(o1["depth"], keep["depth"])
    assert not torch.equal(o1["depth"], o2["depth"])
    with pytest.raises(ValueError, match="mask"):
        GraphedEval(module, _batches(1, targets=False)[0], stage="val")
    assert ops.eval_bn.active is None


# ---- 8. precision
def test_bf16_capture_keeps_its_precision(dev):
    from vision_mtl_amd.graphed import GraphedEval
    from vision_mtl_amd.precision import conv_precision

    module = _module(dev, "basic")
    module.eval()
    b1, b2 = _batches(2, targets=False)
    with conv_precision("bf16"):
        gpred = GraphedEval(module, _batches(1, seed=7, targets=False)[0], stage="predict")
        o1 = gpred(b1)
        with torch.no_grad():
            r1, r2 = module.predict_step(_dev(b1, dev)), module.predict_step(_dev(b2, dev))
    assert torch.equal(o1["depth"], r1["depth"]) and torch.equal(o1["segm"], r1["segm"])
    o2 = gpred(b2)  # replayed outside the context: still bf16
    assert torch.equal(o2["depth"], r2["depth"]) and torch.equal(o2["segm"], r2["segm"])
    assert gpred.conv_precision == "bf16"
