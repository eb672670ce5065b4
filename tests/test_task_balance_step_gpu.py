"""-m gpu: one training step with MTLModule(loss_balancing=...) against the existing fixed-weight step.

A balanced step must be the fixed-weight step run with loss_segm_weight / loss_depth_weight set to the fp32 values read
from task_balancer.weights: the balancing node hands each task loss the gradient grad_out * weights_k, which is what
vmtl_axpby's backward hands it, and everything downstream is the same code.

Yardstick: the fixed-weight step (the code this feature does not touch) run twice on the same inputs, in the same test.
For every parameter, |balanced - fixed| (2-norm over the parameter) may be at most the larger of the run-to-run
difference of that parameter between the two fixed runs and 1e-6 of the whole-gradient norm (fp32 keeps 6e-8; the
weight-gradient sums of the step are not order-fixed, so some run-to-run noise is expected).  The loss uses the same rule
with 1e-6 of the loss.  For "uncertainty" the gradient of log_vars is compared, under the same bound, with
1 - w_k L_k evaluated in fp64 from the step's own per-task losses (captured at calc_losses)."""
import argparse
import gc
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
LOG_VARS = (0.8, -0.2)
DWA_W = (1.3, 0.7)
CASES = [("mtan", "uncertainty"), ("mtan", "dwa"), ("mtan", "geometric"), ("basic", "uncertainty"),
         ("csnet", "uncertainty")]


@pytest.fixture(autouse=True)
def _collect_models():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _setup(name):
    """(model factory, C, batch); every call of the factory gives the same weights"""
    from vision_mtl_amd.data import synthetic_batch

    if name == "mtan":
        from vision_mtl_amd.models.mtan_model import MTANMiniUnet

        fx = torch.load(os.path.join(G, "mtan_tiny.pt"), weights_only=False)
        C, cfg = fx["cfg"]["C"], fx["cfg"]

        def make():
            m = MTANMiniUnet(3, dict(fx["tasks"]), cfg["hidden"], cfg["first"], cfg["levels"])
            m.load_state_dict(fx["state_dict"])
            return m
        return make, C, fx["batch"]
    from vision_mtl_amd.utils.pipeline_utils import build_model

    # basic: the smallest shape tests/test_basic_gpu.py steps; csnet: 2x64x64, its two task streams meet at the loss node
    C, shape = 19, {"basic": (3, 64, 96), "csnet": (2, 64, 64)}[name]
    sd = {}

    def make():
        torch.manual_seed(11)
        m = build_model(argparse.Namespace(model_name=name, backbone_weights=None), argparse.Namespace(num_classes=C))
        if not sd:
            sd.update({k: v.clone() for k, v in m.state_dict().items()})
        m.load_state_dict(sd)
        return m
    return make, C, synthetic_batch(*shape, C, seed=11, masked=0.1)


def _step(module, batch, dev, with_arena):
    """one eager training step; (loss, {name: gradient}, per-task losses, the module's arena)"""
    from vision_mtl_amd import dp

    arena = None
    if with_arena:
        balancer = getattr(module, "task_balancer", None)
        arena = dp.FlatArena(module.model, extra_params=None if balancer is None else list(balancer.parameters()))
        module.dp_arena = arena
    seen, orig = {}, module.calc_losses

    def calc(gt_mask, gt_depth, out):
        r = orig(gt_mask, gt_depth, out)
        seen.update(r)
        return r

    module.calc_losses = calc
    loss = module.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
    loss.backward()
    torch.cuda.synchronize()
    names = [n for n, _ in module.model.named_parameters()] + ["log_vars"]
    grads = {n: p.grad.detach().double().cpu().clone() for n, p in zip(names, module.parameters()) if p.grad is not None}
    return float(loss.detach().double()), grads, {k: float(v.detach().double()) for k, v in seen.items()}, arena


def _norm(d):
    return float(torch.sqrt(sum((v ** 2).sum() for v in d.values())))


@pytest.mark.parametrize("with_arena", [False, True], ids=["plain", "arena"])
@pytest.mark.parametrize("name,method", CASES)
def test_balanced_step_is_the_fixed_weight_step(dev, name, method, with_arena):
    from vision_mtl_amd.balancing import TaskBalancer
    from vision_mtl_amd.lit_module import MTLModule

    make, C, batch = _setup(name)
    balancer = TaskBalancer(method, init_log_vars=LOG_VARS if method == "uncertainty" else None)
    module = MTLModule(make().to(dev).train(), num_classes=C, device=str(dev), loss_balancing=balancer)
    if method == "dwa":
        with torch.no_grad():
            module.task_balancer.dwa_weights.copy_(torch.tensor(DWA_W))
    loss_b, g_b, per_task, arena = _step(module, batch, dev, with_arena)
    w = module.task_balancer.weights
    assert w.is_cuda and w.shape == (2,) and w.dtype == torch.float32
    w = [float(x) for x in w.cpu()]  # the fp32 values, exactly
    if method == "dwa":
        assert w == [float(torch.tensor(x)) for x in DWA_W]
        assert module.task_balancer.dwa_state.tolist()[:3] == [float(torch.tensor(per_task["loss_segm"]).double()),
                                                               float(torch.tensor(per_task["loss_depth"]).double()), 1.0]
    if with_arena and method == "uncertainty":
        s = module.task_balancer.log_vars
        assert s._vmtl_arena is arena and s.grad.data_ptr() == arena.flat_grad.data_ptr() + 4 * arena.offsets[-1]

    fixed = []
    for _ in range(2):  # the yardstick: the parent's step, twice
        m = MTLModule(make().to(dev).train(), num_classes=C, device=str(dev), loss_segm_weight=w[0],
                      loss_depth_weight=w[1])
        fixed.append(_step(m, batch, dev, with_arena))
    (loss_f, g_f, _, _), (loss_f2, g_f2, _, _) = fixed
    offset = sum(LOG_VARS) if method == "uncertainty" else 0.0  # sum_k s_k: the one term the fixed-weight loss lacks
    bound = max(abs(loss_f - loss_f2), 1e-6 * abs(loss_f + offset))
    print(f"{name}/{method}: loss {loss_b!r} vs fixed {loss_f + offset!r} (second run {loss_f2 + offset!r}), weights {w}")
    assert abs(loss_b - (loss_f + offset)) <= bound

    whole = _norm(g_f)
    worst = 0.0
    assert set(g_f) == set(g_b) - {"log_vars"} and whole > 0
    for k in g_f:
        err, noise = float((g_b[k] - g_f[k]).norm()), float((g_f[k] - g_f2[k]).norm())
        worst = max(worst, err / max(noise, 1e-6 * whole))
        assert err <= max(noise, 1e-6 * whole), f"{k}: |balanced - fixed| {err:.3e}, run to run {noise:.3e}, whole {whole:.3e}"
    print(f"{name}/{method}: whole-gradient norm {whole:.6g}, run-to-run {_norm({k: g_f[k] - g_f2[k] for k in g_f}):.3e}, "
          f"balanced vs fixed {_norm({k: g_b[k] - g_f[k] for k in g_f}):.3e}, worst ratio to its bound {worst:.3f}")
    if method == "uncertainty":
        ref = torch.tensor([1.0 - w[0] * per_task["loss_segm"], 1.0 - w[1] * per_task["loss_depth"]], dtype=torch.float64)
        err = float((g_b["log_vars"] - ref).norm())
        print(f"{name}/{method}: d log_vars {g_b['log_vars'].tolist()} vs {ref.tolist()}")
        assert err <= 1e-6 * whole, f"log_vars gradient off by {err:.3e} (whole-gradient norm {whole:.3e})"
    else:
        assert "log_vars" not in g_b
