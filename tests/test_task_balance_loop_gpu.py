"""-m gpu: the reference's train iteration (training_lit.py:82-87) for 4 steps with learned / dynamic task weights, on
tests/golden/mtan_tiny.pt.  Checker: the CPU oracle (oracle/mtan.py + oracle/losses.py, pinned to the reference) with the
balancing formulas written out in torch and driven by torch.optim.Adam, as tests/test_train_loop_gpu.py does it.

"uncertainty": init_log_vars = (0.8, -0.2), so the two log-variances move in opposite directions (the oracle ends near
(0.792, -0.192)).  They only follow the oracle when their gradient reaches the optimizer: through module.parameters(),
through the arena slot and the fused ArenaAdam update, and - replayed - through the pointer the captured kernels read.
Bar on log_vars: 2e-5 absolute = 4 steps x lr 2e-3 x the relative gradient error the 2e-4 loss bar implies (at most
6e-4) = 4.8e-6, with a fourfold margin.
"dwa": temperature 0.1 and one-step epochs, so steps 3 and 4 run with weights near 1 +- 0.04 - far outside the loss bar
if the epoch update or the replayed graph missed them.
Bars on the losses: 2e-4 relative against the oracle and 1e-5 replayed against eager, those of test_train_loop_gpu.py.
The fp32 and fp64 oracles stay within 1e-4 of each other over these 4 steps for both loops (checked on the CPU), so the
inputs themselves sit inside the bar."""
import copy
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
STEPS, LR = 4, 2e-3
LOG_VARS = (0.8, -0.2)
TAU = 0.1
_ORACLE = {}


def _fx():
    return torch.load(os.path.join(G, "mtan_tiny.pt"), weights_only=False)


def _oracle(method):
    """(losses per step, final log_vars | DWA weights per step); computed once per method and left unchanged"""
    if method in _ORACLE:
        return _ORACLE[method]
    from oracle.losses import step_losses
    from oracle.mtan import mtan_forward

    fx = _fx()
    batch = fx["batch"]
    sd = {k: v.clone() for k, v in fx["state_dict"].items()}
    leaves = [v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k]
    s = torch.tensor(LOG_VARS, requires_grad=True)
    opt = torch.optim.Adam(leaves + ([s] if method == "uncertainty" else []), lr=LR)
    w, means, losses, ws = [1.0, 1.0], [], [], []
    for _ in range(STEPS):
        raw = mtan_forward(sd, batch["img"], list(dict(fx["tasks"])), fx["cfg"]["levels"], training=True)
        r = step_losses(raw, batch["mask"], batch["depth"])
        L = [r["loss_segm"], r["loss_depth"]]
        if method == "uncertainty":
            loss = sum(torch.exp(-s[k]) * L[k] + s[k] for k in range(2))
        else:
            ws.append(list(w))
            loss = w[0] * L[0] + w[1] * L[1]
            means.append([float(x.detach().double()) for x in L])  # one-step epochs: the epoch mean is the step's loss
            if len(means) >= 2:  # Liu et al. 2019, eq. 7, T = 2
                e = [math.exp(a / b / TAU) for a, b in zip(means[-1], means[-2])]
                w = [2 * x / sum(e) for x in e]
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    _ORACLE[method] = (losses, s.detach().tolist() if method == "uncertainty" else ws)
    return _ORACLE[method]


def _module(fx, dev, method):
    from vision_mtl_amd.balancing import TaskBalancer
    from vision_mtl_amd.lit_module import MTLModule
    from vision_mtl_amd.models.mtan_model import MTANMiniUnet

    c = fx["cfg"]
    m = MTANMiniUnet(3, dict(fx["tasks"]), c["hidden"], c["first"], c["levels"])
    m.load_state_dict(fx["state_dict"])
    balancer = TaskBalancer(method, init_log_vars=LOG_VARS if method == "uncertainty" else None, temperature=TAU)
    return MTLModule(m.to(dev).train(), num_classes=c["C"], device=str(dev), loss_balancing=balancer)


def _arena(module):
    from vision_mtl_amd import dp

    arena = dp.FlatArena(module.model, extra_params=list(module.task_balancer.parameters()))
    module.dp_arena = arena
    return arena


def _eager_step(module, opt, batch):
    opt.zero_grad()
    if module.dp_arena is not None:
        module.dp_arena.rebind_grads()
    loss = module.training_step(batch, 0)
    loss.backward()
    opt.step()
    module.on_train_epoch_end()  # one-step epochs
    return float(loss.detach())


def _assert_losses(got, ref, bar, what):
    print(f"{what}: {got} vs {ref}")
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert abs(a - b) <= bar * abs(b), f"{what}: step {k} loss {a} vs {b}"


@pytest.mark.parametrize("mode", ["torch_adam", "arena_adam"])
def test_uncertainty_loop_matches_oracle(dev, mode):
    from vision_mtl_amd import dp

    fx = _fx()
    ref, s_ref = _oracle("uncertainty")
    assert ref[-1] < ref[0] and s_ref[0] < LOG_VARS[0] - 5e-3 and s_ref[1] > LOG_VARS[1] + 5e-3  # opposite directions
    module = _module(fx, dev, "uncertainty")
    batch = {k: v.to(dev) for k, v in fx["batch"].items()}
    if mode == "torch_adam":  # exactly run_pipe(): torch.optim.Adam over module.parameters()
        opt = torch.optim.Adam(module.parameters(), lr=LR)
    else:
        opt = dp.ArenaAdam(_arena(module), lr=LR)
        ref_sd = torch.optim.Adam(module.parameters(), lr=LR).state_dict()
        assert opt.state_dict()["param_groups"][0]["params"] == ref_sd["param_groups"][0]["params"]
    got = [_eager_step(module, opt, batch) for _ in range(STEPS)]
    _assert_losses(got, ref, 2e-4, f"uncertainty/{mode}")
    s = module.task_balancer.log_vars.detach().cpu().tolist()
    print(f"uncertainty/{mode}: log_vars {s} vs oracle {s_ref}")
    assert all(abs(a - b) <= 2e-5 for a, b in zip(s, s_ref))


def test_uncertainty_graphed_step_matches_eager_with_changing_batches(dev):
    from vision_mtl_amd import dp
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep

    fx = _fx()
    C = fx["cfg"]["C"]
    B, _, H, W = fx["batch"]["img"].shape
    batches = [synthetic_batch(B, H, W, C, seed=100 + i, masked=0.1) for i in range(STEPS)]
    example = synthetic_batch(B, H, W, C, seed=99)

    def run(graphed):
        module = _module(fx, dev, "uncertainty")
        if graphed:
            gstep = GraphedStep(module, example)  # the default arena takes the balancer's parameters in
            arena = gstep.arena
            assert arena.params[-1] is module.task_balancer.log_vars
            module.model.load_state_dict(fx["state_dict"])  # undo the BatchNorm-buffer drift of the warm-up steps
        else:
            arena = _arena(module)
        opt = dp.ArenaAdam(arena, lr=LR)
        losses, weights = [], []
        for b in batches:
            if graphed:
                opt.zero_grad()
                loss = gstep(b)
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
            else:
                losses.append(_eager_step(module, opt, {k: v.to(dev) for k, v in b.items()}))
            weights.append(module.task_balancer.weights.cpu().tolist())
        return losses, module.task_balancer.log_vars.detach().cpu().tolist(), weights

    le, se, we = run(False)
    lg, sg, wg = run(True)
    _assert_losses(lg, le, 1e-5, "uncertainty replayed vs eager")
    print(f"log_vars replayed {sg} vs eager {se}; weights per step {wg}")
    assert all(abs(a - b) <= 2e-5 for a, b in zip(sg, se))
    assert abs(se[0] - LOG_VARS[0]) > 5e-3 and abs(se[1] - LOG_VARS[1]) > 5e-3  # they trained
    # the replayed graph read the updated log-variances: its weights moved from step to step, as the eager ones did
    assert wg[0] != wg[-1]
    for a, b in zip(wg, we):
        assert all(abs(x - y) <= 1e-5 * abs(y) for x, y in zip(a, b))


def test_graphed_step_refuses_an_arena_without_the_balancer_parameters(dev):
    from vision_mtl_amd import dp
    from vision_mtl_amd.graphed import GraphedStep

    fx = _fx()
    module = _module(fx, dev, "uncertainty")
    with pytest.raises(ValueError, match="extra_params"):
        GraphedStep(module, fx["batch"], arena=dp.FlatArena(module.model))


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_dwa_loop_matches_oracle(dev, graphed):
    from vision_mtl_amd import dp
    from vision_mtl_amd.graphed import GraphedStep

    fx = _fx()
    ref, w_ref = _oracle("dwa")
    assert all(abs(w - 1.0) > 5e-3 for w in w_ref[2] + w_ref[3]) and w_ref[0] == w_ref[1] == [1.0, 1.0]
    module = _module(fx, dev, "dwa")
    bal = module.task_balancer
    batch = {k: v.to(dev) for k, v in fx["batch"].items()}
    got, ws = [], []
    if graphed:
        gstep = GraphedStep(module, fx["batch"])
        # construction ran warm-up and rehearsal steps with gradients enabled: the epoch's accumulators must not show it
        assert bal.dwa_state.tolist() == [0.0] * 8 and bal.dwa_weights.tolist() == [1.0, 1.0]
        module.model.load_state_dict(fx["state_dict"])
        opt = dp.ArenaAdam(gstep.arena, lr=LR)
        for _ in range(STEPS):
            opt.zero_grad()
            loss = gstep(fx["batch"])
            loss.backward()
            opt.step()
            ws.append(bal.weights.cpu().tolist())
            module.on_train_epoch_end()  # between replays: the next replay must use the new weights, no recapture
            got.append(float(loss.detach()))
    else:
        opt = dp.ArenaAdam(_arena(module), lr=LR)
        for _ in range(STEPS):
            got.append(_eager_step(module, opt, batch))
            ws.append(bal.weights.cpu().tolist())
    _assert_losses(got, ref, 2e-4, f"dwa/{'graphed' if graphed else 'eager'}")
    print(f"dwa weights per step {ws} vs oracle {w_ref}")
    for a, b in zip(ws, w_ref):
        assert all(abs(x - y) <= 2e-4 * abs(y) for x, y in zip(a, b))
    st = bal.dwa_state.tolist()
    assert st[:4] == [0.0, 0.0, 0.0, float(STEPS)]  # four completed one-step epochs, nothing pending


@pytest.mark.parametrize("method", ["uncertainty", "dwa"])
def test_checkpoint_round_trip_mid_run(dev, method):
    """module.state_dict() + the optimizer's after step 2, loaded into fresh objects: step 3 is the same step."""
    from vision_mtl_amd import dp

    fx = _fx()
    batch = {k: v.to(dev) for k, v in fx["batch"].items()}
    module = _module(fx, dev, method)
    opt = dp.ArenaAdam(_arena(module), lr=LR)
    for _ in range(2):
        _eager_step(module, opt, batch)
    ckpt = copy.deepcopy({"model": module.state_dict(), "optimizer": opt.state_dict()})
    key = "task_balancer.log_vars" if method == "uncertainty" else "task_balancer.dwa_weights"
    assert key in ckpt["model"] and (method != "dwa" or "task_balancer.dwa_state" in ckpt["model"])
    loss3 = _eager_step(module, opt, batch)

    fresh = _module(fx, dev, method)
    opt2 = dp.ArenaAdam(_arena(fresh), lr=123.0)
    fresh.load_state_dict(ckpt["model"])  # strict; copies in place, so the parameters stay views of the arena
    dp.ops.packs.invalidate()
    opt2.load_state_dict(ckpt["optimizer"])
    assert len(ckpt["optimizer"]["state"]) == len(list(fresh.parameters()))
    got3 = _eager_step(fresh, opt2, batch)
    print(f"{method}: step 3 loss {loss3} / after the round trip {got3}")
    assert abs(got3 - loss3) <= 1e-5 * abs(loss3)
    a, b = (module.task_balancer.state_dict(), fresh.task_balancer.state_dict())
    for k in a:
        assert float((a[k].double() - b[k].double()).abs().max()) <= 2e-5, k
    if method == "dwa":
        assert abs(float(ckpt["model"][key][0]) - 1.0) > 5e-3  # the checkpoint carried weights that had moved
