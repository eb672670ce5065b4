"""dp.FlatArena.grad_norm / clip_grad_norm_ / the extended adam_step and dp.ArenaAdam / ArenaAdamW on the tiny MTAN model
test_host_cpu.py uses (MTANMiniUnet(3, {"depth": 1, "segm": 3}, 8, 4, 2), batch 2 at 16x16).

Checker where a reference exists: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in fp64 on the CPU over double copies
of the flat buffers, at the kernel tolerance of tests/test_optim_kernels_gpu.py (1e-6, max-abs error over the reference's
max magnitude).  Replay against eager (GraphedStep) is held to the bar test_train_loop_gpu.py holds the same comparison to
(1e-5 per tensor): the optimizer is the same code on both sides and adds nothing to it."""
import pytest
import torch

from tests import poison
from tests.util import assert_close

pytestmark = pytest.mark.gpu

TOL = 1e-6
LR = 2e-3
C, B, H, W = 3, 2, 16, 16


def _model(dev, seed=1):
    from vision_mtl_amd.models.mtan_model import MTANMiniUnet

    torch.manual_seed(seed)
    return MTANMiniUnet(3, {"depth": 1, "segm": 3}, 8, 4, 2).to(dev).train()


def _batches(n, first=300):
    from vision_mtl_amd.data import synthetic_batch

    return [synthetic_batch(B, H, W, C, seed=first + i, masked=0.1) for i in range(n)]


def _setup(dev):
    from vision_mtl_amd import dp
    from vision_mtl_amd.lit_module import MTLModule

    model = _model(dev)
    module = MTLModule(model, num_classes=C, device=str(dev))
    return model, module, dp.FlatArena(model)


def _backward(module, arena, batch, dev):
    arena.rebind_grads()
    loss = module.training_step({k: v.to(dev) for k, v in batch.items()}, 0)
    loss.backward()
    return loss.detach()


_NORM0 = []


def _half_first_norm(dev):
    """Half the gradient norm of the first training step: a bound that clips."""
    if not _NORM0:
        _, module, arena = _setup(dev)
        _backward(module, arena, _batches(1)[0], dev)
        n = float(arena.grad_norm())
        assert n > 0 and abs(n - float(arena.flat_grad.double().norm())) <= 1e-6 * n
        _NORM0.append(0.5 * n)
    return _NORM0[0]


def _fp64_steps(p0, grads, lrs, max_norm, gscale=1.0, decoupled=False, wd=0.0):
    p = p0.detach().double().cpu().clone().requires_grad_(True)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], lr=lrs[0], weight_decay=wd)
    norms = []
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = g.double().cpu() * gscale
        norms.append(float(torch.nn.utils.clip_grad_norm_([p], max_norm)))
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], norms


# ----------------------------------------------------------------------------- loop parity
@pytest.mark.parametrize("adamw", [False, True])
def test_fused_clip_matches_clip_then_torch_optimizer(dev, adamw):
    """4 training steps: ArenaAdam(max_grad_norm=c) against arena.clip_grad_norm_(c) + torch.optim.Adam over the views
    (ArenaAdamW against torch.optim.AdamW).  Both run the same HIP backward."""
    from vision_mtl_amd import dp, ops

    c = _half_first_norm(dev)
    batches = _batches(4)
    wd = 0.1 if adamw else 0.0

    def run(fused):
        model, module, arena = _setup(dev)
        if fused:
            opt = (dp.ArenaAdamW if adamw else dp.ArenaAdam)(arena, lr=LR, weight_decay=wd, max_grad_norm=c)
        else:
            opt = (torch.optim.AdamW if adamw else torch.optim.Adam)(module.parameters(), lr=LR, weight_decay=wd)
        norms = []
        with poison.patched("guard"):
            for b in batches:
                _backward(module, arena, b, dev)
                if fused:
                    opt.step()
                    norms.append(float(opt.grad_norm))
                else:
                    norms.append(float(arena.clip_grad_norm_(c)))
                    opt.step()
                    ops.packs.invalidate()
        return arena.flat_param.detach().cpu().clone(), norms

    pf, nf = run(True)
    pt, nt = run(False)
    assert all(n > c for n in nf) and all(n > c for n in nt), (c, nf, nt)  # every step clips
    assert nf[0] == nt[0]  # the same gradient, the same deterministic norm
    err = float((pf.double() - pt.double()).abs().max() / pt.double().abs().max())
    print(f"adamw={adamw}: fused vs clip-then-torch, max-abs error over max magnitude {err:.2e}; norms {nf}")
    assert_close(pf, pt, tol=TOL, what="parameters after 4 clipped steps")


# ----------------------------------------------------------------------------- pending_scale
def test_pending_scale_is_part_of_the_clipped_gradient(dev):
    """What gloo leaves behind: flat_grad holds the SUM over ranks and pending_scale the factor still owed."""
    from vision_mtl_amd import dp

    gen = torch.Generator().manual_seed(7)
    for via_clip in (False, True):
        model, module, arena = _setup(dev)
        p0 = arena.flat_param.detach().clone()
        g = torch.randn(arena.numel, generator=gen)
        max_norm = 0.25 * float(g.double().norm())  # the averaged gradient 0.5 * g has twice this norm
        pr, mr, vr, norms = _fp64_steps(p0, [g], [LR], max_norm, gscale=0.5)
        arena.flat_grad.copy_(g)
        arena.pending_scale = 0.5
        if via_clip:
            opt = dp.ArenaAdam(arena, lr=LR)
            norm = arena.clip_grad_norm_(max_norm).clone()
            assert arena.pending_scale == 1.0
            coef = min(1.0, max_norm / (norms[0] + 1e-6))
            assert_close(arena.flat_grad.cpu(), 0.5 * g.double() * coef, tol=TOL, what="the clipped averaged gradient")
            opt.step()  # plain path: must not apply the factor again
        else:
            opt = dp.ArenaAdam(arena, lr=LR, max_grad_norm=max_norm)
            opt.step()
            norm = opt.grad_norm
        assert arena.pending_scale == 1.0
        assert abs(float(norm) - norms[0]) <= 1e-6 * norms[0]
        assert_close(arena._adam["m"].cpu(), mr, tol=TOL, what=f"via_clip={via_clip} m")
        # via_clip: the update is the parent's vmtl_adam_step, which takes 1 - b2 from the fp32 0.999: half an ulp of
        # 0.999 (2^-25) over 0.001 = 3e-5 of every second-moment increment, by the number format alone (the extended
        # update gets the betas as float pairs).  A factor applied twice would be off by 75 %.
        assert_close(arena._adam["v"].cpu(), vr, tol=TOL + (2.0 ** -25 / 1e-3 if via_clip else 0.0),
                     what=f"via_clip={via_clip} v")
        assert_close(arena.flat_param.detach().cpu(), pr, tol=TOL, what=f"via_clip={via_clip} p")
        assert float(arena._adam["step"]) == 1.0


# ----------------------------------------------------------------------------- capture
def test_captured_step_follows_the_scheduler(dev):
    """opt.step() with capturable=True captured alone: the replays read lr and the step counter from the device."""
    from vision_mtl_amd import dp, ops

    model, module, arena = _setup(dev)
    gen = torch.Generator().manual_seed(9)
    grads = [torch.randn(arena.numel, generator=gen) * s for s in (1.0, 3.0, 0.5, 2.0)]
    max_norm = 0.5 * float(grads[0].double().norm())
    p0 = arena.flat_param.detach().clone()
    opt = dp.ArenaAdam(arena, lr=LR, max_grad_norm=max_norm, capturable=True)
    lr_t = opt.param_groups[0]["lr"]
    assert isinstance(lr_t, torch.Tensor) and lr_t.is_cuda and lr_t.dim() == 0
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=0, factor=0.5)
    arena.flat_grad.copy_(grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()  # uncaptured warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    lrs = [float(lr_t)]
    for k in (1, 2, 3):
        arena.flat_grad.copy_(grads[k])
        if k == 2:
            sched.step(1.0)
        if k == 3:
            sched.step(2.0)  # worse, patience 0: the rate halves, in place
        lrs.append(float(lr_t))
        graph.replay()
        ops.packs.invalidate()  # host-side bookkeeping a replay does not repeat (ArenaAdam's docstring)
    torch.cuda.synchronize()
    assert opt.param_groups[0]["lr"] is lr_t and lrs[3] == pytest.approx(0.5 * LR, rel=1e-6) and lrs[2] == lrs[0]
    assert float(arena._adam["step"]) == 4.0 and float(opt.skipped_steps) == 0.0
    pr, mr, vr, norms = _fp64_steps(p0, grads, lrs, max_norm)
    assert abs(float(opt.grad_norm) - norms[-1]) <= 1e-6 * norms[-1]
    assert_close(arena._adam["m"].cpu(), mr, tol=TOL, what="m")
    assert_close(arena._adam["v"].cpu(), vr, tol=TOL, what="v")
    assert_close(arena.flat_param.detach().cpu(), pr, tol=TOL, what="p")
    # the rate of step 4 matters: the same steps at a constant rate land elsewhere
    pc, _, _, _ = _fp64_steps(p0, grads, [LR] * 4, max_norm)
    assert float((pc - pr).abs().max()) > 100 * TOL * float(pr.abs().max())
    assert isinstance(opt.state_dict()["param_groups"][0]["lr"], float)


# ----------------------------------------------------------------------------- GraphedStep + ArenaAdam(max_grad_norm)
def test_graphed_step_with_clipping_optimizer_matches_eager(dev):
    from vision_mtl_amd import dp
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep

    c = _half_first_norm(dev)
    batches = _batches(3, first=400)
    sd0 = {k: v.detach().clone() for k, v in _model(dev).state_dict().items()}

    def run(graphed):
        model, module, arena = _setup(dev)
        opt = dp.ArenaAdam(arena, lr=LR, max_grad_norm=c)
        if graphed:
            gstep = GraphedStep(module, synthetic_batch(B, H, W, C, seed=399), arena=arena)
        model.load_state_dict(sd0)  # undo the BatchNorm-buffer drift of the warm-up / rehearsal steps
        norms = []
        for b in batches:
            opt.zero_grad()
            if graphed:
                gstep(b).backward()
            else:
                _backward(module, arena, b, dev)
            opt.step()
            norms.append(float(opt.grad_norm))
        return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, norms

    sde, ne = run(False)
    sdg, ng = run(True)
    assert all(n > c for n in ne), (c, ne)
    for a, b in zip(ng, ne):
        assert abs(a - b) <= 1e-5 * b
    for k in sde:
        if sde[k].is_floating_point():
            err, ref = float((sdg[k].double() - sde[k].double()).abs().max()), float(sde[k].double().abs().max())
            assert err <= 1e-5 * ref + 1e-8, f"{k}: {err:.3e} vs magnitude {ref:.3e}"
    assert any(not torch.equal(sde[k], sd0[k].cpu()) for k in sde)
