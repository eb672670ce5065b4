"""The task-balancing launches (vmtl_task_balance_fwd / _bwd, csrc/balance.hip) next to the launch they replace
(vmtl_axpby on two scalar losses, forward; its backward is two more vmtl_axpby launches when a weight is not 1), in the
same process, GPU box only.  All of them are launch-bound single-workgroup kernels: what is compared is the cost of one
launch issued eagerly, timed with HIP events over a warmed-up window of `reps` launches; the variants alternate window by
window, `rounds` windows each; reported are the median and the spread (min, max) in microseconds per call.

--step adds milliseconds per replayed training step of graphed.GraphedStep (`--model` at `--batch` x `--height` x
`--width`, metrics on) for the fixed-weight step and for each balancing method, one model alive at a time, the
fixed-weight step measured first and again last.  Prints ONE JSON line.

    python tools/bench_balance.py [--reps 200] [--rounds 7] [--step] [--out profiles/task_balance/bench_balance.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

METHODS = ("uncertainty", "dwa", "geometric")


def _window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def _ab(fns, reps, rounds):
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(_window(fn, reps))
    return out


def _summary(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def bench_kernels(dev, reps, rounds):
    from vision_mtl_amd import ops

    T = 2
    l0, l1 = torch.tensor(1.66, device=dev), torch.tensor(9.9, device=dev)
    param = torch.tensor([0.8, -0.2], device=dev)
    state = torch.zeros(ops.balance_state_doubles(T), dtype=torch.float64, device=dev)
    total, weights, go = torch.empty((), device=dev), torch.empty(T, device=dev), torch.ones((), device=dev)
    g0, g1, dparam = torch.empty((), device=dev), torch.empty((), device=dev), torch.empty(T, device=dev)
    y = torch.empty((), device=dev)

    def fwd(mode):
        code = ops.BALANCE_MODES[mode]
        return lambda: ops._k("vmtl_task_balance_fwd", l0=l0, l1=l1, l2=None, l3=None, T=T, mode=code, param=param,
                              state=state, accumulate=1 if mode == "dwa" else 0, total=total, weights=weights)

    def bwd(mode):
        code = ops.BALANCE_MODES[mode]
        return lambda: ops._k("vmtl_task_balance_bwd", grad_out=go, weights=weights, l0=l0, l1=l1, l2=None, l3=None,
                              param=param, mode=code, T=T, g0=g0, g1=g1, g2=None, g3=None,
                              dparam=dparam if mode == "uncertainty" else None)

    def axpby():
        ops._k("vmtl_axpby", a=l0, b=l1, y=y, wa=0.7, wb=1.3, total=1)

    def axpby_bwd():  # what _AddScalars.backward issues for weights other than 1
        ops._k("vmtl_axpby", a=go, b=go, y=g0, wa=0.7, wb=0.0, total=1)
        ops._k("vmtl_axpby", a=go, b=go, y=g1, wa=1.3, wb=0.0, total=1)

    f = _ab({"vmtl_axpby": axpby, **{m: fwd(m) for m in METHODS}}, reps, rounds)
    b = _ab({"vmtl_axpby_x2": axpby_bwd, **{m: bwd(m) for m in METHODS}}, reps, rounds)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total)) and bool(torch.isfinite(weights).all())
    return {"unit": "us per call, eager launches", "forward": {k: _summary(v) for k, v in f.items()},
            "backward": {k: _summary(v) for k, v in b.items()}}


def bench_step(dev, args):
    from vision_mtl_amd.data import synthetic_batch
    from vision_mtl_amd.graphed import GraphedStep
    from vision_mtl_amd.utils.pipeline_utils import fetch_data_cfg, init_model

    C = fetch_data_cfg("cityscapes").num_classes
    batch = {k: v.to(dev) for k, v in synthetic_batch(args.batch, args.height, args.width, C, seed=11, masked=0.1).items()}
    ms = {}
    # one model alive at a time: a captured step re-packs the GEMM operands of EVERY live model (ops.packs), so steps
    # captured side by side would time each other's weights.  The fixed-weight step runs first and again last: the
    # difference between its two results is what the order of construction alone is worth.
    for tag, method in (("fixed_weights", None),) + tuple((m, m) for m in METHODS) + (("fixed_weights_again", None),):
        torch.manual_seed(11)
        module = init_model(argparse.Namespace(model_name=args.model, backbone_weights=None, loss_balancing=method),
                            argparse.Namespace(num_classes=C)).to(dev).train()
        gstep = GraphedStep(module, batch)
        ms[tag] = _ab({tag: lambda: gstep(batch)}, args.step_reps, args.rounds)[tag]
        gstep.arena.close()
        del gstep, module
        gc.collect()
        torch.cuda.empty_cache()
    return {"unit": "ms per replayed step", "model": args.model, "shape": [args.batch, args.height, args.width],
            "steps": {k: _summary([x / 1e3 for x in v], 4) for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--model", default="basic")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_balance.py needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
           "kernels": bench_kernels(dev, args.reps, args.rounds)}
    if args.step:
        res["graphed_step"] = bench_step(dev, args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
