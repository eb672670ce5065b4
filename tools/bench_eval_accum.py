"""Cost of the dataset-level evaluation metrics (csrc/eval_accum.hip, metrics.EvalAccumulator).

    python tools/bench_eval_accum.py [--out FILE.jsonl]

EvalAccumulator.update given a step's ready int32 confusion matrix + the depth pair (two launches), given int64
predictions and targets + the depth pair (two launches), given the depth pair alone, and compute()'s finalize launch, on
bs-32 batches already on the GPU at 128x256 and 256x256.  50 calls captured into one graph, the replay timed with device
events, median of 7; `us_per_call_eager`: the same calls issued from Python."""
import argparse
import json
import os
import statistics
import sys
import time

C = 19
SHAPES = [(32, 128, 256), (32, 256, 256)]
CALLS, REPEATS = 50, 7


def _graph_us(fn):
    import torch

    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / CALLS)
    return out


def kernels(emit):
    import torch

    from vision_mtl_amd import metrics as M

    dev = torch.device("cuda:0")
    for B, H, W in SHAPES:
        g = torch.Generator().manual_seed(B + H + W)
        P = B * H * W
        mask = torch.randint(0, C, (P,), generator=g).to(dev)
        pred = torch.randint(0, C, (P,), generator=g).to(dev)
        dp = torch.sigmoid(1.5 * torch.randn(P, generator=g)).to(dev)
        dt = 0.05 + 0.95 * torch.rand(P, generator=g)
        dt[torch.rand(P, generator=g) < 0.2] = 0.0
        dt = dt.to(dev)
        step_cm = M.confusion_matrix(pred, mask, C)
        acc = M.EvalAccumulator(C, device=dev)
        forms = {"update_step_cm_depth": lambda: acc.update(step_cm=step_cm, depth_pred=dp, depth=dt),
                 "update_pixels_depth": lambda: acc.update(segm_pred=pred, mask=mask, depth_pred=dp, depth=dt),
                 "update_depth_only": lambda: acc.update(depth_pred=dp, depth=dt),
                 "finalize": lambda: M._k("vmtl_eval_finalize", cm=acc.cm, acc=acc.acc, C=C, beta=1.0, ignore_index=-1,
                                          out=acc._out, iou=acc._out[len(M.EVAL_SCALARS):])}
        for name, fn in forms.items():
            us = _graph_us(fn)
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            eager = (time.perf_counter() - t0) / CALLS * 1e6
            bytes_ = {"update_step_cm_depth": 8 * P, "update_pixels_depth": 24 * P, "update_depth_only": 8 * P,
                      "finalize": 8 * C * C}[name]
            emit({"bench": "kernels", "what": name, "B": B, "H": H, "W": W, "us_per_call": round(statistics.median(us), 3),
                  "us_all_repeats": [round(u, 3) for u in us], "us_per_call_eager": round(eager, 2), "bytes": bytes_,
                  "GB_per_s": round(bytes_ / statistics.median(us) / 1e3, 1)})
            acc.reset()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_accum.py needs an MI355X")
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    kernels(emit)


if __name__ == "__main__":
    main()
