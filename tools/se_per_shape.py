"""Per-launch durations of the squeeze-excite kernels in a rocprofv3 kernel trace of bench.py, grouped by the launch's
position within the step (eight SE blocks per step in a fixed order: forward launches run block 0 .. 7, backward ones
7 .. 0; the sequence route makes two fc / fc_wgrad launches per block and direction).

    python tools/se_per_shape.py <dir>/..._kernel_trace.csv
"""
import collections
import csv
import sys

def load(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return rows
def series(rows, pred):
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if pred(r["Kernel_Name"])]
def by_pos(vals, n):
    out = collections.defaultdict(list)
    for i, v in enumerate(vals):
        out[i % n].append(v)
    return {k: (sum(v) / len(v), min(v), len(v)) for k, v in out.items()}
path, = sys.argv[1:]
rows = load(path)
steps = len(series(rows, lambda k: "silog_fwd" in k))  # one launch per step execution
for key in ("se_gate_fwd", "se_gate_bwd", "se_wgrad", "hw_reduce", "fc_kernel", "fc_wgrad", "channel_scale_add"):
    v = series(rows, lambda k: key in k)
    if not v:
        continue
    n = len(v) // steps
    print(f"{key}: {len(v)} launches, {n} per step")
    for k, (avg, mn, cnt) in sorted(by_pos(v, n).items()):
        print(f"   pos {k:2d}: avg {avg:7.2f} us  min {mn:7.2f}  n={cnt}")
