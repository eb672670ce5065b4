"""Element-by-element comparison of three `bench.py --dump-outputs` directories: route 0, route 1 and a rerun of route 1.

    python tools/dump_compare.py <dir route 0> <dir route 1> <dir route 1 rerun>
"""
import sys
import numpy as np

def cmp(tag, a, b):
    a, b = np.load(a).astype(np.float64), np.load(b).astype(np.float64)
    d = np.abs(a - b)
    mag = max(np.abs(a).max(), np.abs(b).max())
    q = np.quantile(d, [0.5, 0.99, 0.9999])
    print(f"{tag}: n={a.size} max|x| {mag:.3e} max abs diff {d.max():.3e} (rel {d.max() / mag:.2e}) p50 {q[0]:.1e} "
          f"p99 {q[1]:.1e} p99.99 {q[2]:.1e} identical {np.mean(d == 0):.4f}")

d0, d1, d1b = sys.argv[1:4]
for name in ("loss", "grad", "bn_running_stats"):
    cmp(f"{name} route 1 vs 0", f"{d1}/{name}.npy", f"{d0}/{name}.npy")
    cmp(f"{name} route 1 rerun", f"{d1b}/{name}.npy", f"{d1}/{name}.npy")
