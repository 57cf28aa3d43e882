"""metrics(cloud; k = 20) end to end on uniform Float32 clouds held in host memory, with the library's own spans of the call:
search = hash build + neighbour sweep (wtp_timers_get [0] + [1]), consumer = what runs on the rows afterwards ([2]).

    python tools/exp_metrics.py [--root TREE] [--sizes 1e6,1e7] [--reps 3] [--label NAME]

--root: the checkout whose package is measured (default: the one this script lies in), so that the same script times
another commit's metrics(); profiles/metrics_device.txt holds both."""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--sizes", default="1e6,1e7")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--label", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import wtp_amd as w  # noqa: E402

ctx = w.Context(0)
device_stats = hasattr(ctx, "knn_stats")
print(f"# {a.label or os.path.abspath(a.root)}: statistics on the {'device (wtp_knn_stats)' if device_stats else 'host (numpy over the returned n x k matrices)'}")
print(f"# {'n':>9} {'k':>3} {'end-to-end ms':>14} {'search ms':>10} {'consumer ms':>12} {'consumer/search':>16}   avg, separation")
for size in a.sizes.split(","):
    n = int(float(size))
    x = w.synth.uniform(n, 3, np.float32)
    w.metrics(x, k=20, ctx=ctx, verbose=False)  # buffers, tuning
    best = None
    for _ in range(a.reps):
        ctx.timers_reset()
        t0 = time.perf_counter()
        m = w.metrics(x, k=20, ctx=ctx, verbose=False)
        wall = (time.perf_counter() - t0) * 1e3
        t = ctx.timers()
        row = (wall, t["hash_ms"] + t["sweep_ms"], t["other_ms"])
        best = row if best is None or row[0] < best[0] else best
    ratio = f"{best[2] / best[1]:16.3f}" if best[1] > 0 else f"{'-':>16}"
    print(f"  {n:9d} {20:3d} {best[0]:14.2f} {best[1]:10.3f} {best[2]:12.3f} {ratio}   {m['avg']:.9g}, {m['separation']:.9g}")
