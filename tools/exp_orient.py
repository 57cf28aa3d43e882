"""orient_normals (k = 5) and split_surface (k = 10, 30 degrees) on Fibonacci spheres with PCA normals, through graph="host"
(rows fetched, graph part in Python on the calling thread) and graph="device" (wtp_orient_normals /
wtp_normal_components), with wtp_pca_normals on the same cloud for scale.

    python tools/exp_orient.py [--both 2e4,2e5] [--device 1e6,1e7] [--reps 3] [--dtype float32]
    python tools/exp_orient.py --kernel-csv kernel_stats.csv     # family totals of a rocprofv3 --kernel-trace --stats run
                                                                 # of this script (tools/kstats_cmd.sh)

Times are the best of --reps wall-clock calls after one warm-up call, host arrays in and out; search = hash build +
neighbour sweep and graph = what runs on the rows afterwards are the library's own device spans of that call
(wtp_timers_get).  The host path is timed once: it takes seconds."""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FAMILIES = (("ng_offer", "edge pass (offers)"), ("ng_hook", "hook"), ("ng_jump", "pointer jump"), ("ng_clear", "clear + copy"),
            ("ng_finish", "round end"), ("ng_apply", "flip / label + counts"), ("ng_keep", "split: angles"),
            ("ng_count_edges", "edge count"), ("ng_prep", "prep"), ("ng_start", "prep"), ("ng_ctl", "prep"),
            ("pca_normals", "pca_normals_kernel"))


def kernel_families(path):
    tot, calls, rest = {}, {}, 0.0
    with open(path) as f:
        for row in csv.DictReader(f):
            for key, fam in FAMILIES:
                if key in row["kernel"]:
                    tot[fam] = tot.get(fam, 0.0) + float(row["total_us"])
                    calls[fam] = calls.get(fam, 0) + int(row["calls"])
                    break
            else:
                rest += float(row["total_us"])
    print(f"# {'kernel family':<28} {'launches':>9} {'device ms':>10}")
    for fam, us in sorted(tot.items(), key=lambda kv: -kv[1]):
        print(f"  {fam:<28} {calls[fam]:9d} {us / 1e3:10.3f}")
    print(f"  {'everything else (search)':<28} {'':>9} {rest / 1e3:10.3f}")


def fib_sphere(n, dtype):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + np.sqrt(5)) * i
    return np.ascontiguousarray(np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1).astype(dtype))


def timed(ctx, fn, reps):
    best = None
    for _ in range(reps):
        ctx.timers_reset()
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        t = ctx.timers()
        row = (wall, t["hash_ms"] + t["sweep_ms"], t["other_ms"])
        best = row if best is None or row[0] < best[0] else best
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--both", default="2e4,2e5")
    ap.add_argument("--device", default="1e6,1e7")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--kernel-csv")
    a = ap.parse_args()
    if a.kernel_csv:
        return kernel_families(a.kernel_csv)
    import wtp_amd as w

    dtype = np.dtype(a.dtype).type
    ctx = w.Context(0)
    angle = np.radians(30.0)
    print(f"# Fibonacci sphere, {a.dtype}, PCA normals (k = 5); orient k = 5, split k = 10 at 30 degrees; ms, best of {a.reps}")
    print(f"# {'n':>9} {'call':<22} {'wall':>10} {'search':>8} {'graph':>8}  rounds syncs  result")
    sizes = [(int(float(s)), True) for s in a.both.split(",") if s] + [(int(float(s)), False) for s in a.device.split(",") if s]
    for n, host_too in sizes:
        p = fib_sphere(n, dtype)
        ctx.pca_normals(p, 5)
        (wall, search, graph), nrm = timed(ctx, lambda: ctx.pca_normals(p, 5), a.reps)
        print(f"  {n:9d} {'pca_normals':<22} {wall:10.2f} {search:8.3f} {graph:8.3f}")
        ctx.orient_normals(p, nrm, 5)
        (wall, search, graph), (out, info) = timed(ctx, lambda: ctx.orient_normals(p, nrm, 5), a.reps)
        outward = float(((out * p).sum(axis=1) > 0).mean())
        print(f"  {n:9d} {'orient  graph=device':<22} {wall:10.2f} {search:8.3f} {graph:8.3f}  {info['rounds']:6d} {info['host_syncs']:5d}"
              f"  {info['n_components']} component(s), {info['n_flipped']} flipped, {outward:.4f} outward")
        if host_too:
            mine = nrm.copy()
            t0 = time.perf_counter()
            w.orient_normals(mine, p, k=5, ctx=ctx, graph="host")
            wall = (time.perf_counter() - t0) * 1e3
            print(f"  {n:9d} {'orient  graph=host':<22} {wall:10.2f} {'':>8} {'':>8}  {'':>6} {'':>5}"
                  f"  {int((mine != out).any(axis=1).sum())} normals differ from the device's")
        ctx.normal_components(p, out, 10, angle)
        (wall, search, graph), (labels, info) = timed(ctx, lambda: ctx.normal_components(p, out, 10, angle), a.reps)
        print(f"  {n:9d} {'split   graph=device':<22} {wall:10.2f} {search:8.3f} {graph:8.3f}  {info['rounds']:6d} {info['host_syncs']:5d}"
              f"  {info['n_components']} component(s)")
        if host_too:
            t0 = time.perf_counter()
            ref = w.normals._host_labels(p, out, 10, angle, ctx)
            wall = (time.perf_counter() - t0) * 1e3
            print(f"  {n:9d} {'split   graph=host':<22} {wall:10.2f} {'':>8} {'':>8}  {'':>6} {'':>5}"
                  f"  {int((ref != labels).sum())} labels differ from the device's")
    ctx.close()


if __name__ == "__main__":
    main()
