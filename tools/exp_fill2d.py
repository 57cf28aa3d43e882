"""fill_area on the device (wtp_loops_fill) and the loop index's queries (wtp_loops_query), Float32, host to host.

    python tools/exp_fill2d.py [--targets 1e4,1e5,1e6] [--reps 3] [--batch 0] [--no-graded] [--no-model] [--no-query]

The domain is a circle of radius 10 as 4096 segments with a concentric hole of radius 4 as 1024: constant spacings sized
for about 1e4, 1e5 and 1e6 points and one graded run (BoundaryLayerSpacing measured to both loops' vertices).  Seeds: the
loops' vertices thinned to about one per spacing.  Each run is timed around wtp_loops_fill + wtp_loops_fill_get (the
seeds' upload and the read-back included), best of --reps after one warm-up call; points, darts, inside share, batches,
rounds_max and host syncs are the call's own wtp_fill_info.  For scale only, the same result is composed on the host once
for the first target: the uniform stream (synth.uniform) scaled into the box, wtp_loops_query's inside flag, and the
numpy brute-force serial() of tests/area_fill_cases.py: a model of the contract, not the reference.  The share of the
domain test is a separate pass: tools/kstats_cmd.sh <tag> tools/exp_fill2d.py --targets 1e5 --reps 1 --no-graded
--no-model --no-query.  Last, wtp_loops_query alone: 1e6 uniform queries over the box of a circle of 1e3 and of 1e5
segments, all four outputs, the queries' upload and the read-back included."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

POINTS_R2_PER_AREA = 0.669  # points x r^2 / area a fill saturates at (measured: 476 points at r = 0.0375 in the unit square)
R_OUT, R_HOLE = 10.0, 4.0
AREA = np.pi * (R_OUT ** 2 - R_HOLE ** 2)


def ring(n, radius):
    t = 2 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(t), radius * np.sin(t)], axis=1).astype(np.float32)


def thinned(loops, h):
    """The loops' vertices, about one per h along each loop."""
    out = []
    for l in loops:
        step = float(np.linalg.norm(l[1].astype(np.float64) - l[0].astype(np.float64)))
        out.append(l[::max(1, int(round(h / step)))])
    return np.concatenate(out)


def run(ctx, sp, factor, seeds, batch, reps, seed):
    best, info, got = None, None, None
    for rep in range(reps + 1):  # the first call warms up (code objects, buffers)
        t0 = time.perf_counter()
        info = ctx.loops_fill(sp, factor, seeds, 10_000_000, 2000, seed, batch)
        got = ctx.loops_fill_get(info["n_points"])
        ms = (time.perf_counter() - t0) * 1e3
        if rep and (best is None or ms < best):
            best = ms
    return best, info, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", default="1e4,1e5,1e6")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--no-graded", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--no-query", action="store_true")
    a = ap.parse_args()
    import wtp_amd as w

    import area_fill_cases as A

    loops = [ring(4096, R_OUT), ring(1024, R_HOLE)]
    ctx = w.Context(0)
    tree = w.SegmentQuadtree(loops, ctx=ctx)
    seed, factor = A.SEED, 0.75
    print(f"# circle of 4096 segments, radius {R_OUT:g}, hole of 1024, radius {R_HOLE:g}; Float32, factor {factor}, stall_limit 2000, "
          f"batch {a.batch or 'chosen by the library'}; ms host to host, best of {a.reps}")
    print(f"# {'spacing':<28} {'seeds':>7} {'points':>9} {'darts':>11} {'inside':>7} {'darts/pt':>8} {'batches':>7} {'rounds_max':>10} "
          f"{'syncs':>6} {'ms':>10} {'darts/s':>10}")
    rows = []
    for target in [float(s) for s in a.targets.split(",") if s]:
        h = float(np.sqrt(POINTS_R2_PER_AREA * AREA / target) / factor)
        rows.append((f"constant h = {h:.4f}", h, h))
    if not a.no_graded:
        law = w.BoundaryLayerSpacing(np.concatenate(loops), 0.02, 0.08, 1.5)
        rows.append(("BoundaryLayer 0.02 .. 0.08 / 1.5", law.desc(), 0.02))
    first = None
    for label, sp, h_wall in rows:
        seeds = thinned(loops, h_wall)
        tree._resident(ctx)
        ms, info, got = run(ctx, sp, factor, seeds, a.batch, a.reps, seed)
        first = first or (sp, info, seeds, got)
        print(f"  {label:<28} {len(seeds):7d} {info['n_points']:9d} {info['n_darts']:11d} {info['n_inside'] / info['n_darts']:7.4f} "
              f"{info['n_darts'] / max(info['n_points'], 1):8.1f} {info['n_batches']:7d} {info['rounds_max']:10d} "
              f"{info['host_syncs']:6d} {ms:10.2f} {info['n_darts'] / ms * 1e3:10.3e}", flush=True)
    if not a.no_model and first is not None and not isinstance(first[0], dict):
        sp, info, seeds, got = first
        n = info["n_darts"]
        lo, hi, _ = ctx.loops_bounds()
        lo, hi = lo.astype(np.float32), hi.astype(np.float32)
        t0 = time.perf_counter()
        xy = lo + w.synth.uniform(n, 2, np.float32) * (hi - lo)
        inside = ctx.loops_query(xy, want=("inside",))["inside"]
        r = np.full(n, np.float32(factor) * np.float32(sp), dtype=np.float32)
        sr = np.full(len(seeds), r[0], dtype=np.float32)
        acc, n_darts, reason, n_in = A.serial(xy, inside, r, seeds, sr, 10_000_000, 2000)
        ms = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(acc, got["dart"]) and np.array_equal(xy[acc], got["xy"]) and n_darts == n and n_in == info["n_inside"]
        print(f"# composed on the host for scale (synth.uniform -> wtp_loops_query -> numpy serial(); not the reference): "
              f"{len(acc)} points, {n_darts} darts, {ms:.0f} ms; equal to the device's: {same}")
    if not a.no_query:
        nq = 1_000_000
        print(f"# wtp_loops_query alone: {nq} uniform queries over the box, all four outputs, host to host, best of {a.reps}")
        print(f"# {'segments':>9} {'inside':>7} {'ms':>9} {'queries/s':>10}")
        for ns in (1_000, 100_000):
            ctx.loops_set([ring(ns, R_OUT)])
            q = ((w.synth.uniform(nq, 2, np.float32) - np.float32(0.5)) * np.float32(2 * R_OUT)).astype(np.float32)
            best, out = None, None
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                out = ctx.loops_query(q)
                ms = (time.perf_counter() - t0) * 1e3
                if rep and (best is None or ms < best):
                    best = ms
            print(f"  {ns:9d} {out['inside'].mean():7.4f} {best:9.2f} {nq / best * 1e3:10.3e}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
