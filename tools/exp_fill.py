"""fill_volume on the device (wtp_mesh_fill) on tests/golden/box_mesh.npz (46 786 triangles, a 25^3 box): constant
spacings sized for about 1e4, 1e5 and 1e6 volume points and one graded run (BoundaryLayerSpacing measured to a grid of
points under the box), Float32, seeds = PointBoundary.from_mesh at the same spacing.

    python tools/exp_fill.py [--targets 1e4,1e5,1e6] [--reps 3] [--batch 0] [--no-graded] [--no-model]

Each run is timed host to host around wtp_mesh_fill + wtp_mesh_fill_get (the seeds' upload and the read-back included),
best of --reps after one warm-up call; points, darts, inside share, batches, rounds_max and host syncs are the call's own
wtp_fill_info.  For scale only, the same result is composed on the host once for the first target: the uniform stream
(synth.uniform) scaled into the box, wtp_mesh_query's inside flag, and the numpy brute-force serial() of
tests/volume_fill_cases.py: a model of the contract, not the reference.  The share of the domain test is a separate
pass: tools/kstats_cmd.sh <tag> tools/exp_fill.py --targets 1e5 --reps 1 --no-graded --no-model."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

POINTS_R3_PER_VOLUME = 0.729  # points x r^3 / volume a fill saturates at (measured: 512 points at r = 0.1125 in the unit cube)
VOLUME = 25.0 ** 3


def run(ctx, sp, factor, seeds, batch, reps, seed):
    best, info, got = None, None, None
    for rep in range(reps + 1):  # the first call warms up (code objects, buffers)
        t0 = time.perf_counter()
        info = ctx.mesh_fill(sp, factor, seeds, 10_000_000, 2000, seed, batch)
        got = ctx.mesh_fill_get(info["n_points"])
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
    a = ap.parse_args()
    import wtp_amd as w

    import volume_fill_cases as V

    z = np.load(os.path.join(ROOT, "tests", "golden", "box_mesh.npz"))
    v, t = z["vertices"].astype(np.float32), z["triangles"].astype(np.int32)
    ctx = w.Context(0)
    oc = w.TriangleOctree(v, t, ctx=ctx)
    seed, factor = V.SEED, 0.75
    print(f"# box_mesh.npz, Float32, factor {factor}, stall_limit 2000, batch {a.batch or 'chosen by the library'}; ms host to host, "
          f"best of {a.reps}")
    print(f"# {'spacing':<28} {'seeds':>7} {'points':>9} {'darts':>11} {'inside':>7} {'darts/pt':>8} {'batches':>7} {'rounds_max':>10} "
          f"{'syncs':>6} {'ms':>10} {'darts/s':>10}")
    rows = []
    for target in [float(s) for s in a.targets.split(",") if s]:
        h = float(np.cbrt(POINTS_R3_PER_VOLUME * VOLUME / target) / factor)
        rows.append((f"constant h = {h:.4f}", h, h))
    if not a.no_graded:
        g = np.linspace(1.0, 24.0, 8)
        pts = np.array([(x, y, -1.0) for x in g for y in g], dtype=np.float32)
        law = w.BoundaryLayerSpacing(pts, 0.3, 0.9, 25.0)
        rows.append(("BoundaryLayer 0.3 .. 0.9 / 25", law.desc(), law))
    first = None
    for label, sp, law in rows:
        seeds = w.PointBoundary.from_mesh(oc, law, ctx=ctx).points()
        oc._resident(ctx)
        ms, info, got = run(ctx, sp, factor, seeds, a.batch, a.reps, seed)
        first = first or (sp, info, seeds, got)
        print(f"  {label:<28} {len(seeds):7d} {info['n_points']:9d} {info['n_darts']:11d} {info['n_inside'] / info['n_darts']:7.4f} "
              f"{info['n_darts'] / max(info['n_points'], 1):8.1f} {info['n_batches']:7d} {info['rounds_max']:10d} "
              f"{info['host_syncs']:6d} {ms:10.2f} {info['n_darts'] / ms * 1e3:10.3e}", flush=True)
    if not a.no_model and first is not None and not isinstance(first[0], dict):
        sp, info, seeds, got = first
        n = info["n_darts"]
        lo, hi = (x.astype(np.float32) for x in ctx.mesh_bounds())
        t0 = time.perf_counter()
        xyz = lo + w.synth.uniform(n, 3, np.float32) * (hi - lo)
        inside = ctx.mesh_query(xyz, want=("inside",))["inside"]
        r = np.full(n, np.float32(factor) * np.float32(sp), dtype=np.float32)
        sr = np.full(len(seeds), r[0], dtype=np.float32)
        acc, n_darts, reason, n_in = V.serial(xyz, inside, r, seeds.astype(np.float32), sr, 10_000_000, 2000)
        ms = (time.perf_counter() - t0) * 1e3
        same = np.array_equal(acc, got["dart"]) and np.array_equal(xyz[acc], got["xyz"]) and n_darts == n and n_in == info["n_inside"]
        print(f"# composed on the host for scale (synth.uniform -> wtp_mesh_query -> numpy serial(); not the reference): "
              f"{len(acc)} points, {n_darts} darts, {ms:.0f} ms; equal to the device's: {same}")
    ctx.close()


if __name__ == "__main__":
    main()
