"""front_volume on the device (wtp_mesh_front) next to fill_volume (wtp_mesh_fill) on tests/golden/box_mesh.npz (46 786
triangles, a 25^3 box): the constant spacings and the graded run of tools/exp_fill.py, Float32, seeds =
PointBoundary.from_mesh at the same spacing, both from the same build.

    python tools/exp_front.py [--targets 1e4,1e5,1e6] [--reps 3] [--batch 0] [--n 10] [--no-graded] [--no-fill]

Each run is timed host to host around wtp_mesh_front + wtp_mesh_front_get (the seeds' upload and the read-back included),
best of --reps after one warm-up call; points, parents, candidates, batches, rounds_max and host syncs are the call's own
wtp_front_info.  The fill's time for the same row (factor 0.75, stall_limit 2000) stands beside it.  The share of the
domain test is a separate pass: tools/kstats_cmd.sh <tag> tools/exp_front.py --targets 1e5 --reps 1 --no-graded --no-fill."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

POINTS_R3_PER_VOLUME = 0.729  # as tools/exp_fill.py: the spacings are the fill's, so the rows can be read side by side
VOLUME = 25.0 ** 3
FACTOR = 0.75


def best_of(reps, call):
    best, out = None, None
    for rep in range(reps + 1):  # the first call warms up (code objects, buffers)
        t0 = time.perf_counter()
        out = call()
        ms = (time.perf_counter() - t0) * 1e3
        if rep and (best is None or ms < best):
            best = ms
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", default="1e4,1e5,1e6")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--no-graded", action="store_true")
    ap.add_argument("--no-fill", action="store_true")
    a = ap.parse_args()
    import wtp_amd as w

    import front_cases as Fc

    z = np.load(os.path.join(ROOT, "tests", "golden", "box_mesh.npz"))
    v, t = z["vertices"].astype(np.float32), z["triangles"].astype(np.int32)
    ctx = w.Context(0)
    oc = w.TriangleOctree(v, t, ctx=ctx)
    seed = Fc.SEED
    print(f"# box_mesh.npz, Float32, n = {a.n} candidates per parent, batch {a.batch or 'chosen by the library'}; ms host to host, "
          f"best of {a.reps}; fill: factor {FACTOR}, stall_limit 2000")
    print(f"# {'spacing':<28} {'seeds':>7} {'points':>9} {'parents':>9} {'cand':>10} {'inside':>7} {'cand/pt':>7} {'batches':>7} "
          f"{'rounds_max':>10} {'syncs':>6} {'ms':>9} {'us/pt':>7} {'cand/s':>10} | {'fill pts':>9} {'darts/pt':>8} {'fill ms':>9} {'us/pt':>7}")
    rows = []
    for target in [float(s) for s in a.targets.split(",") if s]:
        h = float(np.cbrt(POINTS_R3_PER_VOLUME * VOLUME / target) / FACTOR)
        rows.append((f"constant h = {h:.4f}", h, h))
    if not a.no_graded:
        g = np.linspace(1.0, 24.0, 8)
        pts = np.array([(x, y, -1.0) for x in g for y in g], dtype=np.float32)
        law = w.BoundaryLayerSpacing(pts, 0.3, 0.9, 25.0)
        rows.append(("BoundaryLayer 0.3 .. 0.9 / 25", law.desc(), law))
    for label, sp, law in rows:
        seeds = w.PointBoundary.from_mesh(oc, law, ctx=ctx).points()
        oc._resident(ctx)

        def front():
            info = ctx.mesh_front(sp, a.n, seeds, 10_000_000, seed, a.batch)
            return info, ctx.mesh_front_get(info["n_points"])

        def fill():
            info = ctx.mesh_fill(sp, FACTOR, seeds, 10_000_000, 2000, seed, 0)
            return info, ctx.mesh_fill_get(info["n_points"])

        ms, (info, _) = best_of(a.reps, front)
        n = max(info["n_points"], 1)
        line = (f"  {label:<28} {len(seeds):7d} {info['n_points']:9d} {info['n_parents']:9d} {info['n_candidates']:10d} "
                f"{info['n_inside'] / max(info['n_candidates'], 1):7.4f} {info['n_candidates'] / n:7.1f} {info['n_batches']:7d} "
                f"{info['rounds_max']:10d} {info['host_syncs']:6d} {ms:9.2f} {ms * 1e3 / n:7.3f} {info['n_candidates'] / ms * 1e3:10.3e}")
        if not a.no_fill:
            fms, (finfo, _) = best_of(a.reps, fill)
            fn = max(finfo["n_points"], 1)
            line += f" | {finfo['n_points']:9d} {finfo['n_darts'] / fn:8.1f} {fms:9.2f} {fms * 1e3 / fn:7.3f}"
        print(line, flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
