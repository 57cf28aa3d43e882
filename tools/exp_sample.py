"""sample_surface on the device (wtp_mesh_sample) on tests/golden/box_mesh.npz (46 786 triangles, a 25^3 box): constant
spacings sized for about 1e4, 1e5 and 1e6 samples and one graded run (BoundaryLayerSpacing measured to a grid of points
under the box), Float32.

    python tools/exp_sample.py [--targets 1e4,1e5,1e6] [--reps 3] [--batch 0] [--no-graded] [--no-model]

Each run is timed host to host around wtp_mesh_sample + wtp_mesh_sample_get (the call ends in its read-back), best of
--reps after one warm-up call; samples, darts, batches, rounds_max and host syncs are the call's own wtp_sample_info.
For scale only, the numpy brute-force model of tests/surface_sampling_cases.py (serial(): one dart at a time against
all accepted samples) is timed once on the first target's darts: it is a model of the contract, not the reference."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

AREA_PER_R2 = 2284.0  # samples x r^2 the box saturates at (measured: 1253 samples at r = 1.35)


def run(ctx, sp, factor, batch, reps, seed):
    best, info, got = None, None, None
    for rep in range(reps + 1):  # the first call warms up (code objects, buffers)
        t0 = time.perf_counter()
        info = ctx.mesh_sample(sp, factor, 10_000_000, 2000, seed, batch)
        got = ctx.mesh_sample_get(info["n_points"])
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

    import surface_sampling_cases as S

    z = np.load(os.path.join(ROOT, "tests", "golden", "box_mesh.npz"))
    v, t = z["vertices"].astype(np.float32), z["triangles"].astype(np.int32)
    ctx = w.Context(0)
    ctx.mesh_set(v, t)
    seed, factor = S.SEED, 0.75
    print(f"# box_mesh.npz, Float32, factor {factor}, stall_limit 2000, batch {a.batch or 'chosen by the library'}; ms host to host, "
          f"best of {a.reps}")
    print(f"# {'spacing':<28} {'samples':>9} {'darts':>11} {'batches':>7} {'rounds_max':>10} {'syncs':>6} {'ms':>10} {'darts/s':>10}")
    rows = []
    for target in [float(s) for s in a.targets.split(",") if s]:
        h = float(np.sqrt(AREA_PER_R2 / target) / factor)
        rows.append((f"constant h = {h:.4f}", h))
    if not a.no_graded:
        g = np.linspace(1.0, 24.0, 8)
        pts = np.array([(x, y, -1.0) for x in g for y in g], dtype=np.float32)
        rows.append(("BoundaryLayer 0.15 .. 0.45 / 25", w.BoundaryLayerSpacing(pts, 0.15, 0.45, 25.0).desc()))
    first = None
    for label, sp in rows:
        ms, info, got = run(ctx, sp, factor, a.batch, a.reps, seed)
        first = first or (sp, info)
        print(f"  {label:<28} {info['n_points']:9d} {info['n_darts']:11d} {info['n_batches']:7d} {info['rounds_max']:10d} "
              f"{info['host_syncs']:6d} {ms:10.2f} {info['n_darts'] / ms * 1e3:10.3e}", flush=True)
    if not a.no_model and first is not None and not isinstance(first[0], dict):
        sp, info = first
        xyz, tri, r = ctx.mesh_sample_darts(sp, factor, seed, 0, info["n_darts"])
        t0 = time.perf_counter()
        acc, n_darts, reason = S.serial(xyz, r, 10_000_000, 2000)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"# numpy brute-force model serial() on the first run's darts (not the reference): {len(acc)} samples, {n_darts} darts, "
              f"{ms:.0f} ms; equal to the device's: {len(acc) == info['n_points'] and n_darts == info['n_darts']}")
    ctx.close()


if __name__ == "__main__":
    main()
