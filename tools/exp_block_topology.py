"""Sharded set_topology (wtp_block_knn / wtp_block_radius_*) on one GPU: 8 ranks as threads, one context each, rows carried
by the loopback transport (host-staged).  Per rank and call: wall time, the device time of the context's stream split
by the library's timers ([0] hash builds, [1] search kernels, [2] the rest: ghost classification, gid ordering,
certificate + translation, scans), ghosts, widening rounds.  Against it: wtp_knn_dev on the whole cloud on one context.

The eight ranks share one GPU, so their kernels overlap and every per-rank device time includes the others' work that
ran at the same moment; the wall time includes the host-staged exchange and the all-gathers.  What several GPUs would
show (one rank per GPU, RCCL) is not measured here.

    python tools/exp_block_topology.py            # 8 M uniform, 4 M graded
"""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import wtp_amd  # noqa: E402
from whatsthepoint_jl_amd import blockc  # noqa: E402

K = 21
R = 8
REPS = 3


def ranks(parts, x, gid, call):
    hub = blockc.LoopbackHub(R)
    out = [None] * R

    def body(r):
        torch.cuda.set_device(0)
        ctx = wtp_amd.Context(0)
        try:
            xs = torch.from_numpy(x[parts[r]]).cuda()
            gs = torch.from_numpy(gid[parts[r]]).cuda()
            tr = blockc.loopback_transport(hub, r)
            rows = []
            for rep in range(REPS + 1):
                ctx._lib.wtp_timers_reset(ctx._h)
                hub.barrier.wait()
                t0 = time.perf_counter()
                info = call(ctx, r, xs, gs, tr)
                dt = time.perf_counter() - t0
                tm = (C.c_double * 4)()
                ctx._lib.wtp_timers_get(ctx._h, tm)
                if rep > 0:  # the first call allocates
                    rows.append((dt * 1e3, tm[0], tm[1], tm[2], info))
            out[r] = rows
        finally:
            ctx.close()

    ts = [threading.Thread(target=body, args=(r,)) for r in range(R)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    assert all(o is not None for o in out), "a rank failed"
    return out


def report(name, n, out):
    print(f"\n== {name}: n = {n}, {R} ranks as threads on one GPU, median of {REPS} calls ==")
    print("rank  n_owned   n_ghost  peers widened   width      wall ms  hash ms  search ms  other ms")
    walls = []
    for r, rows in enumerate(out):
        med = sorted(rows, key=lambda v: v[0])[len(rows) // 2]
        wall, th, tsr, to, info = med
        walls.append(wall)
        print(f"{r:4d} {info['n_owned']:9d} {info['n_ghost']:9d} {info['n_peers']:5d} {info['widened']:7d} {info['width']:9.3e} "
              f"{wall:9.2f} {th:8.2f} {tsr:10.2f} {to:9.2f}")
    print(f"slowest rank: {max(walls):.2f} ms per call")


def single(x, k=K):
    with wtp_amd.Context(0) as ctx:
        d = torch.from_numpy(x).cuda()
        idx = torch.empty((len(x), k), dtype=torch.int32, device="cuda")
        dist = torch.empty((len(x), k), dtype=torch.float32, device="cuda")
        ts = []
        for rep in range(REPS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.knn_dev(d.data_ptr(), len(x), 3, np.float32, k, False, idx.data_ptr(), dist.data_ptr())
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts[1:])[len(ts[1:]) // 2]


def knn_call(width=0.0):
    def call(ctx, r, xs, gs, tr):
        _, _, info = blockc.block_knn(ctx, r, R, xs, gs, K, return_dist=True, width=width, transport=tr)
        info["n_owned"] = len(xs)
        return info

    return call


def radius_call(rad):
    def call(ctx, r, xs, gs, tr):
        _, _, info = blockc.block_radius(ctx, r, R, xs, gs, rad, transport=tr)
        info["n_owned"] = len(xs)
        return info

    return call


def main():
    n = 8_000_000
    x = wtp_amd.synth.uniform(n, 3, np.float32)
    gid = np.random.default_rng(1).permutation(n).astype(np.int64)
    own = blockc.owner_of(x, blockc.orthtree_boxes(None, R, equal_count=False))
    parts = [np.nonzero(own == r)[0] for r in range(R)]
    s = float(n) ** (-1.0 / 3.0)
    cloud = np.empty_like(x)
    cloud[gid] = x
    print(f"wtp_knn_dev, whole uniform cloud, one context: {single(cloud):.2f} ms (n = {n}, k = {K})")
    report("k-NN, uniform, first width estimated", n, ranks(parts, x, gid, knn_call()))
    report("k-NN, uniform, first width 0.25 spacings (widening rounds)", n, ranks(parts, x, gid, knn_call(0.25 * s)))
    report("radius r = 1.5 spacings, uniform", n, ranks(parts, x, gid, radius_call(1.5 * s)))
    del x, cloud, gid

    n = 4_000_000
    x = wtp_amd.synth.graded(n, dtype=np.float32)
    gid = np.random.default_rng(2).permutation(n).astype(np.int64)
    own = blockc.owner_of(x, blockc.orthtree_boxes(x, R))
    parts = [np.nonzero(own == r)[0] for r in range(R)]
    cloud = np.empty_like(x)
    cloud[gid] = x
    print(f"\nwtp_knn_dev, whole graded cloud, one context: {single(cloud):.2f} ms (n = {n}, k = {K})")
    report("k-NN, graded, count-median boxes", n, ranks(parts, x, gid, knn_call()))


if __name__ == "__main__":
    main()
