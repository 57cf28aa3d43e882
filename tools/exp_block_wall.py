"""What a boundary wall costs the C block driver (wtp_block_set_wall): the 10 M uniform cloud in the unit cube with a
cell-centred grid of spacing ~s on each of its six faces (m = round(n^(1/3)) per side: 277 k points for 10 M), ms per
iteration for
  (a) the plain session on [wall ; x] with the wall as fixed head (one wtp_relax_step per iteration);
  (b) a one-rank block session with the wall (rccl path: no peers);
  (c) the 8-ranks-as-threads rehearsal on the one GPU (loopback transport), with and without the wall, three runs
      each in alternating order (median and range).
Usage: python tools/exp_block_wall.py [n] [iters]"""
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

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
FORCE = dict(kind=2, beta=0.2, u0=1.0, gamma=3.0)
K = 21
s = float(n) ** (-1.0 / 3.0)


def face_wall(m):
    g = (np.arange(m, dtype=np.float64) + 0.5) / m
    u, v = np.meshgrid(g, g, indexing="ij")
    faces = []
    for a in range(3):
        for c in (0.0, 1.0):
            f = np.empty((u.size, 3), dtype=np.float32)
            f[:, a] = c
            f[:, (a + 1) % 3] = u.ravel()
            f[:, (a + 2) % 3] = v.ravel()
            faces.append(f)
    return np.concatenate(faces)


wall = face_wall(int(round(1.0 / s)))
wall_d = torch.from_numpy(wall).cuda()
print(f"n = {n}, wall = {len(wall)} points ({100.0 * len(wall) / (n + len(wall)):.1f} % of the snapshot), {iters} timed iterations")


def gen_on(ctx):
    def gen(first, m):
        t = torch.empty((m, 3), dtype=torch.float32, device="cuda")
        # the library writes on its own stream: torch's queued work on this block (it may have just been freed) first
        torch.cuda.synchronize()
        ctx.gen_uniform_dev(wtp_amd.synth.SEED, first, m, 3, np.float32, t.data_ptr())
        return t
    return gen


ctx = wtp_amd.Context(0)
boxes1 = blockc.orthtree_boxes(None, 1, False)
xyz, gid = blockc.shard_stream(gen_on(ctx), boxes1, 0, n)

# (a) plain session, wall as fixed head
snap = torch.cat([wall_d, xyz]).contiguous()
torch.cuda.synchronize()  # (the library reads on its own stream)
with ctx.relax(None, len(wall), s, FORCE, K, s / 2000, s / 20, device_ptr=(snap.data_ptr(), len(snap), 3, np.float32)) as t:
    for _ in range(5):
        t.step(True)
    t0 = time.perf_counter()
    for _ in range(iters):
        t.step(True)
    a_ms = (time.perf_counter() - t0) / iters * 1e3
print(f"(a) plain session [wall ; x], n_fixed = n_wall, one wtp_relax_step per iteration: {a_ms:.3f} ms per iteration")
del snap

# (b) one-rank block session with and without the wall
for name, w in (("with the wall", wall), ("without a wall", None)):
    drv = blockc.BlockRelax(ctx, 0, 1, boxes1, xyz, gid, 2.0 * s, s, FORCE, K, s / 2000, s / 20, wall_xyz=w)
    drv.run(5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = drv.run(iters)
    torch.cuda.synchronize()
    b_ms = (time.perf_counter() - t0) / iters * 1e3
    print(f"(b) one-rank block session {name}: {b_ms:.3f} ms per iteration, host syncs per iteration "
          f"{out['host_syncs'] / iters:.2f}" + (f", (b) - (a) = {b_ms - a_ms:+.3f} ms" if w is not None else ""))
    drv.close()
del xyz, gid
ctx.close()

# (c) eight ranks as threads on the one GPU (the rehearsal of bench.py --gpus 8): three runs per case, in the order
# A B B A A B, so that neither case always runs first
boxes8 = blockc.orthtree_boxes(None, 8, False)
shard_lock = threading.Lock()  # (the shards are generated one rank at a time: torch's sorts do not run side by side)


def rehearsal(w):
    times = [0.0] * 8
    info = [None] * 8

    def worker(rank, hub):
        torch.cuda.set_device(0)
        c = wtp_amd.Context(0)
        try:
            with shard_lock:
                x, g = blockc.shard_stream(gen_on(c), boxes8, rank, n)
                torch.cuda.synchronize()
            d = blockc.BlockRelax(c, rank, 8, boxes8, x, g, 2.2 * s, s, FORCE, K, s / 2000, s / 20,
                                  transport=blockc.loopback_transport(hub, rank), wall_xyz=w)
            d.run(5)
            hub.barrier.wait()  # (aborted by run_threads if a rank fails)
            t0 = time.perf_counter()
            out = d.run(iters)
            times[rank] = time.perf_counter() - t0
            info[rank] = out
            d.close()
        finally:
            c.close()

    blockc.run_threads(8, worker)
    return max(times) / iters * 1e3, info


cases = {"without a wall": None, "with the wall": wall}
runs = {name: [] for name in cases}
for name in ("without a wall", "with the wall", "with the wall", "without a wall", "without a wall", "with the wall"):
    c_ms, info = rehearsal(cases[name])
    runs[name].append(c_ms)
    ghosts = sum(o["n_ghost"] for o in info)
    print(f"(c) 8 ranks as threads, {name}: {c_ms:.3f} ms per iteration (slowest rank), ghost rows of all ranks "
          f"{ghosts}, host syncs per iteration {info[0]['host_syncs'] / iters:.2f}, closest pair "
          f"({info[0]['argmin_i']}, {info[0]['argmin_j']}) r = {info[0]['argmin_r']:.3e}", flush=True)
for name, v in runs.items():
    v = sorted(v)
    print(f"(c) {name}: median {v[len(v) // 2]:.3f} ms, range {v[0]:.3f} .. {v[-1]:.3f} ms over {len(v)} runs")
