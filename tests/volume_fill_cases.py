"""Case table and numpy model of the volume fill (include/wtp.h: wtp_mesh_fill, wtp_mesh_fill_darts).  Shared by
test_volume_fill_cases.py (no GPU: the batch algorithm equals the serial loop; every case has the property it is
there for) and test_gpu_volume_fill.py (the device equals the model).

The model, in the mesh's type T:
  darts()   dart j of seed s: w_a = splitmix64((s << 40) + 3 j + a), u_a = T(float32(w_a >> 40) 2^-24),
            c_a = lo_a + u_a (hi_a - lo_a) over the mesh's vertex box (oracle.mesh_bbox), r = T(factor) h(c),
            inside = oracle.mesh_query(...)["inside"] (brute-force nearest triangle, pseudonormal side, box)
  serial()  darts in order; a dart is accepted iff it is inside and ((dx dx + dy dy) + dz dz) < m m, m = min(r_p, r_q),
            holds for no seed and no accepted q; before each dart the run ends at max_points accepted (2) or
            stall_limit misses in a row (1); seeds are never tested against each other and never returned
  batched() the library's batch algorithm in plain Python: darts outside the mesh and darts in conflict with a seed or
            an accepted point are culled, Jacobi rounds over the rest, stop scan in dart order; batch = 0 is the
            library's own schedule, and the round count is the library's when the darts are those of whole batches

EDGE_CASES are the cases of test_gpu_sampler_edges.py: runs that end beyond the 256th tile of the stop scan.  case_of()
finds a case of either table."""
from __future__ import annotations

import functools
import os

import numpy as np

import oracle
from surface_sampling_cases import F32, F64, DTYPES, SEED, GOLD, LAW_POINTS, _splitmix64, _conflicts, cube, law_h
from surface_sampling_cases import _lower_conflicts, batch_sizes, whole_batches, jacobi_rounds  # noqa: F401


# ---- meshes and seeds ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(stem):
    z = np.load(os.path.join(GOLD, f"{stem}_mesh.npz"))
    return z["vertices"].astype(F64), z["triangles"].astype(np.int32)


def flat_square():
    """Two triangles in the plane z = 2^24, where the widening of a flat axis (100 eps, at least 1e-10) rounds away in
    both types: the box has no height, every dart lies on the mesh, and distance 0 is not inside."""
    v = np.array([(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], dtype=F64) * (1.0, 1.0, 2.0 ** 24)
    return v, np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int32)


def face_grid(m, scale=(1.0, 1.0, 1.0), axes=(0, 1, 2)):
    """m x m points at the cell centres of both faces normal to each of `axes` of the box [0, scale]."""
    g = (np.arange(m) + 0.5) / m
    a, b = (x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij"))
    out = []
    for ax in axes:
        for side in (0.0, 1.0):
            p = np.empty((m * m, 3))
            p[:, ax] = side
            p[:, (ax + 1) % 3], p[:, (ax + 2) % 3] = a, b
            out.append(p * np.asarray(scale))
    return np.concatenate(out)


def needle():
    """A thin tetrahedron from the origin to (1, 1, 1): its bounding box is the unit cube, of which it fills 0.24 %."""
    v = np.array([(0, 0, 0), (1, 1, 1), (0.12, 0, 0), (0, 0.12, 0)], dtype=F64)
    t = np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], dtype=np.int32)
    return v, np.ascontiguousarray(t[:, ::-1])  # each row reversed: the normals point outwards


# ---- the cases --------------------------------------------------------------------------------------------------------
# spacing as in surface_sampling_cases.  seeds: a function returning (n, 3) doubles.  horizon: darts to generate for the
# model (>= n_darts).  Measured n_points / n_darts (n_inside where it differs from n_darts) in the comments, from
# serial() with the oracle's inside test; Float32 and Float64 agree.
_PLAIN = dict(mesh=cube, spacing=("const", 0.15), factor=0.75, stall_limit=2000)
CASES = {
    "cube": dict(_PLAIN, horizon=40000),  # 512 / 36200
    "cube_stall200": dict(_PLAIN, stall_limit=200, horizon=4096),  # 399 / 3347
    # 6 x 8 x 8 seeds at the face cells' centres: 0.125 apart within a face (> r = 0.1125), 0.088 across a cube edge
    "cube_seeds": dict(_PLAIN, seeds=lambda: face_grid(8), horizon=24000),  # 274 / 19791
    "cube_bl": dict(_PLAIN, spacing=("bl", 0.08, 0.24, 1.0), horizon=36000),  # 582 / 30487, r from 0.068 to 0.176
    "cube_max1": dict(_PLAIN, max_points=1, horizon=64),  # 1 / 1
    "cube_max37": dict(_PLAIN, max_points=37, horizon=256),  # 37 / 40
    "cube_const10": dict(_PLAIN, spacing=("const", 10.0), stall_limit=50, horizon=64),  # 1 / 51
    # (ten darts round onto the faces of the far cube, where distance 0 is not inside)
    "cube_far": dict(_PLAIN, mesh=lambda: cube(shift=1000.0), horizon=40000, dtypes=[F32]),  # 512 / 36200, inside 36190
    # r = 0.1125 > the slab's thickness 0.05, and a seed within 0.075 of every point of it: nothing fits
    "slab_seeded": dict(_PLAIN, mesh=lambda: cube((1.0, 1.0, 0.05)), seeds=lambda: face_grid(10, (1.0, 1.0, 0.05), axes=(2,)),
                        horizon=2048),  # 0 / 2000
    "flat": dict(_PLAIN, mesh=flat_square, stall_limit=100, horizon=128),  # 0 / 100, inside 0
    # one seed, 0.05 outside the box: it still keeps darts away from its side of the cube
    "cube_seed_outside": dict(_PLAIN, seeds=lambda: np.array([(1.05, 0.5, 0.5)]), horizon=24000),  # 489 / 19568
    # a closed, non-convex surface that fills less than half of its box [-1, 1]^3
    "cavity": dict(mesh=lambda: _golden("cavity"), spacing=("const", 0.2), factor=0.75, stall_limit=2000, horizon=60000,
                   dtypes=[F32]),  # 718 / 57115, inside 25102
    # 46 786 triangles: stall_limit 200 keeps the oracle's brute-force inside test to ten thousand darts
    "box_stall200": dict(mesh=lambda: _golden("box"), spacing=("const", 2.5), factor=0.75, stall_limit=200, horizon=11000,
                         dtypes=[F32]),  # 1254 / 10167
}

# The stop scan works in tiles of 2048 positions and carries its counts from one chunk of 256 tiles to the next, so the
# carry matters from position 256 * 2048 + 2048 = 526 336 on: the needle's runs end beyond it.  2496 of the first 2^20
# darts are inside (7492 of 3 * 2^20); 557 of the 705 darts accepted among the first 2^20 lie before dart 528 384, and
# the longest miss run before it is 8928.  Float32 and Float64 agree in every number.
_NEEDLE = dict(mesh=needle, spacing=("const", 0.012), factor=1.0, horizon=1 << 20)
SCAN_CARRY_FROM = 257 * 2048
EDGE_CASES = {
    "needle": dict(_NEEDLE, max_points=618, stall_limit=1_000_000),  # 618 / 697597, inside 1677: tile 340
    "needle_stall": dict(_NEEDLE, stall_limit=8929),  # 571 / 560383, inside 1355: tile 273
    # batch = 0: the ninth batch is the first of 2^20 darts; from dart 4096 * 511 = 2 093 056 on, the tenth batch, doubling
    # again is what the library's clamp prevents
    "needle_clamp": dict(_NEEDLE, max_points=900, stall_limit=1_000_000, horizon=3 << 20),  # 900 / 2594928, inside 6135
}
CLAMPED_FROM = 4096 * 511


def case_of(name):
    return CASES[name] if name in CASES else EDGE_CASES[name]


def case_dtypes(name):
    return case_of(name).get("dtypes", DTYPES)


def max_points_of(case):
    return case.get("max_points", 10_000_000)


@functools.lru_cache(maxsize=None)
def mesh_of(name, dtype):
    v, t = case_of(name)["mesh"]()
    return np.ascontiguousarray(v.astype(dtype)), np.ascontiguousarray(t)


@functools.lru_cache(maxsize=None)
def seeds_of(name, dtype):
    """(seed positions (n, 3), their r) in `dtype`; n may be 0."""
    case = case_of(name)
    s = case["seeds"]() if "seeds" in case else np.zeros((0, 3))
    s = np.ascontiguousarray(s.astype(dtype))
    r = np.dtype(dtype).type(case["factor"]) * law_h(case["spacing"], s) if len(s) else np.zeros(0, dtype=dtype)
    for a in (s, r):
        a.setflags(write=False)
    return s, r


def library_spacing(wtp, name, dtype):
    """The case's spacing as the package takes it."""
    sp = case_of(name)["spacing"]
    if sp[0] == "const":
        return sp[1]
    if sp[0] == "bl":
        return wtp.BoundaryLayerSpacing(LAW_POINTS.astype(dtype), sp[1], sp[2], sp[3])
    return wtp.LogLike(LAW_POINTS.astype(dtype), sp[1], sp[2])


# ---- the model: darts -----------------------------------------------------------------------------------------------
def box_of(name, dtype):
    b = oracle.mesh_bbox(mesh_of(name, dtype)[0])
    return b[:3], b[3:]


def bbox_volume(name, dtype):
    lo, hi = (x.astype(F64) for x in box_of(name, dtype))
    return float(((hi[0] - lo[0]) * (hi[1] - lo[1])) * (hi[2] - lo[2]))


def positions(name, dtype, first, n, seed=SEED):
    lo, hi = box_of(name, dtype)
    with np.errstate(over="ignore"):
        j = np.arange(n, dtype=np.uint64) + np.uint64(first)
        base = (np.uint64(seed) << np.uint64(40)) + np.uint64(3) * j
        w = [_splitmix64(base + np.uint64(a)) for a in range(3)]
    u = [((x >> np.uint64(40)).astype(F32) * F32(1.0 / 16777216.0)).astype(dtype) for x in w]
    return np.ascontiguousarray(np.stack([lo[a] + u[a] * (hi[a] - lo[a]) for a in range(3)], axis=1))


def inside_of(name, dtype, xyz):
    v, t = mesh_of(name, dtype)
    return oracle.mesh_query(v, t, xyz)["inside"]


def darts(name, dtype, first, n, seed=SEED):
    """Darts first .. first + n - 1 of the case: (xyz (n, 3) dtype, inside bool, r dtype)."""
    case = case_of(name)
    xyz = positions(name, dtype, first, n, seed)
    r = np.dtype(dtype).type(case["factor"]) * law_h(case["spacing"], xyz)
    return xyz, inside_of(name, dtype, xyz), r


# ---- the model: the serial loop -------------------------------------------------------------------------------------
def serial(xyz, inside, r, sx, sr, max_points, stall_limit):
    """The run over the darts (xyz, inside, r) with seeds (sx, sr): (accepted dart indices int64, n_darts, stop_reason,
    n_inside).  Raises when the darts run out before the run ends."""
    n, ns = len(xyz), len(sx)
    ax, ar = np.empty((ns + n, 3), dtype=xyz.dtype), np.empty(ns + n, dtype=r.dtype)
    ax[:ns], ar[:ns] = sx, sr
    acc, misses, j, n_in = [], 0, 0, 0
    while True:
        if len(acc) >= max_points:
            return np.array(acc, dtype=np.int64), j, 2, n_in
        if misses >= stall_limit:
            return np.array(acc, dtype=np.int64), j, 1, n_in
        if j >= n:
            raise ValueError(f"the run needs more than {n} darts")
        k = ns + len(acc)
        n_in += int(inside[j])
        if not inside[j] or (k and _conflicts(ax[:k], ar[:k], xyz[j], r[j]).any()):
            misses += 1
        else:
            ax[k], ar[k] = xyz[j], r[j]
            acc.append(j)
            misses = 0
        j += 1


# ---- the model: the batch algorithm -----------------------------------------------------------------------------------
def batched_run(xyz, inside, r, sx, sr, max_points, stall_limit, batch):
    """The same run decided in batches of `batch` darts (0: the library's schedule): dict(acc, n_darts, stop_reason,
    n_inside, rounds_max, n_batches)."""
    n = len(xyz)
    acc = np.zeros(0, dtype=np.int64)
    misses, first, rounds_max, n_in, n_batches = 0, 0, 0, 0, 0
    for size in batch_sizes(batch):
        if first >= n:
            raise ValueError(f"the run needs more than {n} darts")
        B = min(size, n - first)
        bx, br, bi = xyz[first:first + B], r[first:first + B], inside[first:first + B]
        px, pr = np.concatenate([sx, xyz[acc]]), np.concatenate([sr, r[acc]])  # seeds first, then the accepted darts
        live = bi.copy()
        for i in np.nonzero(live)[0]:
            if len(px) and _conflicts(px, pr, bx[i], br[i]).any():
                live[i] = False
        ids = np.nonzero(live)[0]
        rows, cols = _lower_conflicts(bx[ids], br[ids])
        taken_by_rounds, rounds = jacobi_rounds(rows, cols, len(ids), B)
        n_batches, rounds_max = n_batches + 1, max(rounds_max, rounds)
        flag = np.zeros(B, dtype=bool)
        flag[ids[taken_by_rounds]] = True
        taken, new, reason = B, [], 0
        for i in range(B + 1):  # the stop scan, position B included; the counts it carries are of accepted darts alone
            if len(acc) + len(new) >= max_points:
                taken, reason = i, 2
                break
            if misses >= stall_limit:
                taken, reason = i, 1
                break
            if i == B:
                break
            if flag[i]:
                new.append(first + i)
                misses = 0
            else:
                misses += 1
        n_in += int(bi[:taken].sum())
        acc = np.concatenate([acc, np.array(new, dtype=np.int64)])
        if reason:
            return dict(acc=acc, n_darts=first + taken, stop_reason=reason, n_inside=n_in, rounds_max=rounds_max,
                        n_batches=n_batches)
        first += B


def batched(xyz, inside, r, sx, sr, max_points, stall_limit, batch):
    """batched_run() as (accepted, n_darts, stop_reason, n_inside, rounds_max)."""
    b = batched_run(xyz, inside, r, sx, sr, max_points, stall_limit, batch)
    return b["acc"], b["n_darts"], b["stop_reason"], b["n_inside"], b["rounds_max"]


@functools.lru_cache(maxsize=None)
def needle_darts(dtype):
    """The first 3 * 2^20 darts of the needle cases (they share mesh, spacing and stream), computed once."""
    out = darts("needle_clamp", dtype, 0, 3 << 20)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_run(name, dtype):
    """(xyz, inside, r of the case's horizon of darts, accepted, n_darts, stop_reason, n_inside) by serial(), once."""
    case = case_of(name)
    xyz, inside, r = (a[:case["horizon"]] for a in needle_darts(dtype)) if case["mesh"] is needle else \
        darts(name, dtype, 0, case["horizon"])
    sx, sr = seeds_of(name, dtype)
    acc, n_darts, reason, n_in = serial(xyz, inside, r, sx, sr, max_points_of(case), case["stall_limit"])
    for a in (xyz, inside, r, acc):
        a.setflags(write=False)
    return xyz, inside, r, acc, n_darts, reason, n_in
