"""Case table and numpy model of the surface sampler (include/wtp.h: wtp_mesh_sample, wtp_mesh_sample_darts).
Shared by test_surface_sampling_cases.py (no GPU: the batch algorithm equals the serial loop; every case has the
property it is there for) and test_gpu_surface_sampling.py (the device equals the model bit for bit).

The model, in the mesh's type T unless said otherwise:
  areas    per triangle in double from the corners converted to double, cum = their running sum, sequentially
  darts()  dart j of seed s: w_a = splitmix64((s << 40) + 3 j + a); triangle = first index with
           cum[t] >= ((w_0 >> 11) 2^-53) total_area, at most nt - 1 (double); u, v = T((w >> 40) 2^-24);
           su = sqrt(u); c = ((1 - su) v1 + (su (1 - v)) v2) + (su v) v3; r = T(factor) h(c)
  serial() darts in order; a dart is accepted iff ((dx dx + dy dy) + dz dz) < m m, m = min(r_p, r_q), holds for no
           accepted q; before each dart the run ends at max_points accepted (2) or stall_limit misses in a row (1)
  batched() the library's batch algorithm in plain Python: cull against the accepted set, Jacobi rounds over the
           batch's live darts, stop scan in dart order; reports the largest round count of a batch.  The library
           always decides a whole batch, so the round count is the library's when the model is given the darts of
           whole batches (whole_batches); batch = 0 is the library's own schedule (batch_sizes)

EDGE_CASES are the cases of test_gpu_sampler_edges.py: runs that end on a batch or tile seam of the stop scan, a batch
that needs more than one group of rounds, and meshes whose cell map is degenerate.  case_of() finds a case of either
table."""
from __future__ import annotations

import functools
import os

import numpy as np

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
SEED = 20260821 & 0xFFFFFF  # the stream key holds 24 bits of a seed (synth.SEED names the same stream)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- meshes -------------------------------------------------------------------------------------------------------
_CUBE_V = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], dtype=F64)
_CUBE_T = np.array([(1, 3, 2), (1, 4, 3), (5, 6, 7), (5, 7, 8), (1, 2, 6), (1, 6, 5), (3, 4, 8), (3, 8, 7), (1, 5, 8),
                    (1, 8, 4), (2, 3, 7), (2, 7, 6)], dtype=np.int32) - 1


def cube(scale=(1.0, 1.0, 1.0), shift=0.0):
    return _CUBE_V * np.asarray(scale, dtype=F64) + shift, _CUBE_T.copy()


def cube_with_zero_area_triangles():
    v, t = cube()
    flat = np.array([(0, 1, 1)], dtype=np.int32)  # two corners coincide: area 0, the running sum is flat there
    return v, np.concatenate([flat, t[:6], flat, t[6:]])


def plate(shift=0.0):
    """The unit square in the plane z = 0 as two triangles: a bounding box without height."""
    v = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], dtype=F64) + shift
    return v, np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int32)


def cube_stretched():
    """The cube and, behind its triangles, one of area 0 whose corners lie 3e5 away: it is never picked, and the box it
    stretches is so much longer than any r that the cell edge is the box's 1e-6 floor, 0.3."""
    v, t = cube()
    far = np.array([(3e5, 0, 0), (3e5, 1, 0)], dtype=F64)
    return np.concatenate([v, far]), np.concatenate([t, np.array([(8, 8, 9)], dtype=np.int32)])


def one_triangle():
    return np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], dtype=F64), np.array([(0, 1, 2)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _box():
    z = np.load(os.path.join(GOLD, "box_mesh.npz"))
    return z["vertices"].astype(F64), z["triangles"].astype(np.int32)


def box():
    return _box()


# the points the graded laws measure their distance to: a 3 x 3 grid on the plane z = -0.05, off the surface
LAW_POINTS = np.array([(x, y, -0.05) for x in (0.1, 0.5, 0.9) for y in (0.1, 0.5, 0.9)], dtype=F64)

# ---- the cases --------------------------------------------------------------------------------------------------------
# spacing: ("const", h) | ("bl", at_wall, bulk, layer_thickness) | ("loglike", base_size, growth_rate), the two laws over
# LAW_POINTS.  horizon: darts to generate for the model (>= n_darts).  Measured n_points / n_darts in the comments, from
# serial() (Float32 and Float64 agree).
CASES = {
    "cube_f075": dict(mesh=cube, spacing=("const", 0.15), factor=0.75, stall_limit=2000, horizon=20000),  # 299 / 17394
    "cube_f100": dict(mesh=cube, spacing=("const", 0.15), factor=1.0, stall_limit=2000, horizon=20000),  # 172 / 17129
    "one_triangle": dict(mesh=one_triangle, spacing=("const", 10.0), factor=0.75, stall_limit=50, horizon=64),  # 1 / 51
    "cube_max1": dict(mesh=cube, spacing=("const", 0.15), factor=0.75, stall_limit=2000, max_points=1, horizon=64),  # 1 / 1
    "cube_max37": dict(mesh=cube, spacing=("const", 0.15), factor=0.75, stall_limit=2000, max_points=37, horizon=256),  # 37 / 41
    "cube_stall3": dict(mesh=cube, spacing=("const", 0.15), factor=0.75, stall_limit=3, horizon=256),  # 70 / 89
    # r = 0.1125 > the slab's thickness 0.05: opposite faces block each other
    "slab": dict(mesh=lambda: cube((1.0, 1.0, 0.05)), spacing=("const", 0.15), factor=0.75, stall_limit=2000,
                 horizon=14000),  # 75 / 11020
    "graded_bl": dict(mesh=cube, spacing=("bl", 0.08, 0.24, 1.0), factor=0.75, stall_limit=2000,
                      horizon=22000),  # 339 / 18884, r from 0.068 to 0.176
    "graded_loglike": dict(mesh=cube, spacing=("loglike", 0.3, 1.5), factor=0.75, stall_limit=2000,
                           horizon=14000),  # 183 / 10982, r from 0.058 to 0.197
    "cube_far": dict(mesh=lambda: cube(shift=1000.0), spacing=("const", 0.15), factor=0.75, stall_limit=2000, horizon=20000,
                     dtypes=[F32]),  # 298 / 17394
    "cube_zero_area": dict(mesh=cube_with_zero_area_triangles, spacing=("const", 0.15), factor=0.75, stall_limit=2000,
                           horizon=20000),  # 299 / 17394
    "box": dict(mesh=box, spacing=("const", 1.8), factor=0.75, stall_limit=2000, horizon=48000),  # 1253 / 41922
}

# Measured with serial() / batched(); Float32 and Float64 agree wherever both run.
EDGE_CASES = {
    # r = 0.02: dart 2047 is accepted as sample 1686 and dart 4095 as sample 2849, so max_points = 1686 / 2849 end the
    # run at n_darts = 2048 / 4096, the seams of the stop scan's tiles of 2048 positions.  The seed was searched for that.
    "cube_fine": dict(mesh=cube, spacing=("const", 0.02), factor=1.0, stall_limit=2000, max_points=2849, seed=3483607,
                      horizon=8192),  # 2849 / 4096
    # a batch of 16384 darts at r = 0.05 needs more rounds than the library runs in one group (8): 10 for the first batch.
    # 1339 samples come from the first batch and sample 1400 is dart 25875, so max_points = 1380 ends the run inside the
    # second batch
    "cube_r005": dict(mesh=cube, spacing=("const", 0.05), factor=1.0, stall_limit=2000, max_points=1380, batch=16384,
                      horizon=32768, dtypes=[F32]),  # 1380 / 22422, rounds_max 10
    # a box without height: one layer of cells (nc[2] = 1)
    "plate": dict(mesh=plate, spacing=("const", 0.05), factor=0.75, stall_limit=2000, horizon=16384),  # 469 / 14960
    "plate_far": dict(mesh=lambda: plate(1000.0), spacing=("const", 0.05), factor=0.75, stall_limit=2000, horizon=16384,
                      dtypes=[F32]),  # 469 / 14960
    # cube_f075's darts in a box of 3e5: ext / 1e6 = 0.3 > r = 0.1125 sets the cell edge
    "cube_stretched": dict(mesh=cube_stretched, spacing=("const", 0.15), factor=0.75, stall_limit=2000,
                           horizon=20000),  # 299 / 17394
}


def case_of(name):
    return CASES[name] if name in CASES else EDGE_CASES[name]


def case_dtypes(name):
    return case_of(name).get("dtypes", DTYPES)


def seed_of(case):
    return case.get("seed", SEED)


def max_points_of(case):
    return case.get("max_points", 10_000_000)


@functools.lru_cache(maxsize=None)
def mesh_of(name, dtype):
    v, t = case_of(name)["mesh"]()
    return np.ascontiguousarray(v.astype(dtype)), np.ascontiguousarray(t)


def library_spacing(wtp, name, dtype):
    """The case's spacing as the package takes it."""
    sp = case_of(name)["spacing"]
    if sp[0] == "const":
        return sp[1]
    if sp[0] == "bl":
        return wtp.BoundaryLayerSpacing(LAW_POINTS.astype(dtype), sp[1], sp[2], sp[3])
    return wtp.LogLike(LAW_POINTS.astype(dtype), sp[1], sp[2])


# ---- the model: darts -----------------------------------------------------------------------------------------------
def _splitmix64(z):
    z = (z + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


@functools.lru_cache(maxsize=None)
def areas_of(name, dtype):
    """(cum, total_area) in double, from the corners of the mesh in `dtype`."""
    v, t = mesh_of(name, dtype)
    c = v.astype(F64)[t]
    e, g = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    cx = e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1]
    cy = e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2]
    cz = e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]
    area = np.sqrt((cx * cx + cy * cy) + cz * cz) / 2
    cum = np.empty(len(area), dtype=F64)
    run = 0.0
    for i, a in enumerate(area):  # sequential addition
        run = run + float(a)
        cum[i] = run
    return cum, float(cum[-1])


def law_h(sp, c):
    """The spacing law at positions c, term by term in c's dtype (csrc/wtp_spacing.hip spacing_law)."""
    T = c.dtype.type
    if sp[0] == "const":
        return np.full(len(c), T(sp[1]), dtype=c.dtype)
    b = LAW_POINTS.astype(c.dtype)
    d2 = None
    for q in b:  # nearest law point under ((dx dx + dy dy) + dz dz)
        dx, dy, dz = c[:, 0] - q[0], c[:, 1] - q[1], c[:, 2] - q[2]
        e = (dx * dx + dy * dy) + dz * dz
        d2 = e if d2 is None else np.minimum(d2, e)
    d = np.sqrt(d2)
    if sp[0] == "loglike":
        p0, p1 = T(sp[1]), T(sp[2])
        a = p0 * (T(1) - (p1 - T(1)))
        return p0 * d / (a + d)
    p0, p1, p2 = T(sp[1]), T(sp[2]), T(sp[3])
    center, width = p2 / T(2), p2 / T(6)
    sig = T(1) / (T(1) + np.exp(-(d - center) / width))
    return p0 + (p1 - p0) * sig


def darts(name, dtype, first, n, seed=None):
    """Darts first .. first + n - 1 of the case (seed: the case's own unless given): (xyz (n, 3) dtype, tri int32, r dtype)."""
    case = case_of(name)
    seed = seed_of(case) if seed is None else seed
    T = np.dtype(dtype).type
    v, t = mesh_of(name, dtype)
    cum, total = areas_of(name, dtype)
    with np.errstate(over="ignore"):
        j = np.arange(n, dtype=np.uint64) + np.uint64(first)
        base = (np.uint64(seed) << np.uint64(40)) + np.uint64(3) * j
        w0, w1, w2 = _splitmix64(base), _splitmix64(base + np.uint64(1)), _splitmix64(base + np.uint64(2))
    x = ((w0 >> np.uint64(11)).astype(F64) * 2.0 ** -53) * total
    tri = np.minimum(np.searchsorted(cum, x, side="left"), len(cum) - 1).astype(np.int32)
    u = ((w1 >> np.uint64(40)).astype(F32) * F32(1.0 / 16777216.0)).astype(dtype)
    w = ((w2 >> np.uint64(40)).astype(F32) * F32(1.0 / 16777216.0)).astype(dtype)
    su = np.sqrt(u)
    a, b, c = (T(1) - su)[:, None], (su * (T(1) - w))[:, None], (su * w)[:, None]
    k = v[t[tri]]
    xyz = (a * k[:, 0] + b * k[:, 1]) + c * k[:, 2]
    r = T(case["factor"]) * law_h(case["spacing"], xyz)
    return np.ascontiguousarray(xyz), tri, r


# ---- the model: the serial loop -------------------------------------------------------------------------------------
def _conflicts(xyz, r, p, rp):
    """bool per row of (xyz, r): in conflict with the dart (p, rp), in the arrays' own type"""
    dx, dy, dz = xyz[:, 0] - p[0], xyz[:, 1] - p[1], xyz[:, 2] - p[2]
    m = np.minimum(r, rp)
    return ((dx * dx + dy * dy) + dz * dz) < m * m


def serial(xyz, r, max_points, stall_limit):
    """The run over the darts (xyz, r): (accepted dart indices int64, n_darts, stop_reason).  Raises when the darts
    run out before the run ends."""
    n = len(xyz)
    ax, ar = np.empty_like(xyz), np.empty_like(r)
    acc, misses, j = [], 0, 0
    while True:
        if len(acc) >= max_points:
            return np.array(acc, dtype=np.int64), j, 2
        if misses >= stall_limit:
            return np.array(acc, dtype=np.int64), j, 1
        if j >= n:
            raise ValueError(f"the run needs more than {n} darts")
        k = len(acc)
        if k and _conflicts(ax[:k], ar[:k], xyz[j], r[j]).any():
            misses += 1
        else:
            ax[k], ar[k] = xyz[j], r[j]
            acc.append(j)
            misses = 0
        j += 1


# ---- the model: the batch algorithm -----------------------------------------------------------------------------------
def _lower_conflicts(xyz, r):
    """(rows, cols): every pair cols < rows of darts in conflict"""
    n = len(xyz)
    rows, cols = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for lo in range(0, n, 256):
        hi = min(lo + 256, n)
        p, rp = xyz[lo:hi], r[lo:hi]
        q, rq = xyz[:hi], r[:hi]
        d2 = None
        for c in range(3):
            d = p[:, None, c] - q[None, :, c]
            d2 = d * d if d2 is None else d2 + d * d
        m = np.minimum(rp[:, None], rq[None, :])
        hit = d2 < m * m
        a, b = np.nonzero(hit)
        keep = b < a + lo
        rows.append(a[keep] + lo)
        cols.append(b[keep])
    return np.concatenate(rows), np.concatenate(cols)


BATCH_FIRST, BATCH_MAX = 4096, 1 << 20  # batch = 0: the library doubles its batches from / up to these


def batch_sizes(batch):
    """The sizes of a run's batches, without end: `batch` every time, or the library's own schedule at batch = 0."""
    B = batch if batch > 0 else BATCH_FIRST
    while True:
        yield B
        if batch == 0:
            B = min(2 * B, BATCH_MAX)


def whole_batches(n_darts, batch):
    """(n_batches, darts in them) of a run of n_darts darts: a run that ends at position B of a batch ends in that batch."""
    k = total = 0
    for B in batch_sizes(batch):
        k, total = k + 1, total + B
        if total >= n_darts:
            return k, total


def jacobi_rounds(rows, cols, n, B):
    """The rounds over n live darts with the conflict pairs cols < rows: (accepted bool (n,), rounds).  0 undecided,
    1 accepted, 2 rejected; a round reads the states the previous one left."""
    st = np.zeros(n, dtype=np.int8)
    rounds = 0
    while True:
        rounds += 1
        prev = st[cols]
        by_acc = np.bincount(rows[prev == 1], minlength=n) > 0
        pending = np.bincount(rows[prev == 0], minlength=n) > 0
        und = st == 0
        st[und & by_acc] = 2
        st[und & ~by_acc & ~pending] = 1
        if not (st == 0).any():
            return st == 1, rounds
        if rounds > B:
            raise AssertionError("a batch needs at most as many rounds as it has darts")


def batched_run(xyz, r, max_points, stall_limit, batch):
    """The same run decided in batches of `batch` darts (0: the library's schedule): dict(acc, n_darts, stop_reason,
    rounds_max, n_batches)."""
    n = len(xyz)
    acc = np.zeros(0, dtype=np.int64)
    misses, first, rounds_max, n_batches = 0, 0, 0, 0
    for size in batch_sizes(batch):
        if first >= n:
            raise ValueError(f"the run needs more than {n} darts")
        B = min(size, n - first)  # (a short last batch only when the darts run out: the run must end inside it)
        bx, br = xyz[first:first + B], r[first:first + B]
        # cull against the accepted set
        live = np.ones(B, dtype=bool)
        ax, ar = xyz[acc], r[acc]
        for i in range(B if len(acc) else 0):
            if _conflicts(ax, ar, bx[i], br[i]).any():
                live[i] = False
        ids = np.nonzero(live)[0]
        rows, cols = _lower_conflicts(bx[ids], br[ids])
        taken_by_rounds, rounds = jacobi_rounds(rows, cols, len(ids), B)
        n_batches, rounds_max = n_batches + 1, max(rounds_max, rounds)
        flag = np.zeros(B, dtype=bool)
        flag[ids[taken_by_rounds]] = True
        # stop scan in dart order, position B included
        taken, new, reason = B, [], 0
        for i in range(B + 1):
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
        acc = np.concatenate([acc, np.array(new, dtype=np.int64)])
        if reason:
            return dict(acc=acc, n_darts=first + taken, stop_reason=reason, rounds_max=rounds_max, n_batches=n_batches)
        first += B


def batched(xyz, r, max_points, stall_limit, batch):
    """batched_run() as (accepted, n_darts, stop_reason, rounds_max)."""
    b = batched_run(xyz, r, max_points, stall_limit, batch)
    return b["acc"], b["n_darts"], b["stop_reason"], b["rounds_max"]


@functools.lru_cache(maxsize=None)
def model_run(name, dtype):
    """(xyz, tri, r of the case's horizon of darts, accepted, n_darts, stop_reason) by serial(), computed once."""
    case = case_of(name)
    xyz, tri, r = darts(name, dtype, 0, case["horizon"])
    acc, n_darts, reason = serial(xyz, r, max_points_of(case), case["stall_limit"])
    for a in (xyz, tri, r, acc):
        a.setflags(write=False)
    return xyz, tri, r, acc, n_darts, reason
