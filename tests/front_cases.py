"""Case table and numpy model of the advancing front (include/wtp.h: wtp_mesh_front, wtp_mesh_front_candidates).
Shared by test_front_cases.py (no GPU: the batch algorithm equals the serial loop; every case has the property it is
there for) and test_gpu_front.py (the device equals the model).

The model, in the mesh's type T:
  directions()  candidate j of seed k: w_a = splitmix64((k << 40) + 2 j + a), u, v = T(float32(w_a >> 40) 2^-24);
                z = 2 u - 1, rho = sqrt(1 - z z); t = 8 v, o = floor(t), f = t - o, g = (o odd) ? 1 - f : f,
                theta = g T(pi / 4), x = theta theta, s = theta (1 + x (S_1 + ... + x S_9)), c = 1 + x (C_1 + ... + x C_9)
                (Horner), (cos, sin) by octant; d = (rho cos, rho sin, z)
  candidates()  of parents (positions, h): c_a = x_{q,a} + h_q d_a, r = h_q, inside = oracle.mesh_query(...)["inside"]
  serial()      parents in queue order, candidates in s order; before each candidate the run ends at max_points accepted
                (2); a candidate is accepted iff it is inside and ((dx dx + dy dy) + dz dz) < r r holds for no queue
                entry but its own parent; the run ends (1) when every entry has been expanded
  batched()     the library's batch algorithm in plain Python: the candidates of a range of parents that were all in the
                queue when the batch began; those outside the mesh or in conflict with a queue entry (the parent
                exempt) are culled, Jacobi rounds over the rest under the one-sided rule, stop scan in candidate order
Both loops take the candidates from a function of (first parent, parent positions), so that the same code replays a run
over the candidates the library returned."""
from __future__ import annotations

import functools
import math
import os

import numpy as np

import oracle
from surface_sampling_cases import F32, F64, DTYPES, SEED, GOLD, LAW_POINTS, _splitmix64, cube, law_h
from volume_fill_cases import face_grid


@functools.lru_cache(maxsize=None)
def _golden(stem):
    z = np.load(os.path.join(GOLD, f"{stem}_mesh.npz"))
    return z["vertices"].astype(F64), z["triangles"].astype(np.int32)


def _box_centres():
    v, t = _golden("box")
    return v[t].mean(axis=1)[::40]  # PointBoundary(mesh) has one point per face: thinned to 1170, about 1.8 apart


_CENTRE = lambda: np.array([(0.5, 0.5, 0.5)])  # noqa: E731

# ---- the cases --------------------------------------------------------------------------------------------------------
# spacing as in surface_sampling_cases; seeds: a function returning (m, 3) doubles; n: candidates per parent.  Measured
# n_points / n_parents / n_candidates in the comments, from serial() with the oracle's inside test (Float32 and Float64
# agree unless both are given).
_PLAIN = dict(mesh=cube, spacing=("const", 0.15), n=10, seeds=lambda: face_grid(8))
CASES = {
    "grid8": dict(_PLAIN),  # 103 / 487 / 4870, 6 batches of all parents available
    "grid12": dict(_PLAIN, spacing=("const", 0.09), seeds=lambda: face_grid(12)),  # 663 / 1527 / 15270, 8 batches
    # one or two queue entries are fewer points than the ball touches cells: the cull's linear scan, where the parent's
    # exemption decides everything (so do seed_outside and coincident)
    "centre": dict(_PLAIN, seeds=_CENTRE),  # 234 / 235 / 2350 over 12 generations; a first batch of 10 candidates
    "centre_n1": dict(_PLAIN, seeds=_CENTRE, n=1),  # 1 / 2 / 2
    # graded 0.06 -> 0.18 away from the plane z = -0.05: a point may sit within its neighbour's h, not within its own r
    "grid12_bl": dict(_PLAIN, spacing=("bl", 0.06, 0.18, 1.0), seeds=lambda: face_grid(12)),  # 377 / 1241 / 12410
    "grid8_max1": dict(_PLAIN, max_points=1),  # 1 / 10 / 100
    "grid8_max37": dict(_PLAIN, max_points=37),  # 37 / 299 / 2986
    # every candidate is outside: no point, one batch, every seed expanded
    "grid8_h10": dict(_PLAIN, spacing=("const", 10.0)),  # 0 / 384 / 3840
    # cells and differences far from the origin, in Float32
    "far": dict(_PLAIN, mesh=lambda: cube(shift=1000.0), seeds=lambda: face_grid(8) + 1000.0, dtypes=[F32]),  # 103 / 487 / 4870
    # a closed, non-convex surface, seeded from every 7th face centre: 42 % of the candidates are outside
    "cavity": dict(mesh=lambda: _golden("cavity"), spacing=("const", 0.2), n=10,
                   seeds=lambda: _golden("cavity")[0][_golden("cavity")[1]].mean(axis=1)[::7], dtypes=[F32]),  # 121 / 752 / 7520
    # the reference's own item (test/discretization.jl:21-35) on every 40th face centre of the 25^3 box: 50 points end
    # the first batch, which keeps the oracle's brute-force inside test (46 786 triangles) to a few hundred candidates
    "box_max50": dict(mesh=lambda: _golden("box"), spacing=("const", 2.5), n=10, seeds=_box_centres, max_points=50),  # 50 / 308 / 3071
    # one seed, 0.05 outside the cube: the candidates it throws inwards start the front
    "seed_outside": dict(_PLAIN, seeds=lambda: np.array([(1.05, 0.5, 0.5)])),  # 230 / 231 / 2310
    # each of two coincident seeds kills the other's candidates (distance h (1 +- eps) from both), not its own
    "coincident": dict(_PLAIN, seeds=lambda: np.array([(0.5, 0.5, 0.5), (0.5, 0.5, 0.5)])),  # f32 231 / 233 / 2330, f64 216 / 218 / 2180
}
# candidate batches of 63, 64 and 65: (n, parents per batch), run on the grid8 seeds
ODD_BATCHES = [(9, 7), (8, 8), (13, 5)]


def case_dtypes(name):
    return CASES[name].get("dtypes", DTYPES)


def max_points_of(case):
    return case.get("max_points", 10_000_000)


@functools.lru_cache(maxsize=None)
def mesh_of(name, dtype):
    v, t = CASES[name]["mesh"]()
    return np.ascontiguousarray(v.astype(dtype)), np.ascontiguousarray(t)


@functools.lru_cache(maxsize=None)
def seeds_of(name, dtype):
    s = np.ascontiguousarray(CASES[name]["seeds"]().astype(dtype))
    s.setflags(write=False)
    return s


def library_spacing(wtp, name, dtype):
    """The case's spacing as the package takes it."""
    sp = CASES[name]["spacing"]
    if sp[0] == "const":
        return sp[1]
    if sp[0] == "bl":
        return wtp.BoundaryLayerSpacing(LAW_POINTS.astype(dtype), sp[1], sp[2], sp[3])
    return wtp.LogLike(LAW_POINTS.astype(dtype), sp[1], sp[2])


# ---- the model: candidates --------------------------------------------------------------------------------------------
def _coefficients(dtype):
    T = np.dtype(dtype).type
    S = [T((-1.0) ** k / math.factorial(2 * k + 1)) for k in range(1, 10)]  # n! is exact in double up to 19!
    C = [T((-1.0) ** k / math.factorial(2 * k)) for k in range(1, 10)]
    return S, C


def cos_sin(v, dtype):
    """(cos, sin) of the azimuth 2 pi v as the contract computes them, v in [0, 1) of `dtype`."""
    T = np.dtype(dtype).type
    S, C = _coefficients(dtype)
    t = T(8) * v
    o = np.floor(t)
    f = t - o
    o = o.astype(np.int64)
    g = np.where(o & 1, T(1) - f, f)
    th = g * T(np.pi / 4)
    x = th * th
    a_s, a_c = np.full_like(x, S[8]), np.full_like(x, C[8])
    for k in range(7, -1, -1):
        a_s, a_c = S[k] + x * a_s, C[k] + x * a_c
    s = th * (T(1) + x * a_s)
    c = T(1) + x * a_c
    cl = np.choose(o, [c, s, -s, -c, -c, -s, s, c])
    sl = np.choose(o, [s, c, c, s, -s, -c, -c, -s])
    return cl, sl


def uv(first, m, dtype, seed=SEED):
    """(u, v) of candidates first .. first + m - 1."""
    with np.errstate(over="ignore"):
        j = np.arange(m, dtype=np.uint64) + np.uint64(first)
        base = (np.uint64(seed) << np.uint64(40)) + np.uint64(2) * j
        w0, w1 = _splitmix64(base), _splitmix64(base + np.uint64(1))
    return tuple(((w >> np.uint64(40)).astype(F32) * F32(1.0 / 16777216.0)).astype(dtype) for w in (w0, w1))


def directions(first, m, dtype, seed=SEED):
    """d of candidates first .. first + m - 1: (m, 3) of `dtype`."""
    T = np.dtype(dtype).type
    u, v = uv(first, m, dtype, seed)
    z = T(2) * u - T(1)
    rho = np.sqrt(T(1) - z * z)
    cl, sl = cos_sin(v, dtype)
    return np.stack([rho * cl, rho * sl, z], axis=1)


@functools.lru_cache(maxsize=None)
def _inside_parts(name, dtype):
    """What oracle.mesh_query derives from the mesh alone (pseudonormals, box), once per case: a serial run asks in
    hundreds of small pieces."""
    v, t = mesh_of(name, dtype)
    return oracle.mesh_pseudonormals(v, t), oracle.mesh_bbox(v)


def inside_of(name, dtype, xyz):
    """oracle.mesh_query(...)["inside"] with the per-mesh part cached: the same two library calls on the same inputs."""
    import ctypes as C

    v, t = mesh_of(name, dtype)
    pn, bbox = _inside_parts(name, dtype)
    pts = np.ascontiguousarray(np.atleast_2d(xyz), dtype=v.dtype)
    n, L, suf, P = len(pts), oracle.lib(), oracle._suf(v.dtype), oracle._p
    d2, tri, cp, feat = np.empty(n, v.dtype), np.empty(n, np.int32), np.empty((n, 3), v.dtype), np.empty(n, np.int32)
    getattr(L, f"wtpo_mesh_nearest_{suf}")(P(v), P(t), C.c_int64(len(t)), P(pts), C.c_int64(n), P(d2), P(tri), P(cp), P(feat))
    sd, inside, proj = np.empty(n, v.dtype), np.empty(n, np.uint8), np.empty((n, 3), v.dtype)
    ct = C.c_float if v.dtype == np.float32 else C.c_double
    getattr(L, f"wtpo_mesh_classify_{suf}")(P(pts), C.c_int64(n), P(d2), P(tri), P(cp), P(feat), P(pn), P(bbox), ct(0.0),
                                            P(sd), P(inside), P(proj))
    return inside.astype(bool)


def candidates(name, dtype, parents, h, first_parent, n, seed=SEED):
    """The n candidates each of the parents (positions (m, 3), h (m,)), parent p being queue entry first_parent + p:
    (xyz (m n, 3), inside bool, r)."""
    m = len(parents)
    d = directions(first_parent * n, m * n, dtype, seed)
    hq = np.repeat(h, n)
    xyz = np.repeat(parents, n, axis=0) + hq[:, None] * d
    return np.ascontiguousarray(xyz), inside_of(name, dtype, xyz), hq


def model_source(name, dtype, n=None, seed=SEED):
    """cand_fn of the case for serial() / batched(): the model's own candidates, h by the law in numpy."""
    case = CASES[name]
    n = case["n"] if n is None else n

    def cand_fn(q0, parents):
        return candidates(name, dtype, parents, law_h(case["spacing"], parents), q0, n, seed)

    return cand_fn


def array_source(xyz, inside, r, n):
    """cand_fn over candidate arrays that start at parent 0 (the library's own, read out in one call)."""
    def cand_fn(q0, parents):
        a, b = q0 * n, (q0 + len(parents)) * n  # (a loop may ask ahead of the parents it goes on to expand)
        return xyz[a:b], inside[a:b], r[a:b]

    return cand_fn


# ---- the model: the serial loop -------------------------------------------------------------------------------------
def _hits(q, p, r):
    """bool per row of q: within r of the candidate p under the library's expression, in the arrays' own type"""
    dx, dy, dz = p[0] - q[:, 0], p[1] - q[:, 1], p[2] - q[:, 2]
    return ((dx * dx + dy * dy) + dz * dz) < r * r


def _result(acc, n, n_cand, n_in, reason, queue, **more):
    acc = np.array(acc, dtype=np.int64)
    return dict(cand=acc, parent=(acc // n).astype(np.int32), n_parents=-(-n_cand // n), n_candidates=n_cand, n_inside=n_in,
                stop_reason=reason, queue=queue, **more)


def serial(seeds, n, max_points, cand_fn):
    """The run from `seeds`: dict(cand, parent, n_parents, n_candidates, n_inside, stop_reason, queue = the positions of
    the seeds and the accepted points)."""
    ns = len(seeds)
    cap = ns + 64
    queue = np.empty((cap, 3), dtype=seeds.dtype)
    queue[:ns] = seeds
    k, acc, n_cand, n_in, q = ns, [], 0, 0, 0
    got0, got1 = 0, 0  # the parents whose candidates are at hand (they depend on nothing accepted after the parent)
    while q < k:
        if q >= got1:
            got0, got1 = q, min(k, q + 64)
            gx, gi, gr = cand_fn(got0, queue[got0:got1])
        o = (q - got0) * n
        cx, ci, cr = gx[o:o + n], gi[o:o + n], gr[o:o + n]
        for s in range(n):
            if len(acc) >= max_points:
                return _result(acc, n, n_cand, n_in, 2, queue[:k].copy())
            if s >= len(cx):
                raise ValueError("the run expands more parents than candidates were given")
            n_cand += 1
            n_in += int(ci[s])
            if not ci[s]:
                continue
            hit = _hits(queue[:k], cx[s], cr[s])
            hit[q] = False  # never against its own parent
            if hit.any():
                continue
            if k == cap:
                cap *= 2
                queue = np.concatenate([queue, np.empty_like(queue)])
            queue[k] = cx[s]
            k += 1
            acc.append(q * n + s)
        q += 1
    return _result(acc, n, n_cand, n_in, 1, queue[:k].copy())


# ---- the model: the batch algorithm -----------------------------------------------------------------------------------
def _lower_hits(xyz, r):
    """(rows, cols): every pair cols < rows with candidate cols within r[rows] of candidate rows"""
    n = len(xyz)
    rows, cols = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for lo in range(0, n, 256):
        hi = min(lo + 256, n)
        p, rp, q = xyz[lo:hi], r[lo:hi], xyz[:hi]
        d2 = None
        for c in range(3):
            d = p[:, None, c] - q[None, :, c]
            d2 = d * d if d2 is None else d2 + d * d
        a, b = np.nonzero(d2 < (rp * rp)[:, None])
        keep = b < a + lo
        rows.append(a[keep] + lo)
        cols.append(b[keep])
    return np.concatenate(rows), np.concatenate(cols)


def batched(seeds, n, max_points, cand_fn, batch):
    """The same run decided in batches of `batch` parents (0: every parent available): serial()'s dict with n_batches and
    rounds_max added."""
    queue = seeds.copy()
    acc, n_cand, n_in, q0, n_batches, rounds_max = [], 0, 0, 0, 0, 0
    while q0 < len(queue):
        q1 = len(queue) if batch == 0 else min(len(queue), q0 + batch)
        bx, bi, br = cand_fn(q0, queue[q0:q1])
        B = len(bx)
        if B < (q1 - q0) * n:
            raise ValueError("the run expands more parents than candidates were given")
        live = bi.copy()
        for i in np.nonzero(live)[0]:  # the cull, the parent exempt
            hit = _hits(queue, bx[i], br[i])
            hit[q0 + i // n] = False
            live[i] = not hit.any()
        ids = np.nonzero(live)[0]
        rows, cols = _lower_hits(bx[ids], br[ids])
        st = np.zeros(len(ids), dtype=np.int8)  # 0 undecided, 1 accepted, 2 rejected
        rounds = 0
        while True:
            rounds += 1
            prev = st[cols]
            by_acc = np.bincount(rows[prev == 1], minlength=len(ids)) > 0
            pending = np.bincount(rows[prev == 0], minlength=len(ids)) > 0
            und = st == 0
            st[und & by_acc] = 2
            st[und & ~by_acc & ~pending] = 1
            if not (st == 0).any():
                break
            if rounds > B:
                raise AssertionError("a batch needs at most as many rounds as it has candidates")
        n_batches, rounds_max = n_batches + 1, max(rounds_max, rounds)
        flag = np.zeros(B, dtype=bool)
        flag[ids[st == 1]] = True
        taken, new, ended = B, [], False
        for i in range(B + 1):  # the stop scan, position B included
            if len(acc) + len(new) >= max_points:
                taken, ended = i, True
                break
            if i == B:
                break
            if flag[i]:
                new.append(i)
        n_cand = q0 * n + taken
        n_in += int(bi[:taken].sum())
        acc += [q0 * n + i for i in new]
        queue = np.concatenate([queue, bx[new]]) if new else queue
        if ended:
            return _result(acc, n, n_cand, n_in, 2, queue, n_batches=n_batches, rounds_max=rounds_max)
        q0 = q1
    return _result(acc, n, n_cand, n_in, 1, queue, n_batches=n_batches, rounds_max=rounds_max)


@functools.lru_cache(maxsize=None)
def model_run(name, dtype):
    """serial() of the case over the model's own candidates, computed once."""
    case = CASES[name]
    out = serial(seeds_of(name, dtype), case["n"], max_points_of(case), model_source(name, dtype))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
