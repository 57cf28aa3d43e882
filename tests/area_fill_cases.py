"""Case table and numpy model of the area fill (include/wtp.h: wtp_loops_fill, wtp_loops_fill_darts).  Shared by
test_area_fill_cases.py (no GPU: the batch algorithm equals the serial loop; every case has the property it is there
for) and test_gpu_area_fill.py (the device equals the model).

The model, in the index's type T:
  darts()   dart j of seed s: w_a = splitmix64((s << 40) + 3 j + a), u_a = T(float32(w_a >> 40) 2^-24), a = 0, 1,
            c_a = lo_a + u_a (hi_a - lo_a) over the index's box (loops_cases.build), r = T(factor) h(c),
            inside = loops_cases.query(...)["inside"] (brute-force nearest segment, pseudonormal side, box)
  serial()  darts in order; a dart is accepted iff it is inside and (dx dx + dy dy) < m m, m = min(r_p, r_q), holds
            for no seed and no accepted q; before each dart the run ends at max_points accepted (2) or stall_limit misses
            in a row (1); seeds are never tested against each other and never returned
  batched() the library's batch algorithm in plain Python, as volume_fill_cases.batched_run in two columns"""
from __future__ import annotations

import functools

import numpy as np

import loops_cases as LC
from surface_sampling_cases import F32, F64, DTYPES, SEED, _splitmix64, law_h, jacobi_rounds, batch_sizes
from surface_sampling_cases import whole_batches  # noqa: F401


# ---- the cases --------------------------------------------------------------------------------------------------------
# loops: a function returning a list of (n, 2) double arrays.  spacing: ("const", h) | ("bl", at_wall, bulk,
# layer_thickness) over the case's own law points (`law`, a function returning (m, 2) doubles).  seeds: a function
# returning (n, 2) doubles.  horizon: darts to generate for the model (>= n_darts).  n_points / n_darts, inside in the
# comments are serial()'s over the model's darts; Float32 and Float64 agree unless said otherwise.
def _annulus():
    return [LC.polygon(48, 2.0), LC.polygon(24, 0.8)]


_SQ = dict(loops=lambda: [LC.square()], spacing=("const", 0.05), factor=0.75, stall_limit=2000)
CASES = {
    "square": dict(_SQ, horizon=24000),  # 476 / 20590, every dart inside
    "star": dict(loops=lambda: [LC.star()], spacing=("const", 0.08), factor=0.75, stall_limit=2000, seeds=LC.star,
                 horizon=32000),  # 512 / 28872, inside 15934
    "annulus": dict(loops=_annulus, spacing=("const", 0.15), factor=0.75, stall_limit=2000,
                    seeds=lambda: np.concatenate(_annulus()), horizon=26000),  # 475 / 21502, inside 14152
    "annulus_rev": dict(loops=lambda: [_annulus()[0], _annulus()[1][::-1]], spacing=("const", 0.15), factor=0.75,
                        stall_limit=2000, seeds=lambda: np.concatenate(_annulus()), horizon=26000),  # the same bytes
    "wedge": dict(loops=lambda: [LC.WEDGE], spacing=("const", 0.02), factor=0.75, stall_limit=2000,
                  horizon=16000),  # 165 / 13894, inside 6883
    # five darts round onto the far square's edges, where distance 0 is not inside
    "square_far": dict(_SQ, loops=lambda: [LC.square(1000.0)], horizon=24000, dtypes=[F32]),  # 475 / 20590, inside 20585
    "circle_bl": dict(loops=lambda: [LC.polygon(64)], spacing=("bl", 0.03, 0.12, 0.3), law=lambda: LC.polygon(64),
                      factor=0.75, stall_limit=2000, horizon=42000),  # 724 / 38250, inside 30040; r from 0.0258 to 0.0900
    "square_max1": dict(_SQ, max_points=1, horizon=64),  # 1 / 1
    "square_max37": dict(_SQ, max_points=37, horizon=256),  # 37 / 37
    "square_stall200": dict(_SQ, stall_limit=200, horizon=4096),  # 413 / 3659
    "square_h10": dict(_SQ, spacing=("const", 10.0), stall_limit=50, horizon=64),  # 1 / 51
    # one seed, 0.01 outside the box: it still keeps darts away from its side of the square
    "seed_outside": dict(_SQ, seeds=lambda: np.array([(1.01, 0.25)]), horizon=24000),  # 474 / 20590
    # a triangle that fills 2.5 % of its box
    "sliver": dict(loops=lambda: [LC.SLIVER], spacing=("const", 0.02), factor=0.75, stall_limit=2000,
                   horizon=24000),  # 86 / 19236, inside 475
}


def case_dtypes(name):
    return CASES[name].get("dtypes", DTYPES)


def max_points_of(case):
    return case.get("max_points", 10_000_000)


@functools.lru_cache(maxsize=None)
def loops_of(name, dtype):
    return tuple(np.ascontiguousarray(l.astype(dtype)) for l in CASES[name]["loops"]())


@functools.lru_cache(maxsize=None)
def index_of(name, dtype):
    return LC.build(list(loops_of(name, dtype)), dtype)


def law_points(name, dtype):
    return np.ascontiguousarray(CASES[name]["law"]().astype(dtype))


def spacing_h(name, xy):
    """The case's spacing law at the positions xy (n, 2), term by term in their type."""
    sp = CASES[name]["spacing"]
    if sp[0] == "const":
        return law_h(sp, xy)
    # surface_sampling_cases.law_h's boundary-layer law, over the case's own points in two columns: (dx dx + dy dy), to
    # which a third column of zeros would add an exact zero
    T = xy.dtype.type
    d2 = None
    for q in law_points(name, xy.dtype):
        dx, dy = xy[:, 0] - q[0], xy[:, 1] - q[1]
        e = dx * dx + dy * dy
        d2 = e if d2 is None else np.minimum(d2, e)
    d = np.sqrt(d2)
    p0, p1, p2 = T(sp[1]), T(sp[2]), T(sp[3])
    center, width = p2 / T(2), p2 / T(6)
    sig = T(1) / (T(1) + np.exp(-(d - center) / width))
    return p0 + (p1 - p0) * sig


@functools.lru_cache(maxsize=None)
def seeds_of(name, dtype):
    """(seed positions (n, 2), their r) in `dtype`; n may be 0."""
    case = CASES[name]
    s = case["seeds"]() if "seeds" in case else np.zeros((0, 2))
    s = np.ascontiguousarray(s.astype(dtype))
    r = np.dtype(dtype).type(case["factor"]) * spacing_h(name, s) if len(s) else np.zeros(0, dtype=dtype)
    for a in (s, r):
        a.setflags(write=False)
    return s, r


def library_spacing(wtp, name, dtype):
    """The case's spacing as the package takes it."""
    sp = CASES[name]["spacing"]
    if sp[0] == "const":
        return sp[1]
    return wtp.BoundaryLayerSpacing(law_points(name, dtype), sp[1], sp[2], sp[3])


# ---- the model: darts -----------------------------------------------------------------------------------------------
def bbox_area(name, dtype):
    idx = index_of(name, dtype)
    lo, hi = idx["lo"].astype(F64), idx["hi"].astype(F64)
    return float((hi[0] - lo[0]) * (hi[1] - lo[1]))


def positions(name, dtype, first, n, seed=SEED):
    idx = index_of(name, dtype)
    lo, hi = idx["lo"], idx["hi"]
    with np.errstate(over="ignore"):
        j = np.arange(n, dtype=np.uint64) + np.uint64(first)
        base = (np.uint64(seed) << np.uint64(40)) + np.uint64(3) * j
        w = [_splitmix64(base + np.uint64(a)) for a in range(2)]
    u = [((x >> np.uint64(40)).astype(F32) * F32(1.0 / 16777216.0)).astype(dtype) for x in w]
    return np.ascontiguousarray(np.stack([lo[a] + u[a] * (hi[a] - lo[a]) for a in range(2)], axis=1))


def darts(name, dtype, first, n, seed=SEED):
    """Darts first .. first + n - 1 of the case: (xy (n, 2) dtype, inside bool, r dtype)."""
    xy = positions(name, dtype, first, n, seed)
    r = np.dtype(dtype).type(CASES[name]["factor"]) * spacing_h(name, xy)
    return xy, LC.inside(index_of(name, dtype), xy), r


# ---- the model: the serial loop -------------------------------------------------------------------------------------
def _conflicts(xy, r, p, rp):
    """bool per row of (xy, r): in conflict with the dart (p, rp), in the arrays' own type"""
    dx, dy = xy[:, 0] - p[0], xy[:, 1] - p[1]
    m = np.minimum(r, rp)
    return (dx * dx + dy * dy) < m * m


def serial(xy, inside, r, sx, sr, max_points, stall_limit):
    """The run over the darts (xy, inside, r) with seeds (sx, sr): (accepted dart indices int64, n_darts, stop_reason,
    n_inside).  Raises when the darts run out before the run ends."""
    n, ns = len(xy), len(sx)
    ax, ar = np.empty((ns + n, 2), dtype=xy.dtype), np.empty(ns + n, dtype=r.dtype)
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
        if not inside[j] or (k and _conflicts(ax[:k], ar[:k], xy[j], r[j]).any()):
            misses += 1
        else:
            ax[k], ar[k] = xy[j], r[j]
            acc.append(j)
            misses = 0
        j += 1


# ---- the model: the batch algorithm -----------------------------------------------------------------------------------
def _lower_conflicts(xy, r):
    """(rows, cols): every pair cols < rows of darts in conflict"""
    n = len(xy)
    rows, cols = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for lo in range(0, n, 256):
        hi = min(lo + 256, n)
        dx, dy = xy[lo:hi, None, 0] - xy[None, :hi, 0], xy[lo:hi, None, 1] - xy[None, :hi, 1]
        m = np.minimum(r[lo:hi, None], r[None, :hi])
        a, b = np.nonzero((dx * dx + dy * dy) < m * m)
        keep = b < a + lo
        rows.append(a[keep] + lo)
        cols.append(b[keep])
    return np.concatenate(rows), np.concatenate(cols)


def batched_run(xy, inside, r, sx, sr, max_points, stall_limit, batch):
    """The same run decided in batches of `batch` darts (0: the library's schedule): dict(acc, n_darts, stop_reason,
    n_inside, rounds_max, n_batches)."""
    n = len(xy)
    acc = np.zeros(0, dtype=np.int64)
    misses, first, rounds_max, n_in, n_batches = 0, 0, 0, 0, 0
    for size in batch_sizes(batch):
        if first >= n:
            raise ValueError(f"the run needs more than {n} darts")
        B = min(size, n - first)
        bx, br, bi = xy[first:first + B], r[first:first + B], inside[first:first + B]
        px, pr = np.concatenate([sx, xy[acc]]), np.concatenate([sr, r[acc]])  # seeds first, then the accepted darts
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


def batched(xy, inside, r, sx, sr, max_points, stall_limit, batch):
    """batched_run() as (accepted, n_darts, stop_reason, n_inside, rounds_max)."""
    b = batched_run(xy, inside, r, sx, sr, max_points, stall_limit, batch)
    return b["acc"], b["n_darts"], b["stop_reason"], b["n_inside"], b["rounds_max"]


@functools.lru_cache(maxsize=None)
def model_run(name, dtype):
    """(xy, inside, r of the case's horizon of darts, accepted, n_darts, stop_reason, n_inside) by serial(), once."""
    case = CASES[name]
    xy, inside, r = darts(name, dtype, 0, case["horizon"])
    sx, sr = seeds_of(name, dtype)
    acc, n_darts, reason, n_in = serial(xy, inside, r, sx, sr, max_points_of(case), case["stall_limit"])
    for a in (xy, inside, r, acc):
        a.setflags(write=False)
    return xy, inside, r, acc, n_darts, reason, n_in
