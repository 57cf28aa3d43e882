"""Loops and numpy model of the 2-D geometry index (include/wtp.h: wtp_loops_set, wtp_loops_query).  Shared by
test_loops_cases.py (no GPU: the reference's own items hold on the model), area_fill_cases.py (the area fill's inside
test) and the GPU tests (the device equals the model bit for bit).

The model restates the header word for word, in the index's type T (numpy rounds every operation on its own, so there
is no contraction):
  build()          dedup per loop (tol = max(8 eps diag, floatmin)), validation (>= 3 vertices before and after, the
                   shoelace area centred on the first vertex against max(1e-10 bbox_area, 4 n eps |hi - lo|^2)),
                   orientation by nesting parity (point_in_loop of the first vertex against the other cleaned loops),
                   segments with unit normals (d_y, -d_x) / |d| and vertex pseudonormals, the box
  query()          brute force over all segments: closest point by the clamped parameter t, the smallest (d2, index),
                   sign from the closest feature's normal, inside = in the box and sd < 0
  point_in_loop()  the even-odd crossing rule
LoopError stands for the library's WTP_ERR_ARG."""
from __future__ import annotations

import functools

import numpy as np

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]


class LoopError(ValueError):
    pass


# ---- the model: build ---------------------------------------------------------------------------------------------------
def _norm(dx, dy):
    return np.sqrt(dx * dx + dy * dy)


def point_in_loop(p, loop):
    """Even-odd crossing test of p against the closed loop (n, 2), in the loop's type."""
    a, b = loop, np.roll(loop, -1, axis=0)
    cross = (a[:, 1] > p[1]) != (b[:, 1] > p[1])
    a, b = a[cross], b[cross]
    x = a[:, 0] + (p[1] - a[:, 1]) / (b[:, 1] - a[:, 1]) * (b[:, 0] - a[:, 0])
    return bool(np.count_nonzero(x > p[0]) % 2)


def _dedup(loop, T):
    lo, hi = loop.min(axis=0), loop.max(axis=0)
    diag = _norm(hi[0] - lo[0], hi[1] - lo[1])
    tol = max(T(8) * np.finfo(T).eps * diag, np.finfo(T).tiny)
    out = []
    for v in loop:
        if not out or _norm(v[0] - out[-1][0], v[1] - out[-1][1]) > tol:
            out.append(v)
    while len(out) > 1 and _norm(out[-1][0] - out[0][0], out[-1][1] - out[0][1]) <= tol:
        out.pop()
    return np.array(out, dtype=T).reshape(-1, 2)


def signed_area(loop):
    o = loop[0]
    a, b = loop - o, np.roll(loop, -1, axis=0) - o
    terms = a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]
    return np.cumsum(terms, dtype=loop.dtype)[-1] / loop.dtype.type(2)  # (cumsum adds in order)


def build(loops, dtype):
    """The index of the loops (a list of (n, 2) arrays) in `dtype`: dict(a, b, nf, na, nb (each (ns, 2)), lo, hi (2,),
    loop_of (ns,), reversed (per loop)).  Raises LoopError where the library returns WTP_ERR_ARG."""
    T = np.dtype(dtype).type
    if len(loops) < 1:
        raise LoopError("at least one boundary loop is needed")
    raw = [np.asarray(l, dtype=T).reshape(-1, 2) for l in loops]
    for l, loop in enumerate(raw):
        if not np.isfinite(loop).all():
            raise LoopError("a coordinate is not finite")
        if len(loop) < 3:
            raise LoopError(f"boundary loop {l} has {len(loop)} vertices")
    cleaned = [_dedup(loop, T) for loop in raw]
    eps = np.finfo(T).eps
    A, B, NF, NA, NB, owner, flipped = [], [], [], [], [], [], []
    for l, loop in enumerate(cleaned):
        n = len(loop)
        if n < 3:
            raise LoopError(f"boundary loop {l} has {n} distinct vertices after dropping duplicates")
        sa = signed_area(loop)
        lo, hi = loop.min(axis=0), loop.max(axis=0)
        ex, ey = hi[0] - lo[0], hi[1] - lo[1]
        noise = (T(n) * eps) * (ex * ex + ey * ey)
        if abs(sa) < max(T(1.0e-10) * (ex * ey), T(4) * noise):
            raise LoopError(f"boundary loop {l} has (near-)zero signed area")
        depth = sum(1 for j, other in enumerate(cleaned) if j != l and point_in_loop(loop[0], other))
        rev = (sa > 0) != (depth % 2 == 0)
        if rev:
            loop = loop[::-1].copy()
        a, b = loop, np.roll(loop, -1, axis=0)
        d = b - a
        mag = _norm(d[:, 0], d[:, 1])
        nf = np.stack([d[:, 1] / mag, -d[:, 0] / mag], axis=1)
        na = np.roll(nf, 1, axis=0) + nf      # vertex i ends segment i - 1 and starts segment i
        A.append(a), B.append(b), NF.append(nf), NA.append(na), NB.append(np.roll(na, -1, axis=0))
        owner.append(np.full(n, l)), flipped.append(rev)
    idx = dict(a=np.concatenate(A), b=np.concatenate(B), nf=np.concatenate(NF), na=np.concatenate(NA),
               nb=np.concatenate(NB), loop_of=np.concatenate(owner), reversed=flipped)
    lo, hi = idx["a"].min(axis=0), idx["a"].max(axis=0)
    e = max(eps * T(100), T(1.0e-10))
    for k in range(2):
        if lo[k] == hi[k]:
            lo[k], hi[k] = lo[k] - e, hi[k] + e
    idx["lo"], idx["hi"] = lo, hi
    for v in idx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return idx


# ---- the model: query ---------------------------------------------------------------------------------------------------
def query(idx, pts, chunk=512):
    """dict(sd, seg int32, closest (n, 2), inside bool) for the points (n, 2), converted once to the index's type and the
    results converted back, by brute force over the segments."""
    pts = np.asarray(pts)
    T = idx["a"].dtype
    q = np.ascontiguousarray(pts.reshape(-1, 2), dtype=T)
    a, b = idx["a"], idx["b"]
    ab = b - a
    den = ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1]
    n = len(q)
    seg, cp, d2 = np.empty(n, dtype=np.int32), np.empty((n, 2), dtype=T), np.empty(n, dtype=T)
    feat = np.empty(n, dtype=np.int8)
    with np.errstate(all="ignore"):
        for s in range(0, n, chunk):
            p = q[s:s + chunk, None, :]
            t = ((p[..., 0] - a[None, :, 0]) * ab[None, :, 0] + (p[..., 1] - a[None, :, 1]) * ab[None, :, 1]) / den[None]
            at_a, at_b = t <= 0, t >= 1
            cx = np.where(at_a, a[None, :, 0], np.where(at_b, b[None, :, 0], a[None, :, 0] + t * ab[None, :, 0]))
            cy = np.where(at_a, a[None, :, 1], np.where(at_b, b[None, :, 1], a[None, :, 1] + t * ab[None, :, 1]))
            dx, dy = p[..., 0] - cx, p[..., 1] - cy
            dd = dx * dx + dy * dy
            k = np.argmin(np.where(np.isnan(dd), np.inf, dd), axis=1)  # the first minimum: the smallest index of a tie
            rows = np.arange(len(k))
            seg[s:s + chunk] = k
            cp[s:s + chunk, 0], cp[s:s + chunk, 1] = cx[rows, k], cy[rows, k]
            d2[s:s + chunk] = dd[rows, k]
            feat[s:s + chunk] = np.where(at_a[rows, k], 1, np.where(at_b[rows, k], 2, 0))
    nrm = np.where((feat == 0)[:, None], idx["nf"][seg], np.where((feat == 1)[:, None], idx["na"][seg], idx["nb"][seg]))
    dv = q - cp
    side = dv[:, 0] * nrm[:, 0] + dv[:, 1] * nrm[:, 1]
    dist = np.sqrt(d2)
    sd = np.where(side > 0, dist, np.where(side < 0, -dist, T.type(0))).astype(T)
    boxed = ~((q < idx["lo"]) | (q > idx["hi"])).any(axis=1)
    return dict(sd=sd.astype(pts.dtype if pts.dtype in (F32, F64) else T), seg=seg,
                closest=cp.astype(pts.dtype if pts.dtype in (F32, F64) else T), inside=boxed & (sd < 0))


def inside(idx, pts):
    return query(idx, pts)["inside"]


# ---- the loops ----------------------------------------------------------------------------------------------------------
def polygon(n, radius=1.0, centre=(0.0, 0.0), phase=0.0):
    """A regular n-gon, counter-clockwise, in double."""
    t = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([centre[0] + radius * np.cos(t), centre[1] + radius * np.sin(t)], axis=1)


def square(off=0.0, side=1.0):
    return np.array([(0, 0), (1, 0), (1, 1), (0, 1)], dtype=F64) * side + off


def star(n=120):
    """The reference's star: r = 1 + 0.3 cos(5 t) at n angles."""
    t = 2 * np.pi * np.arange(n) / n
    r = 1 + 0.3 * np.cos(5 * t)
    return np.stack([np.cos(t) * r, np.sin(t) * r], axis=1)


WEDGE = np.array([(0.0, 0.0), (1.0, -0.05), (1.0, 0.05)], dtype=F64)
SLIVER = np.array([(0.0, 0.0), (1.0, 1.0), (0.05, 0.0)], dtype=F64)


def wedge_probes():
    """216 probes on circles of radius 0.001, 0.01 and 0.05 about the wedge's sharp corner."""
    th = 2 * np.pi * np.arange(72) / 72
    return np.concatenate([np.stack([r * np.cos(th), r * np.sin(th)], axis=1) for r in (0.001, 0.01, 0.05)])


def circle32(n=20_000):
    t = np.linspace(0, 2 * np.pi, n + 1)[:n]
    return np.stack([np.cos(t), np.sin(t)], axis=1).astype(F32)


def small_hole(r):
    """100 vertices of radius r about (5000, 5000), in Float32 arithmetic as the reference's item forms them."""
    t = np.linspace(F32(0), F32(2) * F32(np.pi), 101, dtype=F32)[:100]
    return np.stack([F32(5000) + F32(r) * np.cos(t), F32(5000) + F32(r) * np.sin(t)], axis=1).astype(F32)


@functools.lru_cache(maxsize=None)
def circle32_index():
    return build([circle32()], F32)
