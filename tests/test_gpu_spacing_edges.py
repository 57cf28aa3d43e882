"""The spacing laws' boundary search (wtp_spacing.hip) against the brute-force oracle at its tree, wave and certificate
edges.  test_gpu_spacing.py drives the search at one comfortable size; here every mechanism is taken to its edges.

Stand-alone cases (Context.spacing_eval), a table of (label, dtype, dim, boundary, m, queries, n):
  * the host-built left-balanced kd-tree with buckets of <= 15 nodes: m from 1 to 1000 across every change of the
    bucket / descent mix (`kd_shape` restates kd_left_size and the bucket rule of kd_build_host), coincident, collinear
    and coplanar boundaries with exact repeats (zero-extent boxes, ties in nth_element), a lattice symmetric about the
    cube centre, a boundary translated by +100;
  * the packet walk: n at the wave edges 1 | 63 | 64 | 65, 257, one case beyond the grid-stride cap of 16384 x 256 lanes
    with a partial last wave, waves of one near-wall lane among 63 far ones, queries 10^3 and 10^6 away from the box,
    queries on the boundary points themselves, exact ties on the symmetric lattice, negative coordinates.
LogLike is compared with np.array_equal (the 1-NN distance is the canonical d2 in T), BoundaryLayerSpacing within
4 eps(T) bulk (exp differs by an ulp), as in test_gpu_spacing.py.  test_spacing_cases.py checks on the host that the
table holds what it claims.

Session cases: after every sweep the values the sweep used equal the oracle at the pre-sweep positions, through 2-D
sessions (flat tiles), clustered 3-D clouds at both clamps of the tile height, a first sweep with rebuild = False,
set_points / revert, a replaced fixed head (the re-addressing of hints and certificates) and boundaries of 15 and of
one point.  RelaxSession.spacing_certs() (wtp_relax_get_spacing_certs) is the witness of the certificate that lets a
point skip its walk: for every movable point the winner is a boundary point that attains the brute-force minimum from
x_ref, lb is no larger than the canonical d2 from x_ref to any other boundary point, and x_ref is either the pre-sweep
position (the point walked) or the x_ref it had before (its certificate answered).  A point whose x_ref differs from its
pre-sweep position was answered by its certificate; one whose x_ref was rewritten to that position walked; a point that
stands where it stood at its last walk (no force on it) shows neither.

Measured on an MI355X: see test_tiny_steps_skip_and_walk.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64

# ---- the tree's shape, restated -------------------------------------------------------------------------------------

KD_BUCKET = 15            # wtp_spacing.hip kKdBucket
SP_THREADS = 256          # wtp_spacing.hip kSpThreads
SP_MAX_BLOCKS = 16384     # wtp_spacing.hip sp_grid
SP_TILE_PTS = 160.0       # wtp_spacing.hip kSpTilePts


def kd_left_size(n):
    """Nodes in the left subtree of a left-balanced binary tree with n nodes (wtp_spacing.hip kd_left_size)."""
    if n <= 1:
        return 0
    h = 0
    while (1 << (h + 1)) <= n:
        h += 1
    full = (1 << h) - 1
    last = n - full
    half = 1 << (h - 1)
    return (full - 1) // 2 + min(last, half)


def kd_sizes(m):
    """Subtree size of every node in heap order, top-down from kd_left_size (kd_build_rec)."""
    sz = np.zeros(m, np.int64)
    todo = [(0, m)]
    while todo:
        node, n = todo.pop()
        if n <= 0:
            continue
        sz[node] = n
        left = kd_left_size(n)
        todo.append((2 * node + 1, left))
        todo.append((2 * node + 2, n - left - 1))
    return sz


def kd_bucket_roots(m):
    """Nodes whose record carries a run: maximal subtrees of at most KD_BUCKET nodes (kd_build_host)."""
    sz = kd_sizes(m)
    return [i for i in range(m) if sz[i] <= KD_BUCKET and (i == 0 or sz[(i - 1) // 2] > KD_BUCKET)], sz


def kd_shape(m):
    """What the walk meets below the root: 'bucket-root' (the root itself is a bucket), 'two-buckets' (the root is a
    node and both children are buckets), 'mixed' (one child is a bucket, the other is descended) or 'deep'."""
    roots, sz = kd_bucket_roots(m)
    if 0 in roots:
        return "bucket-root"
    kids = [c for c in (1, 2) if c < m]
    n_b = sum(c in roots for c in kids)
    return "two-buckets" if n_b == len(kids) else "mixed" if n_b == 1 else "deep"


def tile_shape(npts, n3):
    """(W, H, Hz) of spacing_session_kernel's tiles for a grid of n3 cells holding npts points, in its float arithmetic."""
    f = np.float32
    ncells = int(n3[0]) * int(n3[1]) * int(n3[2])
    rho0 = f(npts) / f(max(ncells, 1))
    rho = rho0 if rho0 > f(0.125) else f(0.125)
    flat = n3[2] <= 1
    q = f(SP_TILE_PTS) / rho
    H = int(np.sqrt(q, dtype=f)) if flat else int(np.cbrt(q, dtype=f) + f(0.5))
    H = min(max(H, 1), 8)
    Hz = 1 if flat else H
    W = int(f(SP_TILE_PTS) / (rho * f(H * Hz)) + f(0.5))
    return min(max(W, 1), 32), H, Hz


# ---- boundaries and queries -------------------------------------------------------------------------------------------

M_LIST = (1, 2, 3, 14, 15, 16, 17, 30, 31, 32, 33, 47, 63, 64, 255, 1000)
N_LIST = (1, 63, 64, 65, 257)
N_STRIDE = SP_MAX_BLOCKS * SP_THREADS + 65     # the grid-stride loop and a partial last wave


def faces(m, dim, seed=31):
    """m random points on the faces of the unit cube (the edges of the unit square)."""
    b = np.random.default_rng(seed).random((m, dim))
    f = np.arange(m) % (2 * dim)
    b[np.arange(m), f % dim] = (f // dim).astype(np.float64)
    return b


def sym_lattice(dim):
    """Odd sixteenths on every face of the unit cube: symmetric about the centre and about every plane x_a = 1/2, all
    coordinates dyadic, so mirror images tie exactly in fp32 and fp64."""
    g = (2.0 * np.arange(8) + 1.0) / 16.0
    parts = []
    for a in range(dim):
        for side in (0.0, 1.0):
            mesh = np.stack(np.meshgrid(*[g] * (dim - 1), indexing="ij"), -1).reshape(-1, dim - 1)
            parts.append(np.insert(mesh, a, side, axis=1))
    return np.concatenate(parts)


def boundary(kind, m, dim):
    if kind == "faces":
        return faces(m, dim)
    if kind == "copies":                                     # m copies of one point: every box has zero extent
        return np.tile(np.array([0.25, 0.75, 0.5][:dim]), (m, 1))
    if kind == "collinear":                                  # along x: zero extent on the other axes
        b = np.tile(np.array([0.0, 0.375, 0.625][:dim]), (m, 1))
        b[:, 0] = np.random.default_rng(32).permutation(m) / (m - 1.0)
        return b
    if kind == "coplanar":                                   # a lattice in z = 1/4 (a line y = 1/4 of the square), every fifth point twice
        if dim == 3:
            g = np.arange(8) / 8.0
            b = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
            b = np.concatenate([b, np.full((len(b), 1), 0.25)], 1)
        else:
            b = np.stack([np.arange(40) / 40.0, np.full(40, 0.25)], 1)
        b = np.concatenate([b, b[::5]])
        return b[np.random.default_rng(33).permutation(len(b))]
    if kind == "symmetric":
        return sym_lattice(dim)
    if kind == "translated":
        return faces(m, dim, 34) + 100.0
    raise ValueError(kind)


def boundary_size(kind, m, dim):
    return len(boundary(kind, m, dim))


def queries(kind, n, b, dim):
    """n queries (fp64) of one kind against the boundary b."""
    rng = np.random.default_rng(5 + n % 1000)
    lo, hi = b.min(0), b.max(0)
    ext = np.maximum(hi - lo, 1.0)                           # (a degenerate boundary: queries around it in a unit box)
    if kind == "uniform":                                    # the box inflated by 0.2
        return lo - 0.2 * ext + rng.random((n, dim)) * 1.4 * ext
    if kind == "self":                                       # every boundary point itself: d = 0
        return b.copy()
    if kind in ("far1e3", "far1e6"):
        d = rng.standard_normal((n, dim))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return 0.5 * (lo + hi) + d * float(kind[3:]) + rng.random((n, dim))
    if kind == "ties":                                       # the centre, then points on the symmetry planes (64ths)
        q = rng.integers(0, 65, (n, dim)) / 64.0
        q[np.arange(n), np.arange(n) % dim] = 0.5
        q[0] = 0.5
        return q
    if kind == "mixed":                                      # per run of 64: one query 0.01 off a boundary point among far ones
        q = 0.35 + 0.3 * rng.random((n, dim))
        for r0 in range(0, n, 64):
            j = r0 + int(rng.integers(0, min(64, n - r0)))
            p = b[int(rng.integers(0, len(b)))]
            q[j] = p + 0.01 * np.sign(0.5 - p) * (np.abs(p - 0.5) == 0.5)
        return q
    if kind == "negative":
        return -2.0 * rng.random((n, dim)) - 2.0 ** -20
    raise ValueError(kind)


def _both(label, bkind, m, qkind, n):
    return [(f"f{8 * np.dtype(t).itemsize} {d}d {label}", t, d, bkind, m, qkind, n) for t in (F32, F64) for d in (3, 2)]


# (label, dtype, dim, boundary, m, queries, n); n = 0: as many queries as boundary points ("self")
CASES = []
for _m in M_LIST:                                            # the tree's shapes, at a partial fifth wave
    CASES += _both(f"faces m={_m}", "faces", _m, "uniform", 257)
for _n in N_LIST[:-1]:                                       # the wave edges
    CASES += _both(f"faces m=255 n={_n}", "faces", 255, "uniform", _n)
for _bk, _m in (("copies", 40), ("collinear", 33), ("coplanar", 0), ("symmetric", 0), ("translated", 255)):
    CASES += _both(f"{_bk} uniform", _bk, _m, "uniform", 257)
    CASES += _both(f"{_bk} self", _bk, _m, "self", 0)
for _m in (15, 16, 33, 1000):
    CASES += _both(f"faces m={_m} self", "faces", _m, "self", 0)
for _qk in ("far1e3", "far1e6", "negative"):
    CASES += _both(f"faces m=1000 {_qk}", "faces", 1000, _qk, 257)
    CASES += _both(f"faces m=33 {_qk}", "faces", 33, _qk, 65)
CASES += _both("symmetric ties", "symmetric", 0, "ties", 257)
CASES += _both("faces m=1000 mixed waves", "faces", 1000, "mixed", 353)
CASES += [("f32 3d faces m=33 grid stride", F32, 3, "faces", 33, "uniform", N_STRIDE)]

LL = (0.08, 1.3)            # LogLike base_size, growth_rate
BL = (0.02, 0.09, 0.3)      # BoundaryLayerSpacing at_wall, bulk, layer_thickness


def make_case(dtype, dim, bkind, m, qkind, n):
    b = boundary(bkind, m, dim)
    q = queries(qkind, n, b, dim)
    return np.ascontiguousarray(b.astype(dtype)), np.ascontiguousarray(q.astype(dtype))


def cases():
    return [pytest.param(*c[1:], id=c[0]) for c in CASES]


@pytest.mark.parametrize("dtype,dim,bkind,m,qkind,n", cases())
def test_spacing_eval_edge_matches_oracle(O, wtp, ctx, dtype, dim, bkind, m, qkind, n):
    b, x = make_case(dtype, dim, bkind, m, qkind, n)
    got = ctx.spacing_eval(dict(kind=2, p0=LL[0], p1=LL[1], boundary=b), x)
    want = O.spacing_loglike(x, b, *LL)
    bad = np.flatnonzero(got != want)
    print(f"[spacing] m={len(b)} ({kd_shape(len(b))}) n={len(x)} differing={len(bad)}")
    assert got.dtype == dtype and np.array_equal(got, want), \
        f"{len(bad)} of {len(x)} LogLike values differ, first queries {bad[:5]}: {got[bad[:5]]} for {want[bad[:5]]}"
    if qkind == "self":
        assert np.all(got == 0)
    got = ctx.spacing_eval(dict(kind=3, p0=BL[0], p1=BL[1], p2=BL[2], boundary=b), x)
    want = O.spacing_boundary_layer(x, b, *BL)
    ulp = np.finfo(dtype).eps * BL[1]
    assert np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))) <= 4 * ulp   # exp() differs by an ulp


# ---- sessions ---------------------------------------------------------------------------------------------------------

STRONG = dict(kind=3, beta=0.2, u0=1.0, gamma=3.0)           # unbounded support: every point moves in every sweep
CLIPPED = dict(kind=2, beta=0.2, u0=1.0, gamma=3.0)


def _law_values(O, law, x, b):
    if law["kind"] == 2:
        return O.spacing_loglike(x, b, law["p0"], law["p1"])
    return O.spacing_boundary_layer(x, b, law["p0"], law["p1"], law["p2"])


def _assert_values(O, law, got, x, b, what):
    want = _law_values(O, law, x, b)
    if law["kind"] == 2:
        bad = np.flatnonzero(got != want)
        assert np.array_equal(got, want), f"{what}: {len(bad)} of {len(x)} values differ, first points {bad[:5]}"
    else:
        ulp = np.finfo(x.dtype).eps * law["p1"]
        assert np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))) <= 4 * ulp, what


def _d2_rows(x3, b3):
    """Canonical d2 = (dx dx + dy dy) + dz dz in T of every row of x3 to every row of b3 (z = 0 in 2-D adds an exact 0)."""
    dx = x3[:, None, 0] - b3[None, :, 0]
    dy = x3[:, None, 1] - b3[None, :, 1]
    dz = x3[:, None, 2] - b3[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def check_certs(certs, pre, prev_ref, b, what):
    """The invariants of the module docstring; returns the masks of the points whose certificate answered and of those
    that walked for certain (x_ref rewritten)."""
    T = pre.dtype.type
    n, dim = pre.shape
    b3 = np.zeros((len(b), 3), T)
    b3[:, :dim] = b
    hint, x_ref, lb, win = certs["hint"], certs["x_ref"], certs["lb"], certs["winner"]
    assert x_ref.dtype == pre.dtype and hint.shape == (n,) and x_ref.shape == (n, 3) and win.shape == (n, 3)
    assert (hint >= 0).all() and (hint < len(b)).all(), f"{what}: a point that was searched has no winner"
    if dim == 2:
        assert not x_ref[:, 2].any() and not win[:, 2].any()
    walked = (x_ref[:, :dim] == pre).all(1)
    kept = (x_ref == prev_ref).all(1)
    assert (walked | kept).all(), f"{what}: x_ref is neither the pre-sweep position nor the earlier x_ref " \
                                  f"for points {np.flatnonzero(~(walked | kept))[:5]}"
    for s in range(0, n, 2048):                              # brute force in T, in pieces
        e = min(n, s + 2048)
        d2 = _d2_rows(x_ref[s:e], b3)
        is_win = (b3[None, :, :] == win[s:e, None, :]).all(2)
        assert is_win.any(1).all(), f"{what}: a winner is no boundary point"
        dw = d2[np.arange(e - s), is_win.argmax(1)]
        assert np.array_equal(dw, d2.min(1)), f"{what}: a winner does not attain the brute-force minimum from x_ref"
        d2[np.arange(e - s), is_win.argmax(1)] = np.inf     # one instance of the winner's coordinates removed
        other = d2.min(1)
        bad = np.flatnonzero(~(lb[s:e] <= other))
        assert len(bad) == 0, f"{what}: lb exceeds another boundary point's d2 for points {s + bad[:5]}: " \
                              f"{lb[s:e][bad[:5]]} > {other[bad[:5]]}"
    return ~walked, walked & ~kept


class Driver:
    """A session with a device law, stepped one sweep at a time against the oracle."""

    def __init__(self, O, ctx, head, movable, law_b, law, force, k, alpha_lo, alpha_max, certs=True):
        self.O, self.law_b, self.certs = O, law_b, certs
        self.law = dict(law, boundary=law_b)
        self.n_fixed = len(head)
        snap = np.concatenate([head, movable]) if len(head) else movable.copy()
        self.sess = ctx.relax(snap, len(head), self.law, force, k, alpha_lo, alpha_max)
        self.cur = movable.copy()
        self.sweeps = 0
        self.shares = []
        _assert_values(O, self.law, self.sess.spacings(), snap, law_b, "setup")       # spacing.(snap), the head included
        if certs:
            c = self.sess.spacing_certs()
            self.ref = c["x_ref"]
            check_certs(c, self.cur, self.ref, law_b, "setup")
            assert (self.ref[:, : movable.shape[1]] == movable).all()                 # the setup searched every point

    def step(self, rebuild):
        pre = self.cur
        self.sess.step(rebuild)
        self.sweeps += 1
        what = f"sweep {self.sweeps}"
        _assert_values(self.O, self.law, self.sess.spacings()[self.sess.n_fixed:], pre, self.law_b, what)
        skipped = None
        if self.certs:
            c = self.sess.spacing_certs()
            skipped, self.walked = check_certs(c, pre, self.ref, self.law_b, what)
            self.ref = c["x_ref"]
            self.shares.append((float(skipped.mean()), float(self.walked.mean())))
        self.cur = self.sess.positions()
        return skipped

    def close(self):
        self.sess.close()


def _square(m, dtype):
    return np.ascontiguousarray(faces(m, 2, 41).astype(dtype))


def _cube(m, dtype, seed=42):
    """Points on the faces of the unit cube, the eight corners among them: the cloud's box is the unit cube exactly."""
    b = faces(m, 3, seed)
    b[:8] = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    return np.ascontiguousarray(b.astype(dtype))


def _inside(n, dim, dtype, seed):
    return np.ascontiguousarray((0.05 + 0.9 * np.random.default_rng(seed).random((n, dim))).astype(dtype))


def clustered(n, dtype, seed=43):
    """80 % of n points inside a ball of radius 0.05 around (0.3, 0.6, 0.45), the rest spread over the unit cube."""
    rng = np.random.default_rng(seed)
    nc = int(0.8 * n)
    d = rng.standard_normal((nc, 3))
    d *= (0.05 * rng.random((nc, 1)) ** (1.0 / 3.0)) / np.linalg.norm(d, axis=1, keepdims=True)
    x = np.concatenate([np.array([0.3, 0.6, 0.45]) + d, 0.02 + 0.96 * rng.random((n - nc, 3))])
    return np.ascontiguousarray(x[rng.permutation(n)].astype(dtype))


# The clustered clouds of case (b): (dtype, fixed head, movable points, law, force, what the session's grid and the tiles
# of spacing_session_kernel come to).  test_spacing_cases.py recomputes the last column: its session_grid restates the session's measured grid, tile_shape the tiles.
#   sparse: 300 + 1700 points, a k-nearest law below 4096 points (the explicit k-selection on 4 x 4 x 4 bricks): the
#     tuner shrinks the cells until the grid reaches its cap of 8 n + 4096 cells, 27 x 27 x 27; mean occupancy 0.10,
#     under the floor of 0.125 -> H = Hz = 8 (upper clamp), W = 20, which does not divide n[0] = 27; the cluster's 1360
#     points lie in one or two tiles and most of the 2 x 4 x 4 tiles hold a few points of the background.
#   dense: 1500 + 1500 points in fp64 with the compact-support law and a BoundaryLayerSpacing of 0.3 .. 0.45: the cells
#     cover the support, 1.1 x the mean spacing, an edge in (1/3, 1/2) -> 3 x 3 x 3 cells, 111 points per cell ->
#     H = Hz = 1 (lower clamp), W = 1; the cluster's cell is one tile of about 1250 points.
CLUSTERED = {
    "sparse": dict(dtype=F32, n_fixed=300, n_move=1700, law=dict(kind=2, p0=0.07, p1=1.2), force=STRONG,
                   tiles=(20, 8, 8)),
    "dense": dict(dtype=F64, n_fixed=1500, n_move=1500, law=dict(kind=3, p0=0.3, p1=0.45, p2=0.3), force=CLIPPED,
                  tiles=(1, 1, 1)),
}


def clustered_cloud(name):
    c = CLUSTERED[name]
    return _cube(c["n_fixed"], c["dtype"]), clustered(c["n_move"], c["dtype"])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_session_2d_flat_tiles(O, ctx, dtype):
    """(a) a 2-D session: the flat branch of the tiling (Hz = 1, H from the square root)."""
    b = _square(400, dtype)
    d = Driver(O, ctx, b, _inside(3000, 2, dtype, 44), b, dict(kind=2, p0=0.07, p1=1.2), STRONG, 10, 2e-5, 2e-3)
    try:
        for it in range(5):
            d.step(it % 2 == 0)
    finally:
        d.close()


@pytest.mark.parametrize("name", list(CLUSTERED))
def test_session_clustered_cloud(O, ctx, name):
    """(b) tiles of several hundred points beside empty ones, at each clamp of the tile height (CLUSTERED above)."""
    c = CLUSTERED[name]
    b, v = clustered_cloud(name)
    d = Driver(O, ctx, b, v, b, c["law"], c["force"], 21, 2e-5, 2e-3)
    try:
        for it in range(4):
            d.step(it % 2 == 0)
    finally:
        d.close()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_session_first_sweep_without_rebuild(O, ctx, dtype):
    """(c) rebuild = False before the first tree (the library builds it all the same), then a rebuild every third sweep."""
    b = _cube(1000, dtype)
    d = Driver(O, ctx, b, _inside(4000, 3, dtype, 45), b, dict(kind=2, p0=0.07, p1=1.2), CLIPPED, 21, 2e-5, 2e-3)
    try:
        for it in range(6):
            d.step(it > 0 and it % 3 == 0)
    finally:
        d.close()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_session_set_points_and_revert(O, ctx, dtype):
    """(d) 300 points placed by hand at once, and a reverted sweep: the sweep that follows uses exact values."""
    b = _cube(1000, dtype)
    d = Driver(O, ctx, b, _inside(4000, 3, dtype, 46), b, dict(kind=2, p0=0.07, p1=1.2), CLIPPED, 21, 1e-7, 1e-5)
    try:
        d.step(True)
        d.step(False)
        idx = np.arange(5, 4000, 13)[:300]
        new = _inside(300, 3, dtype, 47)
        d.sess.set_points(idx, new)
        d.cur[idx] = new
        d.step(True)
        assert d.walked[idx].all(), "a point thrown across the box kept its certificate"
        before = d.cur.copy()
        d.step(False)
        d.sess.revert()
        d.cur = before                                       # p .= p_old: the positions the reverted sweep started from
        assert np.array_equal(d.sess.positions(), before)
        d.step(False)
        d.step(True)
    finally:
        d.close()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_session_replaced_head_keeps_hints_and_certificates(O, ctx, dtype):
    """(e) wtp_relax_set_fixed_dev with a device law: the head grows, shrinks to nothing and grows again; hints and
    certificates stay addressed by movable index (aux_off).  Tiny steps, so that certificates are in use throughout."""
    import torch

    def rows4(x):
        r = np.zeros((len(x), 4), dtype)
        r[:, :3] = x
        return torch.from_numpy(r).cuda()

    law_b = _cube(700, dtype)
    d = Driver(O, ctx, _cube(500, dtype, 48), _inside(3000, 3, dtype, 49), law_b, dict(kind=2, p0=0.07, p1=1.2),
               CLIPPED, 21, 1e-7, 1e-5)
    try:
        d.step(True)
        keep = []
        for n_head, seed in ((1200, 50), (0, 0), (800, 51)):
            if n_head:
                keep.append(rows4(_cube(n_head, dtype, seed)))
                d.sess.set_fixed_dev(keep[-1].data_ptr(), n_head)
            else:
                d.sess.set_fixed_dev(0, 0)
            assert d.sess.n_fixed == n_head and len(d.sess.spacing_certs()["hint"]) == 3000
            skipped = d.step(True)
            assert skipped.any(), f"no certificate answered after the head became {n_head} points"
            d.step(False)
    finally:
        d.close()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("m", [15, 1])
def test_session_tiny_boundaries(O, ctx, dtype, m):
    """(f) a boundary that is one bucket, and a boundary of one point: nothing but the winner exists, lb = +inf, and every
    certificate holds for good after the setup's search — x_ref stays the setup position."""
    head = _cube(500, dtype, 52)
    law_b = np.ascontiguousarray(faces(m, 3, 53).astype(dtype))
    v = _inside(3000, 3, dtype, 54)
    d = Driver(O, ctx, head, v, law_b, dict(kind=2, p0=0.07, p1=1.2), STRONG, 21, 2e-5, 2e-3)
    try:
        for it in range(4):
            skipped = d.step(it % 2 == 0)
            if m == 1:
                c = d.sess.spacing_certs()
                assert np.isinf(c["lb"]).all() and (c["lb"] > 0).all() and (c["hint"] == 0).all()
                assert np.array_equal(c["x_ref"][:, :3], v), "a point searched a boundary of one point again"
                if it >= 1:
                    assert skipped.all(), f"sweep {it + 1}: {(~skipped).sum()} points of 3000 walked"
    finally:
        d.close()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_tiny_steps_skip_and_walk(O, ctx, dtype):
    """Steps of 1e-7 .. 1e-5 of a spacing, as in test_gpu_spacing.py, with the witness.  Asserted: every sweep after the
    first has points whose certificate answered, and the point thrown across the box at sweep 7 walks — the one walk the
    construction makes certain; who else walks (a point between two nearly equidistant boundary points, whenever it
    moves) is left to the cloud, so the sweeps taken together hold both, not provably each of them.  The shares are
    printed, not asserted.

    Measured on an MI355X (1200 boundary points on the cube faces, 5000 movable points uniform in [0.05, 0.95]^3,
    LogLike(0.07, 1.2), sweeps 2 .. 10): answered by their certificate fp32 0.912 .. 0.913 of the points in
    every sweep, fp64 0.921 .. 0.922; walked for certain 0.0004 .. 0.0020 (2 .. 10 points) in both; the other 8 % stand
    where their last walk left them (no neighbour inside the clipped law's support) and show neither."""
    b = _cube(1200, dtype, 55)
    d = Driver(O, ctx, b, _inside(5000, 3, dtype, 56), b, dict(kind=2, p0=0.07, p1=1.2), CLIPPED, 21, 1e-7, 1e-5)
    try:
        for it in range(10):
            if it == 6:                                      # the kick of src/repel.jl:431
                far = np.array([0.93, 0.08, 0.51], dtype)
                d.sess.set_point(17, far)
                d.cur[17] = far
            skipped = d.step(it % 3 == 0)
            if it >= 1:
                assert skipped.any(), f"sweep {it + 1}: no certificate answered"
            if it == 6:                                      # (other sweeps: whoever sits between two nearly equidistant boundary points)
                assert d.walked[17], "the point thrown across the box did not walk"
        print(f"[spacing] {np.dtype(dtype).name} shares skipped/walked, sweeps 2..10: "
              + " ".join(f"{a:.4f}/{b:.4f}" for a, b in d.shares[1:]))
    finally:
        d.close()


def test_spacing_certs_needs_a_device_law(wtp, ctx):
    """WTP_ERR_STATE without a session and with a constant spacing; NULL outputs are accepted."""
    x = _inside(500, 3, F32, 57)
    ctx._lib.wtp_relax_end(ctx._h)
    assert ctx._lib.wtp_relax_get_spacing_certs(ctx._h, None, None, None) == 4    # WTP_ERR_STATE (include/wtp.h)
    with ctx.relax(x, 0, 0.1, CLIPPED, 21, 1e-5, 1e-3) as sess:
        with pytest.raises(wtp.WtpError):
            sess.spacing_certs()
    b = _cube(100, F32)
    with ctx.relax(x, 0, dict(kind=2, p0=0.07, p1=1.2, boundary=b), CLIPPED, 21, 1e-5, 1e-3) as sess:
        assert ctx._lib.wtp_relax_get_spacing_certs(ctx._h, None, None, None) == 0
        assert (sess.spacing_certs()["hint"] >= 0).all()


def test_spacing_eval_cannot_replace_the_tree_of_an_open_session(O, wtp, ctx):
    """The context caches one boundary tree.  During a session with a device law, wtp_spacing_eval of the same boundary is
    served from it; another boundary (or the same one in the other type) is refused with WTP_ERR_STATE, and the session's
    values and winners stay those of its own boundary."""
    b = _cube(300, F32, 58)
    other = _cube(300, F32, 59)
    law = dict(kind=2, p0=0.07, p1=1.2)
    d = Driver(O, ctx, b, _inside(2000, 3, F32, 60), b, law, CLIPPED, 21, 2e-5, 2e-3)
    try:
        d.step(True)
        x = _inside(100, 3, F32, 61)
        assert np.array_equal(ctx.spacing_eval(dict(law, boundary=b), x), O.spacing_loglike(x, b, 0.07, 1.2))
        for bad, xx in ((other, x), (b.astype(F64), x.astype(F64)), (b[:, :2].copy(), x[:, :2].copy())):
            with pytest.raises(wtp.WtpError):
                ctx.spacing_eval(dict(law, boundary=bad), xx)
        d.step(False)                                        # values, winners and bounds against b, as before
        d.step(True)
    finally:
        d.close()
    assert np.array_equal(ctx.spacing_eval(dict(law, boundary=other), x), O.spacing_loglike(x, other, 0.07, 1.2))
