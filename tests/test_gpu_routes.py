"""Every KNN and sweep route against the CPU oracle at its k and n edges.

The library runs one of about ten kernels per operation, chosen by dtype, dim, k, include_self, n and force law.
`knn_route` and `sweep_route` restate that choice in Python (each rule names the C++ line it mirrors); the cases
below are generated from labelled cells and the route each cell takes, and test_route_table.py checks on the host
that every route is reached and every threshold is tested on both sides.

Bars.  KNN: rows and distances bit-exact against the oracle's kd-tree and against the exact path
(WTP_FORCE_GENERIC=1).  Sweeps: nn_id and nn_dist bit-exact; Float64 positions and forces bit-exact (LennardJones:
bit-exact against the exact path, within pow()'s last place of the oracle); fp32 positions within 2e-5 spacings and
forces within rtol 2e-4 (the summation order differs inside the fast kernels), the step statistics as in
test_gpu_parity.py.

Route witness.  stats["n_fallback"] counts the queries a route's own kernels handed to the exact wave-per-query
path (the first word of the sweep's counter block).  The Exact route hands nothing back, so it reports 0; a fast
route reports how many queries it could not certify.  The counter therefore bounds how much of a fast route's work
the exact path redid (most queries must be certified by the route itself), and on data with coincident points,
whose zero distances every fast route leaves to the exact path, a non-zero count shows that a fast route ran.  On
uniform data it cannot tell a fast route that certified everything from the Exact route (F64Ksel certifies every
query of a uniform cloud and reports 0, as Exact does).  Where a route cannot certify by design — ClippedSpacingForce
at k = 2, whose support holds more than k points; lattice ties at the cut; a cluster that overfills the bricks — the
count is large, and only k = 2 is asserted (non-zero: the compact-support kernel ran and handed back).  KNN calls
report no counter at all: for them the table and the two bit-exact comparisons are the whole check.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# ---- the dispatch rules ------------------------------------------------------------------------------------------

FAST_KMAX = 32    # csrc/wtp_brick.hip kFastKMax: k >= 32 goes to the wave kernel
KSEL_KMAX = 24    # csrc/wtp_ksel.hip kKsKMax (ksel_kmax()): largest k + self of the x-slowest k-selection
KSEL_NMIN = 4096  # n >= 4096 for the k-selection layout (csrc/wtp_topology.hip knn_dev_t, f64_candidates; wtp_relax.hip sweep_route<T>)
F64_KC_MAX = 31   # csrc/wtp_topology.hip knn_dev_f64: candidate lists longer than 31 take the exact path
F64K_KMAX = 22    # csrc/wtp_relax.hip sweep_route<T> (f64k): Float64 candidate sweeps for k <= 22 (k + 2 candidates <= 24)
CLIPPED = 2       # WTP_FORCE_CLIPPED_SPACING


def _topology32(dim, k, include_self, n):
    """The fp32 KNNTopology kernel of k rows (k + self searched) — knn_dev_t and launch_topology<float>."""
    kq = k if include_self else k + 1                      # wtp_topology.hip knn_dev_t (kq: neighbours sought, self included)
    if k > FAST_KMAX - 1:                                  # wtp_brick.hip:893 (a.k > kFastKMax - 1: the wave kernel)
        return "exact"
    if dim == 3 and kq <= KSEL_KMAX and n >= KSEL_NMIN:    # wtp_topology.hip knn_dev_t: ksel (the x-slowest layout)
        if k == 24:                                        # wtp_ksel.hip:729
            return "ksel<0,24>"
        return "ksel<0,21>" if k == 21 else "ksel<0,0>"    # wtp_ksel.hip:730
    return "brick<0,21,0>" if k == 21 else "brick<0,0,0>"  # wtp_brick.hip:901


def knn_route(dtype, dim, k, include_self, n):
    """Route of ctx.knn: fp32 through knn_dev_t, fp64 through knn_dev_f64 (fp32 candidates, fp64 re-ranking)."""
    if np.dtype(dtype) == np.float32:
        return _topology32(dim, k, include_self, n)
    kq = k if include_self else k + 1                      # wtp_topology.hip knn_dev_f64: kq
    kc = min(kq + 2, n)                                    # wtp_topology.hip knn_dev_f64: kc
    if kc > F64_KC_MAX:                                    # wtp_topology.hip knn_dev_f64 (launch_topology<double>: the wave kernel)
        return "exact"
    cand = _topology32(dim, kc, True, n)                   # wtp_topology.hip f64_candidates: kc with self, fp32
    refine = "slots" if kc == 24 else "refine"             # wtp_topology.hip knn_dev_f64: slots (refine_f64_slots_kernel at kc == 24)
    return f"f64:{cand}+{refine}"


def sweep_route(dtype, dim, k, kind, n, ball64=True):
    """Route of a fresh sweep (wtp_relax.hip: sweep_route<T>, then step_route with a measured grid),
    with the kernel instance it launches (launch_brick_sweep, wtp_brick.hip:910; launch_ksel_sweep, wtp_ksel.hip:735)."""
    clipped = kind == CLIPPED
    f64 = np.dtype(dtype) == np.float64
    if clipped and 2 <= k < 32:                            # wtp_relax.hip sweep_route<T>: compact support
        if f64:
            return "Cs64" if ball64 else "Cs64Wave"        # wtp_relax.hip sweep_route<T>: ctx->ball64
        return "Cs2" if dim == 3 else "Cs<1,0,1>"          # wtp_relax.hip sweep_route<T>: r.dim
    if f64:                                                # wtp_relax.hip sweep_route<T>: f64k (k-nearest laws, 3-D, 2 <= k <= 22)
        return "F64Ksel" if dim == 3 and not clipped and 2 <= k <= F64K_KMAX and n >= KSEL_NMIN else "Exact"
    if k >= 32:                                            # wtp_relax.hip sweep_route<T>: beyond the brick kernels' lists
        return "Exact"
    if dim == 3 and 2 <= k <= KSEL_KMAX and n >= KSEL_NMIN:  # wtp_relax.hip sweep_route<T>: ksel
        return "Ksel<1,21>" if k == 21 else "Ksel<1,0>"
    return "Select<1,21,0>" if k == 21 else "Select<1,0,0>"  # wtp_relax.hip sweep_route<T>: Select


FAST_SWEEP = {"Cs2", "Cs<1,0,1>", "Cs64", "Cs64Wave", "F64Ksel", "Ksel<1,21>", "Ksel<1,0>", "Select<1,21,0>",
              "Select<1,0,0>"}
KNN_ROUTES = {"ksel<0,24>", "ksel<0,21>", "ksel<0,0>", "brick<0,21,0>", "brick<0,0,0>", "exact"} | {
    f"f64:{c}+{r}" for c, r in [("ksel<0,24>", "slots"), ("ksel<0,0>", "refine"), ("ksel<0,21>", "refine"),
                                ("brick<0,0,0>", "slots"), ("brick<0,0,0>", "refine"), ("brick<0,21,0>", "refine")]}
SWEEP_ROUTES = FAST_SWEEP | {"Exact"}

# ---- the cells ----------------------------------------------------------------------------------------------------

F32, F64 = np.float32, np.float64
LAWS = {0: dict(kind=0, beta=0.2, u0=1.0, gamma=3.0), 1: dict(kind=1, beta=0.2, u0=1.0, gamma=3.0),
        2: dict(kind=2, beta=0.2, u0=1.0, gamma=3.0), 3: dict(kind=3, beta=0.2, u0=1.0, gamma=3.0)}
NN_LAWS = (0, 1, 3)  # the k-nearest laws; law 2 (ClippedSpacingForce) has routes of its own

# KNN: (label, dtype, dim, n, k, include_self, data)
KNN_CELLS = [
    # fp32, item 1: the k-selection edge (k + self 24 / 25) and the brick kernel up to k = 31, with and without self
    ("f32 k+self=24 self", F32, 3, 20000, 24, True, "uniform"),
    ("f32 k+self=24", F32, 3, 20000, 23, False, "uniform"),
    ("f32 k+self=25", F32, 3, 20000, 24, False, "uniform"),
    ("f32 k=25 self", F32, 3, 20000, 25, True, "uniform"),
    ("f32 k=25", F32, 3, 20000, 25, False, "uniform"),
    ("f32 k=28", F32, 3, 20000, 28, False, "uniform"),
    ("f32 k=30 self", F32, 3, 20000, 30, True, "uniform"),
    ("f32 k=31 self", F32, 3, 20000, 31, True, "uniform"),
    ("f32 k=31", F32, 3, 20000, 31, False, "uniform"),
    ("f32 k=32 self", F32, 3, 20000, 32, True, "uniform"),
    ("f32 k=32", F32, 3, 20000, 32, False, "uniform"),
    ("f32 k=21 n=4095", F32, 3, 4095, 21, False, "uniform"),
    ("f32 k=21 n=4096", F32, 3, 4096, 21, False, "uniform"),
    ("f32 k=12 n=4095", F32, 3, 4095, 12, True, "uniform"),
    ("f32 k=12 n=4096", F32, 3, 4096, 12, True, "uniform"),
    ("f32 2d k=21", F32, 2, 20000, 21, False, "uniform"),
    ("f32 2d k=31", F32, 2, 20000, 31, False, "uniform"),
    ("f32 2d k=32", F32, 2, 20000, 32, False, "uniform"),
    ("f32 k=31 lattice", F32, 3, 4913, 31, False, "lattice"),
    ("f32 k=24 self lattice", F32, 3, 4913, 24, True, "lattice"),
    ("f32 k=31 coincident", F32, 3, 20000, 31, False, "coincident"),
    ("f32 k=28 cluster", F32, 3, 20000, 28, True, "cluster"),
    ("f32 2d k=31 coincident", F32, 2, 20000, 31, True, "coincident"),
    # fp64, item 2: candidate lists kc = kq + 2 up to 31, the slots kernel at kc = 24, the ksel<0,21> candidates at
    # kc = 21, the general refine kernel at large k, and the first k past the candidate route
    ("f64 k=21 slots", F64, 3, 20000, 21, False, "uniform"),
    ("f64 k=22 self slots", F64, 3, 20000, 22, True, "uniform"),
    ("f64 k=10 self", F64, 3, 20000, 10, True, "uniform"),
    ("f64 k=19 self kc=21", F64, 3, 20000, 19, True, "uniform"),
    ("f64 k=22 kc=25", F64, 3, 20000, 22, False, "uniform"),
    ("f64 k=26 kc=29", F64, 3, 20000, 26, False, "uniform"),
    ("f64 k=28 kc=31", F64, 3, 20000, 28, False, "uniform"),
    ("f64 k=29 kc=32", F64, 3, 20000, 29, False, "uniform"),
    ("f64 k=29 self kc=31", F64, 3, 20000, 29, True, "uniform"),
    ("f64 k=30 self kc=32", F64, 3, 20000, 30, True, "uniform"),
    ("f64 k=21 n=4095", F64, 3, 4095, 21, False, "uniform"),
    ("f64 k=21 n=4096", F64, 3, 4096, 21, False, "uniform"),
    ("f64 k=19 self n=3000", F64, 3, 3000, 19, True, "uniform"),
    ("f64 2d k=21", F64, 2, 20000, 21, False, "uniform"),
    ("f64 2d k=28", F64, 2, 20000, 28, False, "uniform"),
    ("f64 2d k=29", F64, 2, 20000, 29, False, "uniform"),
    ("f64 k=28 lattice", F64, 3, 4913, 28, False, "lattice"),
    ("f64 k=21 coincident", F64, 3, 20000, 21, False, "coincident"),
    ("f64 k=10 self cluster", F64, 3, 20000, 10, True, "cluster"),
    # fp32-collapsing fp64 cloud: clusters distinct in fp64 and coincident in the fp32 copy, a lattice 1e3 away
    ("f64 k=21 collapsing", F64, 3, 20000, 21, False, "collapsing"),
    ("f64 k=10 self collapsing", F64, 3, 20000, 10, True, "collapsing"),
]

# sweeps: (label, dtype, dim, n, k, laws, n_fixed, data, env)
SWEEP_CELLS = [
    # fp32 Select (items 3): 3-D k = 25..31, 3-D n < 4096, 2-D, clipped k = 1
    ("f32 select k=25", F32, 3, 20000, 25, NN_LAWS, 0, "uniform", {}),
    ("f32 select k=31", F32, 3, 20000, 31, NN_LAWS, 2000, "uniform", {}),
    ("f32 select k=21 n=4095", F32, 3, 4095, 21, NN_LAWS, 0, "uniform", {}),
    ("f32 select k=12 n=4095", F32, 3, 4095, 12, NN_LAWS, 300, "uniform", {}),
    ("f32 2d select k=21", F32, 2, 20000, 21, NN_LAWS, 0, "uniform", {}),
    ("f32 2d select k=31", F32, 2, 20000, 31, NN_LAWS, 1000, "uniform", {}),
    ("f32 k=1", F32, 3, 20000, 1, (0, 2), 0, "uniform", {}),
    ("f32 2d k=1", F32, 2, 5000, 1, (2,), 500, "uniform", {}),
    # fp32 Ksel at its k and n edges (item 5)
    ("f32 ksel k=2", F32, 3, 20000, 2, NN_LAWS, 0, "uniform", {}),
    ("f32 ksel k=24", F32, 3, 20000, 24, NN_LAWS, 1000, "uniform", {}),
    ("f32 ksel k=21 n=4096", F32, 3, 4096, 21, NN_LAWS, 0, "uniform", {}),
    ("f32 ksel k=12 n=4096", F32, 3, 4096, 12, (0,), 300, "uniform", {}),
    # fp32 Exact (item 4): k >= 32, every law
    ("f32 exact k=32", F32, 3, 20000, 32, (0, 1, 2, 3), 0, "uniform", {}),
    ("f32 2d exact k=32", F32, 2, 20000, 32, (2, 3), 500, "uniform", {}),
    # compact support (item 5): Cs2, Cs and Cs64 at k = 2 and 31
    ("f32 cs2 k=2", F32, 3, 20000, 2, (2,), 0, "uniform", {}),
    ("f32 cs2 k=31", F32, 3, 20000, 31, (2,), 2000, "uniform", {}),
    ("f32 2d cs k=2", F32, 2, 20000, 2, (2,), 0, "uniform", {}),
    ("f32 2d cs k=31", F32, 2, 20000, 31, (2,), 1000, "uniform", {}),
    ("f64 cs64 k=2", F64, 3, 20000, 2, (2,), 0, "uniform", {}),
    ("f64 cs64 k=31", F64, 3, 20000, 31, (2,), 2000, "uniform", {}),
    ("f64 2d cs64 k=31", F64, 2, 20000, 31, (2,), 0, "uniform", {}),
    ("f64 cs64wave k=31", F64, 3, 20000, 31, (2,), 0, "uniform", {"WTP_BALL64": "0"}),
    ("f64 clipped k=1", F64, 3, 20000, 1, (2,), 0, "uniform", {}),
    ("f64 clipped k=32", F64, 3, 20000, 32, (2,), 0, "uniform", {}),
    # F64Ksel at k = 2 and its k = 22 / 23 edge, and the n edge; the fp64 Exact route (item 4)
    ("f64 f64ksel k=2", F64, 3, 20000, 2, NN_LAWS, 0, "uniform", {}),
    ("f64 f64ksel k=22", F64, 3, 20000, 22, NN_LAWS, 1000, "uniform", {}),
    ("f64 exact k=23", F64, 3, 20000, 23, NN_LAWS, 0, "uniform", {}),
    ("f64 exact k=31", F64, 3, 20000, 31, NN_LAWS, 0, "uniform", {}),
    ("f64 exact k=21 n=4095", F64, 3, 4095, 21, NN_LAWS, 0, "uniform", {}),
    ("f64 f64ksel k=21 n=4096", F64, 3, 4096, 21, (0,), 0, "uniform", {}),
    ("f64 2d exact k=21", F64, 2, 20000, 21, NN_LAWS, 300, "uniform", {}),
    # lists under stress: mass ties, a coincident group larger than k, a dense cluster in a sparse cloud
    ("f32 select k=31 lattice", F32, 3, 4913, 31, (0,), 0, "lattice", {}),
    ("f32 ksel k=24 lattice", F32, 3, 4913, 24, (1,), 0, "lattice", {}),
    ("f32 cs2 k=31 lattice", F32, 3, 4913, 31, (2,), 0, "lattice", {}),
    ("f32 select k=28 coincident", F32, 3, 20000, 28, (0,), 0, "coincident", {}),
    ("f32 ksel k=2 coincident", F32, 3, 20000, 2, (1,), 0, "coincident", {}),
    ("f32 cs2 k=31 coincident", F32, 3, 20000, 31, (2,), 0, "coincident", {}),
    ("f32 2d select k=31 coincident", F32, 2, 20000, 31, (3,), 0, "coincident", {}),
    ("f32 select k=28 cluster", F32, 3, 20000, 28, (1,), 0, "cluster", {}),
    ("f64 f64ksel k=22 lattice", F64, 3, 4913, 22, (0,), 0, "lattice", {}),
    ("f64 f64ksel k=2 coincident", F64, 3, 20000, 2, (3,), 0, "coincident", {}),
    ("f64 cs64 k=31 coincident", F64, 3, 20000, 31, (2,), 0, "coincident", {}),
    ("f64 exact k=23 cluster", F64, 3, 20000, 23, (1,), 0, "cluster", {}),
]


def knn_cases():
    return [pytest.param(dt, dim, n, k, inc, data, id=label) for label, dt, dim, n, k, inc, data in KNN_CELLS]


def sweep_cases():
    return [pytest.param(dt, dim, n, k, kind, nf, data, env, id=f"{label} law{kind}")
            for label, dt, dim, n, k, laws, nf, data, env in SWEEP_CELLS for kind in laws]


# ---- data -----------------------------------------------------------------------------------------------------------

def make_cloud(wtp, data, n, dim, dtype, seed):
    """The cell's points.  lattice: 17^3 (70^2 in 2-D) at spacing 1/16, every distance shell a mass tie (n is the
    lattice's).  coincident: 48 copies of one point, more than any k the cells ask for.  cluster: 3000 points in a
    cube of edge 1e-4 inside the unit cloud.  collapsing (fp64): eight groups of 36 points 1e-9 apart — distinct in
    fp64, one point in the fp32 copy — and a 12^3 unit lattice moved by 1e3."""
    if data == "lattice":
        m = 17 if dim == 3 else 70
        g = np.stack(np.meshgrid(*[np.arange(m, dtype=np.float64)] * dim, indexing="ij"), -1).reshape(-1, dim)
        assert len(g) == n
        return (g / 16.0).astype(dtype)
    x = wtp.synth.uniform(n, dim, dtype, seed)
    if data == "coincident":
        x[100:148] = x[100]
    elif data == "cluster":
        x[2000:5000] = x[2000] + dtype(1e-4) * (x[2000:5000] - dtype(0.5))
    elif data == "collapsing":
        assert dtype == np.float64 and dim == 3
        g = np.stack(np.meshgrid(*[np.arange(12, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)
        x[n - len(g):] = g + 1e3
        step = np.array([1.0, 0.5, 0.25]) * 1e-9
        for c in range(8):
            lo = 500 + 1000 * c
            x[lo:lo + 36] = x[lo] + np.arange(36)[:, None] * step
        assert len(np.unique(x, axis=0)) == n
    elif data != "uniform":
        raise ValueError(data)
    return x


def _oracle_method(n):
    return "kdtree" if n > 2000 else "brute"


def _knn_exact_path(wtp, monkeypatch, x, k, inc):
    monkeypatch.setenv("WTP_FORCE_GENERIC", "1")
    try:
        with wtp.Context(0) as c:
            return c.knn(x, k, include_self=inc, return_dist=True)
    finally:
        monkeypatch.delenv("WTP_FORCE_GENERIC")


def _sweep(wtp, x, n_fixed, s, force, k, alo, amax):
    with wtp.Context(0) as c:
        with c.relax(x, n_fixed, s, force, k, alo, amax) as sess:
            st = sess.step(True)
            return st, sess.positions(), sess.point_data()


# ---- KNN --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dim,n,k,inc,data", knn_cases())
def test_knn_route_matches_oracle_and_exact_path(ctx, O, wtp, monkeypatch, dtype, dim, n, k, inc, data):
    x = make_cloud(wtp, data, n, dim, dtype, 20261016 + 7 * k + n)
    idx, dist = ctx.knn(x, k, include_self=inc, return_dist=True)
    oi, od = O.knn(x, k, inc, _oracle_method(n))
    route = knn_route(dtype, dim, k, inc, n)
    bad = int((idx != oi).any(axis=1).sum())
    assert np.array_equal(idx, oi), f"{route}: {bad} rows differ from the oracle"
    assert np.array_equal(dist, od), f"{route}: distances differ from the oracle"
    ei, ed = _knn_exact_path(wtp, monkeypatch, x, k, inc)
    assert np.array_equal(idx, ei) and np.array_equal(dist, ed), f"{route}: differs from the exact path"


# ---- sweeps -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dim,n,k,kind,n_fixed,data,env", sweep_cases())
def test_sweep_route_matches_oracle(O, wtp, monkeypatch, dtype, dim, n, k, kind, n_fixed, data, env):
    x = make_cloud(wtp, data, n, dim, dtype, 20261017 + 11 * k + kind)
    s = float(n) ** (-1.0 / dim)
    alo, amax = s / 2000, s / 20
    force = LAWS[kind]
    route = sweep_route(dtype, dim, k, kind, n, ball64=env.get("WTP_BALL64", "1") != "0")
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    st, p, pd = _sweep(wtp, x, n_fixed, s, force, k, alo, amax)
    for key in env:
        monkeypatch.delenv(key)
    ref = O.relax_sweep(x, n_fixed, s, kind, force["beta"], force["u0"], force["gamma"], k, alo, amax)
    n_move = n - n_fixed
    assert st["n_move"] == n_move, route
    assert np.array_equal(pd["nn_id"], ref["nn_id"]), f"{route}: nearest-neighbour ids differ from the oracle"
    assert np.array_equal(pd["nn_dist"], ref["nn_dist"]), f"{route}: nearest-neighbour distances differ from the oracle"
    f64 = np.dtype(dtype) == np.float64
    if f64 and kind == 3:
        # LennardJones: pow() of the device library and of the host's differ in the last place; the exact path's
        # rows carry the device's pow() too, so the route must equal it bit for bit
        monkeypatch.setenv("WTP_FORCE_GENERIC", "1")
        est, ep, epd = _sweep(wtp, x, n_fixed, s, force, k, alo, amax)
        monkeypatch.delenv("WTP_FORCE_GENERIC")
        assert np.array_equal(p, ep) and np.array_equal(pd["forces"], epd["forces"]), f"{route}: differs from the exact path"
        assert st["max_force"] == est["max_force"], route
        assert np.abs(p - ref["p"]).max() <= 1e-12 * s, route
        assert np.allclose(pd["forces"], ref["forces"], rtol=1e-12, atol=0), route
        assert st["max_force"] == pytest.approx(float(ref["forces"].max()), rel=1e-12), route
    elif f64:
        assert np.array_equal(p, ref["p"]), f"{route}: positions differ from the oracle"
        assert np.array_equal(pd["forces"], ref["forces"]), f"{route}: forces differ from the oracle"
        assert st["max_force"] == float(ref["forces"].max()), route
    else:
        err = np.abs(p - ref["p"]).max() / s
        assert err <= 2e-5, f"{route}: positions differ from the oracle by {err} spacings"
        assert np.allclose(pd["forces"], ref["forces"], rtol=2e-4, atol=1e-6), f"{route}: forces differ from the oracle"
        assert st["max_force"] == pytest.approx(float(ref["forces"].max()), rel=2e-4), route
    if k >= 2:  # (k = 1: the list holds the point itself only — no neighbour, no pair)
        sp = np.full(n, s, dtype)
        _, s1, s2 = O.dnn_cv(ref["nn_dist"], sp, n_fixed)
        rel = 1e-12 if f64 else 1e-6
        assert st["sum_u"] == pytest.approx(s1, rel=rel) and st["sum_u2"] == pytest.approx(s2, rel=rel), route
        cp = O.closest_pair(ref["nn_dist"], ref["nn_id"], sp, n_fixed)
        assert {st["argmin_i"], st["argmin_j"]} == {cp["idx_a"], cp["idx_b"]}, route
        assert st["argmin_r"] == pytest.approx(cp["r"], rel=0, abs=0), route
    else:
        assert np.array_equal(p, x[n_fixed:]) and st["max_force"] == 0.0, route
    # route witness (module docstring)
    fb = st["n_fallback"]
    print(f"[route] {route} n={n} k={k} law={kind} data={data}: n_fallback={fb}")
    if route == "Exact":
        assert fb == 0, "the Exact route hands nothing back"
    elif kind == CLIPPED and k == 2:
        # the support ball u0*s holds more than k = 2 points for most queries: the compact-support kernels cannot
        # certify those (n_lim > K in wtp_brick.hip, its kin in wtp_cs2.hip and wtp_brick64.hip) and hand them back
        assert fb > 0, f"{route}: a compact-support route at k = 2 hands queries back"
    elif data in ("uniform", "coincident") and k >= 2:
        assert fb <= n_move // 10, f"{route}: {fb} of {n_move} queries went to the exact path"
        if data == "coincident":
            assert fb > 0, f"{route}: coincident points must reach the exact path"
    # (lattice ties at the cut and a cluster that overfills the bricks send most queries to the exact path by design)
