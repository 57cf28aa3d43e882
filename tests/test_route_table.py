"""Host check of the route table of test_gpu_routes.py: every KNN and sweep route is reached by a cell, and every
threshold of the dispatch has cells on both sides of it."""
import numpy as np

from test_gpu_routes import (KNN_CELLS, KNN_ROUTES, SWEEP_CELLS, SWEEP_ROUTES, knn_cases, knn_route, sweep_cases,
                             sweep_route)


def _knn():
    return [dict(dtype=np.dtype(dt), dim=dim, n=n, k=k, inc=inc, data=data, route=knn_route(dt, dim, k, inc, n))
            for _, dt, dim, n, k, inc, data in KNN_CELLS]


def _sweeps():
    return [dict(dtype=np.dtype(dt), dim=dim, n=n, k=k, kind=kind, n_fixed=nf, data=data,
                 route=sweep_route(dt, dim, k, kind, n, ball64=env.get("WTP_BALL64", "1") != "0"))
            for _, dt, dim, n, k, laws, nf, data, env in SWEEP_CELLS for kind in laws]


def test_every_route_is_reached():
    assert {c["route"] for c in _knn()} == KNN_ROUTES
    assert {c["route"] for c in _sweeps()} == SWEEP_ROUTES
    # every force law on every route it can reach: laws 0, 1, 3 on the k-nearest routes, law 2 on its own
    reached = {(c["route"], c["kind"]) for c in _sweeps()}
    for route in SWEEP_ROUTES:
        laws = {kind for r, kind in reached if r == route}
        if route.startswith("Cs"):
            assert laws == {2}, route
        elif route.startswith(("Ksel", "F64Ksel")) or route == "Select<1,21,0>":
            assert laws == {0, 1, 3}, route
        else:  # Select<1,0,0> (clipped k = 1 too) and Exact take every law
            assert laws == {0, 1, 2, 3}, route


def test_every_threshold_has_both_sides():
    knn, sw = _knn(), _sweeps()
    f32 = np.dtype(np.float32)

    def kq(c):
        return c["k"] if c["inc"] else c["k"] + 1

    def has(cells, **want):
        return any(all(f(c) if callable(f) else c[key] == f for key, f in want.items()) for c in cells)

    for side in (24, 25):  # k + self against ksel_kmax(): the k-selection layout or the brick kernel
        assert has(knn, dtype=f32, dim=3, n=lambda c: c["n"] >= 4096, k=lambda c, s=side: kq(c) == s)
        assert has(sw, dtype=f32, dim=3, n=lambda c: c["n"] >= 4096, k=side, kind=lambda c: c["kind"] != 2)
    for side in (31, 32):  # the brick kernels' list length, KNN with and without self, sweeps of every law
        for inc in (True, False):
            assert has(knn, dtype=f32, k=side, inc=inc)
        assert has(sw, dtype=f32, k=side, kind=2) and has(sw, dtype=f32, k=side, kind=lambda c: c["kind"] != 2)
    for side in (4095, 4096):  # the k-selection's n edge: fp32 KNN and sweeps, fp64 candidates and F64Ksel
        assert has(knn, dtype=f32, dim=3, n=side)
        assert has(knn, dtype=np.dtype(np.float64), dim=3, n=side)
        assert has(sw, dtype=f32, dim=3, n=side, kind=lambda c: c["kind"] != 2)
        assert has(sw, dtype=np.dtype(np.float64), dim=3, n=side, kind=lambda c: c["kind"] != 2)
    for kc in (31, 32):  # fp64 KNN: the last candidate list and the first exact one, with and without self
        for inc in (True, False):
            assert has(knn, dtype=np.dtype(np.float64), inc=inc, k=lambda c, kc=kc: kq(c) + 2 == kc)
    for side in (22, 23):  # F64Ksel's k edge
        assert has(sw, dtype=np.dtype(np.float64), dim=3, k=side, n=lambda c: c["n"] >= 4096,
                   kind=lambda c: c["kind"] != 2)
    for side in (1, 2):  # the compact-support and k-selection routes start at k = 2
        assert has(sw, dtype=f32, k=side, kind=2) and has(sw, dtype=f32, k=side, kind=lambda c: c["kind"] != 2)
        assert has(sw, dtype=np.dtype(np.float64), k=side, kind=2)
    for dim in (2, 3):
        assert has(knn, dim=dim, dtype=f32) and has(knn, dim=dim, dtype=np.dtype(np.float64))
        assert has(sw, dim=dim, dtype=f32) and has(sw, dim=dim, dtype=np.dtype(np.float64))


def test_edge_data_and_fixed_heads_are_present():
    for cells in (_knn(), _sweeps()):
        assert {"lattice", "coincident", "cluster"} <= {c["data"] for c in cells}
    assert {"collapsing"} <= {c["data"] for c in _knn()}
    assert any(c["n_fixed"] > 0 for c in _sweeps()) and any(c["k"] == 1 for c in _sweeps())
    assert max(c["n"] for c in _knn() + _sweeps()) <= 60000


def test_case_ids_are_unique():
    for cases in (knn_cases(), sweep_cases()):
        ids = [p.id for p in cases]
        assert len(ids) == len(set(ids))
