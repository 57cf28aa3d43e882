"""Host check of the case table of test_gpu_spacing_edges.py, with the oracle and numpy alone: the tie queries tie, the
d = 0 queries give 0, every run of 64 of the mixed case holds a near-wall and a far query, the list of m covers every
shape of the bucketed tree, the clustered clouds give the tiles their comment states, and the grid-stride case exceeds
one pass of the grid."""
import numpy as np
import pytest

import test_gpu_spacing_edges as E
from test_gpu_spacing_edges import CASES, F32, F64, LL, M_LIST, N_LIST, make_case


def _case(pred):
    return [c for c in CASES if pred(c)]


def _min_dist(O, x, b):
    """1-NN distance through the oracle: LogLike with base_size 1 and growth_rate 1 is x / (1 + x), inverted here."""
    v = O.spacing_loglike(x, b, 1.0, 1.0).astype(np.float64)
    return v / (1.0 - v)


def _d2(x, b):
    T = x.dtype.type
    x3 = np.zeros((len(x), 3), T)
    b3 = np.zeros((len(b), 3), T)
    x3[:, : x.shape[1]] = x
    b3[:, : b.shape[1]] = b
    return E._d2_rows(x3, b3)


def session_grid(x, k, rho_direct=0.0, min_cell=0.0, ctx_rho=9.0):
    """Cells per axis of a relax session's first (measured) hash build of the cloud x: grid_setup_kernel (wtp_hash.hip)
    inside the three rounds of build_hash_tuned (wtp_tune.hip), for a route with the occupancy rho_direct (0: the k-NN
    default) and the cell-edge floor min_cell.  The quantile box the tuner may lay over the bulk is not restated: on the
    clouds below it cuts 0.05 % of the points per side off a box the boundary points fill evenly, which moves no count
    here by more than a cell per axis (test_clustered_clouds_give_the_stated_tiles checks that the stated tiles hold with that slack).
    Nothing on the device reports the grid a session used: this restatement is the only evidence that the clustered
    clouds reach both clamps of the tile height, so a change to the tuner (wtp_tune.hip) or to grid_setup_kernel means
    re-deriving it, and the clouds with it."""
    T = x.dtype.type
    n, dim = x.shape
    lo, hi = x.min(0).astype(np.float64), x.max(0).astype(np.float64)
    ext = np.zeros(3)
    ext[:dim] = hi - lo
    emax = ext.max()
    target = max(rho_direct, 1.0) if rho_direct > 0 else max((0.381 if dim == 3 else 0.436) * k * (ctx_rho / 8.0), 1.0)
    k_cap = int(rho_direct * 21.0 / ctx_rho) if rho_direct > 0 else k
    scale, prev_c, n3 = 1.0, -1.0, None
    for rnd in range(3):
        vol = float(np.prod(np.maximum(ext[:dim], emax * 1e-6)))
        c = (target * vol / n) ** (1.0 / dim) * scale
        c = max(c, min_cell)
        rho_cap = max(ctx_rho * (max(k_cap, 1) / 21.0), 1.0)                 # cell_capacity
        cap = int(min(n / rho_cap * 1.6 / scale ** 3 + 4096.0, 8.0 * n + 4096.0))
        for _ in range(400):
            n3 = [min(int(np.floor(ext[a] / c) + 1.0), 4096) if a < dim else 1 for a in range(3)]
            if all(np.floor(ext[a] / c) + 1.0 <= 4096 for a in range(dim)) and n3[0] * n3[1] * n3[2] <= cap:
                break
            c *= 1.08
        cT = T(c)
        inv_c = T(1) / cT
        cell = np.zeros((n, 3), np.int64)
        for a in range(dim):                                                 # cell_coord (wtp_device.hpp)
            fl = np.floor((x[:, a] - T(lo[a])) * inv_c)
            cell[:, a] = np.clip(fl, 0, n3[a] - 1).astype(np.int64)
        cnt = np.bincount((cell[:, 2] * n3[1] + cell[:, 1]) * n3[0] + cell[:, 0]).astype(np.float64)
        rho_eff = float((cnt * cnt).sum() / cnt.sum())                       # occupancy_kernel
        excess = (rho_eff - 1.0) / target
        if not excess > 1.6 or rnd == 2:
            break
        if prev_c > 0 and not float(cT) < prev_c * 0.999:
            break                                                            # a floor binds: shrinking changes nothing
        prev_c = float(cT)
        scale = max(scale * max((1.15 / excess) ** (1.0 / 3.0), 0.3), 0.02)
    return n3


@pytest.mark.parametrize("dtype,dim", [(F32, 3), (F64, 3), (F32, 2), (F64, 2)])
def test_tie_queries_tie_and_self_queries_give_zero(O, dtype, dim):
    b, x = make_case(dtype, dim, "symmetric", 0, "ties", 257)
    d2 = _d2(x, b)
    ties = (d2 == d2.min(1, keepdims=True)).sum(1)
    assert (ties >= 2).all(), "every tie query has two boundary points at exactly the minimal d2"
    assert ties[0] >= 2 * dim and (x[0] == 0.5).all(), "the centre ties across every face"
    assert np.array_equal(np.sort(b, 0), np.sort(1 - b, 0)) and len(b) == (384 if dim == 3 else 32)
    for label, dt, dm, bkind, m, qkind, n in _case(lambda c: c[5] == "self" and c[1] == dtype and c[2] == dim):
        bb, xx = make_case(dt, dm, bkind, m, qkind, n)
        assert np.array_equal(bb, xx) and (O.spacing_loglike(xx, bb, *LL) == 0).all(), label


@pytest.mark.parametrize("dtype,dim", [(F32, 3), (F64, 3), (F32, 2), (F64, 2)])
def test_mixed_case_has_a_near_and_a_far_query_in_every_run_of_64(O, dtype, dim):
    (case,) = _case(lambda c: c[5] == "mixed" and c[1] == dtype and c[2] == dim)
    b, x = make_case(*case[1:])
    d = _min_dist(O, x, b)
    assert len(x) % 64 not in (0, 1)
    for r0 in range(0, len(x), 64):
        run = d[r0:r0 + 64]
        assert (run < 0.02).sum() == 1 and (run > 0.3).sum() == len(run) - 1, f"run at {r0}"


def test_degenerate_boundaries_are_what_they_claim():
    for dim in (3, 2):
        b = E.boundary("copies", 40, dim)
        assert len(b) == 40 and len(np.unique(b, axis=0)) == 1
        b = E.boundary("collinear", 33, dim)
        assert len(b) == 33 and len(np.unique(b[:, 0])) == 33 and (np.ptp(b[:, 1:], axis=0) == 0).all()
        b = E.boundary("coplanar", 0, dim)
        u, cnt = np.unique(b, axis=0, return_counts=True)
        assert np.ptp(b[:, -1]) == 0 and (cnt == 2).sum() == -(-len(u) // 5) and cnt.max() == 2
        b = E.boundary("translated", 255, dim)
        assert b.min() >= 100 and np.float32(b).min() >= 100
    for kind in ("far1e3", "far1e6"):
        b = E.faces(1000, 3)
        q = E.queries(kind, 257, b, 3)
        away = np.linalg.norm(q - 0.5, axis=1)
        assert (away > 0.99 * float(kind[3:])).all() and (q < 0).any()
    assert (E.queries("negative", 257, E.faces(33, 3), 3) < 0).all()
    q = E.queries("uniform", 257, E.faces(255, 3), 3)
    assert q.min() < -0.1 and q.max() > 1.1 and q.min() >= -0.2 - 1e-9 and q.max() <= 1.2 + 1e-9


def test_m_list_covers_every_shape_of_the_bucketed_tree():
    assert M_LIST == (1, 2, 3, 14, 15, 16, 17, 30, 31, 32, 33, 47, 63, 64, 255, 1000) and E.KD_BUCKET == 15
    shape = {m: E.kd_shape(m) for m in M_LIST}
    assert all((shape[m] == "bucket-root") == (m <= 15) for m in M_LIST)
    assert shape[16] == shape[31] == "two-buckets" and shape[17] == shape[30] == "two-buckets"
    assert shape[32] == shape[33] == shape[47] == "mixed"
    assert shape[63] == shape[64] == shape[255] == shape[1000] == "deep"
    assert set(shape.values()) == {"bucket-root", "two-buckets", "mixed", "deep"}
    for m in list(M_LIST) + [40, 33, 384, 77]:               # the runs partition the nodes: every node in exactly one bucket
        roots, sz = E.kd_bucket_roots(m)
        assert sz[0] == m and all(1 <= sz[r] <= 15 for r in roots)
        covered = np.zeros(m, int)
        for r in roots:
            todo = [r]
            while todo:
                j = todo.pop()
                covered[j] += 1
                todo += [c for c in (2 * j + 1, 2 * j + 2) if c < m]
        inner = [i for i in range(m) if sz[i] > 15]
        assert (covered[inner] == 0).all() and (np.delete(covered, inner) == 1).all() and sum(sz[r] for r in roots) == m - len(inner)
    assert [E.kd_left_size(n) for n in (1, 2, 3, 16, 31, 32, 33, 47)] == [0, 1, 1, 8, 15, 16, 17, 31]
    # bottom-up sizes of the heap order, as kd_build_host computes them, agree with the top-down ones
    for m in (17, 47, 255):
        sz = np.zeros(m, int)
        for i in range(m - 1, -1, -1):
            sz[i] = 1 + (sz[2 * i + 1] if 2 * i + 1 < m else 0) + (sz[2 * i + 2] if 2 * i + 2 < m else 0)
        assert np.array_equal(sz, E.kd_sizes(m))


def test_table_covers_every_m_n_and_kind_in_both_types_and_dimensions():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids))
    for dt in (F32, F64):
        for dim in (3, 2):
            mine = _case(lambda c: c[1] == dt and c[2] == dim)
            assert {c[4] for c in mine if c[3] == "faces" and c[5] == "uniform" and c[6] == 257} >= set(M_LIST)
            assert {c[6] for c in mine if c[5] == "uniform"} >= set(N_LIST)
            assert {c[3] for c in mine} == {"faces", "copies", "collinear", "coplanar", "symmetric", "translated"}
            assert {c[5] for c in mine} == {"uniform", "self", "far1e3", "far1e6", "ties", "mixed", "negative"}
    assert E.boundary_size("copies", 40, 3) == 40 and E.boundary_size("collinear", 33, 2) == 33
    (big,) = _case(lambda c: c[6] > 100000)
    assert big[6] == E.N_STRIDE > E.SP_MAX_BLOCKS * E.SP_THREADS and big[6] % 64 == 1 and big[4] == 33
    assert max(c[6] for c in CASES if c is not big) <= 353


def test_clustered_clouds_give_the_stated_tiles(O):
    for name, c in E.CLUSTERED.items():
        b, v = E.clustered_cloud(name)
        x = np.concatenate([b, v])
        centre = np.array([0.3, 0.6, 0.45])
        in_ball = np.linalg.norm(v.astype(np.float64) - centre, axis=1) <= 0.05 + 1e-6
        assert int(0.8 * len(v)) <= in_ball.sum() <= 0.81 * len(v) and len(v) <= 6000 and len(b) <= 1500
        assert (x.min(0) == 0).all() and (x.max(0) == 1).all()
        if name == "sparse":                                 # Select: the k-NN default occupancy, no floor (wtp_relax.hip route_grid)
            assert len(x) < 4096 and c["force"]["kind"] == 3 and c["dtype"] == F32
            n3 = session_grid(x, 21)
        else:                                                # Cs64: 3.5 points per cell, the floor 1.1 u0 mean(spacing); the
            assert c["dtype"] == F64 and c["force"]["kind"] == 2 and 2 * len(b) >= len(x)   # crowded points are no majority
            law = c["law"]
            typ = float(O.spacing_boundary_layer(x, b, law["p0"], law["p1"], law["p2"]).astype(np.float64).mean())
            assert 1.0 / 3.0 < 1.1 * typ < 0.5
            n3 = session_grid(x, 21, rho_direct=3.5, min_cell=1.1 * c["force"]["u0"] * min(typ, law["p1"]))
            assert n3 == [3, 3, 3]
        assert E.tile_shape(len(x), n3) == c["tiles"], (name, n3)
        if name == "sparse":                                 # a cell more or less per axis (the quantile box) changes nothing
            for slack in (-1, 1):
                assert E.tile_shape(len(x), [k + slack for k in n3]) == c["tiles"]
            assert n3[0] % c["tiles"][0] != 0 and 6 * len(x) < n3[0] * n3[1] * n3[2] <= 8 * len(x) + 4096
    assert E.CLUSTERED["sparse"]["tiles"][1] == 8 and E.CLUSTERED["dense"]["tiles"][1] == 1   # both clamps of H
    # the formula at its edges
    assert E.tile_shape(1000, [10, 10, 10]) == (6, 5, 5) and E.tile_shape(1000, [40, 40, 1])[2] == 1
    assert E.tile_shape(10 ** 6, [4, 4, 4]) == (1, 1, 1) and E.tile_shape(10, [64, 64, 64]) == (20, 8, 8)
