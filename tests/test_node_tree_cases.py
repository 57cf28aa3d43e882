"""No-GPU checks of the node octree's model (node_tree_cases.py): every case has the property it is there for; the
reference's in-place balance sweep and the library's Jacobi rounds reach the same tree; the leaves tile the root box, no
interior leaf is touched by a triangle's box, find_leaf finds every leaf from its centre; the models on arrays
(build_arrays, place_arrays) equal the set and loop models byte for byte; the big cases meet the chunk conditions they
are there for; the header declares the entry points and the built library and the package export them."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import node_tree_cases as N

F32, F64 = N.F32, N.F64
ALL = [(name, dt) for name in N.CASES for dt in N.case_dtypes(name)]
IDS = [f"{name}-{np.dtype(dt).name}" for name, dt in ALL]
ENTRY_POINTS = ["wtp_node_tree_build", "wtp_node_tree_get", "wtp_node_tree_locate", "wtp_node_tree_clear"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,dtype", ALL, ids=IDS)
def test_tree_invariants(name, dtype):
    m = N.model_run(name, dtype)
    d, c, cls, info = m["depth"], m["cell"], m["cls"], m["info"]
    assert info["n_leaves"] <= 20000
    # the leaves tile the root box exactly, and the leaf order is strictly ascending
    assert sum(Fraction(1, 8 ** int(x)) for x in d) == 1
    assert info["n_boxes"] == info["n_leaves"] + (info["n_leaves"] - 1) // 7
    key = N.morton_start(d, c)
    assert (key[1:] > key[:-1]).all()
    assert info["n_interior"] + info["n_boundary"] + info["n_exterior"] == info["n_leaves"]
    # balanced: no leaf that may subdivide needs to
    assert not any(N.needs_balancing(b, m["internal"]) and N.can_subdivide(m["root"], b[0]) for b in m["leaves"])
    # no INTERIOR leaf is touched by a triangle's box (they are trusted without an inside test)
    lo = np.concatenate([N.bounds(m["root"], int(x), y[None])[0] for x, y in zip(d[cls == N.INT], c[cls == N.INT])]
                        or [np.zeros((0, 3), dtype=dtype)])
    hb = np.array([N.h_box(m["root"], int(x)) for x in d[cls == N.INT]], dtype=dtype)
    assert not m["geo"].touch(lo, lo + hb[:, None]).any()
    # h and the integral
    assert (m["h"] >= np.sqrt(np.finfo(dtype).eps)).all() and m["h"].dtype == dtype
    assert info["integral"] > 0 and info["h_min"] == float(m["h"][cls != N.EXT].min())


@pytest.mark.parametrize("name,dtype", ALL, ids=IDS)
def test_in_place_and_jacobi_balance_agree(name, dtype):
    """Splitting only ever adds boxes, so the fixed point does not depend on the order in which leaves are looked at."""
    m = N.model_run(name, dtype)
    leaves, internal = N.balance_in_place(m["root"], m["leaves0"], m["internal0"], m["order"])
    assert leaves == m["leaves"] and internal == m["internal"]
    # and in the reverse creation order
    leaves, internal = N.balance_in_place(m["root"], m["leaves0"], m["internal0"], m["order"][::-1])
    assert leaves == m["leaves"] and internal == m["internal"]


@pytest.mark.parametrize("name,dtype", ALL, ids=IDS)
def test_locate_finds_every_leaf_from_its_centre(name, dtype):
    m = N.model_run(name, dtype)
    pts = N.locate_points(m)
    got = N.locate(m, pts)
    n = m["info"]["n_leaves"]
    assert np.array_equal(got[:n], np.arange(n))
    assert (got[-5:] == -1).all() and (got[:-5] >= 0).all()


def test_every_case_has_the_property_it_is_there_for():
    for dt in N.DTYPES:
        u = N.model_run("cube_uniform", dt)
        assert (u["depth"] == 3).all() and u["info"]["n_leaves"] == 512 and u["info"]["balance_rounds"] == 1
        assert u["info"]["n_interior"] == 216 and u["info"]["n_boundary"] == 296
        s = N.model_run("slab", dt)
        assert min(s["info"][k] for k in ("n_interior", "n_boundary", "n_exterior")) > 0
        assert s["facts"]["balance_splits"] > 0 and len(set(s["depth"])) > 1
        r = N.model_run("cube_shallow", dt)
        assert r["info"]["n_leaves"] == 1 and r["depth"][0] == 0 and r["cls"][0] == N.BND
        g = N.model_run("corner_graded", dt)
        assert g["info"]["balance_rounds"] >= 4 and g["facts"]["balance_splits"] >= 50   # three rounds that split, and more
        assert g["info"]["depth_max"] == 6 and g["info"]["n_leaves"] > len(g["leaves0"])
        e = N.model_run("needle", dt)
        assert e["facts"]["touch_only"] > 0 and e["info"]["n_interior"] == 0 and e["facts"]["demoted"] > 0
        k = N.model_run("min_ratio_stop", dt)
        assert k["info"]["depth_max"] == 4 < g["info"]["depth_max"] and k["facts"]["balance_splits"] > 0
        assert N.h_box(k["root"], 4) <= k["root"]["absmin"] < N.h_box(k["root"], 3)
        # can_subdivide never blocks a balance split: a leaf that needs one has a neighbour two levels deeper, so it is
        # at least two levels above the deepest box the size test allows
        assert all(N.model_run(n, dt)["facts"]["balance_blocked"] == 0 for n in N.CASES if dt in N.case_dtypes(n))
    c = N.model_run("cavity", F32)
    assert c["facts"]["demoted_interior"] > 0 and 1000 < c["info"]["n_leaves"] < 10000
    f = N.model_run("cube_far", F32)
    assert np.array_equal(f["cell"], N.model_run("cube_uniform", F32)["cell"]) and f["info"]["origin"][0] > 999
    for dt in N.DTYPES:
        sqrt_eps = np.sqrt(np.finfo(dt).eps)
        q = N.model_run("deep_loglike", dt)
        i, fq = q["info"], q["facts"]
        assert (i["n_leaves"], i["n_interior"], i["n_boundary"], i["n_exterior"]) == (8352, 7000, 1352, 0)
        # depth 20 is reached by the refinement, not by the balance
        assert i["depth_max"] == 20 == fq["depth_before_balance"] and int((q["depth"] == 20).sum()) == 152
        assert (i["balance_rounds"], fq["balance_splits"], fq["balance_blocked"]) == (6, 218, 0)
        assert int((q["h"] == sqrt_eps).sum()) == (1564 if dt == F32 else 0)
        assert i["h_min"] == (float(sqrt_eps) if dt == F32 else float(q["h"].min())) and (q["h"] >= sqrt_eps).all()
        # the cap and nothing else stops the tree: a depth-20 leaf passes every size test of the criterion but d < 20
        root, sp = q["root"], N.spacing_of("deep_loglike", dt)
        deep = q["depth"] == 20
        hraw = N.law_h(sp, N._centres(root, q["depth"][deep], q["cell"][deep]))
        hb = N.h_box(root, 20)
        assert hb > root["absmin"] and ((hraw > np.finfo(dt).eps) & (hb > dt(0.5) * hraw)).any()
        assert N.h_box(root, 20) > i["absolute_min"] and not N.can_subdivide(root, 20) and N.can_subdivide(root, 19)
        o = N.model_run("loglike_on_centre", dt)
        assert (o["info"]["n_leaves"], o["info"]["depth_max"], o["info"]["balance_rounds"]) == (4656, 5, 2)
        box = (3, N.chain_cells(4)[3])
        assert N.law_h(N.spacing_of("loglike_on_centre", dt), N.bounds(o["root"], *box)[2])[0] == 0    # d = 0: h = 0 <= eps
        assert o["facts"]["balance_splits"] == 1 and box in o["leaves0"] and box in o["internal"]
        assert o["internal"] - o["internal0"] == {box}
        y = N.model_run("loglike_heavy_leaf", dt)
        at = np.nonzero((y["depth"] == 3) & (y["cell"] == N.chain_cells(4)[3]).all(axis=1))[0]
        assert len(at) == 1 and y["cls"][at[0]] == N.INT and y["h"][at[0]] == sqrt_eps and int((y["h"] == sqrt_eps).sum()) == 1
        assert box in y["leaves0"] and y["facts"]["balance_splits"] == 0 and y["info"]["n_interior"] == 258
        assert N.zero_shares(y, N.INT) == ((257, 258) if dt == F64 else (0, 258))
        assert N.zero_shares(q, N.INT) == ((152, 7000) if dt == F32 else (0, 7000))     # Float32: the depth-20 leaves
        z = N.model_run("loglike_root_centre", dt)
        assert np.array_equal(N.spacing_of("loglike_root_centre", dt)[3], np.full((1, 3), 0.5, dtype=dt))
        assert z["info"]["n_leaves"] == 1 and z["h"][0] == sqrt_eps and z["cls"][0] == N.BND
    assert not np.array_equal(N.model_run("deep_loglike", F32)["h"], N.model_run("deep_loglike", F64)["h"].astype(F32))
    assert all(np.array_equal(N.model_run("deep_loglike", F32)[k], N.model_run("deep_loglike", F64)[k]) for k in ("cell", "depth", "cls"))


def test_the_big_cases_meet_their_chunk_conditions():
    """slab_fine: the level-7 pass and the leaf count are above one chunk of 2^18 boxes and no multiple of it, so that the
    probe and the vote pass both run a full chunk and a ragged one.  cube_depth7: 8 full chunks, in closed form."""
    m = N.model_run_arrays("slab_fine", F32)
    front, n = m["facts"]["fronts"][7], m["info"]["n_leaves"]
    print(f"slab_fine: fronts={m['facts']['fronts']} n_leaves={n} by depth={np.bincount(m['depth']).tolist()} facts={m['facts']}")
    assert front > N.CHUNK and front % N.CHUNK and n > N.CHUNK and n % N.CHUNK
    assert len(m["facts"]["fronts"]) == 8 and m["info"]["balance_rounds"] > 1 and m["facts"]["balance_splits"] > 0
    assert min(m["info"][k] for k in ("n_interior", "n_boundary", "n_exterior")) > 0
    key = N.morton_start(m["depth"], m["cell"])
    assert (key[1:] > key[:-1]).all() and m["info"]["n_boxes"] == n + (n - 1) // 7
    assert int((np.float64(1) / 8 ** m["depth"].astype(np.int64)).sum() * 8 ** 7) == 8 ** 7       # the leaves tile the root (exact: powers of two)
    assert not N.needs_balancing_arrays(m["depth"].astype(np.int64), m["cell"].astype(np.int64), m["internal_depth"],
                                        m["internal_cell"]).any()
    # slab_fine_point: boxes that pass the size tests in the ragged chunk of the level-7 front and in no other place of
    # it, so that a chunk reading the first chunk's flags probes none of them; they split
    p = N.model_run_arrays("slab_fine_point", F32)
    wanted = p["facts"]["wanted"][7]
    print(f"slab_fine_point: fronts={p['facts']['fronts']} wanted at level 7={wanted.tolist()} n_leaves={p['info']['n_leaves']}")
    assert p["facts"]["fronts"][:8] == m["facts"]["fronts"] and p["facts"]["fronts"][8] == 8 * len(wanted) > 0
    assert (wanted >= N.CHUNK).all() and p["info"]["n_leaves"] > n and p["info"]["n_leaves"] % N.CHUNK and p["info"]["depth_max"] > 7
    c = N.BIG_CASES["cube_depth7"]
    root = N.root_of(np.zeros(3), np.ones(3), F32, c["ratio"])
    assert N.h_box(root, 6) > F32(c["alpha"]) * F32(c["spacing"][1]) >= N.h_box(root, 7) and 8 ** 7 == 8 * N.CHUNK
    assert 2 * N.h_box(root, 7) > F32(0.01) > N.h_box(root, 7)       # the outer shell of depth-7 cells lies in the 1 % margin


@pytest.mark.parametrize("name,dtype", ALL, ids=IDS)
def test_the_tree_on_arrays_equals_the_set_model(name, dtype):
    m, a = N.model_run(name, dtype), N.model_run_arrays(name, dtype)
    for k in ("cell", "depth", "cls", "h", "terms"):
        assert a[k].dtype == m[k].dtype and a[k].tobytes() == m[k].tobytes(), k
    assert a["info"] == m["info"] and all(a["facts"][k] == m["facts"][k] for k in m["facts"])
    assert set(zip(a["internal_depth"].tolist(), map(tuple, a["internal_cell"].tolist()))) == m["internal"]
    assert set(zip(a["leaves0_depth"].tolist(), map(tuple, a["leaves0_cell"].tolist()))) == m["leaves0"]
    # needs_balancing, leaf by leaf, on the tree before its balance
    d0, c0 = a["leaves0_depth"], a["leaves0_cell"]
    want = np.array([N.needs_balancing((int(x), tuple(int(v) for v in y)), m["internal0"]) for x, y in zip(d0, c0)], dtype=bool)
    idp = np.array([b[0] for b in m["internal0"]], dtype=np.int64)
    ic = np.array([b[1] for b in m["internal0"]], dtype=np.int64).reshape(-1, 3)
    assert np.array_equal(N.needs_balancing_arrays(d0, c0, idp, ic), want)
    assert np.array_equal(N.in_leaf_arrays(m, N._centres(m["root"], m["depth"], m["cell"]), np.arange(len(m["depth"]))),
                          np.ones(len(m["depth"]), dtype=bool))


def test_keys_round_trip_and_order():
    rng = np.random.default_rng(5)
    d = rng.integers(0, 21, 200)
    c = np.array([rng.integers(0, 1 << int(x), 3) if x else (0, 0, 0) for x in d])
    k = N.morton_start(d, c)
    assert k.dtype == np.uint64 and (k < np.uint64(1) << np.uint64(60)).all()
    # a child's lower corner is at or behind its parent's, in child order
    kids = np.array(N.children_of((3, 5, 6)))
    kk = N.morton_start(np.full(8, 4), kids)
    assert (np.diff(kk.astype(np.int64)) > 0).all() and kk[0] == N.morton_start([3], [(3, 5, 6)])[0]


def test_header_library_and_package_export_the_node_tree(wtp):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wtp.h")).read(), flags=re.S)
    lib = ctypes.CDLL(wtp.SO_PATH)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", txt), name
        assert hasattr(lib, name), name
    assert "wtp_node_tree_info" in txt
    assert wtp.NodeOctree is wtp.nodetree.NodeOctree and "NodeOctree" in wtp.__all__
    for meth in ("node_tree_build", "node_tree_get", "node_tree_locate", "node_tree_clear"):
        assert callable(getattr(wtp.Context, meth))


def test_orthtree_checks_its_arguments_like_the_reference(wtp):
    """Orthtree's guards (src/discretization/algorithms/octree.jl:115-120) with the reference's messages; discretize's
    checks that need no device."""
    a = wtp.Orthtree()
    assert (a.placement, a.alpha, a.node_min_ratio, a.boundary_oversampling, a.factor) == ("bridson", 2.0, None, 2.0, 0.75)
    assert a.is_default() and wtp.Orthtree(":jittered").placement == "jittered" and not wtp.Orthtree(alpha=1.0).is_default()
    assert "Orthtree" in wtp.__all__
    for kw, msg in ((dict(placement="grid"), "placement must be :random, :jittered, :lattice, or :bridson"),
                    (dict(alpha=0.0), "alpha must be positive"), (dict(boundary_oversampling=0.0), "boundary_oversampling must be positive"),
                    (dict(factor=-1.0), "bridson_factor must be positive"), (dict(max_growth=-0.1), "max_growth must be ≥ 0"),
                    (dict(max_growth=1.2), "max_growth > 0 is not available"), (dict(node_min_ratio=0.0), "node_min_ratio must be in")):
        with pytest.raises(wtp.WtpArgumentError, match=msg):
            wtp.Orthtree(**kw)
    square = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], dtype=F64)
    for alg in (wtp.Orthtree("lattice"), wtp.Orthtree(alpha=1.0)):       # 2-D takes the default only, under the same sentence
        with pytest.raises(wtp.WtpArgumentError, match="2D discretization supports the Orthtree fill only"):
            wtp.discretize(square, 0.1, alg=alg)
    v, t = N.mesh_of("cube_uniform", F64)
    with pytest.raises(wtp.WtpArgumentError, match="max_points = None asks for the node octree's estimate"):
        wtp.discretize(v[t].mean(axis=1), 0.1, (v, t), max_points=None)
    with pytest.raises(wtp.WtpArgumentError, match="alg must be"):
        wtp.discretize(v[t].mean(axis=1), 0.1, (v, t), alg="orthtree")
    # Orthtree's automatic node_min_ratio (octree.jl:134-159): (h_min / alpha) / the largest extent, else 1 / (4 nt^(1/3))
    oc = wtp.TriangleOctree(*N.mesh_of("slab", F64))
    assert wtp.nodetree.auto_node_min_ratio(oc, 0.1, 2.0) == wtp.nodetree.auto_node_min_ratio(oc, wtp.ConstantSpacing(0.1), 2.0) == 0.05
    assert wtp.nodetree.auto_node_min_ratio(oc, wtp.BoundaryLayerSpacing(np.zeros((1, 3)), 0.02, 0.3, 0.1), 4.0) == 0.005
    assert wtp.nodetree.auto_node_min_ratio(oc, wtp.LogLike(np.zeros((1, 3)), 0.3, 1.5), 2.0) == 1.0 / (4.0 * 12 ** (1.0 / 3.0))


# ---- the placements' model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 26, 27, 28, 64, 65])
def test_grid_divisions_is_the_smallest_cube_that_holds_n(n):
    g = N.grid_divisions(n)
    assert (g - 1) ** 3 < n <= g ** 3


@pytest.mark.parametrize("count", [0, 1, 10, 511, 512, 513, 5000])
def test_the_weighted_pick_hands_out_exactly_count(count):
    m = N.model_run("corner_graded", F64)
    member = m["cls"] == N.INT
    w = np.where(member, m["terms"].astype(F64), 0.0)
    c = N.group_counts(w, float(w.sum()), member, count, 77, N.ST_PICK_INTERIOR)
    assert c.sum() == count and not c[~member].any() and (c >= np.floor(count * w / w.sum())).all()
    # equal weights that leave every fraction at zero fall back to the uniform rule and still hand out count
    flat = N.group_counts(member.astype(F64), float(member.sum()), member, int(member.sum()) * 3, 77, N.ST_PICK_INTERIOR)
    assert (flat[member] == 3).all() and flat.sum() == member.sum() * 3


@pytest.mark.parametrize("placement", list(N.PLACEMENTS))
@pytest.mark.parametrize("name,dtype,max_points", [("cube_uniform", F32, 700), ("corner_graded", F64, 333), ("slab", F64, 200),
                                                   ("cavity", F32, 10), ("cube_uniform", F64, 1), ("cube_shallow", F32, 50)])
def test_placement_returns_max_points_inside_the_named_leaves(name, dtype, max_points, placement):
    m = N.model_run(name, dtype)
    got = N.place(m, placement, max_points, 2.0, 11, N.oracle_inside(name, dtype))
    info = got["info"]
    if info["W_int"] > 0:
        assert info["n_points"] == max_points == len(got["xyz"]) == len(got["leaf"])
    else:                                                             # cube_shallow: the root alone, all candidates
        assert info["n_interior"] == 0 and info["n_deficit"] == 0 and info["n_points"] == info["n_accepted"] <= max_points
        assert info["n_candidates"] == 2 * max_points
    assert info["n_interior"] + info["n_accepted"] + info["n_deficit"] == info["n_points"]
    assert N.in_leaf(m, got["xyz"], got["leaf"]).all() and got["xyz"].dtype == dtype
    ni, na = info["n_interior"], info["n_accepted"]
    assert (m["cls"][got["leaf"][:ni]] == N.INT).all() and (m["cls"][got["leaf"][ni:ni + na]] == N.BND).all()
    assert (m["cls"][got["leaf"][ni + na:]] == N.INT).all()
    if placement == "lattice" and ni:
        assert N.on_cell_centres(m, got["xyz"][:ni], got["leaf"][:ni]).all()


PLACE_ROWS = [("cube_uniform", F32, 700), ("corner_graded", F64, 333), ("slab", F64, 200), ("cavity", F32, 10), ("cube_uniform", F64, 1),
              ("cube_shallow", F32, 50), ("deep_loglike", F32, 1000), ("deep_loglike", F64, 1000), ("deep_loglike", F64, 3),
              ("loglike_heavy_leaf", F64, 1000), ("loglike_heavy_leaf", F32, 333)]


@pytest.mark.parametrize("placement", list(N.PLACEMENTS))
@pytest.mark.parametrize("name,dtype,max_points", PLACE_ROWS)
def test_the_placement_on_arrays_equals_the_loop_model(name, dtype, max_points, placement):
    m = N.model_run(name, dtype)
    for seed in (11, 0, 2 ** 24 - 1)[:3 if max_points == 333 else 1]:
        want = N.place(m, placement, max_points, 2.0, seed, N.oracle_inside(name, dtype))
        got = N.place_arrays(m, placement, max_points, 2.0, seed, N.oracle_inside(name, dtype))
        assert got["info"] == want["info"]
        for k in ("xyz", "leaf"):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
        for x, y in zip(got["candidates"], want["candidates"]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert np.array_equal(N.in_leaf_arrays(m, got["xyz"], got["leaf"]), N.in_leaf(m, want["xyz"], want["leaf"]))


def test_the_integer_helpers_on_arrays_equal_python_integers():
    rng = np.random.default_rng(9)
    x = np.concatenate([rng.integers(0, 2 ** 64, 500, dtype=np.uint64), np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1], dtype=np.uint64)])
    for y in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345, 2 ** 64 - 1, 4294967296 * 7000):
        assert N.mulhi64(x, y).tolist() == [(int(v) * y) >> 64 for v in x]
    for seed, stage in ((0, 0), (1234, 3), (2 ** 24 - 1, 5)):
        j = np.array([0, 1, 255, 2 ** 20 + 3, 2 ** 31, 2 ** 36 - 1], dtype=np.uint64)
        for a in range(3):
            assert N.draw_arrays(seed, stage, j, a).tolist() == [N.draw(seed, stage, int(v), a) for v in j]
            assert N.uniform_arrays(F32, seed, stage, j, a).tolist() == [float(N.uniform(F32, seed, stage, int(v), a)) for v in j]
    n = np.concatenate([np.arange(1, 1100), np.array([10 ** 6 - 1, 10 ** 6, 10 ** 6 + 1, 2 ** 31])]).astype(np.int64)
    assert N.grid_divisions_arrays(n)[:1099].tolist() == [N.grid_divisions(int(v)) for v in n[:1099]]
    assert N.grid_divisions_arrays(n)[1099:].tolist() == [100, 100, 101, 1291]
    for dt in (F32, F64):
        a = rng.integers(0, 4, (500, 3)).astype(dt)
        a[0] = (0.0, -0.0, np.nan)
        b = np.concatenate([a[::7], rng.integers(0, 4, (40, 3)).astype(dt) + dt(0.5)])
        have = {r.tobytes() for r in b}
        assert N.rows_in(a, b).tolist() == [r.tobytes() in have for r in a] and N.rows_in(a, b).any() and not N.rows_in(a, b).all()
        assert not N.rows_in(a, b[:0]).any() and len(N.rows_in(a[:0], b)) == 0
    d = rng.integers(0, 21, 300)
    c = np.array([rng.integers(0, 1 << int(v), 3) if v else (0, 0, 0) for v in d])
    code = N.box_code(d, c)
    assert len(np.unique(code)) == len({(int(a), tuple(b)) for a, b in zip(d, c.tolist())})
    assert np.array_equal(N._compact(N._spread(c[:, 0])), c[:, 0].astype(np.uint64))


def test_header_library_and_package_export_the_placements(wtp):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wtp.h")).read(), flags=re.S)
    lib = ctypes.CDLL(wtp.SO_PATH)
    for name in ("wtp_node_place", "wtp_node_place_get", "wtp_node_place_get_dev"):
        assert re.search(rf"\bint\s+{name}\s*\(", txt) and hasattr(lib, name), name
    assert "wtp_node_place_info" in txt and callable(wtp.NodeOctree.place)
    for meth in ("node_place", "node_place_get", "node_place_get_dev"):
        assert callable(getattr(wtp.Context, meth))
