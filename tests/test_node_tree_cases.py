"""No-GPU checks of the node octree's model (node_tree_cases.py): every case has the property it is there for; the
reference's in-place balance sweep and the library's Jacobi rounds reach the same tree; the leaves tile the root box, no
interior leaf is touched by a triangle's box, find_leaf finds every leaf from its centre; the header declares the entry
points and the built library and the package export them."""
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


def test_header_library_and_package_export_the_placements(wtp):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wtp.h")).read(), flags=re.S)
    lib = ctypes.CDLL(wtp.SO_PATH)
    for name in ("wtp_node_place", "wtp_node_place_get", "wtp_node_place_get_dev"):
        assert re.search(rf"\bint\s+{name}\s*\(", txt) and hasattr(lib, name), name
    assert "wtp_node_place_info" in txt and callable(wtp.NodeOctree.place)
    for meth in ("node_place", "node_place_get", "node_place_get_dev"):
        assert callable(getattr(wtp.Context, meth))
