"""The node octree on the device (include/wtp.h: wtp_node_tree_build, _get, _locate, _clear; host mirror
nodetree.NodeOctree) against the numpy model of node_tree_cases.py.  The model is run over the library's own signed
distances (mesh_query) and spacing values (spacing_eval), so every refinement, balance and class decision has to agree
bit for bit; the integral is held to math.fsum of the model's terms."""
import math

import numpy as np
import pytest

import node_tree_cases as N

pytestmark = pytest.mark.gpu

F32, F64 = N.F32, N.F64
ALL = [(name, dt) for name in N.CASES for dt in N.case_dtypes(name)]
IDS = [f"{name}-{np.dtype(dt).name}" for name, dt in ALL]
INT_KEYS = ("n_leaves", "n_interior", "n_boundary", "n_exterior", "n_boxes", "depth_max", "n_levels", "balance_rounds")


def _set(wtp, ctx, name, dtype):
    v, t = N.mesh_of(name, dtype)
    ctx.mesh_set(v, t)
    return N.CASES[name], wtp.sampling._sampler_spacing(N.library_spacing(wtp, name, dtype))


def _model(ctx, name, dtype, case, law):
    """The model over the library's own distances and spacing values, and the box wtp_mesh_bounds reports."""
    v, t = N.mesh_of(name, dtype)
    h_fn = (lambda p: ctx.spacing_eval(law, p)) if isinstance(law, dict) else (lambda p: np.full(len(p), dtype(law), dtype=dtype))
    return N.build(v, t, h_fn, case["alpha"], case["ratio"], sd_fn=lambda p: ctx.mesh_query(p, want=("sd",))["sd"],
                   bbox=ctx.mesh_bounds())


@pytest.mark.parametrize("name,dtype", ALL, ids=IDS)
def test_tree_equals_the_model(wtp, ctx, name, dtype):
    case, law = _set(wtp, ctx, name, dtype)
    info = ctx.node_tree_build(law, case["alpha"], case["ratio"])
    got = ctx.node_tree_get(info["n_leaves"])
    m = _model(ctx, name, dtype, case, law)
    print(f"{name} {np.dtype(dtype).name}: " + " ".join(f"{k}={info[k]}" for k in INT_KEYS + ("host_syncs", "integral", "h_min")))
    for k in INT_KEYS:
        assert info[k] == m["info"][k], k
    assert np.array_equal(got["depth"], m["depth"]) and np.array_equal(got["cell"], m["cell"])
    assert np.array_equal(got["cls"], m["cls"]) and got["cls"].dtype == np.int8
    assert got["h"].dtype == dtype and np.array_equal(got["h"], m["h"])
    for k in ("origin", "root_size", "absolute_min", "h_min"):
        assert info[k] == m["info"][k], k
    assert abs(info["integral"] - m["info"]["integral"]) <= 1e-12 * m["info"]["integral"]
    assert info["max_points_auto"] == min(math.ceil(1.5 * info["integral"]), 2 ** 63 - 1)     # saturates: Float64 clamps reach 1e23
    assert 0 < info["host_syncs"] <= info["n_levels"] + info["balance_rounds"] + 4
    # the oracle's tree, where its distances decide as the library's do (they are held equal by test_gpu_mesh.py)
    assert all(info[k] == N.model_run(name, dtype)["info"][k] for k in INT_KEYS)
    # two builds give the same bytes, the integral included
    info2 = ctx.node_tree_build(law, case["alpha"], case["ratio"])
    got2 = ctx.node_tree_get(info2["n_leaves"])
    assert all(info2[k] == info[k] for k in info if k != "host_syncs")
    assert all(got2[k].tobytes() == got[k].tobytes() for k in got)


@pytest.mark.parametrize("name,dtype", [("cube_uniform", F32), ("corner_graded", F32), ("corner_graded", F64), ("slab", F64),
                                        ("cube_shallow", F32), ("cube_far", F32), ("min_ratio_stop", F64),
                                        ("deep_loglike", F32), ("deep_loglike", F64), ("loglike_on_centre", F32)])
def test_locate_equals_the_model(wtp, ctx, name, dtype):
    case, law = _set(wtp, ctx, name, dtype)
    info = ctx.node_tree_build(law, case["alpha"], case["ratio"])
    m = _model(ctx, name, dtype, case, law)
    pts = N.locate_points(m)       # leaf centres (deep and shallow leaves side by side), splitting planes, faces, outside
    want = N.locate(m, pts)
    got = ctx.node_tree_locate(pts)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(got[:info["n_leaves"]], np.arange(info["n_leaves"])) and (got[-5:] == -1).all()
    # points of the other type are converted once, as the mesh queries do
    other = F64 if dtype == F32 else F32
    assert np.array_equal(ctx.node_tree_locate(pts.astype(other)), N.locate(m, pts.astype(other)))
    assert len(ctx.node_tree_locate(np.zeros((0, 3), dtype=dtype))) == 0


def test_argument_and_state_errors(wtp, ctx):
    from whatsthepoint_jl_amd import _lib as L

    def state(call):
        with pytest.raises(wtp.WtpError) as e:
            call()
        assert e.value.code == L.WTP_ERR_STATE

    ctx.mesh_clear()
    state(lambda: ctx.node_tree_build(0.1))                              # no mesh
    state(lambda: ctx.node_tree_get(1))
    case, law = _set(wtp, ctx, "cube_uniform", F32)
    state(lambda: ctx.node_tree_get(1))                                  # no tree yet
    state(lambda: ctx.node_tree_locate(np.zeros((1, 3), dtype=F32)))
    for kw in (dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(node_min_ratio=0.0),
               dict(node_min_ratio=-0.1), dict(node_min_ratio=1.5), dict(node_min_ratio=float("nan"))):
        with pytest.raises(wtp.WtpArgumentError):
            ctx.node_tree_build(0.1, **kw)
    for h in (float("nan"), float("inf")):
        with pytest.raises(wtp.WtpArgumentError, match="not finite"):
            ctx.node_tree_build(h)
    per_point = L.SpacingDesc()
    per_point.kind = L.WTP_SPACING_PER_POINT
    with pytest.raises(wtp.WtpArgumentError, match="CONSTANT, LOGLIKE or BOUNDARY_LAYER"):
        ctx.node_tree_build(None, spacing_desc=per_point)
    unknown = L.SpacingDesc()
    unknown.kind = 7
    with pytest.raises(wtp.WtpArgumentError):
        ctx.node_tree_build(None, spacing_desc=unknown)
    # a law that is not a number at a box centre: the BoundaryLayer law with a NaN bulk value
    bad = wtp.sampling._sampler_spacing(wtp.BoundaryLayerSpacing(np.zeros((1, 3), dtype=F32), 0.01, 0.3, 0.1))
    bad = dict(bad, p1=float("nan"))
    try:
        with pytest.raises(wtp.WtpArgumentError):
            ctx.node_tree_build(bad)
    finally:
        state(lambda: ctx.node_tree_get(1))                              # a failed build leaves no tree
    # a value <= eps only stops refinement
    info = ctx.node_tree_build(0.0)
    assert info["n_leaves"] == 1 and ctx.node_tree_get(1)["h"][0] == np.sqrt(np.finfo(F32).eps)
    info = ctx.node_tree_build(law, case["alpha"], case["ratio"])
    assert info["n_leaves"] == 512
    with pytest.raises(wtp.WtpArgumentError):
        ctx.node_tree_locate(np.zeros((2, 2), dtype=F32))
    # the placement: nothing to read before one, and a rebuild, a clear and a new mesh drop it
    state(lambda: ctx.node_place_get(1))
    state(ctx.node_place_get_dev)
    for kw in (dict(placement=3), dict(placement=-1), dict(max_points=0), dict(max_points=2 ** 31 + 1), dict(boundary_oversampling=0.0),
               dict(boundary_oversampling=-1.0), dict(boundary_oversampling=float("nan")), dict(boundary_oversampling=float("inf")),
               dict(boundary_oversampling=1e12, max_points=10 ** 6), dict(seed=2 ** 24)):
        with pytest.raises(wtp.WtpArgumentError):
            ctx.node_place(**{**dict(placement="random", max_points=100), **kw})
    state(lambda: ctx.node_place_get(1))                                 # a refused call leaves no placement
    assert ctx.node_place("lattice", 100)["n_points"] == 100 and len(ctx.node_place_get(100)["leaf"]) == 100
    ctx.node_tree_build(law, case["alpha"], case["ratio"])
    state(lambda: ctx.node_place_get(1))                                 # the placement dropped by a rebuild
    ctx.node_place("random", 10)
    ctx.node_tree_clear()
    state(lambda: ctx.node_tree_get(1))
    state(lambda: ctx.node_place(0, 10))
    state(lambda: ctx.node_place_get(1))
    ctx.node_tree_build(law, case["alpha"], case["ratio"])
    ctx.node_place("random", 10)
    v, t = N.mesh_of("cube_uniform", F32)
    ctx.mesh_set(v, t)                                                   # the same mesh again still drops the tree
    state(lambda: ctx.node_tree_get(1))
    state(lambda: ctx.node_place_get(1))
    ctx.node_tree_build(law, case["alpha"], case["ratio"])
    ctx.mesh_clear()
    state(lambda: ctx.node_tree_get(1))


def test_tree_and_fill_do_not_touch_each_other(wtp, ctx):
    case, law = _set(wtp, ctx, "cube_uniform", F32)
    fill = ctx.mesh_fill(0.15, 0.75, None, 10 ** 6, 200, 7, 0)
    info = ctx.node_tree_build(law, case["alpha"], case["ratio"])         # between a fill and its read-out
    placed = ctx.node_place("jittered", 300, 2.0, 5)                      # and a placement
    pts = ctx.mesh_fill_get(fill["n_points"])
    tree = ctx.node_tree_get(info["n_leaves"])
    fill2 = ctx.mesh_fill(0.15, 0.75, None, 10 ** 6, 200, 7, 0)           # and a fill between a build and its read-out
    tree2 = ctx.node_tree_get(info["n_leaves"])
    got = ctx.node_place_get(placed["n_points"])                          # ... and between a placement and its read-out
    pts2 = ctx.mesh_fill_get(fill2["n_points"])
    assert fill["n_points"] == fill2["n_points"] > 50
    assert all(pts[k].tobytes() == pts2[k].tobytes() for k in pts)
    assert all(tree[k].tobytes() == tree2[k].tobytes() for k in tree)
    ctx.node_place("jittered", 300, 2.0, 5)
    assert all(ctx.node_place_get(300)[k].tobytes() == got[k].tobytes() for k in got) and placed["n_points"] == 300
    ctx.mesh_sample(0.15, 0.75, 10 ** 6, 200, 7, 0)
    assert ctx.node_tree_get(info["n_leaves"])["cell"].tobytes() == tree["cell"].tobytes()


def test_node_octree_mirror(wtp, ctx):
    v, t = N.mesh_of("slab", F64)
    tree = wtp.NodeOctree((v, t), wtp.ConstantSpacing(0.1), ctx=ctx)
    # Orthtree's automatic node_min_ratio: (h_min / alpha) over the largest extent
    assert tree.node_min_ratio == (0.1 / 2.0) / 1.0 and tree.alpha == 2.0
    m = N.build(v, t, lambda p: np.full(len(p), 0.1), 2.0, tree.node_min_ratio,
                sd_fn=lambda p: ctx.mesh_query(p, want=("sd",))["sd"], bbox=ctx.mesh_bounds())
    lv = tree.leaves()
    assert len(tree) == m["info"]["n_leaves"] and np.array_equal(lv["cell"], m["cell"]) and np.array_equal(lv["cls"], m["cls"])
    ctr = N._centres(m["root"], m["depth"], m["cell"])
    assert np.array_equal(lv["centre"], ctr) and np.array_equal(tree.find_leaf(ctr), np.arange(len(tree)))
    assert np.allclose(lv["lo"] + lv["size"][:, None] / 2, ctr, rtol=0, atol=1e-12) and (lv["size"] == 1.02 / 2.0 ** lv["depth"]).all()
    assert tree.find_leaf(ctr[3]) == 3 and tree.find_leaf(np.array([5.0, 5.0, 5.0])) == -1
    assert tree.estimate_volume_points() == math.ceil(1.5 * tree.info["integral"]) > 0
    # another tree takes the context; the first one comes back when it is asked
    other = wtp.NodeOctree((v, t), 0.3, ctx=ctx)
    assert len(other) < len(tree) and np.array_equal(tree.find_leaf(ctr), np.arange(len(tree)))
    assert tree.info["n_leaves"] == m["info"]["n_leaves"]
    bl = wtp.BoundaryLayerSpacing(np.zeros((1, 3)), 0.05, 0.3, 0.2)
    assert wtp.NodeOctree((v, t), bl, ctx=ctx).node_min_ratio == (0.05 / 2.0) / 1.0
    with pytest.raises(wtp.WtpArgumentError, match="alpha must be positive"):
        wtp.NodeOctree((v, t), 0.1, alpha=0.0, ctx=ctx)


def test_discretize_with_an_orthtree_sizes_the_run_from_the_tree(wtp, ctx):
    """discretize(bnd, spacing; alg = Orthtree(mesh; spacing)) with max_points left to the tree (test/octree.jl's cube item):
    the cap is _estimate_volume_points of the node octree, and under it the run is the default fill.  The reference's 1.5
    headroom is sized for its front (about 1.1 / h^3); the dart thrower at factor 0.75 saturates near 1.7 / h^3, so the
    automatic cap ends the run (a prefix of the saturated one, spread over the whole domain); only a cap of the caller's own
    that truncates is warned of."""
    import warnings

    v, t = N.mesh_of("cube_uniform", F64)
    centres = v[t].mean(axis=1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                    # the automatic cap ending the run is no truncation to warn of
        cloud = wtp.discretize(wtp.PointBoundary(centres), wtp.ConstantSpacing(0.15), (v, t), alg=wtp.Orthtree(),
                               max_points=None, ctx=ctx)
    tree = cloud.volume.node_tree
    cap = tree.estimate_volume_points()
    assert cap == math.ceil(1.5 * tree.info["integral"]) == 472 and tree.node_min_ratio == 0.075
    # h_box = 0.255 at depth 2 is the first <= 2 h = 0.3: 64 leaves of 1.02^3 / 64 each, none exterior
    assert len(tree) == 64 and abs(tree.info["integral"] - 1.02 ** 3 / 0.15 ** 3) < 1e-9 * tree.info["integral"]
    assert len(cloud.volume) == cap and cloud.volume.fill_info["stop_reason"] == 2
    with pytest.warns(UserWarning, match="truncated by max_points"):
        plain = wtp.discretize(wtp.PointBoundary(centres), wtp.ConstantSpacing(0.15), (v, t), max_points=cap, ctx=ctx)
    assert np.array_equal(plain.volume.points(), cloud.volume.points())
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                    # a cap of one's own: the run saturates
        full = wtp.discretize(centres, 0.15, (v, t), alg=wtp.Orthtree(), max_points=2000, ctx=ctx)
    assert cap < len(full.volume) < 2000 and full.volume.fill_info["stop_reason"] == 1
    assert np.array_equal(full.volume.points()[:cap], cloud.volume.points()) and len(full.volume.node_tree) == 64
    with pytest.warns(UserWarning, match="truncated by max_points"):
        few = wtp.discretize(centres, 0.15, (v, t), alg=wtp.Orthtree(alpha=1.0, factor=1.0, node_min_ratio=1e-6),
                             max_points=7, ctx=ctx)
    assert len(few.volume) == 7 and len(few.volume.node_tree) == 512 and few.volume.fill_r[0] == 0.15
