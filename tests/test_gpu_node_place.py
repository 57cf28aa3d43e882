"""The per-leaf placements on the device (include/wtp.h: wtp_node_place, wtp_node_place_get*; host mirror
NodeOctree.place, discretize(alg=Orthtree(placement=...))) against the numpy model of node_tree_cases.py, replayed from
the W_int and W_ns the library reports: points, leaves and counts bit for bit; against the oracle's brute force: every
returned point inside the mesh, every candidate the oracle puts outside absent."""
import numpy as np
import pytest

import node_tree_cases as N
import oracle

pytestmark = pytest.mark.gpu

F32, F64 = N.F32, N.F64
PLACEMENTS = list(N.PLACEMENTS)
KEYS = ("n_points", "n_interior", "n_candidates", "n_accepted", "n_deficit", "placement")
SEED = 1234


def _tree(wtp, ctx, name, dtype):
    """The case's tree resident in ctx, and the model of it over the library's own distances and spacing values."""
    v, t = N.mesh_of(name, dtype)
    ctx.mesh_set(v, t)
    case, law = N.CASES[name], wtp.sampling._sampler_spacing(N.library_spacing(wtp, name, dtype))
    ctx.node_tree_build(law, case["alpha"], case["ratio"])
    h_fn = (lambda p: ctx.spacing_eval(law, p)) if isinstance(law, dict) else (lambda p: np.full(len(p), dtype(law), dtype=dtype))
    return N.build(v, t, h_fn, case["alpha"], case["ratio"], sd_fn=lambda p: ctx.mesh_query(p, want=("sd",))["sd"],
                   bbox=ctx.mesh_bounds())


def _replay(ctx, m, placement, max_points, over, seed, info):
    return N.place(m, placement, max_points, over, seed, lambda p: ctx.mesh_query(p, want=("inside",))["inside"],
                   W=(info["W_int"], info["W_ns"]))


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name,dtype,max_points,over", [("cube_uniform", F32, 1500, 2.0), ("cube_uniform", F64, 700, 1.5),
                                                        ("corner_graded", F32, 900, 2.0), ("corner_graded", F64, 600, 3.0),
                                                        ("cavity", F32, 1200, 2.0), ("cavity", F32, 10, 2.0),
                                                        ("cube_uniform", F32, 1, 2.0), ("slab", F64, 400, 0.5)])
def test_placement_equals_the_model(wtp, ctx, name, dtype, max_points, over, placement):
    m = _tree(wtp, ctx, name, dtype)
    info = ctx.node_place(placement, max_points, over, SEED)
    got = ctx.node_place_get(info["n_points"])
    want = _replay(ctx, m, placement, max_points, over, SEED, info)
    print(f"{name} {np.dtype(dtype).name} {placement}: " + " ".join(f"{k}={info[k]}" for k in KEYS + ("W_int", "W_ns", "host_syncs")))
    w = m["terms"].astype(F64)
    for key, cls in (("W_int", N.INT), ("W_ns", N.BND)):                  # the reported sums, to the model's fsum
        ref = float(np.sum(w[m["cls"] == cls])) if (m["cls"] == cls).any() else 0.0
        assert abs(info[key] - ref) <= 1e-12 * max(ref, 1.0)
    for k in KEYS:
        assert info[k] == want["info"][k], k
    assert got["xyz"].dtype == dtype and np.array_equal(got["leaf"], want["leaf"]) and np.array_equal(got["xyz"], want["xyz"])
    assert info["n_points"] == max_points and 0 < info["host_syncs"] < 16
    assert N.in_leaf(m, got["xyz"], got["leaf"]).all()
    # the oracle's brute force: every returned point is inside; every candidate it puts outside is absent
    v, t = N.mesh_of(name, dtype)
    assert oracle.mesh_query(v, t, got["xyz"])["inside"].all()
    cand, _, _ = want["candidates"]
    out = cand[~oracle.mesh_query(v, t, cand)["inside"]] if len(cand) else cand
    have = {p.tobytes() for p in got["xyz"][info["n_interior"]:info["n_interior"] + info["n_accepted"]]}
    assert not any(p.tobytes() in have for p in out)
    if placement == "lattice":
        ni = info["n_interior"]
        assert N.on_cell_centres(m, got["xyz"][:ni], got["leaf"][:ni]).all()
    if name == "cavity" and max_points == 10:                             # most leaves get no point
        assert m["info"]["n_leaves"] >= 1000
    # two calls return identical bytes; another seed does not (the lattice's points move with its counts)
    info2 = ctx.node_place(placement, max_points, over, SEED)
    got2 = ctx.node_place_get(info2["n_points"])
    assert all(info2[k] == info[k] for k in info if k != "host_syncs") and all(got2[k].tobytes() == got[k].tobytes() for k in got)
    if max_points > 10:
        ctx.node_place(placement, max_points, over, SEED + 1)
        assert ctx.node_place_get(max_points)["xyz"].tobytes() != got["xyz"].tobytes()


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name,dtype", [("needle", F32), ("needle", F64), ("cube_shallow", F32)])
def test_without_an_interior_leaf_the_result_is_short(wtp, ctx, name, dtype, placement):
    m = _tree(wtp, ctx, name, dtype)
    assert m["info"]["n_interior"] == 0
    info = ctx.node_place(placement, 300, 2.0, SEED)
    want = _replay(ctx, m, placement, 300, 2.0, SEED, info)
    got = ctx.node_place_get(info["n_points"])
    assert info["W_int"] == 0.0 and info["n_interior"] == 0 and info["n_deficit"] == 0 and info["n_candidates"] == 600
    # the needle fills 0.24 % of its box; the shallow cube's one leaf is 94 % inside, so its candidates alone fill the run
    assert info["n_points"] == info["n_accepted"] and (info["n_points"] < 300 if name == "needle" else info["n_points"] == 300)
    assert all(info[k] == want["info"][k] for k in KEYS)
    assert np.array_equal(got["xyz"], want["xyz"]) and np.array_equal(got["leaf"], want["leaf"])


def test_device_read_out(wtp, ctx):
    import torch

    _tree(wtp, ctx, "cube_uniform", F32)
    info = ctx.node_place("jittered", 257, 2.0, SEED)
    got = ctx.node_place_get(257)
    xyz = torch.empty((257, 3), dtype=torch.float32, device="cuda")
    leaf = torch.empty(257, dtype=torch.int64, device="cuda")
    ctx.node_place_get_dev(xyz.data_ptr(), leaf.data_ptr())
    torch.cuda.synchronize()
    assert info["n_points"] == 257 and np.array_equal(xyz.cpu().numpy(), got["xyz"]) and np.array_equal(leaf.cpu().numpy(), got["leaf"])
    assert np.array_equal(ctx.node_place_get(257, want=("leaf",))["leaf"], got["leaf"])


def test_placements_through_the_host_mirror(wtp, ctx):
    """NodeOctree.place and discretize(..., alg=Orthtree(placement=...)) on the cube of test/octree.jl's items."""
    v, t = N.mesh_of("cube_uniform", F64)
    centres = v[t].mean(axis=1)
    tree = wtp.NodeOctree((v, t), wtp.ConstantSpacing(0.1), node_min_ratio=1e-6, ctx=ctx)
    vol = tree.place("jittered", 800, seed=SEED, ctx=ctx)
    assert len(vol) == 800 and vol.place_info["n_points"] == 800 and len(vol.place_leaf) == 800
    assert np.array_equal(tree.find_leaf(vol.points()), vol.place_leaf)   # find_leaf agrees with the leaf each point came from
    assert oracle.mesh_query(v, t, vol.points())["inside"].all()
    auto = tree.place(":lattice", ctx=ctx)
    assert len(auto) == tree.estimate_volume_points()
    for bad, msg in (("grid", "placement must be"), ("bridson", "fill_volume")):
        with pytest.raises(wtp.WtpArgumentError, match=msg):
            tree.place(bad)
    with pytest.raises(wtp.WtpArgumentError, match="boundary_oversampling must be positive"):
        tree.place("random", 10, boundary_oversampling=0.0)
    cloud = wtp.discretize(wtp.PointBoundary(centres), wtp.ConstantSpacing(0.15), (v, t), alg=wtp.Orthtree(placement="jittered"),
                           max_points=None, ctx=ctx)
    cap = cloud.volume.node_tree.estimate_volume_points()
    assert len(cloud.volume) == cap == 472 and len(cloud.boundary) == 12 and cloud.volume.place_info["placement"] == 1
    assert oracle.mesh_query(v, t, cloud.volume.points())["inside"].all()
    few = wtp.discretize(centres.astype(F32), 0.15, (v, t), alg=wtp.Orthtree("random", boundary_oversampling=4.0), max_points=50, ctx=ctx)
    assert len(few.volume) == 50 and few.volume.points().dtype == F32 and few.volume.place_info["n_candidates"] > 0
    assert len(few.volume.place_leaf) == 50 and few.volume.node_tree is not None
