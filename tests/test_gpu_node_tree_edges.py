"""The node octree and its placements (csrc/wtp_node_tree.hip; mesh_point_class_kernel and mesh_box_touch_kernel of
csrc/wtp_mesh.hip) at the sizes where their code takes another path, against the array models of node_tree_cases.py
(build_arrays, uniform_tree, place_arrays: proved equal to the set and loop models by test_node_tree_cases.py):

  slab_fine      a level of 294 912 boxes and 309 968 leaves: nt_probe_pass runs a full chunk of 2^18 boxes and a ragged
                 one in the refinement and in the vote; nt_finish_kernel and np_weights_kernel (2^18 threads) stride twice
  slab_fine_point  the same with boxes that pass the size tests in the ragged chunk only (at slab_fine's level 7 none does)
  cube_depth7    2 097 152 leaves in closed form: 8 full chunks, two trips of every nt_grid loop (2^20 threads) over leaves
  deep_loglike   the depth cap ends the refinement; Float32 cells of 2^-20 of the root; clamped h beside unclamped
  placements     2^20 + 3 points (second stride trips, more than 2048 scan tiles: p_tile regrown between queued kernels),
                 scans that end on, before and behind a tile seam, shares and base counts of zero, the end seeds

Everything is equality but the integral: it is held to 1e-12 of math.fsum, because all terms are positive and the longest
chain of additions is 2 per thread + 8 levels of the block tree + at most 1 024 host partials, under 1 040 * 2^-53 =
1.2e-13 relative.  Every test prints the counts the device reported.

Mutations run once against this module, each giving wrong values from in-bounds reads, and the test that failed:

  `d_need + f0` -> `d_need` in nt_probe_pass          test_slab_fine_takes_two_chunks_the_second_ragged[slab_fine_point]
      (depth_max 7, not 9: the 8 wanted boxes of the ragged chunk went unprobed; slab_fine itself cannot tell, its level 7
      wants no box)
  `cls[f0 + b]` -> `cls[b]` in nt_vote_kernel          ...[slab_fine]: n_interior 238 169 against 246 016
  the sqrt_eps clamp removed in nt_finish_kernel      test_h_is_clamped_inside_a_graded_tree[deep_loglike]: h differs
  np_points_kernel's stride loop cut to one trip      test_a_million_candidates_all_of_them_needed[random]: n_points
      988 505 against 988 508 (with oversampling 2 the room is full before candidate 2^20 and nothing shows)

Mutations argued from the code, not run:

  the depth cap `d < kNtMaxDepth` of nt_criterion_kernel removed: a depth-20 box of deep_loglike that passes the size
      tests would split, and its children's keys shift by 3 * (20 - 21), a negative count: undefined, so not run.  The
      cap is what stops deep_loglike (test_every_case_has_the_property_it_is_there_for shows a depth-20 leaf that passes
      every other test), so any tree without it differs from the model in test_tree_equals_the_model[deep_loglike-*].
  `d < kNtMaxDepth - 1` of nt_balance_kernel removed: nt_internal(d + 1 = 20) would shift by s = 0 and look for a box
      deeper than 20, which no key is: the balance's answer does not change, the guard only saves the searches.  No test
      can tell, and none claims to.
  `tol + f0` -> `tol` in nt_probe_pass: the tolerance depends on the depth alone and a level's boxes share it, so only
      the vote pass, whose chunks mix depths, can tell: slab_fine's second chunk would take the tolerances of depths 2
      to 7 of the first for its depth-7 boxes, 32 times too wide for some; a class changes where a probe lies within
      that of the surface.  The slab's faces are cell faces only at z, so this is not certain to show; not claimed.
  the memset of pcls shortened or dropped: a box that is not wanted keeps the class of the chunk before, read by
      nt_probe_any_kernel only under flag[f] (wanted boxes are always written), so nothing changes; in the vote every
      box is wanted.  The memset is defensive, and no test claims it.
  `f = f0 + b` -> `b` in nt_probe_any_kernel: the second chunk's verdicts land on the first chunk's boxes.  slab_fine's
      level-7 front has flag = 0 everywhere (h_box(7) <= alpha h) and cannot tell; slab_fine_point's has 8 boxes with
      flag = 1 in the ragged chunk, whose need[] then stays what the level before left at their place (1 only for a box
      that had no probe inside or on the surface): they would not all split, and the tree would lose leaves.
  np_tile_scan_kernel starting at run = tile[0], or np_tile_apply_kernel off by one tile: every placement test compares
      leaf[] and xyz[] of points behind the first tile seam, so test_scans_that_end_at_a_tile_seam[256..] fails.
"""
import math
import time

import numpy as np
import pytest

import node_tree_cases as N
import oracle

pytestmark = pytest.mark.gpu

F32, F64 = N.F32, N.F64
INT_KEYS = ("n_leaves", "n_interior", "n_boundary", "n_exterior", "n_boxes", "depth_max", "n_levels", "balance_rounds")
PLACE_KEYS = ("n_points", "n_interior", "n_candidates", "n_accepted", "n_deficit", "placement")
PLACEMENTS = list(N.PLACEMENTS)
SEED = 1234
_MODELS = {}


def _build(wtp, ctx, name, dtype):
    """The case's mesh and tree resident in ctx.  Returns (info, the functions the model is run over)."""
    v, t = N.mesh_of(name, dtype)
    ctx.mesh_set(v, t)
    case, law = N.case_of(name), wtp.sampling._sampler_spacing(N.library_spacing(wtp, name, dtype))
    info = ctx.node_tree_build(law, case["alpha"], case["ratio"])
    h_fn = (lambda p: ctx.spacing_eval(law, p)) if isinstance(law, dict) else (lambda p: np.full(len(p), dtype(law), dtype=dtype))
    return info, dict(spacing_fn=h_fn, sd_fn=lambda p: ctx.mesh_query(p, want=("sd",))["sd"], bbox=ctx.mesh_bounds())


def _tree(wtp, ctx, name, dtype):
    """(info, model): the tree resident in ctx and its model over the library's own distances and spacing values, the
    model computed once per case and left unchanged."""
    info, fns = _build(wtp, ctx, name, dtype)
    key = (name, np.dtype(dtype).name)
    if key not in _MODELS:
        v, t = N.mesh_of(name, dtype)
        case = N.case_of(name)
        t0 = time.perf_counter()
        if name == "cube_depth7":
            _MODELS[key] = N.uniform_tree(v, t, case["spacing"][1], 7, case["ratio"], sd_fn=fns["sd_fn"], bbox=fns["bbox"])
        elif name in N.BIG_CASES:
            _MODELS[key] = N.build_arrays(v, t, fns["spacing_fn"], case["alpha"], case["ratio"], sd_fn=fns["sd_fn"], bbox=fns["bbox"])
        else:
            _MODELS[key] = N.build(v, t, fns["spacing_fn"], case["alpha"], case["ratio"], sd_fn=fns["sd_fn"], bbox=fns["bbox"])
        print(f"{name} {key[1]}: model in {time.perf_counter() - t0:.2f} s")
    return info, _MODELS[key]


def _show(name, dtype, info):
    print(f"{name} {np.dtype(dtype).name}: " + " ".join(f"{k}={info[k]}" for k in INT_KEYS + ("host_syncs", "integral", "h_min")))


def _assert_tree(ctx, info, m, dtype):
    """Leaves, classes, h and every number of the info equal the model; the integral to its derived bound."""
    got = ctx.node_tree_get(info["n_leaves"])
    for k in INT_KEYS:
        assert info[k] == m["info"][k], k
    assert np.array_equal(got["depth"], m["depth"]) and np.array_equal(got["cell"], m["cell"])
    assert got["cls"].dtype == np.int8 and np.array_equal(got["cls"], m["cls"])
    assert got["h"].dtype == dtype and np.array_equal(got["h"], m["h"])
    for k in ("origin", "root_size", "absolute_min", "h_min"):
        assert info[k] == m["info"][k], k
    assert abs(info["integral"] - m["info"]["integral"]) <= 1e-12 * m["info"]["integral"]
    assert info["max_points_auto"] == min(math.ceil(1.5 * info["integral"]), 2 ** 63 - 1)     # saturates: Float64 clamps reach 1e23
    assert 0 < info["host_syncs"] <= info["n_levels"] + info["balance_rounds"] + 4
    return got


# ---- the tree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["slab_fine", "slab_fine_point"])
def test_slab_fine_takes_two_chunks_the_second_ragged(wtp, ctx, name):
    """slab_fine: no box of the level-7 front passes the size tests.  slab_fine_point: some of its ragged chunk do, are
    probed under need + f0 and split."""
    info, m = _tree(wtp, ctx, name, F32)
    _show(name, F32, info)
    front, n = m["facts"]["fronts"][7], info["n_leaves"]
    print(f"{name}: fronts={m['facts']['fronts']} leaves by depth={np.bincount(m['depth']).tolist()} "
          f"balance_splits={m['facts']['balance_splits']} touch_only={m['facts']['touch_only']} "
          f"wanted at level 7={m['facts']['wanted'][7].tolist()}")
    if name == "slab_fine_point":
        assert len(m["facts"]["wanted"][7]) > 0 and (m["facts"]["wanted"][7] >= N.CHUNK).all() and info["depth_max"] > 7
    assert front > N.CHUNK and front % N.CHUNK and n > N.CHUNK and n % N.CHUNK      # probe and vote: a full chunk, a ragged one
    assert info["balance_rounds"] > 1 and min(info[k] for k in ("n_interior", "n_boundary", "n_exterior")) > 0
    got = _assert_tree(ctx, info, m, F32)
    # classes differ between the two chunks' leaves, so a vote written a chunk too early or late cannot pass
    assert len(set(got["cls"][:N.CHUNK].tolist())) == 3 and len(set(got["cls"][N.CHUNK:].tolist())) == 3
    info2, _ = _build(wtp, ctx, name, F32)
    got2 = ctx.node_tree_get(info2["n_leaves"])
    assert all(info2[k] == info[k] for k in info if k != "host_syncs")
    assert all(got2[k].tobytes() == got[k].tobytes() for k in got)
    ctr = N._centres(m["root"], m["depth"], m["cell"])
    assert np.array_equal(ctx.node_tree_locate(ctr), np.arange(n))


def test_cube_depth7_equals_the_closed_form(wtp, ctx):
    """8 full chunks in the last level and in the vote; every cell of depth 7 in Morton order, one balance round."""
    info, m = _tree(wtp, ctx, "cube_depth7", F32)
    _show("cube_depth7", F32, info)
    n = 8 ** 7
    assert info["n_leaves"] == n == 8 * N.CHUNK and info["n_boxes"] == n + (n - 1) // 7 and info["balance_rounds"] == 1
    assert info["n_exterior"] > 0                                      # the outer shell of cells lies wholly in the 1 % margin
    got = _assert_tree(ctx, info, m, F32)
    assert (got["depth"] == 7).all() and (got["h"] == F32(0.006)).all() and info["h_min"] == float(F32(0.006))
    code = np.arange(n, dtype=np.uint64)
    assert all(np.array_equal(got["cell"][:, a], N._compact(code >> np.uint64(a)).astype(np.int32)) for a in range(3))


@pytest.mark.parametrize("name", ["deep_loglike", "loglike_heavy_leaf", "loglike_root_centre"])
def test_h_is_clamped_inside_a_graded_tree(wtp, ctx, name):
    """Float32: h = max(h(centre), sqrt(eps)) with clamped and unclamped leaves side by side, and what is made of it."""
    info, m = _tree(wtp, ctx, name, F32)
    got = _assert_tree(ctx, info, m, F32)
    _show(name, F32, info)
    sqrt_eps = np.sqrt(np.finfo(F32).eps)
    live = got["cls"] != N.EXT
    clamped = got["h"] == sqrt_eps
    law = wtp.sampling._sampler_spacing(N.library_spacing(wtp, name, F32))
    hraw = ctx.spacing_eval(law, np.ascontiguousarray(N._centres(m["root"], m["depth"], m["cell"])))
    print(f"{name}: clamped={int(clamped.sum())} of {len(clamped)} leaves, raw h from {hraw.min()} to {hraw.max()}")
    assert (got["h"][live] >= sqrt_eps).all() and info["h_min"] == float(sqrt_eps)
    assert np.array_equal(clamped, hraw <= sqrt_eps) and (hraw < sqrt_eps).any() and np.array_equal(got["h"][~clamped], hraw[~clamped])
    if name != "loglike_root_centre":
        assert not clamped.all() and info["depth_max"] == (20 if name == "deep_loglike" else 4)
    hb = np.array([N.h_box(m["root"], int(d)) for d in range(N.MAX_DEPTH + 1)], dtype=F32)[got["depth"]]
    terms = ((hb * hb) * hb) / ((got["h"] * got["h"]) * got["h"])
    ref = math.fsum(terms[live].astype(F64).tolist())
    assert abs(info["integral"] - ref) <= 1e-12 * ref


@pytest.mark.parametrize("dtype", N.DTYPES)
def test_locate_walks_to_depth_20(wtp, ctx, dtype):
    """The model walks while the box is internal, the device always to depth 20: they have to meet at the neighbours of
    a depth-19 split plane and of a depth-20 leaf's corner, one ulp either way."""
    info, m = _tree(wtp, ctx, "deep_loglike", dtype)
    root, T = m["root"], dtype
    assert info["depth_max"] == 20
    box = max(b for b in m["internal"] if b[0] == 19)
    deep = np.nonzero(m["depth"] == 20)[0]
    anchors = [N.bounds(root, 19, np.array([box[1]]))[2][0]]
    anchors += [N.bounds(root, 20, m["cell"][i][None])[0][0] for i in (deep[0], deep[len(deep) // 2], deep[-1])]
    pts = []
    for p in anchors:
        pts.append(p)
        for a in range(3):
            for to in (-np.inf, np.inf):
                q = p.copy()
                q[a] = np.nextafter(p[a], T(to))
                pts.append(q)
    n_near = len(pts)
    for a in range(3):
        for bad in (np.inf, -np.inf, np.nan):
            q = anchors[0].copy()
            q[a] = bad
            pts.append(q)
    pts = np.ascontiguousarray(np.array(pts, dtype=dtype))
    want = N.locate(m, pts)
    got = ctx.node_tree_locate(pts)
    print(f"deep_loglike {np.dtype(dtype).name}: locate want={want.tolist()} depths={m['depth'][want[:n_near]].tolist()}")
    assert np.array_equal(got, want) and (want[:n_near] >= 0).all() and (want[n_near:] == -1).all()
    assert (m["depth"][want[:7]] == 20).all() and len(set(want[:7].tolist())) == 4    # the box's children either side of its planes
    ctr = N._centres(root, m["depth"], m["cell"])
    assert np.array_equal(ctx.node_tree_locate(ctr), np.arange(info["n_leaves"]))


# ---- the placements -----------------------------------------------------------------------------------------------------
def _place_and_check(ctx, m, name, dtype, placement, max_points, over, seed):
    """One placement against place_arrays replayed from the reported sums, in_leaf over all points, and the oracle's
    brute force: every point inside, no candidate it puts outside present.  Returns (info, points, model's result)."""
    t0 = time.perf_counter()
    info = ctx.node_place(placement, max_points, over, seed)
    got = ctx.node_place_get(info["n_points"])
    t1 = time.perf_counter()
    want = N.place_arrays(m, placement, max_points, over, seed, lambda p: ctx.mesh_query(p, want=("inside",))["inside"],
                          W=(info["W_int"], info["W_ns"]))
    print(f"{name} {np.dtype(dtype).name} {placement} max_points={max_points} seed={seed}: "
          + " ".join(f"{k}={info[k]}" for k in PLACE_KEYS + ("W_int", "W_ns", "host_syncs"))
          + f" device {t1 - t0:.2f} s model {time.perf_counter() - t1:.2f} s")
    w = m["terms"].astype(F64)
    for key, cls in (("W_int", N.INT), ("W_ns", N.BND)):
        ref = math.fsum(w[m["cls"] == cls].tolist())
        assert abs(info[key] - ref) <= 1e-12 * ref
    for k in PLACE_KEYS:
        assert info[k] == want["info"][k], k
    assert got["xyz"].dtype == dtype and got["leaf"].dtype == np.int64
    assert np.array_equal(got["leaf"], want["leaf"]) and np.array_equal(got["xyz"], want["xyz"])
    assert 0 < info["host_syncs"] < 16
    assert N.in_leaf_arrays(m, got["xyz"], got["leaf"]).all()
    v, t = N.mesh_of(name, dtype)
    assert oracle.mesh_query(v, t, got["xyz"])["inside"].all()
    cand = want["candidates"][0] if want["candidates"] is not None else got["xyz"][:0]
    out = cand[~oracle.mesh_query(v, t, cand)["inside"].astype(bool)] if len(cand) else cand
    ni, na = info["n_interior"], info["n_accepted"]
    assert not N.rows_in(out, got["xyz"][ni:ni + na]).any()
    return info, got, want


@pytest.mark.parametrize("placement", ["random", "lattice"])
def test_a_million_points_stride_twice_and_regrow_the_scan_tiles(wtp, placement):
    """2^20 + 3 points on the 512 leaves of cube_uniform: np_points_kernel, np_flags_kernel and np_compact_kernel take a
    second stride trip, and the candidates' scan has more than 2 048 tiles, which a context that has placed nothing
    larger has to regrow p_tile for between queued kernels: the context is this test's own."""
    with wtp.Context(0) as ctx:
        info, fns = _build(wtp, ctx, "cube_uniform", F32)
        case = N.CASES["cube_uniform"]
        m = N.build(*N.mesh_of("cube_uniform", F32), fns["spacing_fn"], case["alpha"], case["ratio"], sd_fn=fns["sd_fn"], bbox=fns["bbox"])
        assert info["n_leaves"] == m["info"]["n_leaves"] == 512
        pinfo, got, want = _place_and_check(ctx, m, "cube_uniform", F32, placement, 2 ** 20 + 3, 2.0, SEED)
        assert pinfo["n_candidates"] > 2 ** 20 and -(-pinfo["n_candidates"] // 256) > 2048 and pinfo["n_points"] == 2 ** 20 + 3
        assert pinfo["n_interior"] + pinfo["n_accepted"] + pinfo["n_deficit"] == pinfo["n_points"] and pinfo["n_accepted"] > 0
        again = ctx.node_place(placement, 2 ** 20 + 3, 2.0, SEED)                     # the tiles now large enough: same bytes
        got2 = ctx.node_place_get(again["n_points"])
        assert all(again[k] == pinfo[k] for k in pinfo if k != "host_syncs") and all(got2[k].tobytes() == got[k].tobytes() for k in got)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("max_points", [255, 256, 257, 65536, 65537])
def test_scans_that_end_at_a_tile_seam(wtp, ctx, max_points, placement):
    """cube_shallow is one boundary leaf, so the candidates, and the scan of their inside flags, are max_points long:
    one element before, on and behind the first tile seam, and 256 tiles against 257."""
    info, m = _tree(wtp, ctx, "cube_shallow", F32)
    assert info["n_leaves"] == 1 and info["n_boundary"] == 1
    pinfo, got, want = _place_and_check(ctx, m, "cube_shallow", F32, placement, max_points, 1.0, SEED)
    assert pinfo["n_candidates"] == max_points and pinfo["n_interior"] == 0 and pinfo["n_deficit"] == 0
    assert 0 < pinfo["n_accepted"] == pinfo["n_points"] == int(want["candidates"][2].sum())


@pytest.mark.parametrize("placement", ["random", "lattice"])
def test_a_million_candidates_all_of_them_needed(wtp, ctx, placement):
    """With oversampling 2 the room is full after the first half of the candidates and what the second stride trip wrote is
    never returned.  Here the one leaf's 2^20 + 3 candidates are all there is: every inside one is returned, those past
    2^20 too, so the second trips of np_points_kernel, np_flags_kernel and np_compact_kernel show in the result."""
    info, m = _tree(wtp, ctx, "cube_shallow", F32)
    pinfo, got, want = _place_and_check(ctx, m, "cube_shallow", F32, placement, 2 ** 20 + 3, 1.0, SEED)
    inside = want["candidates"][2]
    assert pinfo["n_candidates"] == 2 ** 20 + 3 and pinfo["n_points"] == pinfo["n_accepted"] == int(inside.sum()) < 2 ** 20 + 3
    assert inside[2 ** 20:].any() and inside[:2 ** 20].sum() < pinfo["n_accepted"]    # points from behind the first trip are returned


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("max_points", [1000, 3])
@pytest.mark.parametrize("name,dtype", [("deep_loglike", F32), ("deep_loglike", F64), ("loglike_heavy_leaf", F32), ("loglike_heavy_leaf", F64)])
def test_shares_and_base_counts_of_zero(wtp, ctx, name, dtype, max_points, placement):
    """Weights that span the clamp: base counts floor(count w / W) of zero for almost every member, integer shares
    floor(w / W 2^32) of zero inside the group, hence runs of equal running sums that a pick must step over.
    deep_loglike in Float32: the 152 depth-20 leaves (w = 2e-8 of W = 156); in Float64 no h is clamped and no share is
    zero.  loglike_heavy_leaf in Float64: one leaf of weight 6e20 and zero shares for the 257 other interior leaves."""
    info, m = _tree(wtp, ctx, name, dtype)
    zero, members = N.zero_shares(m, N.INT)
    pinfo, got, want = _place_and_check(ctx, m, name, dtype, placement, max_points, 2.0, SEED)
    c_int, c_ns = want["counts"]
    base = np.floor(float(pinfo["n_interior"]) * (np.where(m["cls"] == N.INT, m["terms"].astype(F64), 0.0) / pinfo["W_int"]))
    print(f"{name} {np.dtype(dtype).name}: zero shares {zero} of {members} interior leaves, zero base counts "
          f"{int((base[m['cls'] == N.INT] == 0).sum())}, leaves with points {int((c_int > 0).sum())} + {int((c_ns > 0).sum())}")
    assert pinfo["n_points"] == max_points
    assert 2 * int((base[m["cls"] == N.INT] == 0).sum()) > members                   # base counts of zero for most members
    if name == "deep_loglike":
        assert (zero, members) == ((152, 7000) if dtype == F32 else (0, 7000))
    else:
        assert (2 * zero > members) == (dtype == F64)                                  # the zero-share majority
        if dtype == F64:
            assert zero == members - 1 and pinfo["n_interior"] == max_points and int((c_int > 0).sum()) == 1


def test_a_search_over_three_hundred_thousand_running_sums(wtp, ctx):
    """slab_fine: np_first_above over 309 968 sums, scans of 1 211 tiles, two stride trips of np_weights_kernel."""
    info, m = _tree(wtp, ctx, "slab_fine", F32)
    assert -(-info["n_leaves"] // 256) == 1211
    pinfo, got, want = _place_and_check(ctx, m, "slab_fine", F32, "jittered", 5000, 2.0, SEED)
    assert pinfo["n_points"] == 5000 and got["leaf"].max() > N.CHUNK > got["leaf"].min()


def test_the_end_seeds(wtp, ctx):
    """Seeds 0 and 2^24 - 1, the top of seed << 40: each equals the model, and they differ."""
    info, m = _tree(wtp, ctx, "corner_graded", F64)
    res = [_place_and_check(ctx, m, "corner_graded", F64, "jittered", 600, 2.0, seed)[1] for seed in (0, 2 ** 24 - 1)]
    assert res[0]["xyz"].tobytes() != res[1]["xyz"].tobytes() and len(res[0]["xyz"]) == len(res[1]["xyz"]) == 600
