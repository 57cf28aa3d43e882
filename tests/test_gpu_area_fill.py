"""Graded Poisson-disk area fill on the device (include/wtp.h: wtp_loops_fill, wtp_loops_fill_get*, wtp_loops_fill_darts;
host mirror sampling.fill_area / discretize) against the numpy model of area_fill_cases.py: the darts and their inside
flags bit for bit, the accepted set equal to the serial loop over the library's own darts, independent of the batch
size, for both dtypes; the reference's own items (test/segment_quadtree.jl:45-73, 181-226, 256-308) through discretize."""
import warnings

import numpy as np
import pytest

import area_fill_cases as A
import loops_cases as LC
import volume_fill_cases as V

pytestmark = pytest.mark.gpu

F32, F64 = A.F32, A.F64
ALL = [(name, dt) for name in A.CASES for dt in A.case_dtypes(name)]
IDS = [f"{name}-{np.dtype(dt).name}" for name, dt in ALL]


def _set(wtp, ctx, name, dtype):
    """The case's loops resident in ctx; returns (case, the spacing as Context.loops_fill takes it, the seeds)."""
    ctx.loops_set(list(A.loops_of(name, dtype)))
    return A.CASES[name], wtp.sampling._sampler_spacing(A.library_spacing(wtp, name, dtype)), A.seeds_of(name, dtype)[0]


def _fill(ctx, case, sp, seeds, **kw):
    a = dict(factor=case["factor"], max_points=A.max_points_of(case), stall_limit=case["stall_limit"], seed=A.SEED, batch=0)
    a.update(kw)
    info = ctx.loops_fill(sp, a["factor"], seeds, a["max_points"], a["stall_limit"], a["seed"], a["batch"])
    return info, ctx.loops_fill_get(info["n_points"])


def _bytes(got):
    return b"".join(got[k].tobytes() for k in ("xy", "r", "dart"))


def _seed_r(ctx, case, sp, seeds, dtype):
    """r of the seeds as the library evaluates the case's law (the device's exp differs from numpy's by an ulp)."""
    if not len(seeds):
        return np.zeros(0, dtype=dtype)
    if case["spacing"][0] == "const":
        return np.full(len(seeds), dtype(case["factor"]) * dtype(case["spacing"][1]), dtype=dtype)
    return dtype(case["factor"]) * ctx.spacing_eval(sp, seeds)


# ---- darts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("name,dtype", [("square", F32), ("square", F64), ("star", F32), ("star", F64), ("annulus", F32),
                                        ("annulus", F64), ("wedge", F64), ("square_far", F32), ("circle_bl", F32),
                                        ("circle_bl", F64), ("sliver", F32)])
def test_darts_equal_the_model(wtp, ctx, name, dtype, first):
    case, sp, _ = _set(wtp, ctx, name, dtype)
    n = 3001
    xy, inside, r = ctx.loops_fill_darts(sp, case["factor"], A.SEED, first, n)
    mx, mi, mr = A.darts(name, dtype, first, n)
    assert xy.dtype == dtype and xy.shape == (n, 2) and np.array_equal(xy, mx) and np.array_equal(inside, mi)
    if case["spacing"][0] == "bl":   # exp() differs by an ulp between the device and the host: the bound of DESIGN.md §8f.3
        bulk = case["factor"] * case["spacing"][2]
        assert np.abs(r.astype(F64) - mr.astype(F64)).max() <= 4 * np.finfo(dtype).eps * bulk
    else:
        assert np.array_equal(r, mr)


# ---- acceptance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", ALL, ids=IDS)
def test_accepted_set_equals_the_serial_loop_over_the_librarys_darts(wtp, ctx, name, dtype):
    case, sp, seeds = _set(wtp, ctx, name, dtype)
    h = case["horizon"]
    n = A.whole_batches(h, 0)[1]                                        # the darts of every batch a run within the horizon decides
    xy, inside, r = ctx.loops_fill_darts(sp, case["factor"], A.SEED, 0, n)
    sr = _seed_r(ctx, case, sp, seeds, dtype)
    acc, n_darts, reason, n_in = A.serial(xy[:h], inside[:h], r[:h], seeds, sr, A.max_points_of(case), case["stall_limit"])
    info, got = _fill(ctx, case, sp, seeds)
    print(f"{name} {np.dtype(dtype).name}: n_points={info['n_points']} n_darts={info['n_darts']} n_inside={info['n_inside']} "
          f"batches={info['n_batches']} rounds_max={info['rounds_max']} host_syncs={info['host_syncs']}")
    assert np.array_equal(got["dart"], acc) and info["n_darts"] == n_darts and info["stop_reason"] == reason
    assert info["n_points"] == len(acc) and info["n_inside"] == n_in and info["n_seeds"] == len(seeds)
    assert got["xy"].shape == (len(acc), 2) and np.array_equal(got["xy"], xy[acc]) and np.array_equal(got["r"], r[acc])
    assert info["r_min"] == float(r[acc].min()) and info["r_max"] == float(r[acc].max())
    assert info["bbox_volume"] == A.bbox_area(name, dtype)
    # batch = 0 is the schedule of A.batch_sizes: the batch model over the same whole batches counts the same batches and rounds
    nb, whole = A.whole_batches(n_darts, 0)
    b = A.batched_run(xy[:whole], inside[:whole], r[:whole], seeds, sr, A.max_points_of(case), case["stall_limit"], 0)
    assert np.array_equal(b["acc"], acc) and b["n_inside"] == n_in and b["n_batches"] == nb
    assert (info["n_batches"], info["rounds_max"]) == (b["n_batches"], b["rounds_max"])
    if case["spacing"][0] == "const":                                   # the model's own counts
        m = A.model_run(name, dtype)
        assert np.array_equal(acc, m[3]) and (n_darts, reason, n_in) == m[4:]


def test_a_smaller_max_points_gives_a_prefix(wtp, ctx):
    case, sp, seeds = _set(wtp, ctx, "star", F32)
    _, full = _fill(ctx, case, sp, seeds)
    for m in (1, 37):
        info, got = _fill(ctx, case, sp, seeds, max_points=m)
        assert info["stop_reason"] == 2 and info["n_points"] == m and info["n_darts"] == got["dart"][-1] + 1
        assert all(np.array_equal(got[k], full[k][:m]) for k in got)


# ---- batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("square_stall200", F32), ("annulus", F64), ("circle_bl", F32), ("sliver", F64)])
def test_result_does_not_depend_on_the_batch_size(wtp, ctx, name, dtype):
    case, sp, seeds = _set(wtp, ctx, name, dtype)
    info0, got0 = _fill(ctx, case, sp, seeds, batch=0)
    assert info0["rounds_max"] >= 1 and 0 < info0["host_syncs"] < 10 ** 6 and info0["n_points"] > 50
    for batch in (63, 64, 65, 1000, 4096):
        info, got = _fill(ctx, case, sp, seeds, batch=batch)
        assert _bytes(got) == _bytes(got0), batch
        assert (info["n_darts"], info["n_inside"], info["stop_reason"], info["batch"]) == (
            info0["n_darts"], info0["n_inside"], info0["stop_reason"], batch)
        assert 1 <= info["rounds_max"] <= batch


def test_batch_of_one_dart(wtp, ctx):
    case, sp, seeds = _set(wtp, ctx, "square_max37", F32)
    info0, got0 = _fill(ctx, case, sp, seeds)
    info, one = _fill(ctx, case, sp, seeds, batch=1)                   # one host round trip per dart
    assert info["stop_reason"] == 2 and info["rounds_max"] == 1 and info["n_batches"] == info["n_darts"] == info0["n_darts"]
    assert _bytes(one) == _bytes(got0) and info["n_inside"] == info0["n_inside"]


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_two_calls_return_the_same_bits_and_the_seed_matters(wtp, ctx, dtype):
    case, sp, seeds = _set(wtp, ctx, "circle_bl", dtype)
    _, a = _fill(ctx, case, sp, seeds)
    _, b = _fill(ctx, case, sp, seeds)
    assert _bytes(a) == _bytes(b)
    _, c = _fill(ctx, case, sp, seeds, seed=A.SEED + 1)
    assert not np.array_equal(c["dart"], a["dart"])


# ---- properties, by brute force in double --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("square", F32), ("star", F32), ("star", F64), ("annulus", F32), ("annulus", F64),
                                        ("circle_bl", F32), ("circle_bl", F64), ("square_far", F32), ("seed_outside", F64),
                                        ("sliver", F32)])
def test_fill_area_properties(wtp, ctx, name, dtype):
    case = A.CASES[name]
    loops = list(A.loops_of(name, dtype))
    seeds = A.seeds_of(name, dtype)[0]
    law = A.library_spacing(wtp, name, dtype)
    vol = wtp.fill_area(loops, law, seeds=seeds if len(seeds) else None, factor=case["factor"],
                        stall_limit=case["stall_limit"], ctx=ctx)
    p, r, info = vol.points(), vol.fill_r, vol.fill_info
    assert p.dtype == dtype and p.shape == (info["n_points"], 2) and len(p) > 50 and isinstance(vol, wtp.PointVolume)
    assert LC.inside(A.index_of(name, dtype), p).all()                  # every point is inside, by the model
    sr = _seed_r(ctx, case, wtp.sampling._sampler_spacing(law), seeds, dtype)
    q, rq = np.concatenate([seeds, p]), np.concatenate([sr, r])
    ns = len(seeds)
    # no pair conflicts under the library's own expression, in the cloud's type: exact
    dx, dy = p[:, None, 0] - q[None, :, 0], p[:, None, 1] - q[None, :, 1]
    d2 = dx * dx + dy * dy
    m = np.minimum(r[:, None], rq[None, :])
    own = np.zeros((len(p), len(q)), dtype=bool)
    own[np.arange(len(p)), ns + np.arange(len(p))] = True
    assert d2.dtype == dtype and not ((d2 < m * m) & ~own).any()
    # in double every pair, and every point-seed pair, keeps min(r_i, r_j), up to the rounding of the stored differences
    slack = 8 * np.finfo(dtype).eps * float(np.abs(q).max())
    dist = np.sqrt(((p.astype(F64)[:, None] - q.astype(F64)[None]) ** 2).sum(axis=2)) + 1e30 * own
    assert (dist >= m.astype(F64) - slack).all()
    est = info["area_estimate"]
    assert est == info["bbox_volume"] * info["n_inside"] / info["n_darts"]
    exact = sum(abs(float(LC.signed_area(l.astype(F64)))) * (1 if k == 0 else -1) for k, l in enumerate(loops))
    sigma = np.sqrt(info["n_inside"] * (1 - info["n_inside"] / info["n_darts"])) / info["n_darts"] * info["bbox_volume"]
    assert abs(est - exact) <= 6 * sigma + 1e-3 * exact                # six sigma of the run's own darts


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors_leave_the_context_usable(wtp, ctx):
    from whatsthepoint_jl_amd import _lib as L
    import ctypes as C

    ctx.loops_clear()
    with pytest.raises(wtp.WtpError) as e:
        ctx.loops_fill(0.05)                                             # no loops
    assert e.value.code == L.WTP_ERR_STATE
    with pytest.raises(wtp.WtpError) as e:
        ctx.loops_fill_darts(0.05, 0.75, A.SEED, 0, 4)
    assert e.value.code == L.WTP_ERR_STATE
    case, sp, _ = _set(wtp, ctx, "square", F32)
    for call in (lambda: ctx.loops_fill_get(1), ctx.loops_fill_get_dev):  # before a successful fill (loops_set voided any)
        with pytest.raises(wtp.WtpError) as e:
            call()
        assert e.value.code == L.WTP_ERR_STATE
    bad = [dict(factor=0.0), dict(factor=-1.0), dict(factor=float("nan")), dict(factor=float("inf")), dict(stall_limit=0),
           dict(max_points=0), dict(seed=2 ** 24), dict(batch=-1), dict(batch=2 ** 24 + 1)]
    for kw in bad:
        with pytest.raises(wtp.WtpArgumentError):
            _fill(ctx, case, sp, None, **kw)
    per_point = L.SpacingDesc()
    per_point.kind = L.WTP_SPACING_PER_POINT
    with pytest.raises(wtp.WtpArgumentError):
        ctx.loops_fill(None, spacing_desc=per_point)
    with pytest.raises(wtp.WtpArgumentError):
        ctx.loops_fill(dict(kind=3, p0=0.1, p1=0.2, p2=0.0, boundary=LC.square()))       # check_spacing_law: thickness
    with pytest.raises(wtp.WtpArgumentError):
        ctx.loops_fill_darts(0.05, 0.75, 2 ** 24, 0, 4)
    with pytest.raises(wtp.WtpArgumentError):
        ctx.loops_fill_darts(0.05, 0.75, A.SEED, -1, 4)
    # the rows of the raw entry that the mirror cannot reach: n_seeds < 0, seeds NULL with n_seeds > 0
    info = L.FillInfo()
    const = L.SpacingDesc()
    const.kind, const.constant = L.WTP_SPACING_CONSTANT, 0.05
    one = np.zeros((1, 2), dtype=F32)
    for seeds_p, ns in ((one.ctypes.data_as(C.c_void_p), -1), (None, 1)):
        rc = ctx._lib.wtp_loops_fill(ctx._h, C.byref(const), 0.75, seeds_p, ns, 10, 10, C.c_uint64(A.SEED), 0, C.byref(info))
        assert rc == L.WTP_ERR_ARG
    # seeds: a coordinate that is not finite; a spacing that is not > 0 at a seed (named)
    for v in (np.nan, np.inf):
        with pytest.raises(wtp.WtpArgumentError, match="seed 1 "):
            ctx.loops_fill(0.05, 0.75, np.array([(0.5, 0.5), (0.5, v)]))
    wall = np.array([(x, -0.05) for x in (0.1, 0.5, 0.9)])
    law = wtp.BoundaryLayerSpacing(wall.astype(F32), -0.1, 0.24, 0.4).desc()   # negative within 0.14 of the wall y = -0.05
    with pytest.raises(wtp.WtpArgumentError, match="seed 2 "):
        ctx.loops_fill(law, 0.75, np.array([(0.5, 0.9), (0.5, 0.8), (0.5, 0.0)]))
    # ... at an inside dart the run takes: the smallest one is named
    xy, inside, r = ctx.loops_fill_darts(law, 0.75, A.SEED, 0, 4096)      # the read-out returns the values as computed
    first_bad = int(np.nonzero(~(r > 0) & inside)[0][0])
    assert first_bad > 0 and r[0] > 0
    for batch in (0, 7):
        with pytest.raises(wtp.WtpArgumentError, match=f"dart {first_bad} "):
            ctx.loops_fill(law, 0.75, None, 10 ** 6, 2000, A.SEED, batch)
    with pytest.raises(wtp.WtpError) as e:
        ctx.loops_fill_get(1)                                            # the failed call left no fill
    assert e.value.code == L.WTP_ERR_STATE
    assert ctx.loops_fill(law, 0.75, None, 1, 2000, A.SEED, 0)["n_darts"] == 1   # a run that ends before the bad dart is fine
    # a run without a point: WTP_OK at the ABI, an error in the mirror
    grid = np.stack(np.meshgrid((np.arange(20) + 0.5) / 20, (np.arange(20) + 0.5) / 20), axis=2).reshape(-1, 2)
    info = ctx.loops_fill(0.1, 0.75, grid, 10 ** 6, 300, A.SEED, 0)       # a seed within 0.036 of every point: nothing fits
    got = ctx.loops_fill_get(0)
    assert info["n_points"] == 0 and info["stop_reason"] == 1 and info["n_darts"] == 300 and got["xy"].shape == (0, 2)
    assert info["r_min"] == 0.0 and info["r_max"] == 0.0
    with pytest.raises(wtp.WtpArgumentError, match="no points"):
        wtp.fill_area(LC.square(), 0.1, seeds=grid, stall_limit=300, ctx=ctx)
    # the context still works
    case, sp, seeds = _set(wtp, ctx, "square_stall200", F32)
    assert _fill(ctx, case, sp, seeds)[0]["n_points"] > 50


def test_the_area_fill_and_the_mesh_runs_void_one_another(wtp, ctx):
    from whatsthepoint_jl_amd import _lib as L

    def state_error(call):
        with pytest.raises(wtp.WtpError) as e:
            call()
        assert e.value.code == L.WTP_ERR_STATE

    v, t = V.mesh_of("cube", F32)
    ctx.mesh_set(v, t)
    case, sp, seeds = _set(wtp, ctx, "square_stall200", F32)
    info, got = _fill(ctx, case, sp, seeds)
    centres = v[t].mean(axis=1)
    mesh_runs = [
        (lambda: ctx.mesh_sample(0.15, 0.75, 10 ** 6, 200, V.SEED, 0), lambda n: ctx.mesh_sample_get(n)["xyz"]),
        (lambda: ctx.mesh_fill(0.15, 0.75, None, 10 ** 6, 200, V.SEED, 0), lambda n: ctx.mesh_fill_get(n)["xyz"]),
        (lambda: ctx.mesh_front(0.15, 10, centres, 200, V.SEED, 0), lambda n: ctx.mesh_front_get(n)["xyz"]),
    ]
    for run, get in mesh_runs:
        # the area fill is resident: the mesh's reads are state errors, its read-out of darts leaves the fill untouched
        state_error(lambda: get(1))
        darts = ctx.loops_fill_darts(sp, 0.75, A.SEED, 0, 100)
        assert _bytes(ctx.loops_fill_get(info["n_points"])) == _bytes(got)
        m_info = run()                                                    # ... and the mesh's run voids it
        for call in (lambda: ctx.loops_fill_get(1), ctx.loops_fill_get_dev):
            state_error(call)
        m_got = get(m_info["n_points"])
        assert len(m_got) > 20 and np.array_equal(ctx.loops_fill_darts(sp, 0.75, A.SEED, 0, 100)[0], darts[0])
        assert np.array_equal(get(m_info["n_points"]), m_got)             # the area's dart read-out leaves it untouched
        info2, got2 = _fill(ctx, case, sp, seeds)                         # and the area fill voids the mesh's result
        assert _bytes(got2) == _bytes(got)
        state_error(lambda: get(1))
    # wtp_loops_set and wtp_loops_clear void a resident area fill; so do wtp_mesh_set / wtp_mesh_clear
    for void in (lambda: ctx.loops_set(list(A.loops_of("square_stall200", F32))), ctx.loops_clear,
                 lambda: ctx.mesh_set(v, t), ctx.mesh_clear):
        ctx.loops_set(list(A.loops_of("square_stall200", F32)))
        assert _bytes(_fill(ctx, case, sp, seeds)[1]) == _bytes(got)
        void()
        state_error(lambda: ctx.loops_fill_get(1))
    # loops of another type than the mesh: each run is of its own index's type
    ctx.mesh_set(v.astype(F64), t)
    case, sp, seeds = _set(wtp, ctx, "square_stall200", F32)
    assert _bytes(_fill(ctx, case, sp, seeds)[1]) == _bytes(got)
    m = ctx.mesh_fill(0.15, 0.75, None, 10 ** 6, 200, V.SEED, 0)
    assert ctx.mesh_fill_get(m["n_points"])["xyz"].dtype == F64
    assert _bytes(_fill(ctx, case, sp, seeds)[1]) == _bytes(got)


# ---- the reference's own items, in the reference's Float64 -------------------------------------------------------------------
def _min_pair_distance(p):
    p = p.astype(F64)
    return (np.linalg.norm(p[:, None] - p[None], axis=2) + 10 * np.eye(len(p))).min()


def test_reference_star_through_discretize(wtp, ctx):
    bnd = wtp.PointBoundary(LC.star())
    tree = wtp.SegmentQuadtree.from_boundary(bnd, ctx=ctx)
    cloud = wtp.discretize(bnd, wtp.ConstantSpacing(0.08), tree, ctx=ctx)
    vol = cloud.volume.points()
    assert isinstance(cloud, wtp.PointCloud) and vol.shape[1] == 2 and len(vol) > 100 and len(cloud.boundary) == 120
    assert tree.isinside(vol).all()
    assert _min_pair_distance(vol) >= 0.75 * 0.08 * (1 - 1.0e-9)
    m = A.model_run("star", F64)
    assert np.array_equal(vol, m[0][m[3]])                                # the model's run: mesh=None and a quadtree agree
    assert np.array_equal(wtp.discretize(bnd, 0.08, ctx=ctx).volume.points(), vol)


def test_reference_annulus_through_discretize(wtp, ctx):
    outer, hole = LC.polygon(48, 2.0), LC.polygon(24, 0.8)
    bnd = wtp.PointBoundary(surfaces=dict(outer=outer, hole=hole))
    cloud = wtp.discretize(bnd, wtp.ConstantSpacing(0.15), ctx=ctx)
    vol = cloud.volume.points()
    rad = np.hypot(vol[:, 0], vol[:, 1])
    assert len(vol) > 100 and ((0.79 < rad) & (rad < 2.001)).all() and rad.min() < 1.2 and rad.max() > 1.6
    assert wtp.SegmentQuadtree.from_boundary(bnd, ctx=ctx).isinside(vol).all()
    assert cloud.volume.fill_info["n_seeds"] == 72 and abs(cloud.volume.fill_info["area_estimate"] - 10.4) < 0.4


def test_reference_circle_defaults_truncation_and_graded_spacing(wtp, ctx):
    circle = LC.polygon(120)
    bnd = wtp.PointBoundary(circle)
    vol = wtp.discretize(bnd, wtp.ConstantSpacing(0.1), ctx=ctx).volume.points()
    assert len(vol) > 100 and _min_pair_distance(vol) >= 0.75 * 0.1 * (1 - 1.0e-9)
    graded = wtp.BoundaryLayerSpacing(bnd.points(), 0.03, 0.12, 0.3)
    g = wtp.discretize(bnd, graded, ctx=ctx).volume
    assert len(g) > 100 and g.fill_r.min() >= 0.75 * 0.03 * (1 - 1e-6) and g.fill_r.max() > 2 * g.fill_r.min()
    sq = wtp.PointBoundary(LC.square())
    with pytest.warns(UserWarning, match="truncated"):
        cut = wtp.discretize(sq, 0.05, max_points=20, ctx=ctx)
    assert len(cut.volume) == 20 and cut.volume.fill_info["stop_reason"] == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        full = wtp.discretize(sq, 0.05, ctx=ctx)
    assert np.array_equal(full.volume.points()[:20], cut.volume.points())
    sq32 = wtp.discretize(LC.square().astype(F32), 0.05, ctx=ctx)         # the cloud keeps the boundary's type
    assert sq32.points().dtype == F32 and len(sq32.volume) > 100


def test_discretize_rejects_unusable_combinations(wtp, ctx):
    sq = wtp.PointBoundary(LC.square())
    v, t = V.mesh_of("cube", F64)
    with pytest.raises(wtp.WtpArgumentError, match="2D discretization supports the Orthtree fill only"):
        wtp.discretize(sq, 0.2, alg=wtp.SlakKosec(), ctx=ctx)
    with pytest.raises(wtp.WtpArgumentError, match="cannot fill a 2D boundary"):
        wtp.discretize(sq, 0.2, wtp.TriangleOctree(v, t, ctx=ctx), ctx=ctx)
    with pytest.raises(wtp.WtpArgumentError, match="cannot fill a 3D boundary"):
        wtp.discretize(v[t].mean(axis=1), 0.2, wtp.SegmentQuadtree(LC.square(), ctx=ctx), ctx=ctx)
    cloud = wtp.discretize(v[t].mean(axis=1), 0.15, (v, t), max_points=2000, ctx=ctx)   # every 3-D call keeps its behaviour
    assert cloud.volume.points().shape[1] == 3 and len(cloud.volume) > 50


# ---- downstream -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_discretize_feeds_repel(wtp, ctx, dtype):
    circle = LC.polygon(120).astype(dtype)
    bnd = wtp.PointBoundary(circle)
    tree = wtp.SegmentQuadtree.from_boundary(bnd, ctx=ctx)
    cloud = wtp.discretize(bnd, 0.1, tree, ctx=ctx)
    assert cloud.points().dtype == dtype and len(cloud.volume) > 100 and len(cloud.boundary) == 120
    out = wtp.repel(cloud, 0.1, max_iters=5, ctx=ctx)
    assert len(out.boundary) == 120 and len(out.volume) > 100
    assert tree.isinside(out.volume.points(), ctx=ctx).all()


# ---- device read-out -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_get_dev_equals_get(wtp, ctx, dtype):
    import torch

    case, sp, seeds = _set(wtp, ctx, "annulus", dtype)
    info, got = _fill(ctx, case, sp, seeds)
    n = info["n_points"]
    tdt = torch.float32 if dtype == F32 else torch.float64
    xy = torch.zeros((n, 2), dtype=tdt, device="cuda")
    r = torch.zeros(n, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    ctx.loops_fill_get_dev(xy.data_ptr(), r.data_ptr())
    assert np.array_equal(xy.cpu().numpy(), got["xy"]) and np.array_equal(r.cpu().numpy(), got["r"])
    only_r = torch.zeros(n, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    ctx.loops_fill_get_dev(0, only_r.data_ptr())                          # every output may be absent
    assert np.array_equal(only_r.cpu().numpy(), got["r"])
    only_xy = torch.zeros((n, 2), dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    ctx.loops_fill_get_dev(only_xy.data_ptr(), 0)
    assert np.array_equal(only_xy.cpu().numpy(), got["xy"])
