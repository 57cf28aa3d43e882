"""Graded Poisson-disk volume fill on the device (include/wtp.h: wtp_mesh_fill, wtp_mesh_fill_get*, wtp_mesh_fill_darts;
host mirror sampling.fill_volume / discretize) against the numpy model of volume_fill_cases.py: the darts and their
inside flags bit for bit, the accepted set equal to the serial loop over the library's own darts, independent of the
batch size, for both dtypes; the reference's own items (test/octree.jl:112-224) through discretize."""
import warnings

import numpy as np
import pytest

import volume_fill_cases as V

pytestmark = pytest.mark.gpu

F32, F64 = V.F32, V.F64
ALL = [(name, dt) for name in V.CASES for dt in V.case_dtypes(name)]
IDS = [f"{name}-{np.dtype(dt).name}" for name, dt in ALL]


def _set(wtp, ctx, name, dtype):
    """The case's mesh resident in ctx; returns (case, the spacing as Context.mesh_fill takes it, the seeds)."""
    v, t = V.mesh_of(name, dtype)
    ctx.mesh_set(v, t)
    return V.CASES[name], wtp.sampling._sampler_spacing(V.library_spacing(wtp, name, dtype)), V.seeds_of(name, dtype)[0]


def _fill(ctx, case, sp, seeds, **kw):
    a = dict(factor=case["factor"], max_points=V.max_points_of(case), stall_limit=case["stall_limit"], seed=V.SEED, batch=0)
    a.update(kw)
    info = ctx.mesh_fill(sp, a["factor"], seeds, a["max_points"], a["stall_limit"], a["seed"], a["batch"])
    return info, ctx.mesh_fill_get(info["n_points"])


def _bytes(got):
    return b"".join(got[k].tobytes() for k in ("xyz", "r", "dart"))


def _seed_r(ctx, case, sp, seeds, dtype):
    """r of the seeds as the library evaluates the case's law (the device's exp differs from numpy's by an ulp)."""
    if not len(seeds):
        return np.zeros(0, dtype=dtype)
    if case["spacing"][0] == "const":
        return np.full(len(seeds), dtype(case["factor"]) * dtype(case["spacing"][1]), dtype=dtype)
    return dtype(case["factor"]) * ctx.spacing_eval(sp, seeds)


# ---- darts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("name,dtype", [("cube", F32), ("cube", F64), ("cube_bl", F32), ("cube_bl", F64), ("cube_far", F32),
                                        ("flat", F32), ("flat", F64), ("cavity", F32), ("box_stall200", F32)])
def test_darts_equal_the_model(wtp, ctx, name, dtype, first):
    case, sp, _ = _set(wtp, ctx, name, dtype)
    n = 3001 if name != "box_stall200" else 1025                     # (the oracle tests every triangle of the box mesh)
    xyz, inside, r = ctx.mesh_fill_darts(sp, case["factor"], V.SEED, first, n)
    mx, mi, mr = V.darts(name, dtype, first, n)
    assert xyz.dtype == dtype and np.array_equal(xyz, mx) and np.array_equal(inside, mi)
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
    n = V.whole_batches(h, 0)[1]                                        # the darts of every batch a run within the horizon decides
    xyz, inside, r = ctx.mesh_fill_darts(sp, case["factor"], V.SEED, 0, n)
    sr = _seed_r(ctx, case, sp, seeds, dtype)
    acc, n_darts, reason, n_in = V.serial(xyz[:h], inside[:h], r[:h], seeds, sr, V.max_points_of(case), case["stall_limit"])
    info, got = _fill(ctx, case, sp, seeds)
    print(f"{name} {np.dtype(dtype).name}: n_points={info['n_points']} n_darts={info['n_darts']} n_inside={info['n_inside']} "
          f"batches={info['n_batches']} rounds_max={info['rounds_max']} host_syncs={info['host_syncs']}")
    assert np.array_equal(got["dart"], acc) and info["n_darts"] == n_darts and info["stop_reason"] == reason
    assert info["n_points"] == len(acc) and info["n_inside"] == n_in and info["n_seeds"] == len(seeds)
    assert np.array_equal(got["xyz"], xyz[acc]) and np.array_equal(got["r"], r[acc])
    if len(acc):
        assert info["r_min"] == float(r[acc].min()) and info["r_max"] == float(r[acc].max())
    else:
        assert info["r_min"] == 0.0 and info["r_max"] == 0.0         # WTP_OK with no point at the ABI
    assert info["bbox_volume"] == V.bbox_volume(name, dtype)
    # batch = 0 is the schedule of V.batch_sizes: the batch model over the same whole batches counts the same batches and rounds
    nb, whole = V.whole_batches(n_darts, 0)
    b = V.batched_run(xyz[:whole], inside[:whole], r[:whole], seeds, sr, V.max_points_of(case), case["stall_limit"], 0)
    assert np.array_equal(b["acc"], acc) and b["n_inside"] == n_in and b["n_batches"] == nb
    assert (info["n_batches"], info["rounds_max"]) == (b["n_batches"], b["rounds_max"])
    if case["spacing"][0] == "const" and len(V.mesh_of(name, dtype)[1]) <= 12:   # the model's own counts (12 triangles)
        assert (len(acc), n_darts, n_in) == (len(V.model_run(name, dtype)[3]),) + V.model_run(name, dtype)[4:7:2]
    if name == "cube_const10":
        assert info["n_points"] == 1 and info["n_darts"] == 1 + case["stall_limit"] and info["n_batches"] == 1
    if name in ("slab_seeded", "flat"):
        assert info["n_points"] == 0 and info["n_darts"] == case["stall_limit"]


def test_a_smaller_max_points_gives_a_prefix(wtp, ctx):
    case, sp, seeds = _set(wtp, ctx, "cube_seeds", F32)
    _, full = _fill(ctx, case, sp, seeds)
    for m in (1, 37):
        info, got = _fill(ctx, case, sp, seeds, max_points=m)
        assert info["stop_reason"] == 2 and info["n_points"] == m and info["n_darts"] == got["dart"][-1] + 1
        assert all(np.array_equal(got[k], full[k][:m]) for k in got)


# ---- batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("cube_stall200", F32), ("cube_seeds", F64), ("cube_bl", F32), ("cavity", F32)])
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
    case, sp, seeds = _set(wtp, ctx, "cube_max37", F32)
    info0, got0 = _fill(ctx, case, sp, seeds)
    info, one = _fill(ctx, case, sp, seeds, batch=1)                   # one host round trip per dart
    assert info["stop_reason"] == 2 and info["rounds_max"] == 1 and info["n_batches"] == info["n_darts"] == info0["n_darts"]
    assert _bytes(one) == _bytes(got0) and info["n_inside"] == info0["n_inside"]


# ---- determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", V.DTYPES)
def test_two_calls_return_the_same_bits_and_the_seed_matters(wtp, ctx, dtype):
    case, sp, seeds = _set(wtp, ctx, "cube_bl", dtype)
    _, a = _fill(ctx, case, sp, seeds)
    _, b = _fill(ctx, case, sp, seeds)
    assert _bytes(a) == _bytes(b)
    _, c = _fill(ctx, case, sp, seeds, seed=V.SEED + 1)
    assert not np.array_equal(c["dart"], a["dart"])


# ---- properties, by brute force in double --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("cube", F32), ("cube", F64), ("cube_seeds", F32), ("cube_seeds", F64), ("cube_bl", F32),
                                        ("cube_bl", F64), ("cube_far", F32), ("cube_seed_outside", F64), ("cavity", F32)])
def test_fill_volume_properties(wtp, ctx, O, name, dtype):
    case = V.CASES[name]
    v, t = V.mesh_of(name, dtype)
    seeds = V.seeds_of(name, dtype)[0]
    law = V.library_spacing(wtp, name, dtype)
    vol = wtp.fill_volume((v, t), law, seeds=seeds if len(seeds) else None, factor=case["factor"],
                          stall_limit=case["stall_limit"], ctx=ctx)
    p, r, info = vol.points(), vol.fill_r, vol.fill_info
    assert p.dtype == dtype and len(p) == info["n_points"] > 50 and isinstance(vol, wtp.PointVolume)
    assert O.mesh_query(v, t, p)["inside"].all()                     # every point is inside, by the oracle
    sr = _seed_r(ctx, case, wtp.sampling._sampler_spacing(law), seeds, dtype)
    q, rq = np.concatenate([seeds, p]), np.concatenate([sr, r])
    ns = len(seeds)
    # no pair conflicts under the library's own expression, in the cloud's type: exact
    d2 = None
    for c in range(3):
        d = p[:, None, c] - q[None, :, c]
        d2 = d * d if d2 is None else d2 + d * d
    m = np.minimum(r[:, None], rq[None, :])
    own = np.zeros((len(p), len(q)), dtype=bool)
    own[np.arange(len(p)), ns + np.arange(len(p))] = True
    assert d2.dtype == dtype and not ((d2 < m * m) & ~own).any()
    # in double every pair, and every point-seed pair, keeps min(r_i, r_j), up to the rounding of the stored differences
    slack = 8 * np.finfo(dtype).eps * float(np.abs(q).max())
    dist = np.sqrt(((p.astype(F64)[:, None] - q.astype(F64)[None]) ** 2).sum(axis=2)) + 1e30 * own
    assert (dist >= m.astype(F64) - slack).all()
    est = info["volume_estimate"]
    assert est == info["bbox_volume"] * info["n_inside"] / info["n_darts"]
    if name.startswith("cube"):
        assert abs(est - 1.0) <= 1e-3                                  # (all but the darts that round onto a face)
    else:
        assert abs(est - wtp.signed_volume(v, t)) <= 0.03 * wtp.signed_volume(v, t)   # six sigma of 57 000 darts at p = 0.44


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors_leave_the_context_usable(wtp, ctx):
    from whatsthepoint_jl_amd import _lib as L

    ctx.mesh_clear()
    with pytest.raises(wtp.WtpError) as e:
        ctx.mesh_fill(0.15)                                              # no mesh
    assert e.value.code == L.WTP_ERR_STATE
    case, sp, _ = _set(wtp, ctx, "cube", F32)
    for call in (lambda: ctx.mesh_fill_get(1), ctx.mesh_fill_get_dev):   # before a successful fill (mesh_set voided any)
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
        ctx.mesh_fill(None, spacing_desc=per_point)
    with pytest.raises(wtp.WtpArgumentError):
        ctx.mesh_fill(dict(kind=3, p0=0.1, p1=0.2, p2=0.0, boundary=V.LAW_POINTS))     # check_spacing_law: thickness
    with pytest.raises(wtp.WtpArgumentError):
        ctx.mesh_fill_darts(0.15, 0.75, 2 ** 24, 0, 4)
    with pytest.raises(wtp.WtpArgumentError):
        ctx.mesh_fill_darts(0.15, 0.75, V.SEED, -1, 4)
    # the rows of the raw entry that the mirror cannot reach: n_seeds < 0, seeds NULL with n_seeds > 0
    info = L.FillInfo()
    const = L.SpacingDesc()
    const.kind, const.constant = L.WTP_SPACING_CONSTANT, 0.15
    import ctypes as C

    one = np.zeros((1, 3), dtype=F32)
    for seeds_p, ns in ((one.ctypes.data_as(C.c_void_p), -1), (None, 1)):
        rc = ctx._lib.wtp_mesh_fill(ctx._h, C.byref(const), 0.75, seeds_p, ns, 10, 10, C.c_uint64(V.SEED), 0, C.byref(info))
        assert rc == L.WTP_ERR_ARG
    # seeds: a coordinate that is not finite; a spacing that is not > 0 at a seed (named)
    for v in (np.nan, np.inf):
        with pytest.raises(wtp.WtpArgumentError, match="seed 1 "):
            ctx.mesh_fill(0.15, 0.75, np.array([(0.5, 0.5, 0.5), (0.5, v, 0.5)]))
    law = wtp.BoundaryLayerSpacing(V.LAW_POINTS.astype(F32), -0.1, 0.24, 1.0).desc()   # negative near the wall z = -0.05
    with pytest.raises(wtp.WtpArgumentError, match="seed 2 "):
        ctx.mesh_fill(law, 0.75, np.array([(0.5, 0.5, 0.9), (0.5, 0.5, 0.8), (0.5, 0.5, 0.0)]))
    # ... at an inside dart the run takes: the smallest one is named; at a dart that is not inside it is no error
    xyz, inside, r = ctx.mesh_fill_darts(law, 0.75, V.SEED, 0, 4096)     # the read-out returns the values as computed
    first_bad = int(np.nonzero(~(r > 0) & inside)[0][0])
    assert first_bad > 0 and r[0] > 0
    for batch in (0, 7):
        with pytest.raises(wtp.WtpArgumentError, match=f"dart {first_bad} "):
            ctx.mesh_fill(law, 0.75, None, 10 ** 6, 2000, V.SEED, batch)
    with pytest.raises(wtp.WtpError) as e:
        ctx.mesh_fill_get(1)                                             # the failed call left no fill
    assert e.value.code == L.WTP_ERR_STATE
    assert ctx.mesh_fill(law, 0.75, None, 1, 2000, V.SEED, 0)["n_darts"] == 1   # a run that ends before the bad dart is fine
    # the law's wall lies below the half-height cube's bottom... of a cube lifted to z in [0.5, 1] every bad value is outside
    v, t = V.cube((1.0, 1.0, 0.5))
    v = v + (0.0, 0.0, 0.5)
    ctx.mesh_set(np.vstack([v, [(0.0, 0.0, -0.04)]]).astype(F32), t)     # a loose vertex stretches the box down to the wall
    xyz, inside, r = ctx.mesh_fill_darts(law, 0.75, V.SEED, 0, 4096)
    assert (~(r > 0)).any() and (r[inside] > 0).all() and not inside[~(r > 0)].any()
    info = ctx.mesh_fill(law, 0.75, None, 10 ** 6, 300, V.SEED, 0)
    assert info["n_points"] > 20 and info["n_darts"] > int(np.nonzero(~(r > 0))[0][0])
    # zero surface area
    ctx.mesh_set(np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)], dtype=F32), np.array([(0, 1, 2)], dtype=np.int32))
    with pytest.raises(wtp.WtpArgumentError, match="zero surface area"):
        ctx.mesh_fill(0.15)
    # a run without a point: WTP_OK at the ABI, an error in the mirror
    case, sp, seeds = _set(wtp, ctx, "slab_seeded", F64)
    info, got = _fill(ctx, case, sp, seeds)
    assert info["n_points"] == 0 and info["stop_reason"] == 1 and got["xyz"].shape == (0, 3)
    with pytest.raises(wtp.WtpArgumentError, match="no points"):
        wtp.fill_volume(V.mesh_of("slab_seeded", F64), 0.15, seeds=seeds, ctx=ctx)
    # the context still works
    case, sp, seeds = _set(wtp, ctx, "cube_stall200", F32)
    assert _fill(ctx, case, sp, seeds)[0]["n_points"] > 50


def test_sample_and_fill_void_each_other(wtp, ctx):
    from whatsthepoint_jl_amd import _lib as L

    case, sp, seeds = _set(wtp, ctx, "cube_stall200", F32)
    info, got = _fill(ctx, case, sp, seeds)
    darts = ctx.mesh_fill_darts(sp, 0.75, V.SEED, 0, 100)
    ctx.mesh_sample_darts(sp, 0.75, V.SEED, 0, 100)
    assert _bytes(ctx.mesh_fill_get(info["n_points"])) == _bytes(got)     # the read-outs leave a resident fill untouched
    with pytest.raises(wtp.WtpError) as e:
        ctx.mesh_sample_get(1)                                            # a fill is resident, not a sample
    assert e.value.code == L.WTP_ERR_STATE
    s_info = ctx.mesh_sample(sp, 0.75, 10 ** 6, 200, V.SEED, 0)
    for call in (lambda: ctx.mesh_fill_get(1), ctx.mesh_fill_get_dev):
        with pytest.raises(wtp.WtpError) as e:
            call()
        assert e.value.code == L.WTP_ERR_STATE
    s_got = ctx.mesh_sample_get(s_info["n_points"])
    assert np.array_equal(ctx.mesh_fill_darts(sp, 0.75, V.SEED, 0, 100)[0], darts[0])
    assert np.array_equal(ctx.mesh_sample_get(s_info["n_points"])["xyz"], s_got["xyz"])
    info2, got2 = _fill(ctx, case, sp, seeds)
    assert _bytes(got2) == _bytes(got)
    for call in (lambda: ctx.mesh_sample_get(1), ctx.mesh_sample_get_dev):
        with pytest.raises(wtp.WtpError) as e:
            call()
        assert e.value.code == L.WTP_ERR_STATE
    assert np.array_equal(ctx.mesh_sample_get(ctx.mesh_sample(sp, 0.75, 10 ** 6, 200, V.SEED, 0)["n_points"])["xyz"], s_got["xyz"])


# ---- the reference's own items (test/octree.jl:112-224), in the reference's Float64 ------------------------------------------
def _cube_and_face_centres():
    v, t = V.mesh_of("cube", F64)
    return v, t, v[t].mean(axis=1)                                        # PointBoundary(mesh): one point per face


def test_reference_bridson_placement_enforces_global_separation(wtp, ctx):
    v, t, centres = _cube_and_face_centres()
    cloud = wtp.discretize(wtp.PointBoundary(centres), wtp.ConstantSpacing(0.15), (v, t), max_points=2000, ctx=ctx)
    vol = cloud.volume.points()
    assert isinstance(cloud, wtp.PointCloud) and 50 < len(vol) <= 2000 and len(cloud.boundary) == 12
    allp = cloud.points().astype(F64)
    n_bnd = len(centres)
    d = np.linalg.norm(allp[n_bnd:, None] - allp[None], axis=2)
    d[np.arange(len(vol)), n_bnd + np.arange(len(vol))] = np.inf
    print(f"min separation {d.min():.12f}")
    assert d.min() >= 0.75 * 0.15 - 1.0e-9


def test_reference_bridson_placement_with_graded_spacing(wtp, ctx):
    v, t, centres = _cube_and_face_centres()
    law = wtp.BoundaryLayerSpacing(centres, 0.1, 0.25, 0.2)
    cloud = wtp.discretize(wtp.PointBoundary(centres), law, (v, t), factor=1.0, max_points=2000, ctx=ctx)
    vol = cloud.volume.points()
    assert len(vol) > 50
    allp = cloud.points().astype(F64)
    h = np.asarray(law(cloud.points(), ctx=ctx), dtype=F64)
    n_bnd = len(centres)
    assert np.array_equal(h[n_bnd:], cloud.volume.fill_r)                 # factor 1: r is h
    d = np.linalg.norm(allp[n_bnd:, None] - allp[None], axis=2)
    d[np.arange(len(vol)), n_bnd + np.arange(len(vol))] = np.inf
    assert (d >= np.minimum(h[n_bnd:, None], h[None]) - 1.0e-9).all()     # the graded guarantee against the whole cloud


def test_reference_bridson_warns_on_truncation(wtp, ctx):
    v, t, centres = _cube_and_face_centres()
    with pytest.warns(UserWarning, match="truncated by max_points before saturation — parts of the domain may be unfilled"):
        cloud = wtp.discretize(wtp.PointBoundary(centres), 0.15, (v, t), max_points=5, ctx=ctx)
    assert len(cloud.volume) == 5 and cloud.volume.fill_info["stop_reason"] == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        oc = wtp.TriangleOctree(v, t, ctx=ctx)
        full = wtp.discretize(centres, 0.15, oc)                          # a TriangleOctree, through its own context
    assert np.array_equal(full.volume.points()[:5], cloud.volume.points())
    with pytest.raises(wtp.WtpArgumentError, match="inside-out"):
        wtp.discretize(centres, 0.15, (v, t[:, ::-1].copy()), ctx=ctx)    # an inside-out mesh has no inside


# ---- downstream -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", V.DTYPES)
def test_discretize_feeds_repel(wtp, ctx, dtype):
    v, t = V.mesh_of("cube", dtype)
    oc = wtp.TriangleOctree(v, t, ctx=ctx)
    bnd = wtp.PointBoundary.from_mesh(oc, 0.15, ctx=ctx)
    cloud = wtp.discretize(bnd, 0.15, oc, ctx=ctx)
    assert cloud.points().dtype == dtype and len(cloud.volume) > 50 and len(cloud.boundary) == len(bnd)
    out = wtp.repel(cloud, 0.15, oc, max_iters=3, ctx=ctx)
    assert len(out) == len(cloud)                                         # counts conserved
    assert len(out.boundary) >= len(bnd) and oc.isinside(out.volume.points(), ctx=ctx).all()


# ---- device read-out -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", V.DTYPES)
def test_get_dev_equals_get(wtp, ctx, dtype):
    import torch

    case, sp, seeds = _set(wtp, ctx, "cube_seeds", dtype)
    info, got = _fill(ctx, case, sp, seeds)
    n = info["n_points"]
    tdt = torch.float32 if dtype == F32 else torch.float64
    xyz = torch.zeros((n, 3), dtype=tdt, device="cuda")
    r = torch.zeros(n, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    ctx.mesh_fill_get_dev(xyz.data_ptr(), r.data_ptr())
    assert np.array_equal(xyz.cpu().numpy(), got["xyz"]) and np.array_equal(r.cpu().numpy(), got["r"])
    only_r = torch.zeros(n, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    ctx.mesh_fill_get_dev(0, only_r.data_ptr())                          # every output may be absent
    assert np.array_equal(only_r.cpu().numpy(), got["r"])
