"""Graded Poisson-disk surface sampling on the device (include/wtp.h: wtp_mesh_sample, wtp_mesh_sample_get*,
wtp_mesh_sample_darts; host mirror sampling.sample_surface / PointBoundary.from_mesh) against the numpy model of
surface_sampling_cases.py: the darts bit for bit, the accepted set equal to the serial loop over the library's own
darts, independent of the batch size, for both dtypes."""
import warnings

import numpy as np
import pytest

import surface_sampling_cases as S

pytestmark = pytest.mark.gpu

F32, F64 = S.F32, S.F64
ALL = [(name, dt) for name in S.CASES for dt in S.case_dtypes(name)]
IDS = [f"{name}-{np.dtype(dt).name}" for name, dt in ALL]


def _set(wtp, ctx, name, dtype):
    """The case's mesh resident in ctx; returns (case, the spacing as Context.mesh_sample takes it)."""
    v, t = S.mesh_of(name, dtype)
    ctx.mesh_set(v, t)
    return S.CASES[name], wtp.sampling._sampler_spacing(S.library_spacing(wtp, name, dtype))


def _sample(ctx, case, sp, **kw):
    a = dict(factor=case["factor"], max_points=S.max_points_of(case), stall_limit=case["stall_limit"], seed=S.SEED, batch=0)
    a.update(kw)
    info = ctx.mesh_sample(sp, a["factor"], a["max_points"], a["stall_limit"], a["seed"], a["batch"])
    return info, ctx.mesh_sample_get(info["n_points"])


def _bytes(got):
    return b"".join(got[k].tobytes() for k in ("xyz", "tri", "r", "dart"))


# ---- darts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("dtype", S.DTYPES)
@pytest.mark.parametrize("name", ["cube_f075", "cube_zero_area", "box", "graded_loglike", "graded_bl"])
def test_darts_equal_the_model(wtp, ctx, name, dtype, first):
    case, sp = _set(wtp, ctx, name, dtype)
    n = 3001
    xyz, tri, r = ctx.mesh_sample_darts(sp, case["factor"], S.SEED, first, n)
    mx, mt, mr = S.darts(name, dtype, first, n)
    assert xyz.dtype == dtype and np.array_equal(tri, mt) and np.array_equal(xyz, mx)
    if case["spacing"][0] == "bl":   # exp() differs by an ulp between the device and the host: the bound of DESIGN.md §8f.3
        bulk = case["factor"] * case["spacing"][2]
        assert np.abs(r.astype(F64) - mr.astype(F64)).max() <= 4 * np.finfo(dtype).eps * bulk
    else:
        assert np.array_equal(r, mr)


# ---- acceptance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", ALL, ids=IDS)
def test_accepted_set_equals_the_serial_loop_over_the_librarys_darts(wtp, ctx, name, dtype):
    case, sp = _set(wtp, ctx, name, dtype)
    n = S.whole_batches(case["horizon"], 0)[1]                          # the darts of every batch a run within the horizon decides
    xyz, tri, r = ctx.mesh_sample_darts(sp, case["factor"], S.SEED, 0, n)
    acc, n_darts, reason = S.serial(xyz[:case["horizon"]], r[:case["horizon"]], S.max_points_of(case), case["stall_limit"])
    info, got = _sample(ctx, case, sp)
    print(f"{name} {np.dtype(dtype).name}: n_points={info['n_points']} n_darts={info['n_darts']} batches={info['n_batches']} "
          f"rounds_max={info['rounds_max']} host_syncs={info['host_syncs']}")
    assert np.array_equal(got["dart"], acc) and info["n_darts"] == n_darts and info["stop_reason"] == reason
    assert info["n_points"] == len(acc)
    assert np.array_equal(got["xyz"], xyz[acc]) and np.array_equal(got["tri"], tri[acc]) and np.array_equal(got["r"], r[acc])
    assert info["r_min"] == float(r[acc].min()) and info["r_max"] == float(r[acc].max())
    assert info["total_area"] == S.areas_of(name, dtype)[1]
    # batch = 0 is the schedule of S.batch_sizes: the batch model over the same whole batches counts the same batches and rounds
    nb, whole = S.whole_batches(n_darts, 0)
    b = S.batched_run(xyz[:whole], r[:whole], S.max_points_of(case), case["stall_limit"], 0)
    assert np.array_equal(b["acc"], acc) and b["n_batches"] == nb
    assert (info["n_batches"], info["rounds_max"]) == (b["n_batches"], b["rounds_max"])
    if name == "one_triangle":
        assert info["n_points"] == 1 and info["n_darts"] == 1 + case["stall_limit"] and info["stop_reason"] == 1
    if name == "cube_stall3":
        assert info["n_batches"] == 1                                  # the run ends inside the first batch


def test_a_smaller_max_points_gives_a_prefix(wtp, ctx):
    case, sp = _set(wtp, ctx, "cube_f075", F32)
    _, full = _sample(ctx, case, sp)
    for m in (1, 37):
        info, got = _sample(ctx, case, sp, max_points=m)
        assert info["stop_reason"] == 2 and info["n_points"] == m and info["n_darts"] == got["dart"][-1] + 1
        assert all(np.array_equal(got[k], full[k][:m]) for k in got)


# ---- batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("cube_f075", F32), ("graded_bl", F64)])
def test_result_does_not_depend_on_the_batch_size(wtp, ctx, name, dtype):
    case, sp = _set(wtp, ctx, name, dtype)
    info0, got0 = _sample(ctx, case, sp, batch=0)
    assert info0["rounds_max"] >= 1 and 0 < info0["host_syncs"] < 10 ** 6
    for batch in (63, 64, 65, 1000, 4096):
        info, got = _sample(ctx, case, sp, batch=batch)
        assert _bytes(got) == _bytes(got0), batch
        assert (info["n_darts"], info["stop_reason"], info["batch"]) == (info0["n_darts"], info0["stop_reason"], batch)
        assert 1 <= info["rounds_max"] <= batch and np.isfinite(info["host_syncs"])
    info, one = _sample(ctx, case, sp, batch=1, max_points=40)       # one host round trip per dart
    assert info["stop_reason"] == 2 and info["rounds_max"] == 1 and info["n_batches"] == info["n_darts"]
    assert all(np.array_equal(one[k], got0[k][:40]) for k in one)


# ---- properties, by brute force ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("cube_f075", F32), ("cube_f100", F64), ("slab", F32), ("graded_bl", F32),
                                        ("graded_loglike", F64), ("cube_far", F32), ("box", F32)])
def test_sample_surface_properties(wtp, ctx, name, dtype):
    case = S.CASES[name]
    v, t = S.mesh_of(name, dtype)
    surf = wtp.sample_surface((v, t), S.library_spacing(wtp, name, dtype), factor=case["factor"],
                              stall_limit=case["stall_limit"], ctx=ctx)
    p, r, tri, info = surf.points(), surf.sample_r, surf.sample_tri, surf.sample_info
    assert p.dtype == dtype and len(p) == info["n_points"] > (50 if name != "slab" else 10)
    # no pair conflicts under the library's own expression, in the cloud's type: exact
    d2 = None
    for c in range(3):
        d = p[:, None, c] - p[None, :, c]
        d2 = d * d if d2 is None else d2 + d * d
    m = np.minimum(r[:, None], r[None, :])
    assert d2.dtype == dtype and not ((d2 < m * m) & ~np.eye(len(p), dtype=bool)).any()
    # in double every pair keeps min(r_i, r_j), up to the rounding of the stored differences
    slack = 8 * np.finfo(dtype).eps * float(np.abs(p).max())
    pd, rd = p.astype(F64), r.astype(F64)
    dist = np.sqrt(((pd[:, None] - pd[None]) ** 2).sum(axis=2)) + 1e30 * np.eye(len(p))
    assert (dist >= np.minimum(rd[:, None], rd[None]) - slack).all()
    # every sample lies in its parent triangle's plane and inside the triangle, within the same slack
    c = v.astype(F64)[t[tri]]
    nrm = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    assert np.abs(np.einsum("ij,ij->i", pd - c[:, 0], nrm)).max() <= slack
    for a, b in ((0, 1), (1, 2), (2, 0)):
        e = c[:, b] - c[:, a]
        inward = np.cross(nrm, e)
        inward /= np.linalg.norm(inward, axis=1)[:, None]
        assert np.einsum("ij,ij->i", pd - c[:, a], inward).min() >= -slack
    face = ctx.mesh_face_normals()
    assert np.array_equal(surf.normals, face[tri].astype(dtype))
    assert abs(float(surf.areas.astype(F64).sum()) - info["total_area"]) <= (1e-12 + len(p) * np.finfo(dtype).eps) * info["total_area"]
    w = rd ** 2
    shares = info["total_area"] / w.sum() * w                            # the double sum the areas are rounded from
    assert abs(shares.sum() - info["total_area"]) <= 1e-12 * info["total_area"]
    assert np.array_equal(surf.areas, shares.astype(dtype))
    if name in ("cube_f075", "cube_f100"):                                      # the reference's own test on the unit cube
        assert np.minimum(np.abs(pd), np.abs(pd - 1)).min(axis=1).max() <= slack
        assert np.abs(np.abs(surf.normals).max(axis=1) - 1).max() <= 4 * np.finfo(dtype).eps   # unit, axis-aligned
        assert np.abs(np.abs(surf.normals).sum(axis=1) - 1).max() <= 4 * np.finfo(dtype).eps
        assert abs(shares.sum() - 6.0) <= 1e-11


def test_max_points_warns_and_from_mesh_names_the_surface(wtp, ctx):
    v, t = S.mesh_of("cube_f075", F64)
    with pytest.warns(UserWarning, match="truncated by max_points"):
        bnd = wtp.PointBoundary.from_mesh((v, t), wtp.ConstantSpacing(0.15), name="skin", max_points=20, ctx=ctx)
    assert list(bnd.surfaces) == ["skin"] and len(bnd) == 20 and bnd["skin"].sample_info["stop_reason"] == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        oc = wtp.TriangleOctree(v, t, ctx=ctx)
        full = wtp.PointBoundary.from_mesh(oc, 0.15)                     # a TriangleOctree, through its own context
    assert np.array_equal(full.points()[:20], bnd.points())


# ---- determinism -----------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits_and_the_seed_matters(wtp, ctx):
    case, sp = _set(wtp, ctx, "graded_bl", F32)
    _, a = _sample(ctx, case, sp)
    _, b = _sample(ctx, case, sp)
    assert _bytes(a) == _bytes(b)
    _, c = _sample(ctx, case, sp, seed=S.SEED + 1)
    assert not np.array_equal(c["dart"], a["dart"])


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors_leave_the_context_usable(wtp, ctx):
    from whatsthepoint_jl_amd import _lib as L

    ctx.mesh_clear()
    with pytest.raises(wtp.WtpError) as e:
        ctx.mesh_sample(0.15)                                            # no mesh
    assert e.value.code == L.WTP_ERR_STATE
    case, sp = _set(wtp, ctx, "cube_f075", F32)
    with pytest.raises(wtp.WtpError) as e:
        ctx.mesh_sample_get(1)                                           # before a successful sample (mesh_set voided any)
    assert e.value.code == L.WTP_ERR_STATE
    with pytest.raises(wtp.WtpError) as e:
        ctx.mesh_sample_get_dev()
    assert e.value.code == L.WTP_ERR_STATE
    bad = [dict(factor=0.0), dict(factor=-1.0), dict(factor=float("nan")), dict(factor=float("inf")), dict(stall_limit=0),
           dict(max_points=0), dict(seed=2 ** 24), dict(batch=-1)]
    for kw in bad:
        with pytest.raises(wtp.WtpArgumentError):
            _sample(ctx, case, sp, **kw)
    per_point = L.SpacingDesc()
    per_point.kind = L.WTP_SPACING_PER_POINT
    with pytest.raises(wtp.WtpArgumentError):
        ctx.mesh_sample(None, spacing_desc=per_point)
    with pytest.raises(wtp.WtpArgumentError):
        ctx.mesh_sample(dict(kind=3, p0=0.1, p1=0.2, p2=0.0, boundary=S.LAW_POINTS))   # check_spacing_law: thickness
    with pytest.raises(wtp.WtpArgumentError):
        ctx.mesh_sample_darts(0.15, 0.75, 2 ** 24, 0, 4)
    # a law that is negative near the wall (check_spacing_law lets at_wall < 0 through): the smallest bad dart is named
    law = wtp.BoundaryLayerSpacing(S.LAW_POINTS.astype(F32), -0.1, 0.24, 1.0).desc()
    _, _, r = ctx.mesh_sample_darts(law, 0.75, S.SEED, 0, 4096)          # the read-out returns the values as computed
    first_bad = int(np.nonzero(~(r > 0))[0][0])
    for batch in (0, 7):
        with pytest.raises(wtp.WtpArgumentError, match=f"dart {first_bad} "):
            ctx.mesh_sample(law, 0.75, 10 ** 6, 2000, S.SEED, batch)
    with pytest.raises(wtp.WtpError) as e:
        ctx.mesh_sample_get(1)                                           # the failed call left no sample
    assert e.value.code == L.WTP_ERR_STATE
    assert first_bad > 0 and r[0] > 0
    assert ctx.mesh_sample(law, 0.75, 1, 2000, S.SEED, 0)["n_darts"] == 1   # a run that ends before the bad dart is fine
    # zero surface area
    ctx.mesh_set(np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)], dtype=F32), np.array([(0, 1, 2)], dtype=np.int32))
    with pytest.raises(wtp.WtpArgumentError, match="zero surface area"):
        ctx.mesh_sample(0.15)
    # while a relax session evaluates a device law, another boundary's law is refused
    case, sp = _set(wtp, ctx, "graded_bl", F32)
    x = wtp.synth.uniform(2000, 3, F32)
    other = wtp.LogLike(wtp.synth.uniform(50, 3, F32, seed=7), 0.08, 1.3).desc()
    s = 2000.0 ** (-1 / 3)
    with ctx.relax(x, 0, other, dict(kind=2, beta=0.2, u0=1.0, gamma=3.0), 21, s / 2000, s / 20):
        with pytest.raises(wtp.WtpError) as e:
            ctx.mesh_sample(sp, case["factor"])
        assert e.value.code == L.WTP_ERR_STATE
        assert ctx.mesh_sample(0.15)["n_points"] > 50                    # a constant needs no tree
    idx = ctx.knn(x, 5)
    assert idx.shape == (2000, 5) and (idx[:, 0] != np.arange(2000)).all()
    assert _sample(ctx, case, sp)[0]["n_points"] > 50


# ---- downstream -------------------------------------------------------------------------------------------------------------
def test_sampled_boundary_feeds_repel(wtp, ctx):
    v, t = S.mesh_of("cube_f075", F64)
    oc = wtp.TriangleOctree(v, t, ctx=ctx)
    bnd = wtp.PointBoundary.from_mesh(oc, 0.15, ctx=ctx)
    vol = wtp.synth.uniform(400, 3, F64) * 0.8 + 0.1
    cloud = wtp.PointCloud(bnd, wtp.PointVolume(vol))
    out = wtp.repel(cloud, 0.15, oc, max_iters=3, ctx=ctx)
    assert len(out) == len(cloud)
    b = out.boundary.points()
    assert len(b) >= len(bnd) and np.abs(oc.signed_distance(b, ctx=ctx)).max() <= 1e-5
    assert oc.isinside(out.volume.points(), ctx=ctx).all()


# ---- device read-out -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES)
def test_get_dev_equals_get(wtp, ctx, dtype):
    import torch

    case, sp = _set(wtp, ctx, "graded_loglike", dtype)
    info, got = _sample(ctx, case, sp)
    n = info["n_points"]
    tdt = torch.float32 if dtype == F32 else torch.float64
    xyz = torch.zeros((n, 3), dtype=tdt, device="cuda")
    r = torch.zeros(n, dtype=tdt, device="cuda")
    tri = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.mesh_sample_get_dev(xyz.data_ptr(), tri.data_ptr(), r.data_ptr())
    assert np.array_equal(xyz.cpu().numpy(), got["xyz"]) and np.array_equal(r.cpu().numpy(), got["r"])
    assert np.array_equal(tri.cpu().numpy(), got["tri"])
    only_r = torch.zeros(n, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    ctx.mesh_sample_get_dev(0, 0, only_r.data_ptr())                     # every output may be absent
    assert np.array_equal(only_r.cpu().numpy(), got["r"])
