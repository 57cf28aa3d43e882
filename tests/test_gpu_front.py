"""Advancing-front volume fill on the device (include/wtp.h: wtp_mesh_front, wtp_mesh_front_get*,
wtp_mesh_front_candidates; host mirror sampling.front_volume / discretize(alg=SlakKosec())) against the numpy model of
front_cases.py: the candidates bit for bit, the accepted set equal to the serial loop replayed over the library's own
candidates, independent of the batch, for both dtypes; the reference's own items (test/discretization.jl:21-35, :146-161)
through discretize."""
import ctypes as C
import warnings

import numpy as np
import pytest

import front_cases as Fc

pytestmark = pytest.mark.gpu

F32, F64 = Fc.F32, Fc.F64
ALL = [(name, dt) for name in Fc.CASES for dt in Fc.case_dtypes(name)]
IDS = [f"{name}-{np.dtype(dt).name}" for name, dt in ALL]


def _set(wtp, ctx, name, dtype):
    """The case's mesh resident in ctx; returns (case, the spacing as Context.mesh_front takes it, the seeds)."""
    v, t = Fc.mesh_of(name, dtype)
    ctx.mesh_set(v, t)
    return Fc.CASES[name], wtp.sampling._sampler_spacing(Fc.library_spacing(wtp, name, dtype)), Fc.seeds_of(name, dtype)


def _front(ctx, case, sp, seeds, **kw):
    a = dict(n=case["n"], max_points=Fc.max_points_of(case), seed=Fc.SEED, batch=0)
    a.update(kw)
    info = ctx.mesh_front(sp, a["n"], seeds, a["max_points"], a["seed"], a["batch"])
    return info, ctx.mesh_front_get(info["n_points"])


def _bytes(got):
    return b"".join(got[k].tobytes() for k in ("xyz", "h", "cand", "parent"))


def _law_at(ctx, case, sp, xyz, dtype):
    """h as the library evaluates the case's law (the device's exp differs from numpy's by an ulp)."""
    if case["spacing"][0] == "const":
        return np.full(len(xyz), dtype(case["spacing"][1]), dtype=dtype)
    return ctx.spacing_eval(sp, xyz) if len(xyz) else np.zeros(0, dtype=dtype)


def _replay(ctx, case, sp, seeds, info, got, n=None, max_points=None):
    """serial() over the library's own candidates of every parent the run expanded, read out in one call."""
    n = case["n"] if n is None else n
    queue = np.concatenate([seeds, got["xyz"]])
    xyz, inside, r = ctx.mesh_front_candidates(sp, Fc.SEED, queue[:max(info["n_parents"], 1)], 0, n)
    ref = Fc.serial(seeds, n, Fc.max_points_of(case) if max_points is None else max_points, Fc.array_source(xyz, inside, r, n))
    return ref, xyz, inside, r


# ---- candidates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_parent", [0, 2 ** 29 + 3])              # j = q n + s passes 2^32 at n = 10
@pytest.mark.parametrize("name,dtype", [("grid8", F32), ("grid8", F64), ("grid12_bl", F32), ("grid12_bl", F64), ("far", F32),
                                        ("cavity", F32), ("box_max50", F32)])
def test_candidates_equal_the_model(wtp, ctx, name, dtype, first_parent):
    case, sp, seeds = _set(wtp, ctx, name, dtype)
    parents = seeds[:301] if name != "box_max50" else seeds[:103]     # (the oracle tests every triangle of the box mesh)
    n = case["n"]
    assert (first_parent + len(parents)) * n > 2 ** 32 or first_parent == 0
    xyz, inside, r = ctx.mesh_front_candidates(sp, Fc.SEED, parents, first_parent, n)
    if case["spacing"][0] == "bl":   # exp() differs by an ulp between the device and the host: the bound of DESIGN.md §8f.3
        mh = Fc.law_h(case["spacing"], parents)
        assert np.abs(r.astype(F64) - np.repeat(mh, n).astype(F64)).max() <= 4 * np.finfo(dtype).eps * case["spacing"][2]
        mx, mi, mr = Fc.candidates(name, dtype, parents, r[::n].copy(), first_parent, n)   # the positions from the library's h
    else:
        mx, mi, mr = Fc.candidates(name, dtype, parents, Fc.law_h(case["spacing"], parents), first_parent, n)
    assert xyz.dtype == dtype and xyz.shape == (len(parents) * n, 3)
    assert np.array_equal(r, mr) and np.array_equal(xyz, mx) and np.array_equal(inside, mi)


# ---- acceptance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", ALL, ids=IDS)
def test_run_equals_the_serial_loop_over_the_librarys_candidates(wtp, ctx, name, dtype):
    case, sp, seeds = _set(wtp, ctx, name, dtype)
    info, got = _front(ctx, case, sp, seeds)
    print(f"{name} {np.dtype(dtype).name}: n_points={info['n_points']} n_parents={info['n_parents']} "
          f"n_candidates={info['n_candidates']} n_inside={info['n_inside']} batches={info['n_batches']} "
          f"rounds_max={info['rounds_max']} host_syncs={info['host_syncs']}")
    ref, xyz, inside, r = _replay(ctx, case, sp, seeds, info, got)
    assert np.array_equal(got["cand"], ref["cand"]) and np.array_equal(got["parent"], ref["parent"])
    assert all(info[k] == ref[k] for k in ("n_parents", "n_candidates", "n_inside", "stop_reason"))
    assert info["n_points"] == len(ref["cand"]) and info["n_seeds"] == len(seeds)
    assert np.array_equal(got["xyz"], xyz[ref["cand"]])                 # a point is the candidate it names
    h = _law_at(ctx, case, sp, got["xyz"], dtype)
    assert got["h"].dtype == dtype and np.array_equal(got["h"], h)      # ... and carries the law's value there
    if len(h):
        assert info["r_min"] == float(h.min()) and info["r_max"] == float(h.max())
    else:
        assert info["r_min"] == 0.0 and info["r_max"] == 0.0
    if case["spacing"][0] == "const" and len(Fc.mesh_of(name, dtype)[1]) <= 12:   # the model's own run (12 triangles)
        m = Fc.model_run(name, dtype)
        assert np.array_equal(got["cand"], m["cand"]) and info["n_candidates"] == m["n_candidates"]
    if name == "grid8_h10":
        assert info["n_points"] == 0 and info["stop_reason"] == 1 and info["n_batches"] == 1 and info["n_parents"] == 384
    if name == "centre":
        assert info["n_batches"] >= 8 and info["n_parents"] == 1 + info["n_points"]


@pytest.mark.parametrize("dtype", Fc.DTYPES)
def test_a_smaller_max_points_gives_a_prefix(wtp, ctx, dtype):
    case, sp, seeds = _set(wtp, ctx, "grid12_bl", dtype)
    _, full = _front(ctx, case, sp, seeds)
    for m in (1, 37, len(full["cand"])):
        info, got = _front(ctx, case, sp, seeds, max_points=m)
        assert info["stop_reason"] == 2 and info["n_points"] == m
        assert all(np.array_equal(got[k], full[k][:m]) for k in got)
        if m < len(full["cand"]):
            assert info["n_candidates"] == got["cand"][-1] + 1


# ---- batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("grid8", F32), ("grid12", F64), ("grid12_bl", F32), ("centre", F64), ("cavity", F32),
                                        ("coincident", F32)])
def test_result_does_not_depend_on_the_batch(wtp, ctx, name, dtype):
    case, sp, seeds = _set(wtp, ctx, name, dtype)
    info0, got0 = _front(ctx, case, sp, seeds, batch=0)
    assert info0["rounds_max"] >= 1 and 0 < info0["host_syncs"] < 10 ** 6 and info0["n_points"] > 50
    for batch in (1, 7):
        info, got = _front(ctx, case, sp, seeds, batch=batch)
        assert _bytes(got) == _bytes(got0), batch
        assert all(info[k] == info0[k] for k in ("n_parents", "n_candidates", "n_inside", "stop_reason"))
        assert 1 <= info["rounds_max"] <= batch * case["n"] and info["n_batches"] >= info0["n_parents"] / batch


@pytest.mark.parametrize("dtype", Fc.DTYPES)
@pytest.mark.parametrize("n,batch", Fc.ODD_BATCHES)
def test_candidate_batches_of_63_64_and_65(wtp, ctx, n, batch, dtype):
    case, sp, seeds = _set(wtp, ctx, "grid8", dtype)
    info0, got0 = _front(ctx, case, sp, seeds, n=n)
    info, got = _front(ctx, case, sp, seeds, n=n, batch=batch)
    assert info0["n_points"] > 50 and _bytes(got) == _bytes(got0) and info["n_candidates"] == info0["n_candidates"]
    ref, _, _, _ = _replay(ctx, case, sp, seeds, info, got, n=n)
    assert np.array_equal(got["cand"], ref["cand"]) and info["n_candidates"] == ref["n_candidates"]


def test_a_batch_beyond_the_cap_is_clamped(wtp, ctx):
    """2^24 parents of 64 candidates each would be 2^30 threads' worth: the library decides at most 2^20 candidates at once."""
    case, sp, seeds = _set(wtp, ctx, "grid8", F32)
    info0, got0 = _front(ctx, case, sp, seeds, n=64)
    info, got = _front(ctx, case, sp, seeds, n=64, batch=2 ** 24)
    assert info0["n_points"] > 50 and _bytes(got) == _bytes(got0) and info["n_batches"] == info0["n_batches"]
    assert info["batch"] <= 2 ** 20 // 64


# ---- determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", Fc.DTYPES)
def test_two_calls_return_the_same_bits_and_the_seed_matters(wtp, ctx, dtype):
    case, sp, seeds = _set(wtp, ctx, "grid12_bl", dtype)
    _, a = _front(ctx, case, sp, seeds)
    _, b = _front(ctx, case, sp, seeds)
    assert _bytes(a) == _bytes(b)
    _, c = _front(ctx, case, sp, seeds, seed=Fc.SEED + 1)
    assert not np.array_equal(c["cand"], a["cand"])


# ---- properties, by brute force in double --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("grid8", F32), ("grid8", F64), ("grid12_bl", F32), ("grid12_bl", F64), ("far", F32),
                                        ("seed_outside", F64), ("cavity", F32)])
def test_front_volume_properties(wtp, ctx, O, name, dtype):
    case = Fc.CASES[name]
    v, t = Fc.mesh_of(name, dtype)
    seeds = Fc.seeds_of(name, dtype)
    law = Fc.library_spacing(wtp, name, dtype)
    vol = wtp.front_volume((v, t), law, seeds=seeds, n=case["n"], seed=Fc.SEED, ctx=ctx)
    p, h, par, info = vol.points(), vol.front_h, vol.front_parent, vol.front_info
    assert p.dtype == dtype and len(p) == info["n_points"] > 50 and isinstance(vol, wtp.PointVolume) and info["stop_reason"] == 1
    assert O.mesh_query(v, t, p)["inside"].all()                        # every point is inside, by the oracle
    ns, m = len(seeds), len(p)
    q = np.concatenate([seeds, p])
    hq = np.concatenate([_law_at(ctx, case, wtp.sampling._sampler_spacing(law), seeds, dtype), h])
    r = hq[par].astype(F64)                                             # the radius a point was tested with: its parent's h
    dist = np.sqrt(((p.astype(F64)[:, None] - q.astype(F64)[None]) ** 2).sum(axis=2))
    earlier = np.arange(ns + m)[None] < ns + np.arange(m)[:, None]
    earlier[np.arange(m), par] = False                                    # never the parent
    slack = 8 * np.finfo(dtype).eps * float(np.abs(q).max())
    assert (dist[earlier] >= np.broadcast_to(r[:, None], dist.shape)[earlier] - slack).all()
    assert np.abs(dist[np.arange(m), par] - r).max() <= slack + 8 * np.finfo(dtype).eps * r.max()
    # the front died out: no inside candidate of any parent is free of every entry of the final queue but its parent
    cx, ci, cr = ctx.mesh_front_candidates(wtp.sampling._sampler_spacing(law), Fc.SEED, q, 0, case["n"])
    assert info["n_candidates"] == len(cx) and info["n_inside"] == int(ci.sum())
    taken = np.zeros(len(cx), dtype=bool)
    taken[ctx.mesh_front_get(m, want=("cand",))["cand"]] = True
    idx = np.nonzero(ci & ~taken)[0]
    d = np.sqrt(((cx[idx].astype(F64)[:, None] - q.astype(F64)[None]) ** 2).sum(axis=2))
    d[np.arange(len(idx)), idx // case["n"]] = np.inf
    assert (d.min(axis=1) < cr[idx].astype(F64) + slack).all()


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors_leave_the_context_usable(wtp, ctx):
    from whatsthepoint_jl_amd import _lib as L

    ctx.mesh_clear()
    with pytest.raises(wtp.WtpError) as e:
        ctx.mesh_front(0.15, 10, np.zeros((1, 3)))                       # no mesh
    assert e.value.code == L.WTP_ERR_STATE
    case, sp, seeds = _set(wtp, ctx, "grid8", F32)
    for call in (lambda: ctx.mesh_front_get(1), ctx.mesh_front_get_dev):  # before a successful run (mesh_set voided any)
        with pytest.raises(wtp.WtpError) as e:
            call()
        assert e.value.code == L.WTP_ERR_STATE
    bad = [dict(n=0), dict(n=65), dict(n=-1), dict(max_points=0), dict(seed=2 ** 24), dict(batch=-1), dict(batch=2 ** 24 + 1),
           dict(max_points=2 ** 31)]
    for kw in bad:
        with pytest.raises(wtp.WtpArgumentError):
            _front(ctx, case, sp, seeds, **kw)
    per_point = L.SpacingDesc()
    per_point.kind = L.WTP_SPACING_PER_POINT
    with pytest.raises(wtp.WtpArgumentError):
        ctx.mesh_front(None, 10, seeds, spacing_desc=per_point)
    with pytest.raises(wtp.WtpArgumentError):
        ctx.mesh_front(dict(kind=3, p0=0.1, p1=0.2, p2=0.0, boundary=Fc.LAW_POINTS), 10, seeds)   # check_spacing_law
    for kw in (dict(seed=2 ** 24), dict(n=0), dict(n=65), dict(first_parent=-1)):
        a = dict(seed=Fc.SEED, first_parent=0, n=10)
        a.update(kw)
        with pytest.raises(wtp.WtpArgumentError):
            ctx.mesh_front_candidates(0.15, a["seed"], seeds[:4], a["first_parent"], a["n"])
    # the rows of the raw entry that the mirror cannot reach: n_seeds < 0, seeds NULL with n_seeds > 0
    info = L.FrontInfo()
    const = L.SpacingDesc()
    const.kind, const.constant = L.WTP_SPACING_CONSTANT, 0.15
    one = np.zeros((1, 3), dtype=F32)
    for seeds_p, ns in ((one.ctypes.data_as(C.c_void_p), -1), (None, 1)):
        rc = ctx._lib.wtp_mesh_front(ctx._h, C.byref(const), 10, seeds_p, ns, 10, C.c_uint64(Fc.SEED), 0, C.byref(info))
        assert rc == L.WTP_ERR_ARG
    # seeds: a coordinate that is not finite; a spacing that is not > 0 at a seed (named)
    for x in (np.nan, np.inf):
        with pytest.raises(wtp.WtpArgumentError, match="seed 1 "):
            ctx.mesh_front(0.15, 10, np.array([(0.5, 0.5, 0.5), (0.5, x, 0.5)]))
    # negative within 0.16 of the law points below the floor, and steep enough there for a candidate to jump in
    law = wtp.BoundaryLayerSpacing(Fc.LAW_POINTS.astype(F32), -0.3, 0.24, 0.3).desc()
    with pytest.raises(wtp.WtpArgumentError, match="seed 2 "):
        ctx.mesh_front(law, 10, np.array([(0.5, 0.5, 0.9), (0.5, 0.5, 0.8), (0.5, 0.5, 0.0)]))
    # ... at an accepted point: the smallest such candidate is named, whatever the batch
    top = np.array([(0.5, 0.5, 0.95)], dtype=F32)                       # h > 0 up there; the front walks down to the floor
    ok = ctx.mesh_front(law, 10, top, 3, Fc.SEED, 0)
    first3 = ctx.mesh_front_get(3)
    assert ok["n_points"] == 3 and (first3["h"] > 0).all()              # a run that ends before the bad point is fine
    names = set()
    for batch in (0, 1, 7):
        with pytest.raises(wtp.WtpArgumentError, match="accepted from candidate [0-9]+ is not finite and > 0") as e:
            ctx.mesh_front(law, 10, top, 10 ** 6, Fc.SEED, batch)
        names.add(str(e.value))
    assert len(names) == 1
    with pytest.raises(wtp.WtpError) as e:
        ctx.mesh_front_get(1)                                           # the failed call left no result
    assert e.value.code == L.WTP_ERR_STATE
    # no seeds: WTP_OK with no points at the ABI; no points is an error in the mirror
    info = ctx.mesh_front(0.15, 10, None)
    assert info["n_points"] == 0 and info["stop_reason"] == 1 and info["n_candidates"] == 0
    assert ctx.mesh_front_get(0)["xyz"].shape == (0, 3)
    with pytest.raises(wtp.WtpArgumentError, match="no points"):
        wtp.front_volume(Fc.mesh_of("grid8_h10", F64), 10.0, seeds=Fc.seeds_of("grid8_h10", F64), ctx=ctx)
    # zero surface area
    ctx.mesh_set(np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)], dtype=F32), np.array([(0, 1, 2)], dtype=np.int32))
    with pytest.raises(wtp.WtpArgumentError, match="zero surface area"):
        ctx.mesh_front(0.15, 10, one)
    # the context still works
    case, sp, seeds = _set(wtp, ctx, "grid8", F32)
    assert _front(ctx, case, sp, seeds)[0]["n_points"] > 50


def test_front_fill_and_sample_void_one_another(wtp, ctx):
    from whatsthepoint_jl_amd import _lib as L

    case, sp, seeds = _set(wtp, ctx, "grid8", F32)
    info, got = _front(ctx, case, sp, seeds)
    gets = dict(front=[lambda: ctx.mesh_front_get(1), ctx.mesh_front_get_dev], fill=[lambda: ctx.mesh_fill_get(1), ctx.mesh_fill_get_dev],
                sample=[lambda: ctx.mesh_sample_get(1), ctx.mesh_sample_get_dev])
    runs = dict(front=lambda: ctx.mesh_front(sp, 10, seeds, 10 ** 6, Fc.SEED, 0),
                fill=lambda: ctx.mesh_fill(sp, 0.75, seeds, 10 ** 6, 200, Fc.SEED, 0),
                sample=lambda: ctx.mesh_sample(sp, 0.75, 10 ** 6, 200, Fc.SEED, 0))

    def only(kind):
        for k, calls in gets.items():
            if k != kind:
                for call in calls:
                    with pytest.raises(wtp.WtpError) as e:
                        call()
                    assert e.value.code == L.WTP_ERR_STATE

    only("front")
    # the read-outs leave a resident front untouched
    cands = ctx.mesh_front_candidates(sp, Fc.SEED, seeds, 0, 10)
    ctx.mesh_fill_darts(sp, 0.75, Fc.SEED, 0, 100)
    ctx.mesh_sample_darts(sp, 0.75, Fc.SEED, 0, 100)
    assert _bytes(ctx.mesh_front_get(info["n_points"])) == _bytes(got)
    fill0 = sample0 = None
    for first, second in (("front", "fill"), ("fill", "front"), ("front", "sample"), ("sample", "front"), ("fill", "sample"),
                          ("sample", "fill")):
        assert runs[first]()["n_points"] > 0
        only(first)
        i2 = runs[second]()
        only(second)
        if second == "front":
            assert _bytes(ctx.mesh_front_get(i2["n_points"])) == _bytes(got)
            assert np.array_equal(ctx.mesh_front_candidates(sp, Fc.SEED, seeds, 0, 10)[0], cands[0])
        if second == "fill":                                              # the fill and the sample return what they did before
            f = ctx.mesh_fill_get(i2["n_points"])["xyz"]
            fill0 = f if fill0 is None else fill0
            assert np.array_equal(f, fill0)
        if second == "sample":
            s = ctx.mesh_sample_get(i2["n_points"])["xyz"]
            sample0 = s if sample0 is None else sample0
            assert np.array_equal(s, sample0)


def test_runs_in_turn_on_one_context_equal_those_on_fresh_contexts(wtp, ctx):
    """Sample, front, fill and front again share one run-begin path and one set of buffers, also across a change of the
    mesh's dtype: each call returns the bytes and the counts of the same call on a context that has run nothing else."""
    import surface_sampling_cases as Sc
    import volume_fill_cases as Vc

    def sample(c, dtype):
        case = Sc.CASES["cube_f075"]
        sp = wtp.sampling._sampler_spacing(Sc.library_spacing(wtp, "cube_f075", dtype))
        info = c.mesh_sample(sp, case["factor"], Sc.max_points_of(case), case["stall_limit"], Sc.SEED, 0)
        got = c.mesh_sample_get(info["n_points"])
        return [info[k] for k in ("n_points", "n_darts", "stop_reason")], [got[k].tobytes() for k in ("xyz", "tri", "r", "dart")]

    def fill(c, dtype):
        case = Vc.CASES["cube_seeds"]
        sp = wtp.sampling._sampler_spacing(Vc.library_spacing(wtp, "cube_seeds", dtype))
        info = c.mesh_fill(sp, case["factor"], Vc.seeds_of("cube_seeds", dtype)[0], Vc.max_points_of(case), case["stall_limit"],
                           Vc.SEED, 0)
        got = c.mesh_fill_get(info["n_points"])
        return [info[k] for k in ("n_points", "n_darts", "stop_reason")], [got[k].tobytes() for k in ("xyz", "r", "dart")]

    def front(batch):
        def run(c, dtype):
            case = Fc.CASES["grid8"]
            sp = wtp.sampling._sampler_spacing(Fc.library_spacing(wtp, "grid8", dtype))
            info, got = _front(c, case, sp, Fc.seeds_of("grid8", dtype), batch=batch)
            return [info[k] for k in ("n_points", "n_candidates", "stop_reason")], [got[k].tobytes() for k in ("xyz", "h", "cand", "parent")]
        return run

    def mesh(dtype):                                                      # the three cases stand on the same cube
        v, t = Fc.mesh_of("grid8", dtype)
        for other in (Sc.mesh_of("cube_f075", dtype), Vc.mesh_of("cube_seeds", dtype)):
            assert np.array_equal(other[0], v) and np.array_equal(other[1], t)
        return v, t

    steps = [(F32, sample), (F32, front(0)), (F32, fill), (F32, front(7)), (F64, front(0)), (F64, sample)]
    resident = None
    for i, (dtype, run) in enumerate(steps):
        if dtype != resident:
            ctx.mesh_set(*mesh(dtype))
            resident = dtype
        counts, data = run(ctx, dtype)
        with wtp.Context(0) as fresh:
            fresh.mesh_set(*mesh(dtype))
            fresh_counts, fresh_data = run(fresh, dtype)
        assert counts[0] > 50 and counts == fresh_counts, i
        assert data == fresh_data, i


# ---- device read-out -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", Fc.DTYPES)
def test_get_dev_equals_get(wtp, ctx, dtype):
    import torch

    case, sp, seeds = _set(wtp, ctx, "grid12_bl", dtype)
    info, got = _front(ctx, case, sp, seeds)
    n = info["n_points"]
    tdt = torch.float32 if dtype == F32 else torch.float64
    xyz = torch.zeros((n, 3), dtype=tdt, device="cuda")
    h = torch.zeros(n, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    ctx.mesh_front_get_dev(xyz.data_ptr(), h.data_ptr())
    assert np.array_equal(xyz.cpu().numpy(), got["xyz"]) and np.array_equal(h.cpu().numpy(), got["h"])
    only_h = torch.zeros(n, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    ctx.mesh_front_get_dev(0, only_h.data_ptr())                         # every output may be absent
    assert np.array_equal(only_h.cpu().numpy(), got["h"])
    assert np.array_equal(ctx.mesh_front_get(n, want=("parent",))["parent"], got["parent"])   # parent without cand


# ---- the reference's own items (test/discretization.jl:21-35, :146-161), in the reference's Float64 -------------------------
def _box_and_boundary(wtp):
    v, t = Fc.mesh_of("box_max50", F64)
    return v, t, wtp.PointBoundary(v[t].mean(axis=1))                    # PointBoundary(mesh): one point per face


def test_reference_slak_kosec_with_octree(wtp, ctx, O):
    v, t, bnd = _box_and_boundary(wtp)
    oc = wtp.TriangleOctree(v, t, ctx=ctx)
    with pytest.warns(UserWarning, match=r"discretization stopping early, reached max points \(50\)"):
        cloud = wtp.discretize(bnd, wtp.ConstantSpacing(25.0 / 8), oc, alg=wtp.SlakKosec(), max_points=50, ctx=ctx)
    vol = cloud.volume
    assert isinstance(cloud, wtp.PointCloud) and 0 < len(vol) <= 50 and len(cloud.boundary) == len(t)
    assert vol.front_info["stop_reason"] == 2 and vol.front_info["n_seeds"] == len(t)
    assert oc.isinside(vol.points(), ctx=ctx).all() and O.mesh_query(v, t, vol.points())["inside"].all()


def test_reference_slak_kosec_with_boundary_layer_spacing(wtp, ctx, O):
    v, t, bnd = _box_and_boundary(wtp)
    law = wtp.BoundaryLayerSpacing(bnd.points(), 0.5, 5.0, 2.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cloud = wtp.discretize(bnd, law, (v, t), alg=wtp.SlakKosec(10), max_points=30, ctx=ctx)
    assert isinstance(cloud, wtp.PointCloud) and 0 < len(cloud.volume) <= 30
    assert O.mesh_query(v, t, cloud.volume.points())["inside"].all()


# ---- downstream -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", Fc.DTYPES)
def test_discretize_with_the_front_feeds_repel(wtp, ctx, dtype):
    v, t = Fc.mesh_of("grid8", dtype)
    oc = wtp.TriangleOctree(v, t, ctx=ctx)
    bnd = wtp.PointBoundary.from_mesh(oc, 0.15, ctx=ctx)
    cloud = wtp.discretize(bnd, 0.15, oc, alg=wtp.SlakKosec(), ctx=ctx)
    assert cloud.points().dtype == dtype and len(cloud.volume) > 50 and len(cloud.boundary) == len(bnd)
    assert cloud.volume.front_info["stop_reason"] == 1 and len(cloud.volume.front_parent) == len(cloud.volume)
    out = wtp.repel(cloud, 0.15, oc, max_iters=3, ctx=ctx)
    assert len(out) == len(cloud)                                         # counts conserved
    assert len(out.boundary) >= len(bnd) and oc.isinside(out.volume.points(), ctx=ctx).all()


def test_discretize_without_alg_returns_the_fill(wtp, ctx):
    v, t = Fc.mesh_of("grid8", F32)
    seeds = Fc.seeds_of("grid8", F32)
    cloud = wtp.discretize(seeds, 0.15, (v, t), stall_limit=200, ctx=ctx)
    vol = wtp.fill_volume((v, t), 0.15, seeds=seeds, factor=0.75, stall_limit=200, ctx=ctx)
    assert cloud.volume.points().tobytes() == vol.points().tobytes() and cloud.volume.fill_info["n_darts"] == vol.fill_info["n_darts"]
    ctx.mesh_set(v, t)
    info = ctx.mesh_fill(0.15, 0.75, seeds, 10_000_000, 2000, wtp.synth.SEED & 0xFFFFFF, 0)   # today's defaults, spelled out
    plain = wtp.discretize(seeds, 0.15, (v, t), ctx=ctx)
    assert plain.volume.fill_info["n_darts"] == info["n_darts"] and len(plain.volume) == info["n_points"]
    assert not hasattr(plain.volume, "front_info")
