"""No-GPU checks of the advancing front's model (front_cases.py): the batch algorithm the library runs equals the serial
loop for every number of parents per batch; the directions are unit vectors and their azimuth agrees with libm; the cases
have the properties they are there for; the header declares the entry points and the built library exports them."""
import ctypes
import os
import re

import numpy as np
import pytest

import front_cases as Fc

F32, F64 = Fc.F32, Fc.F64
ALL = [(name, dt) for name in Fc.CASES for dt in Fc.case_dtypes(name)]
IDS = [f"{name}-{np.dtype(dt).name}" for name, dt in ALL]
ENTRY_POINTS = ["wtp_mesh_front", "wtp_mesh_front_get", "wtp_mesh_front_get_dev", "wtp_mesh_front_candidates"]
KEYS = ("n_parents", "n_candidates", "n_inside", "stop_reason")


def _same(a, b):
    return np.array_equal(a["cand"], b["cand"]) and np.array_equal(a["parent"], b["parent"]) and all(a[k] == b[k] for k in KEYS) \
        and np.array_equal(a["queue"], b["queue"])


@pytest.mark.parametrize("name,dtype", ALL, ids=IDS)
def test_batches_equal_the_serial_loop(name, dtype):
    case = Fc.CASES[name]
    ref = Fc.model_run(name, dtype)
    src = Fc.model_source(name, dtype)
    for batch in (1, 7, 64, 0):
        got = Fc.batched(Fc.seeds_of(name, dtype), case["n"], Fc.max_points_of(case), src, batch)
        assert _same(got, ref), batch
        assert 1 <= got["rounds_max"] <= (batch * case["n"] if batch else got["n_candidates"])


@pytest.mark.parametrize("name,want", [("grid8", {1: (487, 3), 7: (70, 4), 0: (6, 6)}),
                                       ("grid12_bl", {1: (1241, 3), 7: (178, 8), 0: (7, 9)}),
                                       ("centre", {1: (235, 4), 7: (37, 5), 0: (12, 5)})])
def test_batches_and_rounds_of_the_model(name, want):
    """(n_batches, rounds_max) by batch, as measured (Float32 and Float64 agree): what test_gpu_sampler_edges.py holds the
    library's counts against.  grid12_bl with every parent available needs more rounds than one group of 8."""
    case = Fc.CASES[name]
    for dtype in Fc.DTYPES:
        for batch, (n_batches, rounds_max) in want.items():
            got = Fc.batched(Fc.seeds_of(name, dtype), case["n"], Fc.max_points_of(case), Fc.model_source(name, dtype), batch)
            assert (got["n_batches"], got["rounds_max"]) == (n_batches, rounds_max), (dtype, batch)
            if batch == 1:
                assert got["n_batches"] == got["n_parents"]
    assert want[0][1] <= 8 or name == "grid12_bl"


@pytest.mark.parametrize("n,batch", Fc.ODD_BATCHES)
def test_candidate_batches_of_63_64_and_65(n, batch):
    assert n * batch in (63, 64, 65)
    seeds = Fc.seeds_of("grid8", F32)
    src = Fc.model_source("grid8", F32, n=n)
    ref = Fc.serial(seeds, n, 10_000_000, src)
    assert len(ref["cand"]) > 50 and _same(Fc.batched(seeds, n, 10_000_000, src, batch), ref)


@pytest.mark.parametrize("dtype", Fc.DTYPES)
def test_directions_are_unit_vectors_and_the_azimuth_agrees_with_libm(dtype):
    eps = float(np.finfo(dtype).eps)
    m = 200_000
    d = Fc.directions(0, m, dtype).astype(F64)
    assert Fc.directions(0, m, dtype).dtype == dtype
    norm_err = np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() / eps
    _, v = Fc.uv(0, m, dtype)
    c, s = Fc.cos_sin(v, dtype)
    lam = 2.0 * np.pi * v.astype(F64)                                   # v holds 24 bits: exact in both types
    trig_err = max(np.abs(c.astype(F64) - np.cos(lam)).max(), np.abs(s.astype(F64) - np.sin(lam)).max()) / eps
    print(f"{np.dtype(dtype).name}: | |d| - 1 | <= {norm_err:.2f} eps, cos and sin within {trig_err:.2f} eps of libm")
    assert norm_err <= 2.0 and trig_err <= 4.0
    # every octant is drawn, z spans the sphere, and candidate indices are 64-bit
    assert set(np.floor(8 * v.astype(F64)).astype(int)) == set(range(8)) and d[:, 2].min() < -0.999 and d[:, 2].max() > 0.999
    assert not np.array_equal(Fc.directions(2 ** 32 + 5, 8, dtype), Fc.directions(5, 8, dtype))
    assert np.array_equal(Fc.directions(2 ** 32 + 5, 8, dtype), Fc.directions(2 ** 32, 13, dtype)[5:])


def test_a_smaller_max_points_gives_a_prefix():
    full = Fc.model_run("grid8", F32)
    for name, m in (("grid8_max1", 1), ("grid8_max37", 37)):
        run = Fc.model_run(name, F32)
        assert run["stop_reason"] == 2 and len(run["cand"]) == m and np.array_equal(run["cand"], full["cand"][:m])
        assert run["n_candidates"] == run["cand"][-1] + 1                 # the run ends before the next candidate


@pytest.mark.parametrize("name,dtype", [("grid8", F32), ("grid12", F64), ("grid12_bl", F32), ("cavity", F32), ("coincident", F64)])
def test_points_are_inside_and_keep_their_own_radius(name, dtype):
    case, run = Fc.CASES[name], Fc.model_run(name, dtype)
    q = run["queue"]
    ns = len(Fc.seeds_of(name, dtype))
    assert len(run["cand"]) > 50 and Fc.inside_of(name, dtype, q[ns:]).all()
    h = Fc.law_h(case["spacing"], q).astype(F64)
    r = h[run["parent"]]                                                # the radius a point was tested with: its parent's h
    d = np.linalg.norm(q[ns:, None].astype(F64) - q[None].astype(F64), axis=2)
    later = np.arange(len(q))[None] >= ns + np.arange(len(q) - ns)[:, None]
    d[later] = np.inf                                                     # only the entries then in the queue count
    d[np.arange(len(q) - ns), run["parent"]] = np.inf                    # ... and never the parent
    assert (d >= r[:, None] * (1 - 8 * np.finfo(dtype).eps)).all()
    # a point sits one spacing from its parent
    dp = np.linalg.norm(q[ns:].astype(F64) - q[run["parent"]].astype(F64), axis=1)
    assert np.abs(dp / r - 1).max() <= 8 * np.finfo(dtype).eps * max(1.0, float(np.abs(q).max()) / r.min())


def test_case_properties():
    g8 = Fc.model_run("grid8", F32)
    assert g8["stop_reason"] == 1 and g8["n_candidates"] == 10 * g8["n_parents"] == 10 * (384 + len(g8["cand"]))
    assert (g8["parent"] < 384 + np.arange(len(g8["cand"]))).all() and (np.diff(g8["cand"]) > 0).all()
    g12 = Fc.model_run("grid12", F64)
    assert 500 <= len(g12["cand"]) <= 800 and g12["stop_reason"] == 1
    # one seed: the whole cloud descends from it, generation by generation; small batches
    c = Fc.model_run("centre", F32)
    b = Fc.batched(Fc.seeds_of("centre", F32), 10, 10_000_000, Fc.model_source("centre", F32), 0)
    assert len(c["cand"]) > 150 and c["n_parents"] == 1 + len(c["cand"]) and b["n_batches"] >= 8
    assert c["parent"][0] == 0 and c["cand"][0] < 10
    c1 = Fc.model_run("centre_n1", F64)
    assert c1["n_parents"] == 1 + len(c1["cand"]) == c1["n_candidates"] and 1 <= len(c1["cand"]) <= 20
    # the asymmetry: a point within an earlier entry's own h, but not within the radius it was tested with
    bl = Fc.model_run("grid12_bl", F64)
    q, ns = bl["queue"].astype(F64), 864
    h = Fc.law_h(Fc.CASES["grid12_bl"]["spacing"], bl["queue"]).astype(F64)
    assert h[ns:].max() / h[ns:].min() >= 1.5
    r = h[bl["parent"]]
    d = np.linalg.norm(q[ns:, None] - q[None], axis=2)
    earlier = np.arange(len(q))[None] < ns + np.arange(len(q) - ns)[:, None]
    earlier[np.arange(len(q) - ns), bl["parent"]] = False
    assert (earlier & (d < h[None]) & (d >= r[:, None])).any() and not (earlier & (d < r[:, None] * (1 - 1e-12))).any()
    # nothing is inside: no point, every seed expanded
    h10 = Fc.model_run("grid8_h10", F32)
    assert len(h10["cand"]) == 0 and (h10["n_parents"], h10["n_candidates"], h10["n_inside"], h10["stop_reason"]) == (384, 3840, 0, 1)
    far = Fc.model_run("far", F32)
    assert far["queue"].dtype == F32 and far["queue"].min() >= 1000 and len(far["cand"]) > 50
    cav = Fc.model_run("cavity", F32)
    assert len(cav["cand"]) > 50 and 0.3 < cav["n_inside"] / cav["n_candidates"] < 0.8
    x = cav["queue"][:400] + F32(0.01)                                   # the cached inside test is the oracle's own
    assert np.array_equal(Fc.inside_of("cavity", F32, x), Fc.oracle.mesh_query(*Fc.mesh_of("cavity", F32), x)["inside"])
    assert 0 < Fc.inside_of("cavity", F32, x).sum() < 400
    box = Fc.model_run("box_max50", F32)
    assert len(box["cand"]) == 50 and box["stop_reason"] == 2 and box["n_parents"] < len(Fc.seeds_of("box_max50", F32))
    out = Fc.model_run("seed_outside", F64)
    assert not Fc.inside_of("seed_outside", F64, Fc.seeds_of("seed_outside", F64)).any() and len(out["cand"]) > 150
    # coincident seeds: each one's candidates lie at h (1 +- eps) from the other, so rounding decides them one by one;
    # every candidate of seed 0 that was accepted would have been lost to seed 1 had it not been exempt as ... its twin
    for dt in Fc.DTYPES:
        co = Fc.model_run("coincident", dt)
        s = Fc.seeds_of("coincident", dt)
        cx, ci, cr = Fc.candidates("coincident", dt, s, Fc.law_h(("const", 0.15), s), 0, 10)
        hit_twin = np.array([Fc._hits(s[1 - i // 10:2 - i // 10], cx[i], cr[i])[0] for i in range(20)])
        first = co["cand"][co["cand"] < 20]
        assert ci.all() and hit_twin.any() and not hit_twin[first].any() and len(co["cand"]) > 150
        own = np.array([Fc._hits(s[i // 10:i // 10 + 1], cx[i], cr[i])[0] for i in range(20)])
        assert own.any() or hit_twin.sum() < 20                           # the parent's exemption is what keeps its own


def test_header_declares_the_front_and_the_library_exports_it(wtp):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "wtp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wtp_[a-z_0-9]+)\s*\(", txt))
    assert "wtp_front_info" in txt
    lib = ctypes.CDLL(wtp.SO_PATH)
    from whatsthepoint_jl_amd import _lib as L

    for name in ENTRY_POINTS:
        assert name in declared and hasattr(lib, name) and name in L.SIGNATURES
    assert ctypes.sizeof(L.FrontInfo) == 80                            # six int64, four int32, two doubles


def test_front_argument_errors_before_touching_the_gpu(wtp):
    v, t = Fc.mesh_of("grid8", F64)
    seeds = Fc.seeds_of("grid8", F64)
    with pytest.raises(wtp.WtpArgumentError, match="max_points must be positive"):
        wtp.front_volume((v, t), 0.15, seeds=seeds, max_points=0)
    for n in (0, 65, 2.5, True):
        with pytest.raises(wtp.WtpArgumentError, match="1 to 64"):
            wtp.SlakKosec(n)
        with pytest.raises(wtp.WtpArgumentError, match="1 to 64"):
            wtp.front_volume((v, t), 0.15, seeds=seeds, n=n)
    assert wtp.SlakKosec().n == 10 and repr(wtp.SlakKosec(7)) == "SlakKosec(n=7)"
    with pytest.raises(wtp.WtpArgumentError):
        wtp.front_volume((v, t), lambda p: 0.15, seeds=seeds)           # not a built-in law: nothing to run on the device
    for kw in (dict(factor=0.75), dict(stall_limit=2000)):
        with pytest.raises(wtp.WtpArgumentError, match="do not apply to SlakKosec"):
            wtp.discretize(seeds, 0.15, (v, t), alg=wtp.SlakKosec(), **kw)
    with pytest.raises(wtp.WtpArgumentError, match="alg must be"):
        wtp.discretize(seeds, 0.15, (v, t), alg="SlakKosec")
