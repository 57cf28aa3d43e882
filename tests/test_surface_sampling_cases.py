"""No-GPU checks of the surface sampler's model (surface_sampling_cases.py): the batch algorithm the library runs equals
the serial dart thrower for every batch size, the cases have the properties they are there for, the reference's known
answers hold on the serial result, and the host mirror refuses bad arguments before it touches a device."""
import numpy as np
import pytest

import surface_sampling_cases as S

F32, F64 = S.F32, S.F64


def _run(name, dtype=F32):
    case = S.case_of(name)
    xyz, tri, r, acc, n_darts, reason = S.model_run(name, dtype)
    return case, xyz, tri, r, acc, n_darts, reason


@pytest.mark.parametrize("batch", [63, 64, 65, 1000, 4096, 18000])
def test_batches_equal_the_serial_loop_on_the_cube(batch):
    case, xyz, tri, r, acc, n_darts, reason = _run("cube_f075")
    assert batch != 18000 or batch > n_darts                          # one batch larger than the whole run
    got, nd, why, rounds = S.batched(xyz, r, S.max_points_of(case), case["stall_limit"], batch)
    assert np.array_equal(got, acc) and nd == n_darts and why == reason == 1
    assert 1 <= rounds <= batch
    if batch == 4096:
        assert rounds >= 5                                            # the case really exercises chains of decisions


@pytest.mark.parametrize("name", ["one_triangle", "cube_max1", "cube_max37", "cube_stall3"])
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 1000, 4096])
def test_batches_equal_the_serial_loop_at_the_stop_rules(name, batch):
    case, xyz, tri, r, acc, n_darts, reason = _run(name)
    got, nd, why, rounds = S.batched(xyz, r, S.max_points_of(case), case["stall_limit"], batch)
    assert np.array_equal(got, acc) and nd == n_darts and why == reason


@pytest.mark.parametrize("name", ["slab", "graded_bl", "graded_loglike", "cube_far", "cube_zero_area", "box"])
def test_batches_equal_the_serial_loop_on_every_other_case(name):
    case, xyz, tri, r, acc, n_darts, reason = _run(name)
    got, nd, why, rounds = S.batched(xyz, r, S.max_points_of(case), case["stall_limit"], 4096)
    assert np.array_equal(got, acc) and nd == n_darts and why == reason


def test_a_smaller_max_points_gives_a_prefix():
    _, _, _, _, full, _, _ = _run("cube_f075")
    for name, m in (("cube_max1", 1), ("cube_max37", 37)):
        case, xyz, tri, r, acc, n_darts, reason = _run(name)
        assert reason == 2 and len(acc) == m and np.array_equal(acc, full[:m])
        assert n_darts == acc[-1] + 1                                 # the run ends right behind the last accepted dart


def test_single_triangle_and_early_stall():
    case, xyz, tri, r, acc, n_darts, reason = _run("one_triangle")
    assert r[0] > 2.0                                                 # larger than the triangle's diameter sqrt(2)
    assert list(acc) == [0] and n_darts == 1 + case["stall_limit"] and reason == 1
    case, xyz, tri, r, acc, n_darts, reason = _run("cube_stall3")
    assert reason == 1 and n_darts < 4096 and n_darts == acc[-1] + 1 + 3   # ends inside the first batch


@pytest.mark.parametrize("name", ["cube_f075", "cube_f100"])
@pytest.mark.parametrize("dtype", S.DTYPES)
def test_reference_known_answers_on_the_cube(name, dtype):
    """test/surface_sampling.jl on the unit cube: n > 50, every point on a face, unit axis-aligned normals, areas sum
    to 6, and no pair closer than min(r_i, r_j)."""
    case, xyz, tri, r, acc, n_darts, reason = _run(name, dtype)
    p, rr = xyz[acc].astype(F64), r[acc].astype(F64)
    assert len(acc) > 50
    on_face = np.minimum(np.abs(p), np.abs(p - 1)).min(axis=1)
    assert on_face.max() <= 4 * np.finfo(dtype).eps
    v, t = S.mesh_of(name, dtype)
    c = v.astype(F64)[t[tri[acc]]]
    nrm = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    assert np.allclose(np.abs(nrm).max(axis=1), 1) and np.allclose(np.abs(nrm).sum(axis=1), 1)
    cum, total = S.areas_of(name, dtype)
    w = rr ** 2
    assert abs((total / w.sum() * w).sum() - 6.0) <= 1e-12 * 6
    d = np.linalg.norm(p[:, None] - p[None], axis=2) + 10 * np.eye(len(p))
    assert (d >= np.minimum(rr[:, None], rr[None]) * (1 - 8 * np.finfo(dtype).eps)).all()


def test_case_properties():
    # opposite faces of the slab block each other: far fewer samples than two free 1 x 1 faces would take
    _, xyz, tri, r, acc, _, _ = _run("slab")
    _, _, _, _, cube_acc, _, _ = _run("cube_f075")
    assert r[0] > 0.05 and len(acc) < len(cube_acc) / 3
    # the graded cases span about 3x in r, and the law's points are off the surface (r stays well above 0)
    for name in ("graded_bl", "graded_loglike"):
        _, xyz, tri, r, acc, _, _ = _run(name)
        ra = r[acc]
        assert 2.4 <= ra.max() / ra.min() <= 4.0 and ra.min() > 0.04
    # cell coordinates far from the origin, in Float32
    _, xyz, _, _, acc, _, _ = _run("cube_far")
    assert xyz.dtype == F32 and xyz[acc].min() >= 999.999    # (a sample may round an ulp outside the box)
    # the zero-area triangles are never picked and change nothing else
    _, xyz0, tri0, _, acc0, nd0, _ = _run("cube_zero_area")
    _, xyz1, tri1, _, acc1, nd1, _ = _run("cube_f075")
    assert not np.isin(tri0, [0, 7]).any() and np.array_equal(xyz0, xyz1) and np.array_equal(acc0, acc1) and nd0 == nd1
    _, _, _, _, acc, _, _ = _run("box")
    assert 1000 <= len(acc) <= 2000


# ---- the edge cases of test_gpu_sampler_edges.py: the numbers its runs rely on -------------------------------------------
def test_whole_batches_and_the_schedule_of_batch_0():
    assert S.whole_batches(2048, 2048) == (1, 2048)                   # a run that ends at position B ends in that batch
    assert S.whole_batches(2049, 2048) == (2, 4096) and S.whole_batches(1, 7) == (1, 7)
    assert S.whole_batches(4096, 0) == (1, 4096) and S.whole_batches(4097, 0) == (2, 4096 + 8192)
    # batch = 0 doubles from 4096 up to 2^20: the ninth batch is the first of 2^20 darts, and it ends at dart 4096 * 511
    assert S.whole_batches(4096 * 511, 0) == (9, 4096 * 511) and S.whole_batches(4096 * 511 + 1, 0) == (10, 4096 * 511 + 2 ** 20)
    sizes = S.batch_sizes(0)
    assert [next(sizes) for _ in range(11)] == [4096 << k for k in range(8)] + [2 ** 20] * 3
    # the schedule changes neither the result nor, given whole batches of darts, what a fixed batch of its size computes
    case, xyz, tri, r, acc, n_darts, reason = _run("cube_f075")
    nb, nd = S.whole_batches(n_darts, 0)
    assert (nb, nd) == (3, 4096 + 8192 + 16384) and nd > case["horizon"]
    wx, _, wr = S.darts("cube_f075", F32, 0, nd)
    b = S.batched_run(wx, wr, S.max_points_of(case), case["stall_limit"], 0)
    assert np.array_equal(b["acc"], acc) and (b["n_darts"], b["stop_reason"], b["n_batches"]) == (n_darts, reason, 3)
    assert b["rounds_max"] == 7                                       # measured: one group of the library's rounds


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_cube_fine_accepts_the_darts_in_front_of_the_tile_seams(dtype):
    case, xyz, tri, r, acc, n_darts, reason = _run("cube_fine", dtype)
    assert case["max_points"] == 2849 and (len(acc), n_darts, reason) == (2849, 4096, 2)
    assert acc[1685] == 2047 and acc[2848] == 4095                  # sample 1686 is dart 2047, sample 2849 is dart 4095
    got, nd, why = S.serial(xyz, r, 1686, case["stall_limit"])
    assert np.array_equal(got, acc[:1686]) and (nd, why) == (2048, 2)
    for max_points, batch in ((1686, 2048), (1686, 2047), (1686, 4096), (2849, 4096)):
        nb, whole = S.whole_batches(2048 if max_points == 1686 else 4096, batch)
        b = S.batched_run(xyz[:whole], r[:whole], max_points, case["stall_limit"], batch)
        assert np.array_equal(b["acc"], acc[:max_points]) and b["n_batches"] == nb and b["stop_reason"] == 2
        assert b["n_darts"] == (2048 if max_points == 1686 else 4096)


@pytest.mark.parametrize("name", ["cube_max37", "cube_stall3", "one_triangle"])
def test_batches_that_end_with_the_run(name):
    case, xyz, tri, r, acc, n_darts, reason = _run(name)
    batches = [n_darts - 1, n_darts, n_darts + 1] + ([1, 7, 10, 25] if name == "one_triangle" else [])
    for batch in batches:
        nb, whole = S.whole_batches(n_darts, batch)
        assert nb == -(-n_darts // batch)
        wx, _, wr = (xyz, tri, r) if whole <= case["horizon"] else S.darts(name, F32, 0, whole)
        b = S.batched_run(wx[:whole], wr[:whole], S.max_points_of(case), case["stall_limit"], batch)
        assert np.array_equal(b["acc"], acc) and (b["n_darts"], b["stop_reason"], b["n_batches"]) == (n_darts, reason, nb)
    if name == "one_triangle":                                        # whole batches that accept nothing carry the miss run
        assert list(acc) == [0] and n_darts == 51 and S.whole_batches(51, 7)[0] == 8


def test_cube_r005_needs_more_than_one_group_of_rounds():
    case, xyz, tri, r, acc, n_darts, reason = _run("cube_r005")
    batch = case["batch"]
    assert (len(acc), n_darts, reason) == (1380, 22422, 2) and (acc < batch).sum() == 1339
    assert batch < n_darts < 2 * batch == case["horizon"]            # the run ends inside the second batch
    b = S.batched_run(xyz, r, case["max_points"], case["stall_limit"], batch)
    assert np.array_equal(b["acc"], acc) and (b["n_darts"], b["stop_reason"], b["n_batches"]) == (n_darts, reason, 2)
    assert b["rounds_max"] == 10 > 8                                  # the library runs its rounds in groups of 8


def test_edge_cell_maps():
    # a box without height; the same far from the origin in Float32
    for name in ("plate", "plate_far"):
        for dtype in S.case_dtypes(name):
            case, xyz, tri, r, acc, n_darts, reason = _run(name, dtype)
            v, _ = S.mesh_of(name, dtype)
            assert v[:, 2].min() == v[:, 2].max() == (0.0 if name == "plate" else 1000.0)
            assert np.abs(xyz[:, 2] - v[0, 2]).max() <= (0.0 if name == "plate" else 4 * np.spacing(F32(1000.0)))
            # (three products and two sums round: far from the origin a dart may leave the plane, and with it the box)
            assert name == "plate" or (xyz[:, 2] != v[0, 2]).any()
            assert (len(acc), n_darts, reason) == (469, 14960, 1) and n_darts <= case["horizon"]
    assert S.case_dtypes("plate_far") == [F32] and S.mesh_of("plate_far", F32)[0].min() == 1000.0
    # the stretched cube: the extra triangle has no area and is never picked, so the darts are cube_f075's, but the box
    # is 3e5 long and a millionth of that is more than r
    for dtype in S.DTYPES:
        case, xyz, tri, r, acc, n_darts, reason = _run("cube_stretched", dtype)
        _, xyz0, tri0, r0, acc0, nd0, why0 = _run("cube_f075", dtype)
        v, t = S.mesh_of("cube_stretched", dtype)
        cum, total = S.areas_of("cube_stretched", dtype)
        assert len(t) == 13 and cum[12] == cum[11] and total == 6.0 and not (tri == 12).any()
        assert np.array_equal(xyz, xyz0) and np.array_equal(tri, tri0) and np.array_equal(r, r0)
        assert np.array_equal(acc, acc0) and (n_darts, reason) == (nd0, why0) == (17394, 1)
        ext = float(v.max(axis=0)[0] - v.min(axis=0)[0])
        assert ext == 3e5 and ext / 1e6 > float(r[0]) == float(dtype(0.75) * dtype(0.15))


def test_darts_are_the_uniform_stream(wtp):
    """u and v of dart j are the values synth.uniform (and wtp_gen_uniform_dev) produce for point j, axes 1 and 2."""
    xyz, tri, r = S.darts("one_triangle", F64, 5, 100)
    u = wtp.synth.uniform(100, 3, F64, first=5)                       # synth.SEED: the same stream as S.SEED
    su = np.sqrt(u[:, 1])
    assert np.array_equal(xyz[:, 0], su * (1 - u[:, 2])) and np.array_equal(xyz[:, 1], su * u[:, 2])
    far = S.darts("cube_f075", F32, 2 ** 32 + 5, 8)[0]
    assert not np.array_equal(far, S.darts("cube_f075", F32, 5, 8)[0])   # 64-bit dart indices


def test_sample_surface_argument_errors_before_touching_the_gpu(wtp):
    v, t = S.mesh_of("cube_f075", F64)
    with pytest.raises(wtp.WtpArgumentError, match="factor must be positive"):
        wtp.sample_surface((v, t), 0.15, factor=0)
    with pytest.raises(wtp.WtpArgumentError, match="stall_limit must be positive"):
        wtp.sample_surface((v, t), 0.15, stall_limit=0)
    with pytest.raises(wtp.WtpArgumentError):
        wtp.sample_surface((v, t), lambda p: 0.15)                    # not a built-in law: nothing to run on the device
    with pytest.raises(wtp.WtpArgumentError):
        wtp.PointBoundary.from_mesh((v, t), 0.15, factor=-1.0)


def test_generate_shadows(wtp):
    rng = np.random.default_rng(3)
    p, n = rng.random((11, 3)), rng.random((11, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    assert np.array_equal(wtp.generate_shadows(p, n, wtp.ShadowPoints(0.1)), p - 0.1 * n)
    delta = lambda q: 0.05 + 0.1 * q[0]                               # Δ as a function of one point
    want = np.array([q - delta(q) * m for q, m in zip(p, n)])
    assert np.allclose(wtp.generate_shadows(p, n, wtp.ShadowPoints(delta, 2)), want, rtol=0, atol=1e-15)
    surf = wtp.PointSurface(p, n, np.ones(11))
    assert np.array_equal(wtp.generate_shadows(surf, wtp.ShadowPoints(0.1)), p - 0.1 * n)
    cloud = wtp.PointCloud(wtp.PointBoundary(surf), wtp.PointVolume(p + 2))
    assert np.array_equal(wtp.generate_shadows(cloud, wtp.ShadowPoints(0.1)), p - 0.1 * n)
    assert wtp.ShadowPoints(0.1).order == 1 and repr(wtp.ShadowPoints(0.1, 2)).startswith("ShadowPoints{2}")
    with pytest.raises(wtp.WtpArgumentError):
        wtp.generate_shadows(wtp.PointSurface(p), wtp.ShadowPoints(0.1))   # no normals
