"""No-GPU checks of the surface sampler's model (surface_sampling_cases.py): the batch algorithm the library runs equals
the serial dart thrower for every batch size, the cases have the properties they are there for, the reference's known
answers hold on the serial result, and the host mirror refuses bad arguments before it touches a device."""
import numpy as np
import pytest

import surface_sampling_cases as S

F32, F64 = S.F32, S.F64


def _run(name, dtype=F32):
    case = S.CASES[name]
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
