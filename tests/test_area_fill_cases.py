"""No-GPU checks of the area fill's model (area_fill_cases.py): the batch algorithm the library runs equals the serial
dart thrower for every batch size and type, with seeds, holes and darts outside the domain; the cases have the
properties they are there for; the host mirror refuses bad arguments before it touches a device."""
import numpy as np
import pytest

import area_fill_cases as A
import loops_cases as LC

F32, F64 = A.F32, A.F64
ALL = [(n, dt) for n in A.CASES for dt in A.case_dtypes(n)]


def _run(name, dtype=F32):
    return (A.CASES[name],) + A.model_run(name, dtype) + A.seeds_of(name, dtype)


@pytest.mark.parametrize("name,dtype", ALL)
def test_batches_equal_the_serial_loop(name, dtype):
    case, xy, inside, r, acc, n_darts, reason, n_in, sx, sr = _run(name, dtype)
    for batch in (63, 64, 65, 1000, 0):
        got, nd, why, nin, rounds = A.batched(xy, inside, r, sx, sr, A.max_points_of(case), case["stall_limit"], batch)
        assert np.array_equal(got, acc) and (nd, why, nin) == (n_darts, reason, n_in), batch
        assert 1 <= rounds <= (batch or 1 << 20)


# n_points, n_darts, n_inside of every case (area_fill_cases.py's comments), the same in both types
COUNTS = {"square": (476, 20590, 20590), "star": (512, 28872, 15934), "annulus": (475, 21502, 14152),
          "annulus_rev": (475, 21502, 14152), "wedge": (165, 13894, 6883), "square_far": (475, 20590, 20585),
          "circle_bl": (724, 38250, 30040), "square_max1": (1, 1, 1), "square_max37": (37, 37, 37),
          "square_stall200": (413, 3659, 3659), "square_h10": (1, 51, 51), "seed_outside": (474, 20590, 20590),
          "sliver": (86, 19236, 475)}


@pytest.mark.parametrize("name,dtype", ALL)
def test_counts_are_the_recorded_ones(name, dtype):
    _, _, _, _, acc, n_darts, reason, n_in, _, _ = _run(name, dtype)
    assert (len(acc), n_darts, n_in) == COUNTS[name]
    assert reason == (2 if "max" in name else 1)


@pytest.mark.parametrize("name,dtype", [("square", F64), ("star", F32), ("annulus", F64), ("circle_bl", F32), ("sliver", F32)])
def test_points_are_inside_and_keep_their_distance(name, dtype):
    case, xy, inside, r, acc, n_darts, reason, n_in, sx, sr = _run(name, dtype)
    assert len(acc) > 50 and inside[acc].all()
    p = np.concatenate([sx, xy[acc]]).astype(F64)
    rr = np.concatenate([sr, r[acc]]).astype(F64)
    d = np.linalg.norm(p[:, None] - p[None], axis=2) + 10 * np.eye(len(p))
    d[:len(sx), :len(sx)] = 10                                        # seeds are never tested against each other
    assert (d >= np.minimum(rr[:, None], rr[None]) * (1 - 8 * np.finfo(dtype).eps)).all()


def test_case_properties():
    _, xy, inside, r, acc, n_darts, reason, n_in, _, _ = _run("square")
    assert reason == 1 and n_in == n_darts                             # every dart of a box-shaped domain is inside
    # the reference's star item: more than 100 points, minimum pairwise distance >= 0.06 (1 - 1e-9)
    _, xs, ins_s, _, acc_s, nd_s, _, nin_s, sx, _ = _run("star", F64)
    assert len(acc_s) > 100 and len(sx) == 120 and 0.5 < nin_s / nd_s < 0.6
    p = xs[acc_s]
    d = np.linalg.norm(p[:, None] - p[None], axis=2) + 10 * np.eye(len(p))
    assert d.min() >= 0.75 * 0.08 * (1 - 1.0e-9) and d.min() < 0.0601   # 1.0002 r in the model
    # the reference's annulus item
    _, xa, _, _, acc_a, _, _, _, sxa, _ = _run("annulus", F64)
    rad = np.hypot(xa[acc_a, 0], xa[acc_a, 1])
    assert len(acc_a) > 100 and len(sxa) == 72
    assert ((0.79 < rad) & (rad < 2.001)).all() and rad.min() < 1.2 and rad.max() > 1.6
    for dt in A.DTYPES:  # the hole's orientation changes nothing: the same darts, flags and run
        a, b = A.model_run("annulus", dt), A.model_run("annulus_rev", dt)
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:]
    # the wedge's sharp corner: the flags are the even-odd rule's wherever a dart is not within rounding of the boundary
    _, xw, ins_w, _, acc_w, _, _, _, _, _ = _run("wedge", F64)
    par = np.array([LC.point_in_loop(q, LC.WEDGE) for q in xw[:2000]])
    assert np.array_equal(par, ins_w[:2000]) and 0.45 < ins_w.mean() < 0.55
    # box arithmetic far from the origin, in Float32: five darts round onto the boundary, where distance 0 is not inside
    _, xf, inf_, _, accf, ndf, _, ninf, _, _ = _run("square_far")
    assert xf.dtype == F32 and xf.min() >= 1000 and xf.max() <= 1001 and ndf - ninf == 5
    on_edge = ~inf_[:ndf]
    assert (np.isin(xf[:ndf][on_edge], (1000, 1001)).any(axis=1)).all()
    # graded r spanning about 3.5x
    _, _, _, r_bl, acc_bl, _, _, _, _, _ = _run("circle_bl")
    ra = r_bl[acc_bl]
    assert 3.0 <= ra.max() / ra.min() <= 4.0 and ra.min() >= 0.75 * 0.03
    # the stop rules
    full = acc
    for name, m in (("square_max1", 1), ("square_max37", 37)):
        _, _, _, _, a, nd, why, _, _, _ = _run(name)
        assert why == 2 and np.array_equal(a, full[:m]) and nd == a[-1] + 1
    _, _, _, _, early, nd_e, why_e, _, _, _ = _run("square_stall200")
    assert why_e == 1 and nd_e < n_darts / 5 and np.array_equal(early, full[:len(early)]) and len(early) < len(full)
    case, _, _, r10, a10, nd10, why10, _, _, _ = _run("square_h10")
    assert r10[0] > np.sqrt(2) and list(a10) == [0] and nd10 == 1 + case["stall_limit"] and why10 == 1
    # a seed outside the box still blocks
    _, xo, _, _, acc_o, _, _, _, sx, sr = _run("seed_outside")
    assert len(sx) == 1 and sx[0, 0] > 1 and not np.array_equal(acc_o, full[:len(acc_o)])
    assert np.linalg.norm(xo[acc_o].astype(F64) - sx[0].astype(F64), axis=1).min() >= float(sr[0]) * (1 - 1e-6)
    # the sliver fills 2.5 % of its box, and the run's own area estimate says so
    _, _, _, _, acc_v, nd_v, _, nin_v, _, _ = _run("sliver", F64)
    assert A.bbox_area("sliver", F64) == 1.0 and abs(nin_v / nd_v - 0.025) < 0.004 and len(acc_v) > 50


def test_darts_are_the_uniform_stream(wtp):
    """Dart j is point j of synth.uniform's dim-2 stream (and wtp_gen_uniform_dev's) scaled into the box."""
    for dt in A.DTYPES:
        u = wtp.synth.uniform(100, 2, dt, first=5)                    # synth.SEED: the same stream as A.SEED
        assert np.array_equal(A.positions("square", dt, 5, 100), u)    # the unit square's box is [0, 1]^2
    idx = A.index_of("annulus", F32)
    u = wtp.synth.uniform(100, 2, F32)
    assert np.array_equal(A.positions("annulus", F32, 0, 100), idx["lo"] + u * (idx["hi"] - idx["lo"]))
    far = A.positions("square", F32, 2 ** 32 + 5, 8)
    assert not np.array_equal(far, A.positions("square", F32, 5, 8))  # 64-bit dart indices


def test_fill_area_argument_errors_before_touching_the_gpu(wtp):
    sq = LC.square()
    with pytest.raises(wtp.WtpArgumentError, match="factor must be positive"):
        wtp.fill_area(sq, 0.05, factor=0)
    with pytest.raises(wtp.WtpArgumentError, match="stall_limit must be positive"):
        wtp.fill_area(sq, 0.05, stall_limit=0)
    with pytest.raises(wtp.WtpArgumentError, match="max_points must be positive"):
        wtp.fill_area(sq, 0.05, max_points=0)
    with pytest.raises(wtp.WtpArgumentError):
        wtp.fill_area(sq, lambda p: 0.05)                             # not a built-in law: nothing to run on the device
    with pytest.raises(wtp.WtpArgumentError, match="2D discretization supports the Orthtree fill only"):
        wtp.discretize(sq, 0.05, alg=wtp.SlakKosec())
    with pytest.raises(wtp.WtpArgumentError, match="needs its surface mesh"):
        wtp.discretize(np.zeros((4, 3)), 0.05)
