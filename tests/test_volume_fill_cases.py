"""No-GPU checks of the volume fill's model (volume_fill_cases.py): the batch algorithm the library runs equals the
serial dart thrower for every batch size, with seeds and with darts outside the domain; the cases have the properties
they are there for; the host mirror refuses bad arguments before it touches a device."""
import numpy as np
import pytest

import volume_fill_cases as V

F32, F64 = V.F32, V.F64


def _run(name, dtype=F32):
    case = V.case_of(name)
    return (case,) + V.model_run(name, dtype) + V.seeds_of(name, dtype)


def _batched_equals_serial(name, batch, dtype=F32):
    case, xyz, inside, r, acc, n_darts, reason, n_in, sx, sr = _run(name, dtype)
    got, nd, why, nin, rounds = V.batched(xyz, inside, r, sx, sr, V.max_points_of(case), case["stall_limit"], batch)
    assert np.array_equal(got, acc) and (nd, why, nin) == (n_darts, reason, n_in)
    return rounds


@pytest.mark.parametrize("batch", [63, 64, 65, 1000, 4096])
@pytest.mark.parametrize("name", ["cube_stall200", "cube_seeds"])
def test_batches_equal_the_serial_loop_with_and_without_seeds(name, batch):
    rounds = _batched_equals_serial(name, batch)
    assert 1 <= rounds <= batch
    if batch == 4096:
        assert rounds >= 5                                            # the case really exercises chains of decisions


@pytest.mark.parametrize("name", ["cube_max1", "cube_max37", "cube_const10", "flat"])
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 1000, 4096])
def test_batches_equal_the_serial_loop_at_the_stop_rules(name, batch):
    _batched_equals_serial(name, batch)                                # (batch 1: cases of at most 40 points)


@pytest.mark.parametrize("name", ["cube", "cube_bl", "cube_far", "slab_seeded", "cube_seed_outside", "cavity", "box_stall200"])
def test_batches_equal_the_serial_loop_on_every_other_case(name):
    _batched_equals_serial(name, 4096)


def test_a_smaller_max_points_gives_a_prefix():
    full = _run("cube")[4]
    for name, m in (("cube_max1", 1), ("cube_max37", 37)):
        _, _, _, _, acc, n_darts, reason, n_in, _, _ = _run(name)
        assert reason == 2 and len(acc) == m and np.array_equal(acc, full[:m])
        assert n_darts == acc[-1] + 1 and n_in == n_darts


@pytest.mark.parametrize("name,dtype", [("cube", F32), ("cube", F64), ("cube_seeds", F64), ("cube_bl", F32), ("cavity", F32)])
def test_points_are_inside_and_keep_their_distance(name, dtype):
    case, xyz, inside, r, acc, n_darts, reason, n_in, sx, sr = _run(name, dtype)
    assert len(acc) > 50 and inside[acc].all()
    p = np.concatenate([sx, xyz[acc]]).astype(F64)
    rr = np.concatenate([sr, r[acc]]).astype(F64)
    d = np.linalg.norm(p[:, None] - p[None], axis=2) + 10 * np.eye(len(p))
    d[:len(sx), :len(sx)] = 10                                        # seeds are never tested against each other
    assert (d >= np.minimum(rr[:, None], rr[None]) * (1 - 8 * np.finfo(dtype).eps)).all()


def test_case_properties():
    _, xyz, inside, r, acc, n_darts, reason, n_in, _, _ = _run("cube")
    assert reason == 1 and 400 <= len(acc) <= 700 and n_in == n_darts          # every dart of a box-shaped domain is inside
    _, _, _, _, early, nd_early, _, _, _, _ = _run("cube_stall200")
    assert nd_early < n_darts / 5 and np.array_equal(early, acc[:len(early)]) and len(early) < len(acc)
    # seeds block but are not tested: some are in mutual conflict, all are kept, and the fill loses its outer layer
    _, xs, _, rs, acc_s, _, _, _, sx, sr = _run("cube_seeds")
    assert len(sx) == 384
    d = np.linalg.norm(sx[:, None].astype(F64) - sx[None].astype(F64), axis=2) + 10 * np.eye(len(sx))
    assert (d < sr[0]).any() and len(acc_s) < 0.6 * len(acc)
    assert np.minimum(xs[acc_s], 1 - xs[acc_s]).min() >= 0.0695       # sqrt(r^2 - 0.125^2 / 2) = 0.0696: no point hugs a face
    # graded r spanning about 2.6x: a large ball touches many cells of edge sqrt(r_min r_max)
    _, _, _, r_bl, acc_bl, _, _, _, _, _ = _run("cube_bl")
    ra = r_bl[acc_bl]
    assert 2.4 <= ra.max() / ra.min() <= 4.0 and ra.min() > 0.04
    # one point, then stall_limit misses
    case, _, _, r10, acc10, nd10, why10, _, _, _ = _run("cube_const10")
    assert r10[0] > np.sqrt(3) and list(acc10) == [0] and nd10 == 1 + case["stall_limit"] and why10 == 1
    # box arithmetic and cells far from the origin, in Float32
    _, xf, inf, _, accf, _, _, nin_f, _, _ = _run("cube_far")
    assert xf.dtype == F32 and xf.min() >= 1000 and xf.max() <= 1001 and nin_f == inf[:36200].sum() < 36200
    # nothing fits between the seeded faces of the slab; nothing is inside a surface without volume
    case, _, ins, r_sl, acc_sl, nd, why, nin, sx, _ = _run("slab_seeded")
    assert len(acc_sl) == 0 and (nd, why) == (case["stall_limit"], 1) and nin == nd and r_sl[0] > 0.05 and len(sx) == 200
    case, xfl, ins, _, acc_fl, nd, why, nin, _, _ = _run("flat")
    assert len(acc_fl) == 0 and (nd, why, nin) == (case["stall_limit"], 1, 0) and (xfl[:, 2] == 2.0 ** 24).all()
    for dt in V.DTYPES:
        lo, hi = V.box_of("flat", dt)
        assert lo[2] == hi[2] and V.bbox_volume("flat", dt) == 0.0
    # a seed outside the box still blocks: the run differs from the plain one and nothing is within r of the seed
    _, xo, _, ro, acc_o, _, _, _, sx, sr = _run("cube_seed_outside")
    assert len(sx) == 1 and sx[0, 0] > 1 and not np.array_equal(acc_o, acc[:len(acc_o)])
    assert np.linalg.norm(xo[acc_o].astype(F64) - sx[0].astype(F64), axis=1).min() >= float(sr[0]) * (1 - 1e-6)
    # part of the cavity's box is empty: the run's own volume estimate is well below the box
    _, _, ins_c, _, acc_c, nd_c, _, nin_c, _, _ = _run("cavity")
    assert 300 <= len(acc_c) <= 3000 and 0.3 < nin_c / nd_c < 0.6 and V.bbox_volume("cavity", F32) == 8.0
    _, _, _, _, acc_b, nd_b, why_b, nin_b, _, _ = _run("box_stall200")
    assert 300 <= len(acc_b) <= 3000 and why_b == 1 and nin_b == nd_b
    est = V.bbox_volume("box_stall200", F32) * nin_b / nd_b
    assert abs(est - 15625.0) <= 1e-3 * 15625.0                         # the box mesh fills its bounding box


# ---- the edge cases of test_gpu_sampler_edges.py: the numbers its runs rely on -------------------------------------------
@pytest.mark.parametrize("dtype", V.DTYPES)
def test_needle_runs_end_beyond_the_256th_tile_of_the_stop_scan(dtype):
    v, t = V.mesh_of("needle", dtype)
    lo, hi = V.box_of("needle", dtype)
    assert (lo == 0).all() and (hi == 1).all() and len(t) == 4       # the bounding box is the unit cube
    vol = sum(np.linalg.det(v.astype(F64)[tri]) for tri in t) / 6
    assert abs(vol - 0.12 * 0.12 / 6) <= 1e-9                           # positive: the inside is inside
    xyz, inside, r = V.needle_darts(dtype)
    assert xyz.dtype == dtype and len(xyz) == 3 << 20
    assert inside[:1 << 20].sum() == 2496 and inside.sum() == 7492      # 0.24 % of the darts
    # max_points = 618: tile 340 of a batch of 2^20 darts
    case, mx, mi, mr, acc, n_darts, reason, n_in, sx, sr = _run("needle", dtype)
    assert len(mx) == 1 << 20 and np.array_equal(mx, xyz[:1 << 20]) and len(sx) == 0
    assert (len(acc), n_darts, reason, n_in) == (618, 697597, 2, 1677) and n_darts // 2048 == 340
    # stall_limit = 8929, one more than the longest miss run in front of the tile behind the carry: tile 273
    case, _, _, _, acc_s, nd_s, why_s, nin_s, _, _ = _run("needle_stall", dtype)
    assert (len(acc_s), nd_s, why_s, nin_s) == (571, 560383, 1, 1355) and nd_s // 2048 == 273
    miss = np.diff(np.concatenate([[-1], acc_s])) - 1
    assert miss.max() == 8928 == case["stall_limit"] - 1 and (acc_s < 528384).sum() == 557
    assert min(n_darts, nd_s) >= V.SCAN_CARRY_FROM == 526336            # both stops need the scan's carry
    # batch = 0: the run ends in a batch of 2^20 darts, the tenth
    case, cx, ci, cr, acc_c, nd_c, why_c, nin_c, _, _ = _run("needle_clamp", dtype)
    assert len(cx) == 3 << 20 and (len(acc_c), nd_c, why_c, nin_c) == (900, 2594928, 2, 6135)
    assert nd_c > V.CLAMPED_FROM == 2093056 and V.whole_batches(nd_c, 0) == (10, V.CLAMPED_FROM + 2 ** 20)
    assert np.array_equal(acc_c[:618], acc) and np.array_equal(acc_c[:571], acc_s)


def test_needle_in_one_batch_equals_the_serial_loop():
    for name in ("needle", "needle_stall"):
        case, xyz, inside, r, acc, n_darts, reason, n_in, sx, sr = _run(name)
        b = V.batched_run(xyz, inside, r, sx, sr, V.max_points_of(case), case["stall_limit"], 1 << 20)
        assert np.array_equal(b["acc"], acc) and (b["n_darts"], b["stop_reason"], b["n_inside"]) == (n_darts, reason, n_in)
        assert b["n_batches"] == 1


@pytest.mark.parametrize("name", ["cube_stall200", "cube_const10"])
def test_batches_that_end_with_the_run(name):
    case, xyz, inside, r, acc, n_darts, reason, n_in, sx, sr = _run(name)
    for batch in (n_darts - 1, n_darts, n_darts + 1):
        nb, whole = V.whole_batches(n_darts, batch)
        assert nb == -(-n_darts // batch)
        if whole > case["horizon"]:
            xyz, inside, r = V.darts(name, F32, 0, whole)
        b = V.batched_run(xyz[:whole], inside[:whole], r[:whole], sx, sr, V.max_points_of(case), case["stall_limit"], batch)
        assert np.array_equal(b["acc"], acc) and b["n_batches"] == nb
        assert (b["n_darts"], b["stop_reason"], b["n_inside"]) == (n_darts, reason, n_in)


def test_darts_are_the_uniform_stream(wtp):
    """Dart j is point j of synth.uniform (and wtp_gen_uniform_dev) scaled into the box."""
    for dt in V.DTYPES:
        u = wtp.synth.uniform(100, 3, dt, first=5)                    # synth.SEED: the same stream as V.SEED
        assert np.array_equal(V.positions("cube", dt, 5, 100), u)       # the unit cube's box is [0, 1]^3
    lo, hi = V.box_of("cavity", F32)
    u = wtp.synth.uniform(100, 3, F32)
    assert np.array_equal(V.positions("cavity", F32, 0, 100), lo + u * (hi - lo))
    far = V.positions("cube", F32, 2 ** 32 + 5, 8)
    assert not np.array_equal(far, V.positions("cube", F32, 5, 8))    # 64-bit dart indices


def test_fill_volume_argument_errors_before_touching_the_gpu(wtp):
    v, t = V.mesh_of("cube", F64)
    with pytest.raises(wtp.WtpArgumentError, match="factor must be positive"):
        wtp.fill_volume((v, t), 0.15, factor=0)
    with pytest.raises(wtp.WtpArgumentError, match="stall_limit must be positive"):
        wtp.fill_volume((v, t), 0.15, stall_limit=0)
    with pytest.raises(wtp.WtpArgumentError, match="max_points must be positive"):
        wtp.discretize(np.zeros((1, 3)), 0.15, (v, t), max_points=0)
    with pytest.raises(wtp.WtpArgumentError):
        wtp.fill_volume((v, t), lambda p: 0.15)                       # not a built-in law: nothing to run on the device
    with pytest.raises(wtp.WtpArgumentError, match="inside-out"):
        wtp.fill_volume((v, t[:, ::-1].copy()), 0.15)                 # the orientation guards stay on: no inside to fill
    from whatsthepoint_jl_amd import _lib as L
    import ctypes

    assert ctypes.sizeof(L.FillInfo) == 80                            # five int64, four int32, three doubles
