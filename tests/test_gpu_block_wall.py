"""The block driver with a boundary wall (wtp_block_set_wall; csrc/wtp_block.hip) and the global closest pair.

The reference's volume-only repel pushes the volume points off a fixed wall: snapshot [boundary ; volume] with
n_fixed = n_boundary (src/repel.jl:75-87).  A block session holds the whole wall on every rank and keeps the part
inside its coverage box at the head of its snapshot.  What one GPU can show: (a) one rank with a wall IS the plain
session [wall ; x] (positions, max |F| and the closest pair bit for bit; the sums to the last bits, which the plain
session itself does not reproduce); (b) 2 x 2 x 2 and 4 ranks as threads on the one GPU, rows
carried by a loopback transport, reproduce the single-domain run with the same wall, also when the ghost layer is
widened (the wall is selected again); (c) the closest pair is reported in the numbering of the assembled snapshot on
every rank, across a face and against a wall point; (d) a graded cloud with BoundaryLayerSpacing of the wall; (e) the
stop rules, every exit of wtp_block_run_until against the plain session's; (f) the entry point's argument and state
checks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORCE = dict(kind=2, beta=0.2, u0=1.0, gamma=3.0)
K = 21
STATS = ("max_force", "sum_u", "sum_u2", "n_move", "argmin_i", "argmin_j", "argmin_r")


def _face_wall(m):
    """m x m cell-centred grids on the six faces of the unit cube (spacing 1/m, no point shared by two faces)."""
    g = (np.arange(m, dtype=np.float64) + 0.5) / m
    u, v = np.meshgrid(g, g, indexing="ij")
    faces = []
    for a in range(3):
        for c in (0.0, 1.0):
            f = np.empty((u.size, 3), dtype=np.float32)
            f[:, a] = c
            f[:, (a + 1) % 3] = u.ravel()
            f[:, (a + 2) % 3] = v.ravel()
            faces.append(f)
    return np.concatenate(faces)


def _single_domain(wtp, x, wall, spacing, iters, alpha):
    """Plain session on [wall ; x] with the wall as fixed head: (per-step stats, positions of x)."""
    snap = np.ascontiguousarray(np.vstack([wall, x]).astype(np.float32))
    with wtp.Context(0) as c:
        with c.relax(snap, len(wall), spacing, FORCE, K, alpha / 100, alpha) as sess:
            hist = [sess.step(True) for _ in range(iters)]
            return hist, sess.positions()


def _run_blocks(wtp, x, boxes, spacing, iters, alpha, w, margin, wall, body=None):
    """Every rank a thread with its own context on the one GPU; returns (positions in gid order, histories)."""
    import torch
    from whatsthepoint_jl_amd import blockc

    n = len(x)
    own = blockc.owner_of(x, boxes)
    nranks = len(boxes)

    def worker(rank, hub):
        torch.cuda.set_device(0)
        ctx = wtp.Context(0)
        try:
            idx = np.nonzero(own == rank)[0]
            drv = blockc.BlockRelax(ctx, rank, nranks, boxes, x[idx], idx.astype(np.int64), w, spacing, FORCE, K, alpha / 100,
                                    alpha, margin=margin, transport=blockc.loopback_transport(hub, rank), wall_xyz=wall)
            hist = body(drv) if body else [drv.step() for _ in range(iters)]
            xyz, gid = drv.owned()
            out = (xyz.cpu().numpy(), gid.cpu().numpy(), hist)
            drv.close()
            return out
        finally:
            ctx.close()

    res = blockc.run_threads(nranks, worker)
    p = np.full((n, 3), np.nan, dtype=np.float32)
    seen = np.zeros(n, dtype=np.int64)
    for xyz, gid, _ in res:
        p[gid] = xyz
        seen[gid] += 1
    assert (seen == 1).all(), "every volume point is owned by exactly one rank (wall points are never returned)"
    return p, [r[2] for r in res]


def _same_on_every_rank(hists):
    for i in range(len(hists[0])):
        for f in STATS:
            assert len({hh[i][f] for hh in hists}) == 1, (i, f, [hh[i][f] for hh in hists])


def test_one_rank_with_a_wall_is_the_plain_session(wtp):
    from whatsthepoint_jl_amd import blockc

    n, iters = 300_000, 5
    x = wtp.synth.uniform(n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    wall = _face_wall(int(round(1.0 / s)))
    ref, p0 = _single_domain(wtp, x, wall, s, iters, s / 20)
    boxes = blockc.orthtree_boxes(None, 1, equal_count=False)
    with wtp.Context(0) as ctx:
        drv = blockc.BlockRelax(ctx, 0, 1, boxes, x, None, 2.0 * s, s, FORCE, K, s / 2000, s / 20, wall_xyz=wall)
        hist = [drv.step() for _ in range(iters)]
        xyz, gid = drv.owned()
        drv.close()
    assert np.array_equal(gid.cpu().numpy(), np.arange(n)), "wall points are not owned points"
    assert np.array_equal(xyz.cpu().numpy(), p0), "a one-rank block run with a wall equals the plain session bit for bit"
    for i in range(iters):
        for f in ("max_force", "n_move", "argmin_i", "argmin_j", "argmin_r"):
            assert hist[i][f] == ref[i][f], (i, f, hist[i][f], ref[i][f])
        # (the sums are not reproducible in the last bit from one plain run to the next either: queries that leave the
        # fast path are summed in the order an atomic counter lists them)
        for f in ("sum_u", "sum_u2"):
            assert hist[i][f] == pytest.approx(ref[i][f], rel=1e-13, abs=0), (i, f, hist[i][f], ref[i][f])
    assert hist[0]["argmin_i"] >= len(wall), "the closest pair's query is a volume point: n_wall + gid"
    assert all(h["host_syncs"] == 1 for h in hist[1:]), [h["host_syncs"] for h in hist]
    assert all(h["n_ghost"] == 0 and h["n_move"] == n for h in hist)


def test_octants_with_a_wall_match_single_domain(wtp):
    """2 x 2 x 2, margin 0: the wall on the cube faces is cut between the octants like the cloud."""
    from whatsthepoint_jl_amd import blockc

    n, iters = 240_000, 6
    x = wtp.synth.uniform(n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    wall = _face_wall(int(round(1.0 / s)))
    ref, p0 = _single_domain(wtp, x, wall, s, iters, s / 20)
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False)
    p, hists = _run_blocks(wtp, x, boxes, s, iters, s / 20, w=2.2 * s, margin=0.0, wall=wall)
    err = np.abs(p - p0).max() / s
    assert err <= 2e-5, f"block run with a wall differs from the single-domain run by {err} spacings"
    assert all(h[-1]["n_peers"] == 7 for h in hists)
    assert sum(h["n_emigrated"] for hh in hists for h in hh) > 0, "margin 0: somebody crossed a face"
    assert all(h["n_uncovered"] == 0 for hh in hists for h in hh)
    _same_on_every_rank(hists)
    for i in range(iters):
        assert hists[0][i]["n_move"] == n
    # the first step sweeps the same snapshot as the single domain: the same pair, in the same numbering
    assert (hists[0][0]["argmin_i"], hists[0][0]["argmin_j"]) == (ref[0]["argmin_i"], ref[0]["argmin_j"])
    assert hists[0][0]["argmin_r"] == pytest.approx(ref[0]["argmin_r"], rel=1e-6)
    # the wall is felt: without it the points near the faces end elsewhere
    p_free, _ = _run_blocks(wtp, x, boxes, s, iters, s / 20, w=2.2 * s, margin=0.0, wall=None)
    near = np.minimum(x, 1.0 - x).min(axis=1) < s
    assert np.abs(p_free[near] - p0[near]).max() / s > 1e-2, "the wall made no difference near the faces"


def test_thin_ghost_layer_with_a_wall_is_widened_and_the_wall_selected_again(wtp):
    from whatsthepoint_jl_amd import blockc

    n, iters = 120_000, 3
    x = wtp.synth.uniform(n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    wall = _face_wall(int(round(1.0 / s)))
    _, p0 = _single_domain(wtp, x, wall, s, iters, s / 20)
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False)
    p, hists = _run_blocks(wtp, x, boxes, s, iters, s / 20, w=0.5 * s, margin=0.05 * s, wall=wall)
    assert all(h[0]["redone"] == 1 and h[-1]["widened"] >= 1 for h in hists)
    err = np.abs(p - p0).max() / s
    assert err <= 2e-5, f"widened block run with a wall differs from the single-domain run by {err} spacings"
    _same_on_every_rank(hists)


def _knn1(wtp, pts, queries):
    """Distance from every query row to its nearest other point of pts."""
    with wtp.Context(0) as c:
        _, d = c.knn(pts, 1, include_self=False, return_dist=True)
    return d[queries, 0]


def test_global_closest_pair_across_a_face_and_against_the_wall(wtp):
    from whatsthepoint_jl_amd import blockc

    n = 240_000
    s = float(n) ** (-1.0 / 3.0)
    wall = _face_wall(int(round(1.0 / s)))
    nw = len(wall)
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False)
    gap = np.float32(1e-3 * s)

    # (a) two volume points on either side of the face x = 0.5 (octants 0 and 1 on the x axis)
    x = wtp.synth.uniform(n, 3, np.float32)
    ga, gb = 1234, 98765
    x[ga] = (np.float32(0.5) - np.float32(gap / 2), 0.3, 0.3)
    x[gb] = (np.float32(0.5) + np.float32(gap / 2), 0.3, 0.3)
    own = blockc.owner_of(x, boxes)
    assert own[ga] != own[gb], "the planted pair straddles a face"
    snap = np.vstack([wall, x])
    d1 = _knn1(wtp, snap, np.arange(nw, nw + n))
    r_pair = float(x[gb, 0] - x[ga, 0])
    others = np.delete(d1, [ga, gb])
    assert others.min() > 2 * r_pair, "no other pair comes near the planted one"
    ref, _ = _single_domain(wtp, x, wall, s, 1, s / 20)
    assert (ref[0]["argmin_i"], ref[0]["argmin_j"]) == (nw + ga, nw + gb)
    _, hists = _run_blocks(wtp, x, boxes, s, 1, s / 20, w=2.2 * s, margin=0.0, wall=wall)
    for hh in hists:
        assert (hh[0]["argmin_i"], hh[0]["argmin_j"]) == (nw + ga, nw + gb)
        assert hh[0]["argmin_r"] == pytest.approx(ref[0]["argmin_r"], rel=1e-6)

    # (b) a volume point next to a wall point of the face y = 1
    x = wtp.synth.uniform(n, 3, np.float32)
    kw = int(np.nonzero((wall[:, 1] == 1.0) & (np.abs(wall[:, 0] - 0.3) < 0.6 * s) & (np.abs(wall[:, 2] - 0.7) < 0.6 * s))[0][0])
    gv = 4321
    x[gv] = wall[kw]
    x[gv, 1] = np.float32(1.0) - gap
    snap = np.vstack([wall, x])
    d1 = _knn1(wtp, snap, np.arange(nw, nw + n))
    assert np.delete(d1, [gv]).min() > 2 * float(np.float32(1.0) - x[gv, 1])
    ref, _ = _single_domain(wtp, x, wall, s, 1, s / 20)
    assert (ref[0]["argmin_i"], ref[0]["argmin_j"]) == (nw + gv, kw)
    _, hists = _run_blocks(wtp, x, boxes, s, 1, s / 20, w=2.2 * s, margin=0.0, wall=wall)
    for hh in hists:
        assert (hh[0]["argmin_i"], hh[0]["argmin_j"]) == (nw + gv, kw)
        assert hh[0]["argmin_r"] == pytest.approx(ref[0]["argmin_r"], rel=1e-6)


def test_graded_cloud_with_the_wall_as_the_boundary_layer_law(wtp):
    """BoundaryLayerSpacing whose boundary is the wall itself, evaluated on the device; count-median boxes."""
    from whatsthepoint_jl_amd import blockc

    n, iters = 150_000, 4
    x = wtp.synth.graded(n, 4.0, 0.2, np.float32)
    shell = (np.minimum(x, 1 - x).min(axis=1) < 0.02).sum()  # wall spacing from the density in the outer 2 % shell
    hw = float(((1 - 0.96 ** 3) / shell) ** (1 / 3))
    wall = _face_wall(int(round(1.0 / hw)))
    law = dict(kind=3, p0=hw, p1=4.0 * hw, p2=0.2, boundary=wall)
    alpha = hw / 20
    _, p0 = _single_domain(wtp, x, wall, law, iters, alpha)
    boxes = blockc.orthtree_boxes(x, 4, equal_count=True)
    p, hists = _run_blocks(wtp, x, boxes, law, iters, alpha, w=1.05 * 4.0 * hw, margin=0.1 * hw, wall=wall)
    err = np.abs(p - p0).max() / hw
    assert err <= 5e-5, f"graded block run with a wall differs from the single-domain run by {err} wall spacings"
    _same_on_every_rank(hists)


def _cv(st):
    mu = st["sum_u"] / st["n_move"]
    return float(np.sqrt(max(st["sum_u2"] / st["n_move"] - mu * mu, 0.0)) / mu)


def test_stop_rules_with_a_wall(wtp):
    from whatsthepoint_jl_amd import blockc

    n = 120_000
    x = wtp.synth.uniform(n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    wall = _face_wall(int(round(1.0 / s)))
    snap = np.ascontiguousarray(np.vstack([wall, x]))
    ref, _ = _single_domain(wtp, x, wall, s, 12, s / 20)
    cvs = [_cv(st) for st in ref]
    # a target crossed between two sweeps with room on both sides
    i = next(j for j in range(3, len(cvs) - 1) if cvs[j + 1] < min(cvs[: j + 1]) * (1 - 1e-3))
    cv_target = 0.5 * (cvs[i + 1] + min(cvs[: i + 1]))
    boxes = blockc.orthtree_boxes(None, 4, equal_count=False)
    for tol, cv_t, max_iters in ((0.0, 0.0, 5), (0.0, cv_target, 12)):
        with wtp.Context(0) as c, c.relax(snap, len(wall), s, FORCE, K, s / 2000, s / 20) as sess:
            conv0, why0, _ = sess.run_until(max_iters, 1, tol, 0, cv_t)
            p0 = sess.positions()
        why0 = ("max_iters", "tol", "cv_target", "stall")[why0]
        p, res = _run_blocks(wtp, x, boxes, s, 0, s / 20, w=2.2 * s, margin=0.1 * s, wall=wall,
                             body=lambda drv: drv.run_until(max_iters, tol, 0, cv_t))
        for conv, why, _ in res:
            assert why == why0 and len(conv) == len(conv0), (why, len(conv), why0, len(conv0))
            assert np.allclose(conv, conv0, rtol=1e-5)
        assert np.abs(p - p0).max() / s <= 2e-5
    assert why0 == "cv_target" and len(conv0) == i + 2


def _stall_walk(cvs, stall_after):
    """The stall rule (src/repel.jl:318-329) restated on a list of CVs: (the sweep, from 1, at which it fires or None,
    the improvements it saw before, the smallest |cv / (best (1 - 1e-3)) - 1| it met)."""
    best, last_impr, n_impr, margin = np.inf, 0, 0, np.inf
    for i, cv in enumerate(cvs, 1):
        margin = min(margin, abs(cv / (best * (1 - 1e-3)) - 1.0))
        if cv < best * (1 - 1e-3):
            best, last_impr, n_impr = cv, i, n_impr + 1
        elif i - last_impr >= stall_after:
            return i, n_impr, margin
    return None, n_impr, margin


_STOP_SWEEPS = 40
_STALL_AFTER = 2


def _plain_steps(wtp, x, s, alpha):
    with wtp.Context(0) as c, c.relax(x, 0, s, FORCE, K, alpha / 100, alpha) as sess:
        return [sess.step(True) for _ in range(_STOP_SWEEPS)]


def _stalling_step_limit(wtp, x, s):
    """A step limit at which the plain session's own trajectory improves several times and then stalls before sweep 40.

    This selects the INPUT, from the plain session's sweeps alone.  At the file's usual limit (s / 20), and at every
    limit from s down to s / 200, the CV of a uniform cloud of these sizes still falls by about 1 % per sweep at sweep
    40, ten times the 0.1 % the stall rule asks for: the rule cannot fire within 40 sweeps.  Below s / 400 the gain per
    sweep is proportional to the limit and decays slowly (0.147 % per sweep at s / 1200 for 30 000 points).  Where it
    starts just above 0.05 %, every second sweep is an improvement until the gain of two sweeps drops below 0.1 %:
    then two sweeps in a row bring none and stall_after = 2 fires.  Larger limits never stall, smaller ones stall at
    sweep 3 after the one improvement from +inf, so the limit is bisected for a stall between sweeps 12 and 36."""
    lo, hi = 1500.0, 6000.0
    for _ in range(14):
        div = 0.5 * (lo + hi)
        ref = _plain_steps(wtp, x, s, s / div)
        at, n_impr, margin = _stall_walk([_cv(st) for st in ref], _STALL_AFTER)
        if at is None or at > 36:
            lo = div
        elif at < 12:
            hi = div
        elif margin < 1e-7:  # too close to the threshold for a fair input (see _assert_clear_of_the_stall_threshold)
            hi = div * (1 - 1e-4)
        else:
            assert n_impr >= 4, (div, at, n_impr)
            return s / div, ref
    raise AssertionError(f"no step limit between s / {hi:.0f} and s / {lo:.0f} stalls between sweeps 12 and 36: choose another input")


def _assert_clear_of_the_stall_threshold(cvs):
    """Guards the INPUT, not the code: sum_u / sum_u2 are reproducible only to their last bits from run to run, so a
    trajectory is a fair one for the stall rule only if no sweep's CV sits within 1e-9 (relative) of the improvement
    threshold best * (1 - 1e-3), where a last-bit difference could flip the rule's verdict."""
    at, _, margin = _stall_walk(cvs, _STOP_SWEEPS + 1)  # (never fires: the whole list is walked)
    assert at is None and margin > 1e-9, margin


@pytest.fixture(scope="module")
def one_rank_trajectory(wtp):
    """30 000 uniform points, no wall: (x, s, step limit, per-sweep conv, per-sweep cv) of 40 plain-session sweeps."""
    n = 30_000
    x = wtp.synth.uniform(n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    alpha, ref = _stalling_step_limit(wtp, x, s)
    return x, s, alpha, [st["max_force"] for st in ref], [_cv(st) for st in ref]


def _plain_and_one_rank_block(wtp, x, s, alpha, tol, stall_after):
    """The same run_until on the plain session and on a one-rank block session (which IS the plain session)."""
    from whatsthepoint_jl_amd import blockc

    with wtp.Context(0) as c, c.relax(x, 0, s, FORCE, K, alpha / 100, alpha) as sess:
        conv0, why0, _ = sess.run_until(_STOP_SWEEPS, 1, tol, stall_after, 0.0)
    boxes = blockc.orthtree_boxes(None, 1, equal_count=False)
    with wtp.Context(0) as ctx:
        drv = blockc.BlockRelax(ctx, 0, 1, boxes, x, None, 2.0 * s, s, FORCE, K, alpha / 100, alpha)
        conv, why, _ = drv.run_until(_STOP_SWEEPS, tol, stall_after, 0.0)
        drv.close()
    return np.asarray(conv0), ("max_iters", "tol", "cv_target", "stall")[why0], np.asarray(conv), why


def test_block_run_until_tol_exit_is_the_plain_sessions(wtp, one_rank_trajectory):
    x, s, alpha, conv_ref, _ = one_rank_trajectory
    # a tolerance crossed between two consecutive sweeps after the fifth, with room on both sides
    j = next(j for j in range(5, _STOP_SWEEPS - 1) if conv_ref[j + 1] < conv_ref[j] == min(conv_ref[: j + 1]))
    tol = float(np.sqrt(conv_ref[j] * conv_ref[j + 1]))
    conv0, why0, conv, why = _plain_and_one_rank_block(wtp, x, s, alpha, tol, 0)
    print(f"tol exit: tol = {tol:.6e} between sweeps {j + 1} and {j + 2}; plain {why0} after {len(conv0)}, block {why} after {len(conv)}")
    assert why0 == "tol" and why == "tol", (why0, why)
    assert len(conv0) == len(conv) == j + 2, (len(conv0), len(conv), j + 2)
    assert np.array_equal(conv0, conv), "a one-rank block session is the plain session bit for bit in max |F|"


def test_block_run_until_stall_exit_is_the_plain_sessions(wtp, one_rank_trajectory):
    x, s, alpha, _, cvs = one_rank_trajectory
    _assert_clear_of_the_stall_threshold(cvs)
    at, n_impr, margin = _stall_walk(cvs, _STALL_AFTER)
    conv0, why0, conv, why = _plain_and_one_rank_block(wtp, x, s, alpha, 0.0, _STALL_AFTER)
    print(f"stall exit: step limit s / {s / alpha:.1f}, restated rule fires at sweep {at} after {n_impr} improvements "
          f"(margin {margin:.2e}); plain {why0} after {len(conv0)}, block {why} after {len(conv)}")
    assert why0 == "stall" and why == "stall", (why0, why)
    assert len(conv0) == len(conv) == at, (len(conv0), len(conv), at)
    assert np.array_equal(conv0, conv), "a one-rank block session is the plain session bit for bit in max |F|"


def test_block_run_until_stall_exit_on_four_ranks(wtp):
    """2 x 2 ranks as threads over the loopback transport: every rank stops at the sweep the restated rule names on the
    four-rank run's own (gathered, rank-ordered) CVs."""
    from whatsthepoint_jl_amd import blockc

    n = 60_000
    x = wtp.synth.uniform(n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    alpha, ref = _stalling_step_limit(wtp, x, s)
    boxes = blockc.orthtree_boxes(None, 4, equal_count=False)
    _, hists = _run_blocks(wtp, x, boxes, s, _STOP_SWEEPS, alpha, w=2.2 * s, margin=0.1 * s, wall=None)
    _same_on_every_rank(hists)
    cvs = [_cv(st) for st in hists[0]]
    _assert_clear_of_the_stall_threshold(cvs)
    at, n_impr, margin = _stall_walk(cvs, _STALL_AFTER)
    assert at is not None and at < _STOP_SWEEPS and n_impr >= 4, ("the four-rank trajectory does not stall: choose another input", at, n_impr)
    _, res = _run_blocks(wtp, x, boxes, s, 0, alpha, w=2.2 * s, margin=0.1 * s, wall=None,
                         body=lambda drv: drv.run_until(_STOP_SWEEPS, 0.0, _STALL_AFTER, 0.0))
    print(f"four ranks: step limit s / {s / alpha:.1f}, restated rule fires at sweep {at} after {n_impr} improvements "
          f"(margin {margin:.2e}); ranks stop {[(why, len(conv)) for conv, why, _ in res]}")
    for conv, why, _ in res:
        assert why == "stall" and len(conv) == at, (why, len(conv), at)
        assert np.allclose(conv, [st["max_force"] for st in ref[:at]], rtol=1e-5)


def test_set_wall_arguments_and_state(wtp):
    import torch
    from whatsthepoint_jl_amd import _lib as L
    from whatsthepoint_jl_amd import blockc

    n, iters = 50_000, 3
    x = wtp.synth.uniform(n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    wall = _face_wall(int(round(1.0 / s)))
    boxes = blockc.orthtree_boxes(None, 1, equal_count=False)
    with wtp.Context(0) as ctx:
        lib, h = ctx._lib, ctx._h
        d_wall = torch.from_numpy(wall).cuda()
        torch.cuda.synchronize()
        assert lib.wtp_block_set_wall(h, C.c_void_p(d_wall.data_ptr()), -1) == L.WTP_ERR_ARG
        assert lib.wtp_block_set_wall(h, None, 5) == L.WTP_ERR_ARG
        assert lib.wtp_block_set_wall(None, None, 0) == L.WTP_ERR_ARG
        drv = blockc.BlockRelax(ctx, 0, 1, boxes, x, None, 2.0 * s, s, FORCE, K, s / 2000, s / 20, wall_xyz=wall)
        drv.step()
        assert lib.wtp_block_set_wall(h, C.c_void_p(d_wall.data_ptr()), len(wall)) == L.WTP_ERR_STATE
        assert lib.wtp_block_set_wall(h, None, 0) == L.WTP_ERR_STATE
        drv.close()

        def run(wall_arg=None):
            d = blockc.BlockRelax(ctx, 0, 1, boxes, x, None, 2.0 * s, s, FORCE, K, s / 2000, s / 20, wall_xyz=wall_arg)
            hist = [d.step() for _ in range(iters)]
            p = d.owned()[0].cpu().numpy()
            d.close()
            return hist, p

        # set by hand: the next open takes it; cleared (n_wall = 0): the next open is the wall-less session
        assert lib.wtp_block_set_wall(h, C.c_void_p(d_wall.data_ptr()), len(wall)) == L.WTP_OK
        hw_, pw = run()
        assert lib.wtp_block_set_wall(h, None, 0) == L.WTP_OK
        h0, p_free = run()
        # an open that fails after BlockRelax set the wall leaves no wall behind for the next session
        with pytest.raises(L.WtpArgumentError):
            blockc.BlockRelax(ctx, 0, 1, boxes, x, None, 0.0, s, FORCE, K, s / 2000, s / 20, wall_xyz=wall)
        h1, p_after_fail = run()
    ref_w, p0w = _single_domain(wtp, x, wall, s, iters, s / 20)
    ref_0, p0 = _single_domain(wtp, x, wall[:0], s, iters, s / 20)
    assert np.array_equal(pw, p0w) and [h_["max_force"] for h_ in hw_] == [r["max_force"] for r in ref_w]
    assert np.array_equal(p_free, p0), "after n_wall = 0 the block session is the wall-less session bit for bit"
    assert [h_["max_force"] for h_ in h0] == [r["max_force"] for r in ref_0]
    assert (h0[0]["argmin_i"], h0[0]["argmin_j"]) == (ref_0[0]["argmin_i"], ref_0[0]["argmin_j"])
    assert np.array_equal(p_after_fail, p0), "a failed open with a wall leaves the context without one"
    assert [h_["max_force"] for h_ in h1] == [r["max_force"] for r in ref_0]
