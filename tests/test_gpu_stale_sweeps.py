"""Sweeps against a stale snapshot at steps of a full spacing (rebuild_every > 1, src/repel.jl:245-291).

A stale sweep queries every movable point at its MOVED position against the tree of the last rebuild and skips its own
snapshot entry by index, not by position (src/repel.jl:263-265).  A step is s*alpha_i*F with alpha_i = 1/|F| clamped to
[alpha_lo, alpha_max] and capped at one spacing (:282-291): with alpha_max = 1 nearly every point moves a full spacing per
sweep, so after a sweep or two the snapshot self lies outside the support ball of radius u0*s, and a ball may hold other
points only — one of them alone, or several.  The other parity tests use alpha_max = s/20, where self never leaves its ball.

The per-sweep harness steps a session with an explicit schedule (rebuilds at sweeps 0 and 3) and compares every sweep
with the oracle's sweep fed the same inputs: the tree holds the positions of the last rebuild (fixed head included),
the queries are the session's positions before the sweep.  Each stale sweep starts from the GPU's own previous state, so
fp32 rounding does not grow into chaotic divergence at these step sizes.  Every large-step case first checks on the host,
independently of libwtp (scipy's cKDTree), that its stale sweeps reach the regime: self outside the ball for at least a
tenth of the queries, balls holding exactly one point that is not self, and balls of 2..k points without self."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu

SCHEDULE = (True, False, False, True, False, False)  # step(rebuild): sweeps 0 and 3 rebuild the snapshot
K = 21
ALPHA_LO, ALPHA_MAX = 0.01, 1.0                      # |F| >= 1: a step of one spacing


def _force(kind, u0=1.0):
    return dict(kind=kind, beta=0.2, u0=u0, gamma=3.0)


def ball_census(tree, n_fixed, cur, radius):
    """Support balls of one stale sweep, counted on the host: tree = snapshot positions (n, dim), cur = the movable
    points' positions before the sweep (the queries), radius = u0*s per query."""
    t = cKDTree(tree.astype(np.float64))
    q = cur.astype(np.float64)
    r = np.broadcast_to(np.asarray(radius, np.float64), (len(q),))
    d_self = np.sqrt(((q - tree[n_fixed:].astype(np.float64)) ** 2).sum(axis=1))
    balls = t.query_ball_point(q, r, return_sorted=False)
    count = np.fromiter((len(b) for b in balls), np.int64, len(q))
    own = np.arange(n_fixed, n_fixed + len(q))
    has_self = np.fromiter((o in b for o, b in zip(own, balls)), bool, len(q))
    return dict(queries=len(q), self_far=int((d_self > r).sum()),
                lone_other=int(((count == 1) & ~has_self).sum()),
                few_other=int(((count >= 2) & (count <= K) & ~has_self).sum()))


def _add(total, c):
    for key, v in c.items():
        total[key] = total.get(key, 0) + v
    return total


def assert_large_step_regime(census):
    """What the large-step cases exist for; without it a change to the step or the cloud could stop them reaching it."""
    assert census["self_far"] >= 0.1 * census["queries"], census
    assert census["lone_other"] >= 1, census   # a ball of one whose member is another point
    assert census["few_other"] >= 1, census    # balls of 2..k points, self not among them


def drive_sweeps(sess, O, snap, n_fixed, u0, force, alo, amax, spacing, exact, check_stats=True):
    """Steps `sess` by SCHEDULE and compares each sweep with the oracle's sweep on the same inputs.  spacing: a constant,
    or a callable (full positions -> per-point values) for a law the session evaluates itself.  exact: Float64 (the
    same bits as the oracle) or fp32 (bounds of test_gpu_parity.py).  Returns the census of the stale sweeps."""
    n = len(snap)
    dtype = snap.dtype
    cur = snap[n_fixed:].copy()
    tree = snap.copy()
    census = {}
    for it, rebuild in enumerate(SCHEDULE):
        if rebuild:
            tree = np.concatenate([snap[:n_fixed], cur])
        if callable(spacing):
            sp = spacing(np.concatenate([snap[:n_fixed], cur]))
            s_q = sp[n_fixed:]
            s_typ = float(np.median(s_q))
        else:
            sp = s_q = s_typ = spacing
        if not rebuild:
            census = _add(census, ball_census(tree, n_fixed, cur, u0 * np.asarray(s_q, np.float64)))
        st = sess.step(rebuild)
        p = sess.positions()
        pd = sess.point_data()
        ref = O.relax_sweep(tree, n_fixed, sp, force["kind"], force["beta"], force["u0"], force["gamma"], K, alo, amax,
                            p_old=cur)
        if callable(spacing):
            assert np.array_equal(sess.spacings()[n_fixed:], sp[n_fixed:]), it   # the values this sweep used
        if exact and force["kind"] == 3:  # LennardJones: the device's pow() and the host's differ in the last place
            assert np.array_equal(pd["nn_dist"], ref["nn_dist"]), it
            assert np.array_equal(pd["nn_id"], ref["nn_id"]), it
            assert np.abs(p - ref["p"]).max() <= 1e-12 * s_typ, it
            assert np.allclose(pd["forces"], ref["forces"], rtol=1e-12, atol=0), it
            assert st["max_force"] == pytest.approx(float(ref["forces"].max()), rel=1e-12), it
        elif exact:
            assert np.array_equal(p, ref["p"]), it
            assert np.array_equal(pd["forces"], ref["forces"]), it
            assert np.array_equal(pd["nn_dist"], ref["nn_dist"]), it
            assert np.array_equal(pd["nn_id"], ref["nn_id"]), it
            assert st["max_force"] == float(ref["forces"].max()), it
        else:
            assert np.array_equal(pd["nn_id"], ref["nn_id"]), it
            assert np.array_equal(pd["nn_dist"], ref["nn_dist"]), it
            tol = (1e-5 if force["kind"] == 2 else 2e-5) * s_typ
            assert np.abs(p - ref["p"]).max() <= tol, it
            assert np.allclose(pd["forces"], ref["forces"], rtol=1e-4, atol=1e-6), it
            assert st["max_force"] == pytest.approx(float(ref["forces"].max()), rel=1e-4), it
        assert st["n_move"] == n - n_fixed, it
        if check_stats:
            sp_full = np.broadcast_to(np.asarray(sp, dtype), (n,)).copy()
            cp = O.closest_pair(ref["nn_dist"], ref["nn_id"], sp_full, n_fixed)
            assert {st["argmin_i"], st["argmin_j"]} == {cp["idx_a"], cp["idx_b"]}, it
            assert st["argmin_r"] == pytest.approx(cp["r"], rel=0, abs=0), it
        cur = p
    return census


def _cloud(wtp, n, dim, dtype, seed=20261015):
    return wtp.synth.uniform(n, dim, dtype, seed)


def _open(wtp, monkeypatch, env):
    """A context whose switches are read from `env` (read once, when a context is created)."""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    try:
        return wtp.Context(0)
    finally:
        for key in env:
            monkeypatch.delenv(key)


def _run_routes(wtp, O, monkeypatch, envs, x, n_fixed, s, u0, force, exact, alo=ALPHA_LO, amax=ALPHA_MAX):
    """The harness once per env setting, one context at a time; returns the census and the final positions per setting."""
    out = {}
    census = None
    for env in envs:
        with _open(wtp, monkeypatch, env) as c, c.relax(x, n_fixed, s, force, K, alo, amax) as sess:
            census = drive_sweeps(sess, O, x, n_fixed, u0, force, alo, amax, s, exact)
            out[tuple(sorted(env.items()))] = (sess.positions(), sess.point_data())
    return census, out


@pytest.mark.parametrize("u0", [1.0, 0.8])
@pytest.mark.parametrize("n_fixed", [0, 2000])
def test_float64_ball_and_wave_paths_match_oracle_at_full_spacing_steps(wtp, O, monkeypatch, u0, n_fixed):
    # stale sweeps: the Ball route (cs_ball64_kernel, then the wave path for what it hands back), and with WTP_BALL64=0
    # the exact wave path alone with its support-ball shortcut; both the oracle's bits, and so each other's
    n = 30000
    x = _cloud(wtp, n, 3, np.float64)
    s = float(n) ** (-1.0 / 3.0)
    census, out = _run_routes(wtp, O, monkeypatch, [{}, {"WTP_BALL64": "0"}], x, n_fixed, s, u0, _force(2, u0), True)
    assert_large_step_regime(census)
    (pa, da), (pb, db) = out.values()
    assert np.array_equal(pa, pb)
    for key in ("forces", "nn_dist", "nn_id"):
        assert np.array_equal(da[key], db[key])


@pytest.mark.parametrize("u0", [1.0, 0.8])
@pytest.mark.parametrize("n_fixed", [0, 4000])
def test_float32_ball_and_exact_paths_match_oracle_at_full_spacing_steps(wtp, O, monkeypatch, u0, n_fixed):
    # stale sweeps: the Ball route (cs_ball_kernel), and with WTP_FULL_SELECT=1 the Exact route
    n = 40000
    x = _cloud(wtp, n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    census, _ = _run_routes(wtp, O, monkeypatch, [{}, {"WTP_FULL_SELECT": "1"}], x, n_fixed, s, u0, _force(2, u0), False)
    assert_large_step_regime(census)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_dimensional_stale_sweeps_at_full_spacing_steps(wtp, O, monkeypatch, dtype):
    n, n_fixed, u0 = 20000, 500, 0.8
    x = _cloud(wtp, n, 2, dtype)
    s = float(n) ** (-1.0 / 2.0)
    census, _ = _run_routes(wtp, O, monkeypatch, [{}], x, n_fixed, s, u0, _force(2, u0), dtype == np.float64)
    assert_large_step_regime(census)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", [0, 1, 3])
def test_other_laws_stale_sweeps_at_full_spacing_steps(wtp, O, monkeypatch, dtype, kind):
    # no compact support: the stale sweeps take the wave path's general selection (Exact).  Float64 LennardJones
    # (kind 3) is exact up to pow() in the last place, as in test_gpu_sweep64.py
    n = 20000
    x = _cloud(wtp, n, 3, dtype)
    s = float(n) ** (-1.0 / 3.0)
    census, _ = _run_routes(wtp, O, monkeypatch, [{}], x, 0, s, 1.0, _force(kind), dtype == np.float64)
    assert_large_step_regime(census)


def test_small_step_control_keeps_self_in_its_ball(wtp, O, monkeypatch):
    # alpha = [s/2000, s/20], the steps of the other stale-snapshot tests: self never leaves its support ball
    n, n_fixed = 30000, 2000
    x = _cloud(wtp, n, 3, np.float64)
    s = float(n) ** (-1.0 / 3.0)
    census, out = _run_routes(wtp, O, monkeypatch, [{}, {"WTP_BALL64": "0"}], x, n_fixed, s, 1.0, _force(2), True,
                              alo=s / 2000, amax=s / 20)
    assert census["self_far"] == 0 and census["lone_other"] == 0 and census["few_other"] == 0, census
    (pa, _), (pb, _) = out.values()
    assert np.array_equal(pa, pb)


def _boundary(wtp, dtype, m, seed=31):
    b = wtp.synth.uniform(m, 3, dtype, seed)
    f = np.arange(m) % 6
    b[np.arange(m), f % 3] = (f // 3).astype(dtype)      # points on the faces of the unit cube
    return b


def test_float64_device_spacing_law_stale_sweeps_at_full_spacing_steps(wtp, O, monkeypatch):
    # a LogLike law evaluated by the session at every sweep: per-point spacing on the stale sweeps, and wide supports
    # in the bulk, which the rebuild sweeps hand to the ball kernel
    n_fixed, n_move, u0 = 3000, 20000, 1.0
    b = _boundary(wtp, np.float64, n_fixed)
    v = _cloud(wtp, n_move, 3, np.float64) * 0.9 + 0.05
    snap = np.concatenate([b, v])
    law = wtp.LogLike(b, 0.07, 1.2)
    sp0 = O.spacing_loglike(snap, b, 0.07, 1.2)

    def spacing(pos):
        sp = O.spacing_loglike(pos, b, 0.07, 1.2)
        sp[:n_fixed] = sp0[:n_fixed]
        return sp

    force = _force(2, u0)
    with wtp.Context(0) as c, c.relax(snap, n_fixed, law.desc(), force, K, ALPHA_LO, ALPHA_MAX) as sess:
        census = drive_sweeps(sess, O, snap, n_fixed, u0, force, ALPHA_LO, ALPHA_MAX, spacing, True)
    assert_large_step_regime(census)


def _loop_case(wtp):
    n, n_fixed, u0 = 30000, 2000, 0.8
    x = _cloud(wtp, n, 3, np.float64)
    return x, n_fixed, float(n) ** (-1.0 / 3.0), u0


def test_float64_loop_at_full_spacing_steps_is_bit_exact(wtp, O, monkeypatch):
    # the whole loop with rebuild_every = 3: positions and the convergence history bit for bit, on the default route and
    # on the exact wave path
    x, n_fixed, s, u0 = _loop_case(wtp)
    ref = O.relax_loop(x, n_fixed, s, 2, 0.2, u0, 3.0, K, ALPHA_LO, ALPHA_MAX, max_iters=6, tol=0.0, rebuild_every=3,
                       stall_after=0)
    for env in ({}, {"WTP_BALL64": "0"}):
        with _open(wtp, monkeypatch, env) as c, c.relax(x, n_fixed, s, _force(2, u0), K, ALPHA_LO, ALPHA_MAX) as sess:
            conv, last = sess.run(6, 3)
            p = sess.positions()
        assert np.array_equal(p, ref["p"]), env
        assert np.array_equal(np.asarray(conv), ref["conv"]), env
        assert last["n_move"] == len(x) - n_fixed


def test_float64_device_stop_rule_at_full_spacing_steps(wtp, O, monkeypatch):
    # wtp_relax_run_until with rebuild_every = 3 stops in the sweep, and for the reason, of the oracle's loop
    x, n_fixed, s, u0 = _loop_case(wtp)
    O.set_cv_double(False)
    ref = O.relax_loop(x, n_fixed, s, 2, 0.2, u0, 3.0, K, ALPHA_LO, ALPHA_MAX, max_iters=40, tol=1e-12, rebuild_every=3,
                       stall_after=2, cv_target=0.0)
    assert ref["stop_reason"] == 3, ref["stop_reason"]   # the stall rule fires before max_iters
    with wtp.Context(0) as c, c.relax(x, n_fixed, s, _force(2, u0), K, ALPHA_LO, ALPHA_MAX) as sess:
        conv, reason, _ = sess.run_until(40, 3, 1e-12, 2, 0.0)
        p = sess.positions()
    assert reason == ref["stop_reason"] and len(conv) == len(ref["conv"]), (reason, len(conv), len(ref["conv"]))
    assert np.array_equal(np.asarray(conv), ref["conv"])
    assert np.array_equal(p, ref["p"])
