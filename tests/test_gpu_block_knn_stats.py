"""wtp_block_knn_stats: the metrics' sums of a cloud that stays split across ranks (include/wtp.h, csrc/wtp_block_topo.hip).

Ranks run as threads on the one GPU, one Context each, words carried by the loopback transport.  The expected answer is
Context.knn_stats of the assembled cloud (cloud[gid[i]] = xyz[i]) on a fresh context: sums to 1e-12 relative (both sides
are fixed trees with chains below 4096 additions, cut at different places), everything else exact, and every rank must hold
the same bytes.  Every join has a timeout: a collective that leaves a rank waiting fails the test instead of hanging it."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

JOIN_S = 300
REL = 1e-12
SUMS = ("sum_mean", "sum_std", "sum_max", "sum_min", "sum_err", "ssd_err", "sum_u", "ssd_u")
EXACT = ("n", "k_eff", "has_spacing", "nn_min", "nn_max", "nn_min_i", "nn_max_i", "max_err", "sum_coord")


def _ranks(nranks, worker):
    """worker(rank, hub) on one thread per rank; returns (results, errors) in rank order.  No rank is helped out of a
    collective when another fails: every rank must return on its own."""
    from whatsthepoint_jl_amd import blockc

    hub = blockc.LoopbackHub(nranks)
    out, err = [None] * nranks, [None] * nranks

    def body(r):
        try:
            out[r] = worker(r, hub)
        except BaseException as e:  # noqa: BLE001 - inspected by the test
            err[r] = e

    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(nranks)]
    for t in ts:
        t.start()
    deadline = time.time() + JOIN_S
    for t in ts:
        t.join(max(0.0, deadline - time.time()))
    if any(t.is_alive() for t in ts):
        hub.barrier.abort()
        for t in ts:
            t.join(30)
        pytest.fail("a rank was left waiting in a collective")
    return out, err


def _ok(res):
    out, err = res
    for e in err:
        if e is not None:
            raise e
    return out


def _stats_ranks(wtp, x, gid, parts, k, h=None, coord_radius=1.4):
    """h: None, a number, or one value per gid (of the assembled cloud)"""
    import torch
    from whatsthepoint_jl_amd import blockc

    R = len(parts)

    def worker(rank, hub):
        torch.cuda.set_device(0)
        with wtp.Context(0) as ctx:
            sel = parts[rank]
            hr = h[gid[sel]] if isinstance(h, np.ndarray) else h
            st, nn, info = blockc.block_knn_stats(ctx, rank, R, x[sel], gid[sel], k, h=hr, coord_radius=coord_radius, return_nn=True,
                                                  transport=blockc.loopback_transport(hub, rank) if R > 1 else None)
            return st, nn.cpu().numpy(), info

    return _ok(_ranks(R, worker))


def _bytes(s):
    return b"".join(np.asarray(v).tobytes() for _, v in sorted(s.items()))


def _check(wtp, x, gid, parts, res, k, h=None, coord_radius=1.4):
    cloud = np.empty_like(x)
    cloud[gid] = x
    with wtp.Context(0) as c:
        want = c.knn_stats(cloud, k, h=h, coord_radius=coord_radius, return_nn=True)
    got = res[0][0]
    for f in EXACT:
        assert got[f] == want[f], f"{f}: {got[f]!r} != {want[f]!r}"
    for f in SUMS:
        assert got[f] == pytest.approx(want[f], rel=REL, abs=0.0), f"{f}: {got[f]!r} != {want[f]!r}"
    for sel, (st, nn, _) in zip(parts, res):
        assert _bytes(st) == _bytes(got), "every rank holds the same struct"
        assert nn.dtype == np.float32 and nn.tobytes() == want["nn"][gid[sel]].tobytes(), "nearest-neighbour distances differ in their bits"
    return got


def _graded_h(n, seed):
    return float(n) ** (-1.0 / 3.0) * 2.0 ** np.random.default_rng(seed).uniform(-3.0, 3.0, n)


def test_one_rank_equals_knn_stats(wtp):
    n = 50_000
    x = wtp.synth.uniform(n, 3, np.float32)
    gid = np.arange(n, dtype=np.int64)
    parts = [np.arange(n)]
    h = _graded_h(n, 1)
    res = _stats_ranks(wtp, x, gid, parts, 21, h=h)
    got = _check(wtp, x, gid, parts, res, 21, h=h)
    assert got["n"] == n and got["has_spacing"] == 1 and res[0][2]["n_ghost"] == 0
    res = _stats_ranks(wtp, x, gid, parts, 21)
    got = _check(wtp, x, gid, parts, res, 21)
    assert got["has_spacing"] == 0 and got["sum_coord"] == 0 and got["sum_u"] == 0.0


def _octants(wtp, n, seed=1):
    from whatsthepoint_jl_amd import blockc

    x = wtp.synth.uniform(n, 3, np.float32)
    gid = np.random.default_rng(seed).permutation(n).astype(np.int64)  # gid order is not spatial order
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False)
    own = blockc.owner_of(x, boxes)
    return x, gid, [np.nonzero(own == r)[0] for r in range(8)]


def test_octants_uniform_permuted_gids(wtp):
    n = 8 * 40_000
    x, gid, parts = _octants(wtp, n)
    h = _graded_h(n, 2)
    res = _stats_ranks(wtp, x, gid, parts, 21, h=h)
    got = _check(wtp, x, gid, parts, res, 21, h=h)
    assert got["n"] == n and all(r[2]["n_ghost"] > 0 for r in res)
    # a constant spacing through h_const
    s = float(n) ** (-1.0 / 3.0)
    res = _stats_ranks(wtp, x, gid, parts, 21, h=s, coord_radius=1.2)
    _check(wtp, x, gid, parts, res, 21, h=s, coord_radius=1.2)


def test_ties_resolve_to_the_smaller_gid(wtp):
    """A lattice: every nearest-neighbour distance is the same, so separation and fill are attained everywhere; gid 0 wins."""
    from whatsthepoint_jl_amd import blockc

    m = 16
    g = np.arange(m, dtype=np.float32) / np.float32(64.0)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    gid = np.random.default_rng(5).permutation(len(x)).astype(np.int64)
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False, lo=(0.0, 0.0, 0.0), hi=(m / 64.0,) * 3)
    own = blockc.owner_of(x, boxes)
    parts = [np.nonzero(own == r)[0] for r in range(8)]
    res = _stats_ranks(wtp, x, gid, parts, 7, h=1.0 / 64.0, coord_radius=1.0)
    got = _check(wtp, x, gid, parts, res, 7, h=1.0 / 64.0, coord_radius=1.0)
    assert got["nn_min_i"] == 0 and got["nn_max_i"] == 0 and got["nn_min"] == got["nn_max"] == 1.0 / 64.0
    assert got["sum_coord"] == 2 * 3 * m * m * (m - 1)


def test_an_empty_rank_contributes_the_neutral_element(wtp):
    from whatsthepoint_jl_amd import blockc

    x = wtp.synth.uniform(120_000, 3, np.float32)
    x = x[~(x >= 0.5).all(axis=1)]  # the (1, 1, 1) octant stays empty
    n = len(x)
    gid = np.random.default_rng(7).permutation(n).astype(np.int64)
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False)
    own = blockc.owner_of(x, boxes)
    parts = [np.nonzero(own == r)[0] for r in range(8)]
    assert sum(len(p) == 0 for p in parts) == 1
    h = _graded_h(n, 3)
    res = _stats_ranks(wtp, x, gid, parts, 21, h=h)
    assert _check(wtp, x, gid, parts, res, 21, h=h)["n"] == n


def _expect_all(nranks, worker, exc):
    out, err = _ranks(nranks, worker)
    for r, e in enumerate(err):
        assert isinstance(e, exc), f"rank {r}: {e!r}"
    return err


def test_a_bad_argument_on_one_rank_fails_every_rank(wtp):
    import torch
    from whatsthepoint_jl_amd import blockc

    x = wtp.synth.uniform(2000, 3, np.float32)
    parts = [np.arange(1000), np.arange(1000, 2000)]

    def run(k_of, h_of=lambda rank: None):
        def worker(rank, hub):
            torch.cuda.set_device(0)
            with wtp.Context(0) as ctx:
                sel = parts[rank]
                return blockc.block_knn_stats(ctx, rank, 2, x[sel], sel.astype(np.int64), k_of(rank), h=h_of(rank),
                                              transport=blockc.loopback_transport(hub, rank))

        return worker

    assert _ok(_ranks(2, run(lambda r: 21)))[0][0]["n"] == 2000  # the same set-up succeeds
    # one rank passes k = 1, the other k = 21: both fail, neither is left waiting
    errs = _expect_all(2, run(lambda r: 1 if r == 0 else 21), wtp.WtpArgumentError)
    assert all("rank 0" in str(e) and "k must be >= 2" in str(e) for e in errs)
    _expect_all(2, run(lambda r: 21 if r == 0 else 1), wtp.WtpArgumentError)
    _expect_all(2, run(lambda r: 129), wtp.WtpArgumentError)  # beyond the library's longest row

    # a bad spacing value on rank 1 only: found on the device there, reported everywhere
    def h_of(rank):
        h = np.full(1000, 0.08)
        if rank == 1:
            h[123] = 0.0
        return h

    errs = _expect_all(2, run(lambda r: 21, h_of), wtp.WtpArgumentError)
    assert all("rank 1" in str(e) and "h[123]" in str(e) for e in errs)
    # one rank with a spacing, one without
    _expect_all(2, run(lambda r: 21, lambda rank: 0.08 if rank == 0 else None), wtp.WtpArgumentError)


def test_a_busy_context_is_refused(wtp):
    from whatsthepoint_jl_amd import blockc

    n = 20_000
    x = wtp.synth.uniform(n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    boxes = blockc.orthtree_boxes(None, 1, equal_count=False)
    force = dict(kind=2, beta=0.2, u0=1.0, gamma=3.0)
    with wtp.Context(0) as ctx:
        drv = blockc.BlockRelax(ctx, 0, 1, boxes, x, None, 2.0 * s, s, force, 21, s / 2000, s / 20)
        with pytest.raises(wtp.WtpError) as ei:
            blockc.block_knn_stats(ctx, 0, 1, x, np.arange(n, dtype=np.int64), 21)
        assert ei.value.code == 4  # WTP_ERR_STATE
        drv.close()
        assert blockc.block_knn_stats(ctx, 0, 1, x, np.arange(n, dtype=np.int64), 21)[0]["n"] == n
