"""Sharded set_topology (include/wtp.h: wtp_block_knn, wtp_block_radius_*; csrc/wtp_block_topo.hip).

Ranks run as threads on the one GPU, one Context each, rows carried by the loopback transport.  The expected answer is
always ctx.knn / ctx.radius of the assembled cloud (cloud[gid[i]] = xyz[i]) on a fresh context, and every comparison is
exact: ids with array_equal, distances as bits.  Every join has a timeout: a collective that leaves a rank waiting fails
the test instead of hanging it."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

JOIN_S = 300


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


def _assemble(x, gid):
    cloud = np.empty_like(x)
    cloud[gid] = x
    return cloud


def _shares(x, boxes):
    from whatsthepoint_jl_amd import blockc

    own = blockc.owner_of(x, boxes)
    return [np.nonzero(own == r)[0] for r in range(len(boxes))]


def _knn_ranks(wtp, x, gid, parts, k, include_self=False, width=0.0):
    import torch
    from whatsthepoint_jl_amd import blockc

    R = len(parts)

    def worker(rank, hub):
        torch.cuda.set_device(0)
        with wtp.Context(0) as ctx:
            sel = parts[rank]
            idx, dist, info = blockc.block_knn(ctx, rank, R, x[sel], gid[sel], k, include_self=include_self, return_dist=True,
                                               width=width, transport=blockc.loopback_transport(hub, rank) if R > 1 else None)
            return idx.cpu().numpy(), dist.cpu().numpy(), info

    return _ok(_ranks(R, worker))


def _check_knn(wtp, x, gid, parts, res, k, include_self=False):
    cloud = _assemble(x, gid)
    with wtp.Context(0) as c:
        ri, rd = c.knn(cloud, k, include_self=include_self, return_dist=True)
    seen = np.zeros(len(x), dtype=np.int64)
    for sel, (idx, dist, _) in zip(parts, res):
        g = gid[sel]
        seen[g] += 1
        assert idx.shape == (len(sel), k) and dist.shape == (len(sel), k)
        assert np.array_equal(idx, ri[g].astype(np.int64)), "sharded rows differ from the single-GPU rows"
        assert np.array_equal(dist.view(np.uint32), rd[g].view(np.uint32)), "sharded distances differ in their bits"
    assert (seen == 1).all(), "every gid is a query exactly once"


def test_one_rank_equals_wtp_knn(wtp):
    n = 50_000
    x = wtp.synth.uniform(n, 3, np.float32)
    gid = np.arange(n, dtype=np.int64)
    parts = [np.arange(n)]
    for include_self, k in ((False, 21), (True, 21)):
        res = _knn_ranks(wtp, x, gid, parts, k, include_self)
        _check_knn(wtp, x, gid, parts, res, k, include_self)
        assert res[0][2]["n_ghost"] == 0 and res[0][2]["widened"] == 0


def _octants(wtp, n, seed=1):
    from whatsthepoint_jl_amd import blockc

    x = wtp.synth.uniform(n, 3, np.float32)
    gid = np.random.default_rng(seed).permutation(n).astype(np.int64)  # gid order is not spatial order
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False)
    return x, gid, _shares(x, boxes)


def test_octants_uniform_rows_and_distances_exact(wtp):
    x, gid, parts = _octants(wtp, 400_000)
    res = _knn_ranks(wtp, x, gid, parts, 21)
    _check_knn(wtp, x, gid, parts, res, 21)
    infos = [r[2] for r in res]
    assert all(i["widened"] == 0 for i in infos), "the first width certifies a uniform cloud"
    assert all(i["n_ghost"] > 0 and i["n_peers"] == 7 for i in infos)


def _lattice(seed=5):
    from whatsthepoint_jl_amd import blockc

    m = 40
    g = np.arange(m, dtype=np.float32) / np.float32(64.0)  # exact in fp32
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    gid = np.random.default_rng(seed).permutation(len(x)).astype(np.int64)
    # cut planes ON lattice planes (20 / 64): ghosts at exactly the layer width, rows whose k-th distance equals the gap
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False, lo=(0.0, 0.0, 0.0), hi=(m / 64.0,) * 3)
    return x, gid, _shares(x, boxes)


@pytest.mark.parametrize("k", [10, 18])
def test_lattice_exact_ties(wtp, k):
    """k = 10 splits the sqrt(2) shell (gid decides the k-th place); k = 18 closes it exactly."""
    x, gid, parts = _lattice()
    res = _knn_ranks(wtp, x, gid, parts, k)
    _check_knn(wtp, x, gid, parts, res, k)
    res = _knn_ranks(wtp, x, gid, parts, k, width=2.0 / 64.0)  # a width on the lattice: gaps equal to k-th distances
    _check_knn(wtp, x, gid, parts, res, k)
    assert len({r[2]["widened"] for r in res}) == 1


def _radius_ranks(wtp, x, gid, parts, r):
    import torch
    from whatsthepoint_jl_amd import blockc

    R = len(parts)

    def worker(rank, hub):
        torch.cuda.set_device(0)
        with wtp.Context(0) as ctx:
            sel = parts[rank]
            off, idx, info = blockc.block_radius(ctx, rank, R, x[sel], gid[sel], r,
                                                 transport=blockc.loopback_transport(hub, rank) if R > 1 else None)
            return off.cpu().numpy(), idx.cpu().numpy(), info

    return _ok(_ranks(R, worker))


def _check_radius(wtp, x, gid, parts, res, r):
    cloud = _assemble(x, gid)
    with wtp.Context(0) as c:
        ro, ri = c.radius(cloud, r)
    for sel, (off, idx, _) in zip(parts, res):
        g = gid[sel]
        lens = ro[g + 1] - ro[g]
        assert off.shape == (len(sel) + 1,) and off[0] == 0
        assert np.array_equal(np.diff(off), lens), "row lengths differ from the single-GPU rows"
        pos = np.arange(int(lens.sum())) - np.repeat(off[:-1], lens) + np.repeat(ro[g], lens)
        assert np.array_equal(idx, ri[pos].astype(np.int64)), "radius rows differ from the single-GPU rows"


def test_lattice_radius_inclusive_boundary(wtp):
    """r = 1/64: the 6-shell lies exactly at r."""
    x, gid, parts = _lattice()
    r = 1.0 / 64.0
    res = _radius_ranks(wtp, x, gid, parts, r)
    _check_radius(wtp, x, gid, parts, res, r)
    assert sum(len(i) for _, i, _ in res) > 6 * len(x) // 2


def test_thin_first_width_is_widened(wtp):
    n = 400_000
    x, gid, parts = _octants(wtp, n)
    s = float(n) ** (-1.0 / 3.0)
    res = _knn_ranks(wtp, x, gid, parts, 21, width=0.05 * s)
    _check_knn(wtp, x, gid, parts, res, 21)
    widened = {r[2]["widened"] for r in res}
    assert len(widened) == 1 and widened.pop() >= 1


def test_graded_cloud_over_count_median_boxes(wtp):
    from whatsthepoint_jl_amd import blockc

    n = 500_000
    x = wtp.synth.graded(n, dtype=np.float32)
    gid = np.random.default_rng(3).permutation(n).astype(np.int64)
    boxes = blockc.orthtree_boxes(x, 4)
    parts = _shares(x, boxes)
    res = _knn_ranks(wtp, x, gid, parts, 21)
    _check_knn(wtp, x, gid, parts, res, 21)
    assert len({r[2]["width"] for r in res}) > 1, "each rank's width follows its own density"


def test_after_a_block_repel(wtp):
    """Owned points after a lazy-migration repel stray up to `margin` outside their box: still exact."""
    import torch
    from whatsthepoint_jl_amd import blockc

    n, k = 200_000, 21
    x = wtp.synth.uniform(n, 3, np.float32)
    s = float(n) ** (-1.0 / 3.0)
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False)
    parts = _shares(x, boxes)
    force = dict(kind=2, beta=0.2, u0=1.0, gamma=3.0)

    def worker(rank, hub):
        torch.cuda.set_device(0)
        with wtp.Context(0) as ctx:
            sel = parts[rank]
            tr = blockc.loopback_transport(hub, rank)
            drv = blockc.BlockRelax(ctx, rank, 8, boxes, x[sel], sel.astype(np.int64), 2.2 * s, s, force, k, s / 2000, s / 20,
                                    margin=0.75 * s, transport=tr)
            for _ in range(4):
                drv.step()
            xyz, g = drv.owned()
            drv.close()
            idx, dist, info = blockc.block_knn(ctx, rank, 8, xyz, g, k, return_dist=True, transport=tr)
            return xyz.cpu().numpy(), g.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy(), info

    res = _ok(_ranks(8, worker))
    xs = np.concatenate([r[0] for r in res])
    gs = np.concatenate([r[1] for r in res])
    assert np.array_equal(np.sort(gs), np.arange(n))
    b32 = boxes.astype(np.float32)
    outside = 0
    for rank, r in enumerate(res):
        p = r[0]
        inb = np.ones(len(p), dtype=bool)
        for a in range(3):
            inb &= (p[:, a] >= b32[rank, a]) & (p[:, a] < b32[rank, 3 + a])
        outside += int((~inb).sum())
    assert outside > 0, "lazy migration left some owned points outside their box"
    cloud = _assemble(xs, gs)
    with wtp.Context(0) as c:
        ri, rd = c.knn(cloud, k, return_dist=True)
    for _, g, idx, dist, _ in res:
        assert np.array_equal(idx, ri[g].astype(np.int64))
        assert np.array_equal(dist.view(np.uint32), rd[g].view(np.uint32))


def test_an_empty_rank_takes_part(wtp):
    from whatsthepoint_jl_amd import blockc

    x = wtp.synth.uniform(300_000, 3, np.float32)
    x = x[~(x >= 0.5).all(axis=1)]  # the (1, 1, 1) octant stays empty
    n = len(x)
    gid = np.random.default_rng(7).permutation(n).astype(np.int64)
    boxes = blockc.orthtree_boxes(None, 8, equal_count=False)
    parts = _shares(x, boxes)
    empty = [r for r in range(8) if len(parts[r]) == 0]
    assert len(empty) == 1
    res = _knn_ranks(wtp, x, gid, parts, 21)
    assert res[empty[0]][0].shape == (0, 21)
    _check_knn(wtp, x, gid, parts, res, 21)


def _expect_all(nranks, worker, exc, code=None):
    out, err = _ranks(nranks, worker)
    for r, e in enumerate(err):
        assert isinstance(e, exc), f"rank {r}: {e!r}"
        if code is not None:
            assert e.code == code
    return err


def test_collective_errors_fail_every_rank(wtp):
    import torch
    from whatsthepoint_jl_amd import blockc

    x = wtp.synth.uniform(40, 3, np.float32)
    parts = [np.arange(20), np.arange(20, 40)]

    def run(k, gid_of):
        def worker(rank, hub):
            torch.cuda.set_device(0)
            with wtp.Context(0) as ctx:
                sel = parts[rank]
                return blockc.block_knn(ctx, rank, 2, x[sel], gid_of(rank, sel), k, transport=blockc.loopback_transport(hub, rank))

        return worker

    plain = lambda rank, sel: sel.astype(np.int64)  # noqa: E731
    assert _ok(_ranks(2, run(21, plain)))[0][0].shape == (20, 21)  # the same set-up succeeds
    # k + 1 > N_total
    _expect_all(2, run(40, plain), wtp.WtpArgumentError)

    def big(rank, sel):
        g = sel.astype(np.int64)
        if rank == 1:
            g[3] = 2**31
        return g

    _expect_all(2, run(5, big), wtp.WtpArgumentError)

    def twice(rank, sel):
        g = sel.astype(np.int64)
        if rank == 1:
            g[0] = 0  # gid 0 is rank 0's too (and gid 20 is nobody's)
        return g

    errs = _expect_all(2, run(5, twice), wtp.WtpArgumentError)
    assert all("more than one rank" in str(e) for e in errs)


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
            blockc.block_knn(ctx, 0, 1, x, np.arange(n, dtype=np.int64), 21)
        assert ei.value.code == 4  # WTP_ERR_STATE
        drv.close()
        idx, _, _ = blockc.block_knn(ctx, 0, 1, x, np.arange(n, dtype=np.int64), 21)
        assert idx.shape == (n, 21)


def test_radius_octants_uniform(wtp):
    n = 400_000
    x, gid, parts = _octants(wtp, n, seed=11)
    r = 1.5 * float(n) ** (-1.0 / 3.0)
    res = _radius_ranks(wtp, x, gid, parts, r)
    _check_radius(wtp, x, gid, parts, res, r)
    assert all(i["widened"] == 0 and i["n_ghost"] > 0 for _, _, i in res)
