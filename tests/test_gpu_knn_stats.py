"""wtp_knn_stats: the metrics' reductions over the device k-NN distance rows (include/wtp.h, csrc/wtp_stats.hip).

The expected values are float64 reductions of the oracle's distances O.knn(x, k, True, "kdtree"), which the device search
reproduces bit for bit.  Per point they follow the call's definition (mean in slot order, two-pass deviation); over the cloud
they are exactly rounded sums (math.fsum), so the 1e-12 below is the device's own error: no chain of the reduction is longer
than 4096 additions, 4096 * 2^-53 = 4.5e-13.  Exact: separation, fill, their indices, max_err, sum_coord, the bits of nn."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-12
F32, F64 = np.float32, np.float64


def _expected(d, h=None, coord_radius=1.4):
    """d: (n, k) oracle distances, self slot included.  h: None, a number or n values."""
    r = d[:, 1:].astype(np.float64)
    n, ke = r.shape
    s = np.zeros(n)
    for j in range(ke):
        s = s + r[:, j]
    mean = s / ke
    q = np.zeros(n)
    for j in range(ke):
        q = q + (r[:, j] - mean) * (r[:, j] - mean)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(q / (ke - 1))
    nn = r[:, 0]
    e = dict(n=n, k_eff=ke, has_spacing=0, sum_mean=math.fsum(mean), sum_std=math.fsum(std) if ke > 1 else math.nan,
             sum_max=math.fsum(r.max(axis=1)), sum_min=math.fsum(nn), nn_min=nn.min(), nn_max=nn.max(),
             nn_min_i=int(np.argmin(nn)), nn_max_i=int(np.argmax(nn)), sum_err=0.0, ssd_err=0.0, max_err=0.0, sum_u=0.0, ssd_u=0.0,
             sum_coord=0, nn=d[:, 1], mean=mean)
    if h is not None:
        h = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,))
        err, u = np.abs(mean - h) / h, nn / h
        me, mu = math.fsum(err) / n, math.fsum(u) / n
        e.update(has_spacing=1, sum_err=math.fsum(err), ssd_err=math.fsum((err - me) ** 2), max_err=err.max(), sum_u=math.fsum(u),
                 ssd_u=math.fsum((u - mu) ** 2), sum_coord=int((r <= (coord_radius * h)[:, None]).sum()))
    return e


SUMS = ("sum_mean", "sum_std", "sum_max", "sum_min", "sum_err", "ssd_err", "sum_u", "ssd_u")
EXACT = ("n", "k_eff", "has_spacing", "nn_min", "nn_max", "nn_min_i", "nn_max_i", "max_err", "sum_coord")


def _check(got, want, what=""):
    for f in EXACT:
        assert got[f] == want[f], f"{what}{f}: {got[f]!r} != {want[f]!r}"
    for f in SUMS:
        if isinstance(want[f], float) and math.isnan(want[f]):
            assert math.isnan(got[f]), f"{what}{f}: {got[f]!r} is not NaN"
        else:
            assert got[f] == pytest.approx(want[f], rel=REL, abs=0.0), f"{what}{f}: {got[f]!r} != {want[f]!r}"
    if "nn" in got:
        assert got["nn"].dtype == want["nn"].dtype and got["nn"].tobytes() == want["nn"].tobytes(), what + "nn bits"
    if "mean" in got:
        assert np.array_equal(got["mean"], want["mean"]), what + "per-point means"


def _cloud(wtp, n, dim, dtype, seed):
    return wtp.synth.uniform(n, dim, dtype, seed)


def _graded_h(n, dtype_seed=0):
    """a per-point spacing spanning 64x around the cloud's mean spacing"""
    rng = np.random.default_rng(100 + dtype_seed)
    return float(n) ** (-1.0 / 3.0) * 2.0 ** rng.uniform(-3.0, 3.0, n)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_and_row_lengths(ctx, O, wtp, n, dtype, dim):
    """n around the wave and the block, k at 2 (NaN deviations), inside one tile, across tiles, and the whole cloud."""
    x = _cloud(wtp, n, dim, dtype, 7 + n)
    h = _graded_h(n)
    ks = sorted({k for k in (2, 3, 21, min(n, 60), n) if 2 <= k <= min(n, 128)})
    assert ks
    for k in ks:
        _, d = O.knn(x, k, True, "kdtree")
        got = ctx.knn_stats(x, k, h=h, coord_radius=1.4, return_nn=True, return_mean=True)
        _check(got, _expected(d, h, 1.4), f"n={n} k={k}: ")


def test_many_blocks_ragged_last_block_and_finishing_pass(ctx, O, wtp):
    n, k = 20_001, 21
    for dtype in (F32, F64):
        x = _cloud(wtp, n, 3, dtype, 5)
        h = _graded_h(n, 1)
        _, d = O.knn(x, k, True, "kdtree")
        _check(ctx.knn_stats(x, k, h=h, return_nn=True, return_mean=True), _expected(d, h), f"{np.dtype(dtype).name}: ")


def _lattice(m=10, dtype=F32):
    g = np.arange(m, dtype=dtype)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(dtype)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_lattice_all_ties_and_inclusive_coordination_radius(ctx, O, wtp, dtype):
    x = _lattice(10, dtype)
    _, d = O.knn(x, 27, True, "kdtree")
    got = ctx.knn_stats(x, 27, h=1.0, coord_radius=1.0, return_nn=True, return_mean=True)
    want = _expected(d, 1.0, 1.0)
    _check(got, want)
    # every point's nearest neighbour is at exactly 1 = coord_radius * h: the inclusive <= counts the 6-shell, 2 * 3 * 10 * 10 * 9
    assert got["sum_coord"] == 5400 and got["nn_min"] == got["nn_max"] == 1.0 and got["nn_min_i"] == got["nn_max_i"] == 0
    assert got["sum_u"] == 1000.0 and got["ssd_u"] == 0.0
    assert ctx.knn_stats(x, 27, h=1.0, coord_radius=np.nextafter(1.0, 0.0))["sum_coord"] == 0


def test_coincident_points(ctx, O, wtp):
    x = _cloud(wtp, 500, 3, F32, 11)
    twins = [7, 100, 101, 300, 499]
    x[twins] = x[7]
    _, d = O.knn(x, 21, True, "kdtree")
    s = 500.0 ** (-1.0 / 3.0)
    got = ctx.knn_stats(x, 21, h=s, return_nn=True, return_mean=True)
    _check(got, _expected(d, s))
    assert got["nn_min"] == 0.0 and got["nn_min_i"] == 7, "separation 0 at the smallest index of the cluster"
    assert (got["nn"][twins] == 0).all() and (got["nn"][twins].astype(np.float64) / s == 0).all()  # u = 0
    m = wtp.metrics(x, k=21, ctx=ctx, verbose=False)
    assert m["separation"] == 0.0 and m["mesh_ratio"] == math.inf


def test_collinear_known_answer(ctx, wtp):
    # test/metrics.jl:115-143
    pts = np.array([(i * 1.0, 0.0, 0.0) for i in range(1, 26)])
    s = ctx.knn_stats(pts, 10, return_nn=True)
    assert s["n"] == 25 and s["k_eff"] == 9 and s["has_spacing"] == 0
    assert s["nn_min"] == s["nn_max"] == 1.0 and s["nn_min_i"] == s["nn_max_i"] == 0 and s["sum_min"] == 25.0
    assert (s["nn"] == 1.0).all()
    # interior points: neighbours at 1, 1, 2, 2, 3, 3, 4, 4, 5
    assert s["sum_max"] == sum(max(5, 9 - min(i, 24 - i)) for i in range(25))


def test_spacing_per_point_constant_and_none(ctx, O, wtp):
    n, k = 3000, 30
    x = _cloud(wtp, n, 3, F32, 21)
    _, d = O.knn(x, k, True, "kdtree")
    h = _graded_h(n, 2)
    assert h.max() / h.min() > 50
    _check(ctx.knn_stats(x, k, h=h, coord_radius=1.4, return_nn=True, return_mean=True), _expected(d, h, 1.4), "per-point: ")
    hc = float(n) ** (-1.0 / 3.0)
    const = ctx.knn_stats(x, k, h=hc, coord_radius=1.4)
    _check(const, _expected(d, hc, 1.4), "constant: ")
    assert _bytes(ctx.knn_stats(x, k, h=np.full(n, hc), coord_radius=1.4)) == _bytes(const), "an array of one value is that constant"
    none = ctx.knn_stats(x, k)
    _check(none, _expected(d), "no spacing: ")
    assert none["has_spacing"] == 0
    assert all(none[f] == 0 for f in ("sum_err", "ssd_err", "max_err", "sum_u", "ssd_u", "sum_coord"))


def _bytes(s):
    return b"".join(np.asarray(v).tobytes() for _, v in sorted(s.items()))


def test_two_calls_return_the_same_bytes(ctx, wtp):
    x = _cloud(wtp, 20_001, 3, F32, 31)
    h = _graded_h(len(x), 3)
    a = ctx.knn_stats(x, 21, h=h, return_nn=True, return_mean=True)
    ctx.knn_stats(_cloud(wtp, 777, 2, F64, 1), 5)  # another cloud in between
    b = ctx.knn_stats(x, 21, h=h, return_nn=True, return_mean=True)
    assert _bytes(a) == _bytes(b)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_device_entry_point_equals_the_host_call(ctx, wtp, dtype):
    import torch

    n, k = 5000, 21
    x = _cloud(wtp, n, 3, dtype, 41)
    h = _graded_h(n, 4)
    want = ctx.knn_stats(x, k, h=h, coord_radius=1.3, return_nn=True, return_mean=True)
    dev = torch.device("cuda", 0)
    xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(h).to(dev)
    nnd = torch.empty(n, dtype=xd.dtype, device=dev)
    md = torch.empty(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    got = ctx.knn_stats_dev(xd.data_ptr(), n, 3, dtype, k, hd.data_ptr(), 0.0, 1.3, nnd.data_ptr(), md.data_ptr())
    got["nn"], got["mean"] = nnd.cpu().numpy(), md.cpu().numpy()
    assert _bytes(got) == _bytes(want)
    # no spacing, no arrays
    assert _bytes(ctx.knn_stats_dev(xd.data_ptr(), n, 3, dtype, k)) == _bytes(ctx.knn_stats(x, k))


def test_argument_errors(ctx, wtp):
    import ctypes as C

    from whatsthepoint_jl_amd import _lib as L

    x = _cloud(wtp, 100, 3, F32, 51)
    for k in (1, 0, 101, 129):
        with pytest.raises(wtp.WtpArgumentError):
            ctx.knn_stats(x, k)
    with pytest.raises(wtp.WtpArgumentError):
        ctx.knn_stats(x[:1], 2)  # n = 1: the reference's minimum of an empty row throws
    with pytest.raises(wtp.WtpArgumentError):
        ctx.knn_stats(x[:1], 1)
    # a zero, a NaN, a negative or an infinite spacing: the first offending index is named, later ones or not
    for entries, first in (({17: 0.0}, 17), ({0: math.nan, 50: -2.0}, 0), ({99: -1.0}, 99), ({64: math.inf, 70: 0.0}, 64)):
        h = np.full(100, 0.2)
        for at, bad in entries.items():
            h[at] = bad
        with pytest.raises(wtp.WtpArgumentError, match=rf"h\[{first}\]"):
            ctx.knn_stats(x, 21, h=h)
    with pytest.raises(wtp.WtpArgumentError):
        ctx.knn_stats(x, 21, h=0.2, coord_radius=math.nan)
    # NULL out
    rc = ctx._lib.wtp_knn_stats(ctx._h, x.ctypes.data_as(C.c_void_p), 100, 3, L.WTP_F32, 21, None, 0.0, 1.4, None, None, None)
    assert rc == L.WTP_ERR_ARG and b"out is NULL" in ctx._lib.wtp_last_error(ctx._h)
    # the context still works
    assert ctx.knn_stats(x, 21)["n"] == 100


def test_refused_during_a_relax_session(wtp):
    x = _cloud(wtp, 2000, 3, F32, 61)
    s = 2000.0 ** (-1.0 / 3.0)
    with wtp.Context(0) as c:
        with c.relax(x, 0, s, dict(kind=2, beta=0.2, u0=1.0, gamma=3.0), 21, s / 2000, s / 20):
            with pytest.raises(wtp.WtpError) as ei:
                c.knn_stats(x, 21)
            assert ei.value.code == 4  # WTP_ERR_STATE
        assert c.knn_stats(x, 21)["n"] == 2000


def test_ends_a_pending_radius_pair(ctx, wtp):
    x = _cloud(wtp, 1000, 3, F32, 71)
    counts = np.empty(1000, dtype=np.int32)
    import ctypes as C

    assert ctx._lib.wtp_radius_count(ctx._h, x.ctypes.data_as(C.c_void_p), 1000, 3, 0, 0.1, counts.ctypes.data_as(C.c_void_p)) == 0
    ctx.knn_stats(x, 5)
    assert ctx._lib.wtp_radius_fill(ctx._h, None, None) == 4  # WTP_ERR_STATE: the pair is over


def test_metrics_float32_cloud_against_float64_reductions(ctx, O, wtp):
    """The three functions on a Float32 cloud: accumulated in double on the device, so they match the float64 reductions of
    the oracle's float32 distances (the earlier numpy path took the per-point means in float32)."""
    n = 4000
    x = _cloud(wtp, n, 3, F32, 81)
    law = wtp.ConstantSpacing(float(n) ** (-1.0 / 3.0))
    s = np.broadcast_to(np.asarray(law(x), dtype=np.float64), (n,))  # spacing.(points), as the functions evaluate it
    _, d = O.knn(x, 20, True, "kdtree")
    e = _expected(d, s)
    m = wtp.metrics(x, k=20, ctx=ctx, verbose=False)
    assert m["avg"] == pytest.approx(e["sum_mean"] / n, rel=REL) and m["std"] == pytest.approx(e["sum_std"] / n, rel=REL)
    assert m["max"] == pytest.approx(e["sum_max"] / n, rel=REL) and m["min"] == pytest.approx(e["sum_min"] / n, rel=REL)
    assert m["separation"] == e["nn_min"] and m["fill"] == e["nn_max"]
    sm = wtp.spacing_metrics(x, law, k=20, ctx=ctx)
    assert sm["max_error"] == e["max_err"] and sm["mean_error"] == pytest.approx(e["sum_err"] / n, rel=REL)
    assert sm["std_error"] == pytest.approx(math.sqrt(e["ssd_err"] / (n - 1)), rel=REL)
    _, d30 = O.knn(x, 30, True, "kdtree")
    e30 = _expected(d30, s, 1.4)
    fm = wtp.spacing_fidelity_metrics(x, law, k=30, ctx=ctx)
    u = d30[:, 1].astype(np.float64) / s
    q = np.quantile(u, [0.05, 0.5, 0.95])
    assert fm["mean_dnn_h"] == pytest.approx(e30["sum_u"] / n, rel=REL)
    assert fm["cv"] == pytest.approx(math.sqrt(e30["ssd_u"] / (n - 1)) / (e30["sum_u"] / n), rel=REL)
    assert (fm["p05"], fm["p50"], fm["p95"]) == (q[0], q[1], q[2]) and fm["coordination"] == e30["sum_coord"] / n
