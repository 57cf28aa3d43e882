"""metrics / spacing_metrics / spacing_fidelity_metrics on top of Context.knn_stats, without a GPU: a stub context hands
back canned sums, and the three functions must turn them into the reference's dictionaries (src/metrics.jl:19-129) without
ever asking for the (n, k) matrices."""
import math

import numpy as np
import pytest


class StubCtx:
    """knn raises; knn_stats records its arguments and returns the canned struct."""

    def __init__(self, canned, nn=None):
        self.canned, self.nn, self.calls = dict(canned), nn, []

    def knn(self, *a, **kw):
        raise AssertionError("the metrics must not fetch the (n, k) matrices")

    def knn_stats(self, xyz, k, h=None, coord_radius=1.4, return_nn=False, return_mean=False):
        self.calls.append(dict(n=len(xyz), k=k, h=None if h is None else np.array(h, dtype=np.float64), coord_radius=coord_radius,
                               return_nn=return_nn, return_mean=return_mean))
        out = dict(self.canned)
        if return_nn:
            out["nn"] = self.nn
        return out


def _canned(n, k_eff, **kw):
    s = dict(n=n, k_eff=k_eff, has_spacing=0, sum_mean=0.0, sum_std=0.0, sum_max=0.0, sum_min=0.0, nn_min=0.0, nn_max=0.0,
             nn_min_i=0, nn_max_i=0, sum_err=0.0, ssd_err=0.0, max_err=0.0, sum_u=0.0, ssd_u=0.0, sum_coord=0)
    s.update(kw)
    return s


PTS = np.arange(30, dtype=np.float64).reshape(10, 3)


def test_metrics_divides_the_sums_by_n(wtp, capsys):
    c = StubCtx(_canned(10, 4, sum_mean=25.0, sum_std=5.0, sum_max=40.0, sum_min=15.0, nn_min=0.5, nn_max=2.0))
    m = wtp.metrics(PTS, k=5, ctx=c)
    assert m == dict(avg=2.5, std=0.5, max=4.0, min=1.5, separation=0.5, fill=2.0, k=5, mesh_ratio=4.0)
    out = capsys.readouterr().out
    assert out.startswith("Cloud Metrics\n-------------\n") and "avg. distance to 5 nearest neighbors: 2.5" in out
    assert "mesh ratio (fill / separation, ≥1):         4.0" in out
    assert c.calls == [dict(n=10, k=5, h=None, coord_radius=1.4, return_nn=False, return_mean=False)]


def test_metrics_clamps_k_and_keeps_inf_ratio_and_nan_std(wtp):
    # k = min(n, k); separation 0 (coincident points) -> inf; k_eff = 1 -> the device's NaN std passes through
    c = StubCtx(_canned(10, 9, sum_mean=10.0, sum_std=1.0, sum_max=20.0, sum_min=0.0, nn_min=0.0, nn_max=1.0))
    m = wtp.metrics(PTS, k=20, ctx=c, verbose=False)
    assert m["k"] == 10 and c.calls[0]["k"] == 10
    assert m["separation"] == 0.0 and m["mesh_ratio"] == math.inf
    c = StubCtx(_canned(10, 1, sum_mean=10.0, sum_std=math.nan, sum_max=10.0, sum_min=10.0, nn_min=1.0, nn_max=1.0))
    m = wtp.metrics(PTS, k=2, ctx=c, verbose=False)
    assert math.isnan(m["std"]) and m["avg"] == 1.0 and m["mesh_ratio"] == 1.0


def test_spacing_metrics_uses_n_minus_one(wtp):
    c = StubCtx(_canned(10, 4, has_spacing=1, sum_err=2.0, ssd_err=0.36, max_err=0.7))
    sm = wtp.spacing_metrics(PTS, wtp.ConstantSpacing(0.25), k=5, ctx=c)
    assert sm == dict(max_error=0.7, mean_error=0.2, std_error=math.sqrt(0.36 / 9), k=5)
    call = c.calls[0]
    assert call["h"].shape == (10,) and (call["h"] == 0.25).all() and not call["return_nn"]
    # a per-point array goes through as float64
    h = np.linspace(1, 2, 10, dtype=np.float32)
    wtp.spacing_metrics(PTS, h, k=5, ctx=c)
    assert c.calls[1]["h"].dtype == np.float64 and np.array_equal(c.calls[1]["h"], h.astype(np.float64))


def test_spacing_fidelity_metrics_cv_quantiles_coordination(wtp):
    nn = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0], dtype=np.float32)
    h = np.full(10, 2.0)
    u = nn.astype(np.float64) / h
    c = StubCtx(_canned(10, 4, has_spacing=1, sum_u=float(u.sum()), ssd_u=float(((u - u.mean()) ** 2).sum()), sum_coord=37), nn=nn)
    fm = wtp.spacing_fidelity_metrics(PTS, wtp.ConstantSpacing(2.0), k=5, coord_radius=1.25, ctx=c)
    q = np.quantile(u, [0.05, 0.5, 0.95])
    assert fm["mean_dnn_h"] == pytest.approx(u.mean(), rel=1e-15)
    assert fm["cv"] == pytest.approx(u.std(ddof=1) / u.mean(), rel=1e-14)
    assert (fm["p05"], fm["p50"], fm["p95"]) == (q[0], q[1], q[2])
    assert fm["coordination"] == 3.7 and fm["k"] == 5 and fm["coord_radius"] == 1.25
    assert c.calls[0]["return_nn"] and c.calls[0]["coord_radius"] == 1.25 and not c.calls[0]["return_mean"]


def test_binding_mirrors_the_struct(wtp):
    import ctypes

    from whatsthepoint_jl_amd import _lib

    assert ctypes.sizeof(_lib.KnnStats) == 128
    assert [f for f, _ in _lib.KnnStats._fields_][:3] == ["n", "k_eff", "has_spacing"]
    assert _lib.KnnStats.nn_min_i.offset == 64 and _lib.KnnStats.sum_coord.offset == 120
