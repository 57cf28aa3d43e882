"""Quality metrics of the reference (src/metrics.jl:19-129), reduced on the device.

The neighbour search and the statistics over its (n, k) distance rows both run on the GPU (Context.knn_stats, wtp_knn_stats):
what comes back is a struct of sums and, for the quantiles of spacing_fidelity_metrics, the n nearest-neighbour distances.
The (n, k) index and distance matrices never reach the host.

Numerical effect against reducing the returned matrix with numpy: every per-point statistic is accumulated in float64 from
the distances converted exactly, in slot order, and the sums over the cloud in a fixed tree whose chains stay below 4096
additions.  Float64 clouds therefore agree with the numpy reductions to ~1e-13 relative; Float32 clouds differ from the
earlier float32 numpy means at the float32 rounding level, because nothing is accumulated in float32 any more."""
from __future__ import annotations

import math

import numpy as np

from .engine import default_context


def _stats(cloud, k, ctx, spacing=None, **kw):
    pts = cloud.points() if hasattr(cloud, "points") else np.asarray(cloud)
    k = min(len(pts), int(k))
    h = None
    if spacing is not None:
        h = np.asarray(spacing(pts) if callable(spacing) else spacing, dtype=np.float64)
        h = np.ascontiguousarray(np.broadcast_to(h, (len(pts),)))
    # k counts the point itself: the statistics cover slots [2:end] (src/metrics.jl:22)
    return (ctx or default_context()).knn_stats(pts, k, h=h, **kw), h, k


def _sample_std(ssd, n):
    return math.sqrt(ssd / (n - 1)) if n > 1 else float("nan")


def metrics(cloud, k: int = 20, ctx=None, verbose: bool = True):
    """metrics(cloud; k): avg/std/max/min distance to the k nearest neighbours, separation, fill,
    mesh_ratio (src/metrics.jl:19-41).  std is the sample standard deviation (Julia `std`)."""
    s, _, k = _stats(cloud, k, ctx)
    n = s["n"]
    out = dict(avg=s["sum_mean"] / n, std=s["sum_std"] / n, max=s["sum_max"] / n, min=s["sum_min"] / n,
               separation=float(s["nn_min"]), fill=float(s["nn_max"]), k=k)
    out["mesh_ratio"] = out["fill"] / out["separation"] if out["separation"] > 0 else float("inf")
    if verbose:
        print("Cloud Metrics\n-------------")
        print(f"avg. distance to {k} nearest neighbors: {out['avg']}")
        print(f"std. distance to {k} nearest neighbors: {out['std']}")
        print(f"max. distance to {k} nearest neighbors: {out['max']}")
        print(f"min. distance to {k} nearest neighbors: {out['min']}")
        print(f"separation (min nearest-neighbor distance): {out['separation']}")
        print(f"fill (max nearest-neighbor distance):       {out['fill']}")
        print(f"mesh ratio (fill / separation, ≥1):         {out['mesh_ratio']}")
    return out


def spacing_metrics(cloud, spacing, k: int = 20, ctx=None):
    """Relative error of the local mean neighbour distance against the target spacing
    (src/metrics.jl:56-71)."""
    s, _, k = _stats(cloud, k, ctx, spacing)
    n = s["n"]
    return dict(max_error=float(s["max_err"]), mean_error=s["sum_err"] / n, std_error=_sample_std(s["ssd_err"], n), k=k)


def spacing_fidelity_metrics(cloud, spacing, k: int = 30, coord_radius: float = 1.4, ctx=None):
    """d_NN/h distribution and coordination number (src/metrics.jl:88-129)."""
    s, h, k = _stats(cloud, k, ctx, spacing, coord_radius=coord_radius, return_nn=True)
    n = s["n"]
    mu = s["sum_u"] / n
    q = np.quantile(s["nn"].astype(np.float64) / h, [0.05, 0.5, 0.95])
    return dict(mean_dnn_h=mu, cv=_sample_std(s["ssd_u"], n) / mu, p05=float(q[0]), p50=float(q[1]), p95=float(q[2]),
                coordination=s["sum_coord"] / n, k=k, coord_radius=coord_radius)
