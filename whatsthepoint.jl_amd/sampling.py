"""Boundary preprocessing that makes points: `sample_surface` / `PointBoundary.from_mesh`
(src/surface_sampling.jl) and `generate_shadows` (src/shadow.jl).

`sample_surface` is graded Poisson-disk dart throwing on the continuous mesh surface.  The reference draws
its darts from `rand`; here they come from the library's counter-based stream (include/wtp.h,
wtp_mesh_sample), and the result is the serial loop over that stream, decided in batches on the device
(csrc/wtp_sample.hip).  There is no CPU path: the host only checks arguments, looks up the parent
triangles' normals and divides the area shares."""
from __future__ import annotations

import warnings

import numpy as np

from . import synth
from ._lib import WtpArgumentError
from .spacings import BoundaryLayerSpacing, ConstantSpacing, LogLike


def _sampler_spacing(spacing):
    """What Context.mesh_sample takes: a float (ConstantSpacing) or the dict of a device-evaluated law."""
    if isinstance(spacing, (LogLike, BoundaryLayerSpacing)):
        return spacing.desc()
    if isinstance(spacing, ConstantSpacing):
        return float(spacing.dx)
    if isinstance(spacing, (int, float, np.integer, np.floating)) and not isinstance(spacing, bool):
        return float(spacing)
    raise WtpArgumentError("sample_surface evaluates the spacing on the device at every dart: pass a number, "
                           f"ConstantSpacing, LogLike or BoundaryLayerSpacing, not {type(spacing).__name__}")


def sample_surface(mesh, spacing, *, factor: float = 0.75, max_points: int = 10_000_000, stall_limit: int = 2000,
                   seed: int = synth.SEED, batch: int = 0, ctx=None):
    """sample_surface(mesh, spacing; factor, max_points, stall_limit) -> PointSurface (src/surface_sampling.jl:34-104).

    mesh: a TriangleOctree or a (vertices, triangles) pair.  Samples keep min(r_i, r_j) from each other,
    r = factor * spacing(x); each carries its parent triangle's normal, and the areas share the mesh's total area in
    proportion to r^2.  seed selects the dart stream (the stream's key holds 24 bits of it, as synth.uniform's does:
    seeds equal modulo 2^24 name the same stream); batch = 0 lets the library choose the darts per batch, which
    changes time only.  The returned surface carries the run's wtp_sample_info as `sample_info`, the samples' r as
    `sample_r` and their parent triangles as `sample_tri`."""
    from .cloud import PointSurface
    from .octree import TriangleOctree

    if not factor > 0:
        raise WtpArgumentError("factor must be positive")
    if not stall_limit > 0:
        raise WtpArgumentError("stall_limit must be positive")
    if not max_points > 0:
        raise WtpArgumentError("max_points must be positive")
    law = _sampler_spacing(spacing)
    if not isinstance(mesh, TriangleOctree):
        vertices, triangles = mesh
        mesh = TriangleOctree(vertices, triangles, classify_leaves=False, verify_orientation=False, ctx=ctx)
    if len(mesh) == 0:
        raise WtpArgumentError("mesh has no elements")
    c = mesh._resident(ctx)
    info = c.mesh_sample(law, factor, max_points, stall_limit, int(seed) & 0xFFFFFF, batch)
    n = int(info["n_points"])
    if n == 0:
        raise WtpArgumentError("surface sampling produced no points — check spacing vs mesh size")
    if info["stop_reason"] == 2:
        warnings.warn("Surface sampling truncated by max_points before saturation — the surface is under-sampled "
                      f"(max_points = {max_points})")
    got = c.mesh_sample_get(n, want=("xyz", "tri", "r"))
    dt = got["xyz"].dtype
    normals = c.mesh_face_normals()[got["tri"]].astype(dt)
    w = got["r"].astype(np.float64) ** 2
    areas = info["total_area"] / w.sum() * w  # total-area-preserving shares, proportional to the local disk area
    surf = PointSurface(got["xyz"], normals, areas.astype(dt))
    surf.sample_info, surf.sample_r, surf.sample_tri = info, got["r"], got["tri"]
    return surf


class ShadowPoints:
    """ShadowPoints(Δ, order=1) (src/shadow.jl:9-17): Δ is the inward offset, a number or a callable of the
    points ((n, dim) array -> n values, or one point -> one value); order is the derivative order of the
    Hermite-type boundary condition the shadow points serve."""

    def __init__(self, delta, order: int = 1):
        self.delta, self.order = delta, int(order)

    def __call__(self, pts):
        pts = np.asarray(pts)
        if not callable(self.delta):
            return self.delta if pts.ndim == 1 else np.full(len(pts), self.delta, dtype=pts.dtype)
        if pts.ndim == 1:
            return self.delta(pts)
        try:
            d = np.asarray(self.delta(pts), dtype=pts.dtype)
            if d.shape == (len(pts),):
                return d
        except Exception:
            pass
        return np.array([self.delta(p) for p in pts], dtype=pts.dtype)  # a callable of one point

    def __repr__(self):
        return f"ShadowPoints{{{self.order}}}: {self.delta}"


def generate_shadows(points, normals=None, shadow: ShadowPoints = None):
    """generate_shadows(points, normals, shadow) / (surf, shadow) / (cloud, shadow) (src/shadow.jl:27-38):
    point - Δ(point) * normal for every boundary point, as an (n, dim) array."""
    if isinstance(normals, ShadowPoints) and shadow is None:
        normals, shadow = None, normals
    if normals is None:  # a PointSurface, PointBoundary or PointCloud that carries its normals
        src = points.boundary if hasattr(points, "boundary") else points
        if hasattr(src, "elements"):
            el = src.elements()
            if el is None:
                raise WtpArgumentError("generate_shadows needs normals on every surface")
            points, normals = el[0], el[1]
        else:
            if src.normals is None:
                raise WtpArgumentError("generate_shadows needs the surface's normals")
            points, normals = src.points(), src.normals
    if not isinstance(shadow, ShadowPoints):
        raise WtpArgumentError("generate_shadows takes a ShadowPoints")
    p = np.asarray(points)
    nrm = np.asarray(normals, dtype=p.dtype)
    if nrm.shape != p.shape:
        raise WtpArgumentError("normals need the shape of the points")
    d = np.asarray(shadow(p), dtype=p.dtype)
    return p - (d[:, None] if d.ndim == 1 else d) * nrm
