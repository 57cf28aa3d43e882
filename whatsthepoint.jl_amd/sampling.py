"""Preprocessing that makes points: `sample_surface` / `PointBoundary.from_mesh` (src/surface_sampling.jl),
`fill_volume` / `discretize` (the Bridson placement of src/discretization/algorithms/octree.jl), `front_volume` /
`discretize(alg=SlakKosec())` (src/discretization/algorithms/slak_kosec.jl) and `generate_shadows` (src/shadow.jl).

`sample_surface` is graded Poisson-disk dart throwing on the continuous mesh surface.  The reference draws
its darts from `rand`; here they come from the library's counter-based stream (include/wtp.h,
wtp_mesh_sample), and the result is the serial loop over that stream, decided in batches on the device
(csrc/wtp_sample.hip, csrc/wtp_sample_streams.hip).  There is no CPU path: the host only checks arguments, looks
up the parent triangles' normals and divides the area shares.

`fill_volume` is the same run over darts uniform in the mesh's bounding box, of which those inside the mesh may be
taken, with the boundary points as seeds that occupy space from the start (include/wtp.h, wtp_mesh_fill).

`front_volume` is the advancing front of Slak & Kosec: the boundary points head a queue, every queue entry throws n
candidates at its own spacing, and a candidate inside the mesh that keeps that spacing from every entry joins the queue
(include/wtp.h, wtp_mesh_front)."""
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
    raise WtpArgumentError("the spacing is evaluated on the device at every dart: pass a number, "
                           f"ConstantSpacing, LogLike or BoundaryLayerSpacing, not {type(spacing).__name__}")


def _check_positive(**args):
    """The first of the named arguments, in the order given, that is not > 0 is the error."""
    for name, value in args.items():
        if not value > 0:
            raise WtpArgumentError(f"{name} must be positive")


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

    _check_positive(factor=factor, stall_limit=stall_limit, max_points=max_points)
    law = _sampler_spacing(spacing)
    mesh = _as_octree(mesh, ctx, False)
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


def _as_octree(mesh, ctx, guards: bool):
    from .octree import TriangleOctree

    if not isinstance(mesh, TriangleOctree):
        vertices, triangles = mesh
        mesh = TriangleOctree(vertices, triangles, classify_leaves=guards, verify_orientation=guards, ctx=ctx)
    if len(mesh) == 0:
        raise WtpArgumentError("mesh has no elements")
    return mesh


def fill_volume(mesh, spacing, *, seeds=None, factor: float = 0.75, max_points: int = 10_000_000, stall_limit: int = 2000,
                seed: int = synth.SEED, batch: int = 0, ctx=None):
    """Graded Poisson-disk points inside a closed triangle mesh -> PointVolume: the placement of the reference's default
    discretize (Orthtree(mesh; spacing, placement = :bridson), src/discretization/algorithms/octree.jl:804-902).

    mesh: a TriangleOctree or a (vertices, triangles) pair (a pair passes the TriangleOctree orientation guards here:
    an inside-out mesh has no inside).  Every point keeps min(r_i, r_j), r = factor * spacing(x), from every other
    point and from the seeds (the boundary points, (n, 3) or None), which are not returned.  seed and batch as for
    sample_surface.  The returned volume carries the run's wtp_fill_info as `fill_info` (with `volume_estimate` =
    bbox_volume * n_inside / n_darts added) and the points' r as `fill_r`."""
    from .cloud import PointVolume

    _check_positive(factor=factor, stall_limit=stall_limit, max_points=max_points)
    law = _sampler_spacing(spacing)
    mesh = _as_octree(mesh, ctx, True)
    c = mesh._resident(ctx)
    info = c.mesh_fill(law, factor, seeds, max_points, stall_limit, int(seed) & 0xFFFFFF, batch)
    n = int(info["n_points"])
    if n == 0:
        raise WtpArgumentError("volume fill produced no points — check spacing vs domain size and mesh orientation")
    if info["stop_reason"] == 2:
        warnings.warn("Volume fill truncated by max_points before saturation — parts of the domain may be unfilled "
                      f"(max_points = {max_points})")
    got = c.mesh_fill_get(n, want=("xyz", "r"))
    info["volume_estimate"] = info["bbox_volume"] * info["n_inside"] / info["n_darts"]
    vol = PointVolume(got["xyz"])
    vol.fill_info, vol.fill_r = info, got["r"]
    return vol


def fill_area(loops, spacing, *, seeds=None, factor: float = 0.75, max_points: int = 10_000_000, stall_limit: int = 2000,
              seed: int = synth.SEED, batch: int = 0, ctx=None):
    """Graded Poisson-disk points inside a 2-D domain -> PointVolume of 2-D points: the placement of the reference's
    default 2-D discretize (Orthtree(bnd; spacing), _generate_bridson with N = 2,
    src/discretization/algorithms/octree.jl:816-902).

    loops: a SegmentQuadtree, one (n, 2) loop or a list of loops (outer boundaries and holes, by nesting parity).
    Everything else as for fill_volume, with (n, 2) seeds.  The returned volume carries the run's wtp_fill_info as
    `fill_info` (with `area_estimate` = bbox_volume * n_inside / n_darts added, bbox_volume being the box's area) and
    the points' r as `fill_r`."""
    from .cloud import PointVolume
    from .quadtree import SegmentQuadtree

    _check_positive(factor=factor, stall_limit=stall_limit, max_points=max_points)
    law = _sampler_spacing(spacing)
    tree = loops if isinstance(loops, SegmentQuadtree) else SegmentQuadtree(loops, ctx=ctx)
    c = tree._resident(ctx)
    info = c.loops_fill(law, factor, seeds, max_points, stall_limit, int(seed) & 0xFFFFFF, batch)
    n = int(info["n_points"])
    if n == 0:
        raise WtpArgumentError("area fill produced no points — check spacing vs domain size")
    if info["stop_reason"] == 2:
        warnings.warn("Area fill truncated by max_points before saturation — parts of the domain may be unfilled "
                      f"(max_points = {max_points})")
    got = c.loops_fill_get(n, want=("xy", "r"))
    info["area_estimate"] = info["bbox_volume"] * info["n_inside"] / info["n_darts"]
    vol = PointVolume(got["xy"])
    vol.fill_info, vol.fill_r = info, got["r"]
    return vol


class SlakKosec:
    """SlakKosec(n = 10) (src/discretization/algorithms/slak_kosec.jl:59-67): the advancing front with n candidates per
    expanded point, for discretize(..., alg=SlakKosec(n)).  The mesh is discretize's own argument."""

    def __init__(self, n: int = 10):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= 64:
            raise WtpArgumentError("SlakKosec takes 1 to 64 candidates per point")
        self.n = int(n)

    def __repr__(self):
        return f"SlakKosec(n={self.n})"


def front_volume(mesh, spacing, *, seeds, n: int = 10, max_points: int = 10_000_000, seed: int = synth.SEED,
                 batch: int = 0, ctx=None):
    """Advancing-front points inside a closed triangle mesh -> PointVolume: the placement of
    discretize(bnd, spacing; alg = SlakKosec(octree)) (src/discretization/algorithms/slak_kosec.jl:72-123).

    mesh as for fill_volume.  seeds ((m, 3), the boundary points) head the queue and are not returned; every queue entry
    throws n candidates onto the sphere of its own spacing, and a candidate inside the mesh that is farther than that
    spacing from every entry but its parent joins the queue.  Unlike the reference, expanded boundary points keep
    counting (include/wtp.h).  seed and batch (parents per batch) as for sample_surface.  The returned volume carries the
    run's wtp_front_info as `front_info`, the points' own spacing as `front_h` and their parents' queue indices as
    `front_parent`."""
    from .cloud import PointVolume

    _check_positive(max_points=max_points)
    n = SlakKosec(n).n
    law = _sampler_spacing(spacing)
    mesh = _as_octree(mesh, ctx, True)
    c = mesh._resident(ctx)
    info = c.mesh_front(law, n, seeds, max_points, int(seed) & 0xFFFFFF, batch)
    m = int(info["n_points"])
    if m == 0:
        raise WtpArgumentError("the advancing front produced no points — check the seeds, spacing vs domain size and "
                               "mesh orientation")
    if info["stop_reason"] == 2:
        warnings.warn(f"discretization stopping early, reached max points ({max_points})")
    got = c.mesh_front_get(m, want=("xyz", "h", "parent"))
    vol = PointVolume(got["xyz"])
    vol.front_info, vol.front_h, vol.front_parent = info, got["h"], got["parent"]
    return vol


_EXTRAS = {"fill": ("fill_info", "fill_r"), "front": ("front_info", "front_h", "front_parent")}


def discretize(boundary, spacing, mesh=None, *, alg=None, factor: float = None, max_points: int = 10_000_000,
               stall_limit: int = None, seed: int = synth.SEED, ctx=None):
    """discretize(bnd, spacing; alg, max_points) -> PointCloud(boundary, volume); the boundary itself is returned
    unchanged.  alg = None: Orthtree(mesh; spacing, placement = :bridson), the boundary's points being the seeds of
    fill_volume (factor 0.75, stall_limit 2000 unless given).  alg = SlakKosec(n): the advancing front from the boundary's
    points (front_volume), which has no factor and no stall_limit.

    A 2-D boundary takes the reference's 2-D default, Orthtree(bnd; spacing) (src/discretization/discretization.jl:63):
    mesh = None indexes the boundary's surfaces as loops (SegmentQuadtree.from_boundary), or mesh is a SegmentQuadtree;
    the placement is fill_area with the boundary's points as seeds.  2-D has no SlakKosec."""
    from .cloud import PointBoundary, PointCloud
    from .quadtree import SegmentQuadtree

    if alg is not None and not isinstance(alg, SlakKosec):
        raise WtpArgumentError(f"alg must be None or SlakKosec(n), not {type(alg).__name__}")
    if alg is not None and (factor is not None or stall_limit is not None):
        raise WtpArgumentError("factor and stall_limit do not apply to SlakKosec: the front tests at the spacing itself "
                               "and ends when no point is left to expand")
    if not isinstance(boundary, PointBoundary):
        boundary = PointBoundary(boundary)
    dim = boundary.points().shape[1]
    if dim == 2 and alg is not None:
        raise WtpArgumentError(f"2D discretization supports the Orthtree fill only (the default: drop `alg`); got {alg!r}")
    if dim == 2 and mesh is not None and not isinstance(mesh, SegmentQuadtree):
        raise WtpArgumentError(f"this geometry index is 3D ({type(mesh).__name__}) and cannot fill a 2D boundary — pass "
                               "mesh=None or SegmentQuadtree.from_boundary(boundary), which indexes the boundary loops")
    if dim == 3 and isinstance(mesh, SegmentQuadtree):
        raise WtpArgumentError("this geometry index is 2D (SegmentQuadtree) and cannot fill a 3D boundary — pass the "
                               "surface mesh or its TriangleOctree")
    if dim == 3 and mesh is None:
        raise WtpArgumentError("a 3D boundary needs its surface mesh: pass a TriangleOctree or a (vertices, triangles) pair")
    if dim == 2:
        tree = mesh if mesh is not None else SegmentQuadtree.from_boundary(boundary, ctx=ctx)
        vol = fill_area(tree, spacing, seeds=boundary.points(), factor=0.75 if factor is None else factor,
                        max_points=max_points, stall_limit=2000 if stall_limit is None else stall_limit, seed=seed, ctx=ctx)
    elif alg is None:
        vol = fill_volume(mesh, spacing, seeds=boundary.points(), factor=0.75 if factor is None else factor,
                          max_points=max_points, stall_limit=2000 if stall_limit is None else stall_limit, seed=seed,
                          ctx=ctx)
    else:
        vol = front_volume(mesh, spacing, seeds=boundary.points(), n=alg.n, max_points=max_points, seed=seed, ctx=ctx)
    bp = boundary.points()
    if vol.points().dtype != bp.dtype:  # the cloud keeps the boundary's type (the mesh's decided the run)
        extras = {k: getattr(vol, k) for k in _EXTRAS["fill" if alg is None else "front"]}
        vol = type(vol)(vol.points().astype(bp.dtype))
        for k, v in extras.items():
            setattr(vol, k, v)
    return PointCloud(boundary, vol)


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
