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


class Orthtree:
    """Orthtree(placement="bridson", alpha=2.0, node_min_ratio=None, boundary_oversampling=2.0, factor=0.75)
    (src/discretization/algorithms/octree.jl:102-170) for discretize(..., alg=Orthtree(...)): the spacing-driven node octree
    (nodetree.NodeOctree) sizes the run, so that max_points=None means _estimate_volume_points of the tree.  The mesh and
    the spacing are discretize's own arguments; factor is the reference's bridson_factor.  "bridson" runs fill_volume under the tree's cap;
    "random", "jittered" and "lattice" are the per-leaf placements (NodeOctree.place), which use neither seeds nor factor.
    max_growth is accepted only as 0: the limited field needs a spacing kind of its own."""

    PLACEMENTS = ("random", "jittered", "lattice", "bridson")

    def __init__(self, placement: str = "bridson", alpha: float = 2.0, node_min_ratio=None, boundary_oversampling: float = 2.0,
                 factor: float = 0.75, max_growth: float = 0.0):
        placement = str(placement).lstrip(":")
        if not boundary_oversampling > 0:
            raise WtpArgumentError("boundary_oversampling must be positive")
        if placement not in self.PLACEMENTS:
            raise WtpArgumentError("placement must be :random, :jittered, :lattice, or :bridson")
        if not alpha > 0:
            raise WtpArgumentError("alpha must be positive")
        if not factor > 0:
            raise WtpArgumentError("bridson_factor must be positive")
        if not max_growth >= 0:
            raise WtpArgumentError("max_growth must be ≥ 0 (0 disables the limiter)")
        if max_growth > 0:
            raise WtpArgumentError("max_growth > 0 is not available: the gradient-limited field is not served as a spacing "
                                   "law on the device yet (gradient_limit_field limits the leaf values themselves)")
        if node_min_ratio is not None and not 0 < node_min_ratio <= 1:
            raise WtpArgumentError("node_min_ratio must be in (0, 1]")
        self.placement, self.alpha, self.node_min_ratio = placement, float(alpha), node_min_ratio
        self.boundary_oversampling, self.factor, self.max_growth = float(boundary_oversampling), float(factor), 0.0

    def is_default(self):
        return (self.placement, self.alpha, self.node_min_ratio, self.boundary_oversampling, self.factor) == (
            "bridson", 2.0, None, 2.0, 0.75)

    def __repr__(self):
        return (f"Orthtree(placement={self.placement!r}, alpha={self.alpha}, node_min_ratio={self.node_min_ratio}, "
                f"boundary_oversampling={self.boundary_oversampling}, factor={self.factor})")


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


_EXTRAS = {"fill": ("fill_info", "fill_r"), "front": ("front_info", "front_h", "front_parent"),
           "place": ("place_info", "place_leaf")}


_MAX_POINTS_DEFAULT = 10_000_000


def discretize(boundary, spacing, mesh=None, *, alg=None, factor: float = None, max_points: int = _MAX_POINTS_DEFAULT,
               stall_limit: int = None, seed: int = synth.SEED, ctx=None):
    """discretize(bnd, spacing; alg, max_points) -> PointCloud(boundary, volume); the boundary itself is returned
    unchanged.  alg = None: Orthtree(mesh; spacing, placement = :bridson), the boundary's points being the seeds of
    fill_volume (factor 0.75, stall_limit 2000 unless given).  alg = SlakKosec(n): the advancing front from the boundary's
    points (front_volume), which has no factor and no stall_limit.  alg = Orthtree(...): the node octree of the mesh under
    the spacing is built first (NodeOctree, alpha and node_min_ratio from alg); max_points = None then means the tree's
    estimate, ceil(1.5 * the spacing integral), and the "bridson" placement runs fill_volume under that cap with alg's
    factor unless one is given; the placements "random", "jittered" and "lattice" run NodeOctree.place (the volume then
    carries `place_info` and `place_leaf`).  The cloud's volume carries the tree as `node_tree`.  (The reference sizes its 1.5 headroom
    for its front, about 1.1 / h^3; the dart thrower at factor 0.75 saturates near 1.7 / h^3, so under the automatic cap a
    run usually ends by max_points: a prefix of the saturated run, spread over the whole domain.  That is the estimate
    doing its job, so no truncation warning is raised for it; fill_info["stop_reason"] == 2 still says so.)

    A 2-D boundary takes the reference's 2-D default, Orthtree(bnd; spacing) (src/discretization/discretization.jl:63):
    mesh = None indexes the boundary's surfaces as loops (SegmentQuadtree.from_boundary), or mesh is a SegmentQuadtree;
    the placement is fill_area with the boundary's points as seeds.  2-D has no SlakKosec and no node quadtree: of the
    Orthtree objects only the default Orthtree() is taken, as another name for alg = None."""
    from .cloud import PointBoundary, PointCloud
    from .quadtree import SegmentQuadtree

    if alg is not None and not isinstance(alg, (SlakKosec, Orthtree)):
        raise WtpArgumentError(f"alg must be None, SlakKosec(n) or Orthtree(...), not {type(alg).__name__}")
    tree_alg = alg if isinstance(alg, Orthtree) else None
    if max_points is None and tree_alg is None:
        raise WtpArgumentError("max_points = None asks for the node octree's estimate: pass alg=Orthtree(...)")
    if tree_alg is not None:
        alg = None  # the placement below is the default one, sized by the tree
    if alg is not None and (factor is not None or stall_limit is not None):
        raise WtpArgumentError("factor and stall_limit do not apply to SlakKosec: the front tests at the spacing itself "
                               "and ends when no point is left to expand")
    if not isinstance(boundary, PointBoundary):
        boundary = PointBoundary(boundary)
    dim = boundary.points().shape[1]
    if dim == 2 and (alg is not None or (tree_alg is not None and not tree_alg.is_default())):
        raise WtpArgumentError("2D discretization supports the Orthtree fill only (the default: drop `alg`); got "
                               f"{(alg or tree_alg)!r}")
    if dim == 2 and tree_alg is not None:  # Orthtree() is the 2-D default by name; there is no node quadtree to size it
        tree_alg, max_points = None, _MAX_POINTS_DEFAULT if max_points is None else max_points
    if dim == 2 and mesh is not None and not isinstance(mesh, SegmentQuadtree):
        raise WtpArgumentError(f"this geometry index is 3D ({type(mesh).__name__}) and cannot fill a 2D boundary — pass "
                               "mesh=None or SegmentQuadtree.from_boundary(boundary), which indexes the boundary loops")
    if dim == 3 and isinstance(mesh, SegmentQuadtree):
        raise WtpArgumentError("this geometry index is 2D (SegmentQuadtree) and cannot fill a 3D boundary — pass the "
                               "surface mesh or its TriangleOctree")
    if dim == 3 and mesh is None:
        raise WtpArgumentError("a 3D boundary needs its surface mesh: pass a TriangleOctree or a (vertices, triangles) pair")
    node_tree, auto_cap = None, False
    if tree_alg is not None:
        from .nodetree import NodeOctree

        mesh = _as_octree(mesh, ctx, True)
        node_tree = NodeOctree(mesh, spacing, alpha=tree_alg.alpha, node_min_ratio=tree_alg.node_min_ratio, ctx=ctx)
        if max_points is None:
            auto_cap = True
            max_points = node_tree.estimate_volume_points()
            if max_points < 1:
                raise WtpArgumentError("the node octree has no leaf inside or on the domain: nothing to fill — check the "
                                       "spacing vs domain size and the mesh's orientation")
        if factor is None:
            factor = tree_alg.factor
    kind = "fill" if alg is None else "front"
    if dim == 3 and tree_alg is not None and tree_alg.placement != "bridson":
        kind = "place"  # a per-leaf placement: no seeds, no factor, no stall_limit (the reference's have none either)
        vol = node_tree.place(tree_alg.placement, max_points, tree_alg.boundary_oversampling, seed, ctx=ctx)
        if len(vol) == 0:
            raise WtpArgumentError("the placement produced no points — check spacing vs domain size and mesh orientation")
    elif dim == 2:
        tree = mesh if mesh is not None else SegmentQuadtree.from_boundary(boundary, ctx=ctx)
        vol = fill_area(tree, spacing, seeds=boundary.points(), factor=0.75 if factor is None else factor,
                        max_points=max_points, stall_limit=2000 if stall_limit is None else stall_limit, seed=seed, ctx=ctx)
    elif alg is None:
        with warnings.catch_warnings():
            if auto_cap:  # ending at the tree's own estimate is the run's plan, not a truncation to warn of
                warnings.filterwarnings("ignore", message="Volume fill truncated by max_points")
            vol = fill_volume(mesh, spacing, seeds=boundary.points(), factor=0.75 if factor is None else factor,
                              max_points=max_points, stall_limit=2000 if stall_limit is None else stall_limit, seed=seed,
                              ctx=ctx)
    else:
        vol = front_volume(mesh, spacing, seeds=boundary.points(), n=alg.n, max_points=max_points, seed=seed, ctx=ctx)
    bp = boundary.points()
    if vol.points().dtype != bp.dtype:  # the cloud keeps the boundary's type (the mesh's decided the run)
        extras = {k: getattr(vol, k) for k in _EXTRAS[kind]}
        vol = type(vol)(vol.points().astype(bp.dtype))
        for k, v in extras.items():
            setattr(vol, k, v)
    if node_tree is not None:
        vol.node_tree = node_tree
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
