"""NodeOctree: the spacing-driven node octree of the reference's Orthtree algorithm (build_node_octree +
classify_node_octree, src/octree/spacing_criterion.jl:88-215) over a closed triangle mesh, built, balanced and
classified on the device (include/wtp.h, wtp_node_tree_*; csrc/wtp_node_tree.hip).  The host checks arguments, picks
the automatic node_min_ratio and derives the leaves' geometry from their cells; there is no CPU path."""
from __future__ import annotations

import numpy as np

from ._lib import WtpArgumentError
from .spacings import BoundaryLayerSpacing, ConstantSpacing

LEAF_EXTERIOR, LEAF_BOUNDARY, LEAF_INTERIOR = 0, 1, 2


def auto_node_min_ratio(octree, spacing, alpha: float) -> float:
    """Orthtree's rule for node_min_ratio (src/discretization/algorithms/octree.jl:134-159, 288-308): (h_min / alpha) over
    the mesh's largest extent, h_min being Δx of a constant spacing and at_wall of a BoundaryLayerSpacing; for any other
    spacing the geometry tree's 1 / (4 nt^(1/3))."""
    if isinstance(spacing, (int, float, np.integer, np.floating)) and not isinstance(spacing, bool):
        h_min = float(spacing)
    elif isinstance(spacing, ConstantSpacing):
        h_min = spacing.dx
    elif isinstance(spacing, BoundaryLayerSpacing):
        h_min = spacing.at_wall
    else:
        return 1.0 / (4.0 * len(octree) ** (1.0 / 3.0))
    T = octree.dtype.type
    max_extent = T((octree.bbox_max - octree.bbox_min).max())
    return float(T(T(h_min) / T(alpha)) / max_extent)


class NodeOctree:
    """NodeOctree(mesh, spacing, *, alpha=2.0, node_min_ratio=None, ctx=None).

    mesh: a TriangleOctree or a (vertices, triangles) pair; spacing: a number, ConstantSpacing, LogLike or
    BoundaryLayerSpacing.  The tree is built at once and its leaves are read back; `info` is the build's
    wtp_node_tree_info.  A context holds one tree at a time: find_leaf builds this one again if another took its place."""

    def __init__(self, mesh, spacing, *, alpha: float = 2.0, node_min_ratio=None, ctx=None):
        from .sampling import _as_octree, _sampler_spacing

        if not alpha > 0:
            raise WtpArgumentError("alpha must be positive")
        self._law = _sampler_spacing(spacing)
        self.mesh = _as_octree(mesh, ctx, True)
        self.alpha = float(alpha)
        self.node_min_ratio = float(auto_node_min_ratio(self.mesh, spacing, alpha) if node_min_ratio is None else node_min_ratio)
        self._ctx = ctx
        self._token = object()
        self._build(ctx)
        got = self._resident(ctx).node_tree_get(self.info["n_leaves"])
        self.cell, self.depth, self.classes, self.h = got["cell"], got["depth"], got["cls"], got["h"]

    def _build(self, ctx):
        c = self.mesh._resident(ctx or self._ctx)
        self.info = c.node_tree_build(self._law, self.alpha, self.node_min_ratio)
        c._node_tree_owner = (self._token, getattr(c, "_mesh_owner", None))
        return c

    def _resident(self, ctx=None):
        c = self.mesh._resident(ctx or self._ctx)  # a mesh set anew drops the tree
        if getattr(c, "_node_tree_owner", None) != (self._token, getattr(c, "_mesh_owner", None)):
            c = self._build(ctx)
        return c

    def __len__(self):
        return int(self.info["n_leaves"])

    def leaves(self):
        """The leaves in leaf order: dict(cell, depth, cls, h, lo, size, centre), lo / size / centre in the mesh's type as
        the tree computes them (box_bounds, box_size, box_center)."""
        T = self.h.dtype.type
        org = np.asarray(self.info["origin"], dtype=self.h.dtype)
        size = (T(self.info["root_size"]) / (2.0 ** self.depth).astype(self.h.dtype)).astype(self.h.dtype)
        lo = org + self.cell.astype(self.h.dtype) * size[:, None]
        centre = org + ((2 * self.cell + 1).astype(self.h.dtype) * size[:, None]) / T(2)
        return dict(cell=self.cell, depth=self.depth, cls=self.classes, h=self.h, lo=lo, size=size, centre=centre)

    def find_leaf(self, points, ctx=None):
        """find_leaf for (n, 3) points (or one point): the leaf's index in leaf order, -1 outside the root box."""
        p = np.asarray(points)
        out = self._resident(ctx).node_tree_locate(np.atleast_2d(p))
        return int(out[0]) if p.ndim == 1 else out

    def place(self, placement, max_points=None, boundary_oversampling: float = 2.0, seed: int = None, ctx=None):
        """The per-leaf placements "random", "jittered" and "lattice" of the Orthtree algorithm (wtp_node_place) ->
        PointVolume carrying the run's wtp_node_place_info as `place_info` and each point's leaf as `place_leaf`.
        max_points = None: the tree's estimate.  Points of interior leaves are taken as they are, near-surface candidates
        (boundary_oversampling times their share) pass the mesh's inside test, and interior leaves fill what is missing."""
        from . import synth
        from .cloud import PointVolume

        placement = str(placement).lstrip(":")
        if placement not in ("random", "jittered", "lattice"):
            raise WtpArgumentError("placement must be :random, :jittered, :lattice, or :bridson"
                                   if placement != "bridson" else "placement :bridson is fill_volume's, not a per-leaf one")
        if not boundary_oversampling > 0:
            raise WtpArgumentError("boundary_oversampling must be positive")
        if max_points is None:
            max_points = self.estimate_volume_points()
        if not max_points > 0:
            raise WtpArgumentError("max_points must be positive")
        c = self._resident(ctx)
        info = c.node_place(placement, max_points, boundary_oversampling, (synth.SEED if seed is None else int(seed)) & 0xFFFFFF)
        got = c.node_place_get(int(info["n_points"]))
        vol = PointVolume(got["xyz"])
        vol.place_info, vol.place_leaf = info, got["leaf"]
        return vol

    def estimate_volume_points(self) -> int:
        """_estimate_volume_points: ceil(1.5 * the spacing integral over the non-exterior leaves), the automatic max_points."""
        return int(self.info["max_points_auto"])

    def __repr__(self):
        i = self.info
        return (f"NodeOctree({i['n_leaves']} leaves: {i['n_interior']} interior, {i['n_boundary']} boundary, "
                f"{i['n_exterior']} exterior; depth {i['depth_max']})")
