"""`SegmentQuadtree` — host mirror of the reference's 2-D geometry index (src/octree/segment_quadtree.jl): one or more
closed boundary loops, outer boundaries and holes resolved by nesting parity, with `isinside`, signed distance and
nearest segment.

The reference subdivides a quadtree over the segments.  Here the loops go to the GPU once (csrc/wtp_loops.hip: dedup,
validation, orientation, normals and pseudonormals, a bounding-volume tree in heap order) and every query is a device
kernel; there is no host search structure and no CPU path."""
from __future__ import annotations

import numpy as np

from ._lib import WtpArgumentError
from .engine import default_context


def _as_loops(loops):
    if isinstance(loops, np.ndarray) and loops.ndim == 2:
        loops = [loops]
    out = [np.ascontiguousarray(l) for l in loops]
    if not out:
        raise WtpArgumentError("SegmentQuadtree requires at least one boundary loop")
    for l in out:
        if l.ndim != 2 or l.shape[1] != 2:
            raise WtpArgumentError("SegmentQuadtree requires 2-D boundary loops: (n, 2) arrays of ordered vertices")
    dt = out[0].dtype if out[0].dtype in (np.float32, np.float64) else np.dtype(np.float64)
    return [l.astype(dt, copy=False) for l in out]


class SegmentQuadtree:
    def __init__(self, loops, ctx=None):
        """loops: one (n, 2) array or a list of them, each a closed loop in order around it (either orientation,
        explicitly closed or not); float32 / float64 is the index's machine type.  The library's checks (fewer than 3
        distinct vertices, no area) surface here as WtpArgumentError."""
        self.loops = _as_loops(loops)
        self.dtype = self.loops[0].dtype
        self._ctx = ctx
        self._token = object()
        c = self._resident(ctx)  # builds and validates
        self.bbox_min, self.bbox_max, self._n = c.loops_bounds()

    @classmethod
    def from_boundary(cls, boundary, ctx=None):
        """SegmentQuadtree(boundary): every surface of a 2-D PointBoundary is one loop, in the boundary's order."""
        loops = [s.points() for s in boundary.surfaces.values()]
        if not loops or any(l.shape[1] != 2 for l in loops):
            raise WtpArgumentError("SegmentQuadtree.from_boundary needs a 2-D PointBoundary")
        return cls(loops, ctx=ctx)

    # the loops live in a context; another quadtree (or context) re-uploads on first use
    def _resident(self, ctx=None):
        ctx = ctx or self._ctx or default_context()
        if getattr(ctx, "_loops_owner", None) is not self._token:
            ctx.loops_set(self.loops)
            ctx._loops_owner = self._token
        return ctx

    def __len__(self):
        return self._n

    num_segments = property(lambda self: self._n)

    def bounds(self):
        return self.bbox_min.copy(), self.bbox_max.copy()

    def query(self, pts, want=("sd", "seg", "closest", "inside"), ctx=None):
        pts = np.asarray(pts)
        single = pts.ndim == 1
        out = self._resident(ctx).loops_query(np.atleast_2d(pts), want)
        return {k: v[0] for k, v in out.items()} if single else out

    def isinside(self, pts, ctx=None):
        """isinside(point(s), quadtree): inside the box and signed distance < 0."""
        return self.query(pts, want=("inside",), ctx=ctx)["inside"]

    def signed_distance(self, pts, ctx=None):
        """Negative inside the domain, from the closest feature's (pseudo)normal."""
        return self.query(pts, want=("sd",), ctx=ctx)["sd"]

    def nearest_segment(self, pts, ctx=None):
        q = self.query(pts, want=("seg", "closest"), ctx=ctx)
        return q["seg"], q["closest"]
