"""Case table and numpy model of the node octree (include/wtp.h: wtp_node_tree_build, _get, _locate).  Shared by
test_node_tree_cases.py (no GPU: every case has the property it is there for, the two balance orders agree) and
test_gpu_node_tree.py (the device equals the model).

The model follows the header word for word, in the mesh's type T.  The signed distance and the spacing law are
parameters: without a GPU they are oracle.mesh_query and law_h below; the GPU tests pass the library's own mesh_query
and spacing_eval, because the BoundaryLayer law agrees with numpy only to 4 ulp and a refinement
decision must not hang on that.

  build()    refinement level by level (a box's verdict depends on the box alone, so this is the reference's recursion),
             then the balance in Jacobi rounds (every leaf decides on the tree the round began with: the library's),
             then the leaf classes, h, the leaf order and the info
  balance_in_place()   the reference's sweep: leaves in creation order, each deciding on the tree as it stands

Classes: 0 exterior, 1 boundary, 2 interior."""
from __future__ import annotations

import functools
import math
import os

import numpy as np

import oracle
from surface_sampling_cases import F32, F64, DTYPES, GOLD, cube
from volume_fill_cases import needle

EXT, BND, INT = 0, 1, 2
MAX_DEPTH = 20

# _box_probe_points: per axis 0 = lo, 1 = hi, 2 = mid; the point m, 8 corners, 6 face centres, 12 edge midpoints
_CORNERS = [(m & 1, (m >> 1) & 1, (m >> 2) & 1) for m in range(8)]
PROBES = [(2, 2, 2)] + _CORNERS + [(0, 2, 2), (1, 2, 2), (2, 0, 2), (2, 1, 2), (2, 2, 0), (2, 2, 1)] + [
    (2, 0, 0), (2, 1, 0), (2, 0, 1), (2, 1, 1), (0, 2, 0), (1, 2, 0), (0, 2, 1), (1, 2, 1), (0, 0, 2), (1, 0, 2), (0, 1, 2),
    (1, 1, 2)]


@functools.lru_cache(maxsize=None)
def _cavity():
    z = np.load(os.path.join(GOLD, "cavity_mesh.npz"))
    return z["vertices"].astype(F64), z["triangles"].astype(np.int32)


# ---- the cases --------------------------------------------------------------------------------------------------------
# spacing: ("const", h) | ("bl", at_wall, bulk, layer_thickness, points) | ("loglike", base, growth, points), the points an
# array or a function dtype -> points.  h is chosen so that h_box = 1.02 / 2^d (2.04 / 2^d for the cavity) never equals
# alpha h.
def chain_cells(depth=6):
    """Cells of a chain of nested boxes, depth k = 0 .. depth - 1: the root, its child (0, 0, 0), then always the child
    (1, 1, 1), so that every box of the chain touches the faces of its parent's siblings."""
    cells = [(0, 0, 0), (0, 0, 0)]
    while len(cells) < depth:
        cells.append(tuple(2 * x + 1 for x in cells[-1]))
    return cells[:depth]


def chain_points(dtype, depth=6):
    """The centres of the chain's boxes in the unit cube's tree, as the tree computes them."""
    v, _ = cube()
    v = v.astype(dtype)
    root = root_of(v.min(axis=0), v.max(axis=0), dtype, 1.0e-6)
    return np.concatenate([bounds(root, k, np.array([c]))[2] for k, c in enumerate(chain_cells(depth))])


# The refinement looks at a box's centre only, so a layer shorter than a box is seen only where a centre falls into it.
# The law's boundary is therefore the centres of a chain of nested boxes that closes in on the cube's centre from below:
# each box of the chain sees h(0) = at_wall + 0.047 (bulk - at_wall) = 0.0152 and splits while h_box > 0.0304, down to depth
# 6; every sibling sees the bulk value 0.3 and stops (1.02 / 2 < 0.6).  A sibling then lies face to face with a box four
# levels deeper, and the balance has to ripple outward round by round.
_CHAIN = ("bl", 0.001, 0.3, 0.001, chain_points)
CASES = {
    # uniform at depth 3; the root box is the cube widened by 1 %, so every outer cell holds a face and no leaf is exterior
    # (an exterior box is never refined: a uniform tree has none)
    "cube_uniform": dict(mesh=cube, spacing=("const", 0.1), alpha=2.0, ratio=1.0e-6),
    # a slab: the root is a cube over the longest edge; what lies above the slab is exterior and stays coarse
    "slab": dict(mesh=lambda: cube((1.0, 1.0, 0.3)), spacing=("const", 0.1), alpha=2.0, ratio=1.0e-6),
    # so coarse that the root is the only leaf
    "cube_shallow": dict(mesh=cube, spacing=("const", 1.0), alpha=2.0, ratio=1.0e-6),
    "corner_graded": dict(mesh=cube, spacing=_CHAIN, alpha=2.0, ratio=1.0e-6),
    # 0.24 % of its box.  Its four faces are long triangles whose bounding boxes cover the unit cube, so touch holds for
    # every box: refinement goes on where all 27 probes are exterior, and every leaf is demoted to BOUNDARY
    "needle": dict(mesh=needle, spacing=("const", 0.04), alpha=2.0, ratio=1.0e-6),
    "cavity": dict(mesh=_cavity, spacing=("const", 0.1), alpha=2.0, ratio=1.0e-6, dtypes=[F32]),
    # the chain again, but absolute_min = 0.05 diagonal = 0.088 ends it at depth 4 (h_box = 0.064) where the law wants 6
    "min_ratio_stop": dict(mesh=cube, spacing=_CHAIN, alpha=2.0, ratio=0.05),
    "cube_far": dict(mesh=lambda: cube(shift=1000.0), spacing=("const", 0.1), alpha=2.0, ratio=1.0e-6, dtypes=[F32]),
    # LogLike: h = 0.3 d / (0.24 + d) falls to zero at its point, so h_box > 0.5 h holds all the way down: the depth cap
    # (absolute_min is 1.8e-9, below h_box(20) = 9.7e-7) is what ends the refinement about the point.  In Float32 the
    # deepest leaves' h lies under sqrt(eps) = 3.5e-4 and is clamped; in Float64 (1.5e-8) none is.
    "deep_loglike": dict(mesh=cube, spacing=("loglike", 0.3, 1.2, lambda dtype: np.full((1, 3), 0.3, dtype=dtype)), alpha=0.5,
                         ratio=1.0e-9),
    # the law's point is the centre of the chain's depth-3 box: d = 0 there, h = 0 <= eps, the box refuses to split while
    # its siblings go on to depth 5, and the balance has to split it
    "loglike_on_centre": dict(mesh=cube, spacing=("loglike", 0.3, 1.2, lambda dtype: chain_points(dtype, 4)[3:4]), alpha=0.5,
                              ratio=1.0e-9),
    # the same point under alpha = 1: the depth-3 box stays a leaf, INTERIOR, with h clamped to sqrt(eps).  In Float64 its
    # weight (0.1275 / 1.5e-8)^3 = 6e20 leaves every other interior leaf an integer share floor(w / W 2^32) of zero
    "loglike_heavy_leaf": dict(mesh=cube, spacing=("loglike", 0.3, 1.2, lambda dtype: chain_points(dtype, 4)[3:4]), alpha=1.0,
                               ratio=1.0e-9),
    # ... and the root's centre: the tree is the root alone
    "loglike_root_centre": dict(mesh=cube, spacing=("loglike", 0.3, 1.2, lambda dtype: chain_points(dtype, 1)[0:1]), alpha=0.5,
                                ratio=1.0e-9),
}
# Cases too large for the set model and the parametrised tests (build_arrays below; test_gpu_node_tree_edges.py), Float32.
BIG_CASES = {
    # 36 864 internal boxes at depth 6: the level-7 pass is 294 912 = 2^18 + 32 768 boxes, the tree 309 968 leaves
    "slab_fine": dict(mesh=lambda: cube((1.0, 1.0, 0.14)), spacing=("const", 0.006), alpha=2.0, ratio=1.0e-6, dtypes=[F32]),
    # the same slab under LogLike(0.006, 1.2) about a point whose level-7 boxes come in the second chunk of that front:
    # h falls below h_box(7) / 2 within 0.0095 of it, so a few boxes of the ragged chunk, and none of the full one, pass the
    # size tests and are probed; the refinement goes on about the point until absolute_min ends it
    "slab_fine_point": dict(mesh=lambda: cube((1.0, 1.0, 0.14)), spacing=("loglike", 0.006, 1.2, np.array([[0.9, 0.9, 0.07]])),
                            alpha=2.0, ratio=1.0e-6, dtypes=[F32]),
    # uniform at depth 7: 2 097 152 leaves, 8 full chunks
    "cube_depth7": dict(mesh=cube, spacing=("const", 0.006), alpha=2.0, ratio=1.0e-6, dtypes=[F32]),
}
CHUNK = 1 << 18                                                       # kNtChunk of csrc/wtp_node_tree.hip


def case_of(name):
    return CASES[name] if name in CASES else BIG_CASES[name]


def case_dtypes(name):
    return case_of(name).get("dtypes", DTYPES)


@functools.lru_cache(maxsize=None)
def mesh_of(name, dtype):
    v, t = case_of(name)["mesh"]()
    return np.ascontiguousarray(v.astype(dtype)), np.ascontiguousarray(t)


def spacing_of(name, dtype):
    """The case's spacing with its boundary points as an array of `dtype`."""
    sp = case_of(name)["spacing"]
    if sp[0] == "const":
        return sp
    pts = sp[-1](dtype) if callable(sp[-1]) else sp[-1]
    return sp[:-1] + (np.ascontiguousarray(np.asarray(pts, dtype=dtype)),)


def library_spacing(wtp, name, dtype):
    sp = spacing_of(name, dtype)
    if sp[0] == "const":
        return sp[1]
    if sp[0] == "loglike":
        return wtp.LogLike(sp[3], sp[1], sp[2])
    return wtp.BoundaryLayerSpacing(sp[4], sp[1], sp[2], sp[3])


def law_h(sp, c):
    """The spacing law at positions c, term by term in c's dtype (csrc/wtp_spacing.hip spacing_law)."""
    T = c.dtype.type
    if sp[0] == "const":
        return np.full(len(c), T(sp[1]), dtype=c.dtype)
    d2 = None
    for q in np.asarray(sp[-1], dtype=c.dtype):
        dx, dy, dz = c[:, 0] - q[0], c[:, 1] - q[1], c[:, 2] - q[2]
        e = (dx * dx + dy * dy) + dz * dz
        d2 = e if d2 is None else np.minimum(d2, e)
    d = np.sqrt(d2)
    if sp[0] == "loglike":                                            # base d / (a + d), a = base (1 - (growth - 1))
        base, growth = T(sp[1]), T(sp[2])
        inv_growth = T(1) - (growth - T(1))
        a = base * inv_growth
        return base * d / (a + d)
    p0, p1, p2 = T(sp[1]), T(sp[2]), T(sp[3])
    center, width = p2 / T(2), p2 / T(6)
    with np.errstate(over="ignore"):
        sig = T(1) / (T(1) + np.exp(-(d - center) / width))
    return p0 + (p1 - p0) * sig


# ---- geometry, in T -------------------------------------------------------------------------------------------------
def root_of(lo, hi, dtype, ratio):
    """The root box from the mesh's vertex box (wtp_mesh_bounds): dict(org (3,), size, absmin), all of type T."""
    T = np.dtype(dtype).type
    lo, hi = np.asarray(lo, dtype=dtype), np.asarray(hi, dtype=dtype)
    centre = (lo + hi) * T(0.5)
    half = ((hi - lo) * T(0.5)) * T(1.02)
    org, top = centre - half, centre + half
    size = (top - org).max()
    e = (org + size) - org
    diag = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return dict(org=org, size=size, absmin=diag * T(ratio), T=T)


def h_box(root, d):
    return root["size"] / root["T"](1 << d)


def bounds(root, d, c):
    """(lo, hi, centre) of boxes (d, c[n, 3]) as box_bounds and box_center compute them."""
    T, h = root["T"], h_box(root, d)
    c = np.asarray(c, dtype=np.int64).reshape(-1, 3)
    lo = root["org"] + c.astype(T) * h
    hi = lo + h
    ctr = root["org"] + ((2 * c + 1).astype(T) * h) / T(2)
    return lo, hi, ctr


def tol_of(root, d):
    T = root["T"]
    return max(T(1.0e-8), h_box(root, d) * T(1.0e-6))


def probe_points(lo, hi, sel, first=None):
    """(n, len(sel), 3): the probes of `sel` for every box; `first`, if given, replaces the first probe."""
    mid = (lo + hi) / lo.dtype.type(2)
    src = np.stack([lo, hi, mid])  # (3, n, 3)
    out = np.empty((len(lo), len(sel), 3), dtype=lo.dtype)
    for p, s in enumerate(sel):
        for a in range(3):
            out[:, p, a] = src[s[a], :, a]
    if first is not None:
        out[:, 0] = first
    return out


class Geometry:
    """What the model asks of the mesh: cls(p, tol) and touch(box)."""

    def __init__(self, verts, tris, sd_fn=None, bbox=None):
        self.v, self.t = verts, tris
        self.T = verts.dtype.type
        bb = oracle.mesh_bbox(verts) if bbox is None else np.concatenate([np.asarray(b, dtype=verts.dtype) for b in bbox])
        self.lo, self.hi = bb[:3], bb[3:]
        self.sd_fn = sd_fn or (lambda p: oracle.mesh_query(verts, tris, p)["sd"])
        tv = verts[tris]
        self.tlo, self.thi = tv.min(axis=1), tv.max(axis=1)

    def cls(self, p, tol):
        """classify_point for points p (n, 3) with per-point tolerances tol (n,) or one."""
        p = np.asarray(p, dtype=self.v.dtype).reshape(-1, 3)
        tol = np.broadcast_to(np.asarray(tol, dtype=self.v.dtype), (len(p),))
        out = ((p < self.lo - tol[:, None]) | (p > self.hi + tol[:, None])).any(axis=1)
        res = np.zeros(len(p), dtype=np.int8)
        idx = np.nonzero(~out)[0]
        if len(idx):
            sd = np.asarray(self.sd_fn(np.ascontiguousarray(p[idx])))
            res[idx] = np.where(np.abs(sd) <= tol[idx], BND, np.where(sd < 0, INT, EXT))
        return res

    def touch(self, lo, hi):
        """Per box: does some triangle's bounding box overlap the closed box?  Brute force."""
        out = np.zeros(len(lo), dtype=bool)
        for i in range(0, len(lo), 2048):
            a, b = lo[i:i + 2048, None, :], hi[i:i + 2048, None, :]
            apart = (a > self.thi[None]) | (b < self.tlo[None])
            out[i:i + 2048] = (~apart.any(axis=2)).any(axis=1)
        return out


# ---- keys -----------------------------------------------------------------------------------------------------------
def _spread(v):
    x = np.asarray(v, dtype=np.uint64) & np.uint64(0x1FFFFF)
    for s, m in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3),
                 (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(s))) & np.uint64(m)
    return x


def morton_start(d, c):
    """Morton key (x lowest bit) of the lower corner at depth 20 of boxes (d[n], c[n, 3])."""
    d, c = np.asarray(d, dtype=np.int64), np.asarray(c, dtype=np.int64).reshape(-1, 3)
    m = _spread(c[:, 0]) | (_spread(c[:, 1]) << np.uint64(1)) | (_spread(c[:, 2]) << np.uint64(2))
    return m << (np.uint64(3) * (MAX_DEPTH - d).astype(np.uint64))


def children_of(c):
    return [(2 * c[0] + (m & 1), 2 * c[1] + ((m >> 1) & 1), 2 * c[2] + ((m >> 2) & 1)) for m in range(8)]


# ---- the model --------------------------------------------------------------------------------------------------------
def refine(root, geo, h_fn, alpha):
    """_subdivide_node_octree! from the root.  Returns (leaves, internal, order, facts): sets of (d, cell), the boxes in
    creation order, and facts["touch_only"] = boxes subdivided although none of their 27 probes was non-exterior."""
    T = root["T"]
    eps = np.finfo(T).eps
    leaves, internal, order = set(), set(), [(0, (0, 0, 0))]
    front = [(0, 0, 0)]
    touch_only = 0
    d = 0
    while front:
        c = np.array(front, dtype=np.int64)
        lo, hi, ctr = bounds(root, d, c)
        hb = h_box(root, d)
        h = np.asarray(h_fn(np.ascontiguousarray(ctr)), dtype=T)
        assert np.isfinite(h).all()
        size_ok = np.full(len(c), d < MAX_DEPTH and hb > root["absmin"]) & (h > eps) & (hb > T(alpha) * h)
        split = np.zeros(len(c), dtype=bool)
        idx = np.nonzero(size_ok)[0]
        if len(idx):
            pts = probe_points(lo[idx], hi[idx], PROBES)
            k = geo.cls(pts.reshape(-1, 3), np.repeat(np.full(len(idx), tol_of(root, d), dtype=T), 27)).reshape(-1, 27)
            seen = (k != EXT).any(axis=1)
            rest = idx[~seen]
            touched = geo.touch(lo[rest], hi[rest]) if len(rest) else np.zeros(0, dtype=bool)
            split[idx[seen]] = True
            split[rest[touched]] = True
            touch_only += int(touched.sum())
        nxt = []
        for cell, s in zip(front, split):
            if s:
                internal.add((d, cell))
                kids = children_of(cell)
                nxt.extend(kids)
                order.extend((d + 1, k) for k in kids)
            else:
                leaves.add((d, cell))
        front, d = nxt, d + 1
    return leaves, internal, order, dict(touch_only=touch_only)


def needs_balancing(box, internal):
    d, c = box
    for a in range(3):
        for s in (-1, 1):
            nc = list(c)
            nc[a] += s
            if nc[a] < 0 or nc[a] >= (1 << d):
                continue
            nb = (d, tuple(nc))
            if nb in internal and any((d + 1, k) in internal for k in children_of(nb[1])):
                return True
    return False


def can_subdivide(root, d):
    return d < MAX_DEPTH and h_box(root, d) > root["absmin"]


def balance_jacobi(root, leaves, internal):
    """Rounds in which every leaf decides on the tree the round began with.  Returns (leaves, internal, rounds, n_split,
    n_blocked): rounds counts the last, empty one; n_blocked = leaves that needed balancing but may not subdivide."""
    leaves, internal = set(leaves), set(internal)
    rounds = n_split = n_blocked = 0
    while True:
        rounds += 1
        assert rounds <= 100
        want = [b for b in leaves if needs_balancing(b, internal)]
        todo = [b for b in want if can_subdivide(root, b[0])]
        n_blocked += len(want) - len(todo)
        if not todo:
            return leaves, internal, rounds, n_split, n_blocked
        for b in todo:
            leaves.remove(b)
            internal.add(b)
            leaves.update((b[0] + 1, k) for k in children_of(b[1]))
        n_split += len(todo)


def balance_in_place(root, leaves, internal, order):
    """balance_octree!: sweeps over the boxes in creation order, every leaf deciding on the tree as it stands."""
    leaves, internal, order = set(leaves), set(internal), list(order)
    for _ in range(100):
        any_split = False
        for b in order[:len(order)]:
            if b in leaves and needs_balancing(b, internal) and can_subdivide(root, b[0]):
                leaves.remove(b)
                internal.add(b)
                kids = [(b[0] + 1, k) for k in children_of(b[1])]
                leaves.update(kids)
                order.extend(kids)
                any_split = True
        if not any_split:
            return leaves, internal
    raise AssertionError("balance did not settle")


def classify(root, geo, d, c):
    """_classify_leaf_conservative, then the touch demotion.  Returns (class int8[n], vote int8[n], touched bool[n])."""
    T = root["T"]
    d, c = np.asarray(d), np.asarray(c).reshape(-1, 3)
    vote = np.empty(len(d), dtype=np.int8)
    touched = np.zeros(len(d), dtype=bool)
    for depth in np.unique(d):
        idx = np.nonzero(d == depth)[0]
        lo, hi, ctr = bounds(root, int(depth), c[idx])
        pts = probe_points(lo, hi, PROBES[:9], first=ctr)
        k = geo.cls(pts.reshape(-1, 3), np.repeat(np.full(len(idx), tol_of(root, int(depth)), dtype=T), 9)).reshape(-1, 9)
        same = (k == k[:, :1]).all(axis=1)
        vote[idx] = np.where((k == BND).any(axis=1) | ~same, BND, k[:, 0])
        touched[idx] = geo.touch(lo, hi)
    return np.where(touched, BND, vote).astype(np.int8), vote, touched


def build(verts, tris, spacing_fn, alpha, ratio, sd_fn=None, bbox=None):
    """The whole of wtp_node_tree_build.  spacing_fn(points (n, 3) of T) -> h (n,) of T."""
    dtype = verts.dtype
    T = dtype.type
    geo = Geometry(verts, tris, sd_fn, bbox)
    root = root_of(geo.lo, geo.hi, dtype, ratio)
    leaves0, internal0, order, facts = refine(root, geo, spacing_fn, alpha)
    leaves, internal, rounds, n_split, n_blocked = balance_jacobi(root, leaves0, internal0)
    d = np.array([b[0] for b in leaves], dtype=np.int32)
    c = np.array([b[1] for b in leaves], dtype=np.int32).reshape(-1, 3)
    o = np.argsort(morton_start(d, c), kind="stable")
    d, c = d[o], c[o]
    cls, vote, touched = classify(root, geo, d, c)
    ctr = _centres(root, d, c)
    hraw = np.asarray(spacing_fn(np.ascontiguousarray(ctr)), dtype=dtype)
    assert np.isfinite(hraw).all()
    h = np.maximum(hraw, np.sqrt(np.finfo(T).eps).astype(dtype))
    hb = np.array([h_box(root, int(x)) for x in d], dtype=dtype)
    live = cls != EXT
    terms = ((hb * hb) * hb) / ((h * h) * h)
    integral = math.fsum(float(x) for x in terms[live])
    info = dict(n_leaves=len(d), n_interior=int((cls == INT).sum()), n_boundary=int((cls == BND).sum()),
                n_exterior=int((cls == EXT).sum()), n_boxes=len(leaves) + len(internal), depth_max=int(d.max()),
                n_levels=int(d.max()) + 1, balance_rounds=rounds, integral=integral,
                h_min=float(h[live].min()) if live.any() else 0.0,
                origin=tuple(float(x) for x in root["org"]), root_size=float(root["size"]), absolute_min=float(root["absmin"]))
    facts.update(balance_splits=n_split, balance_blocked=n_blocked, demoted=int((touched & (vote != BND)).sum()),
                 demoted_interior=int((touched & (vote == INT)).sum()), depth_before_balance=max(b[0] for b in leaves0))
    return dict(cell=c, depth=d, cls=cls, h=h, info=info, facts=facts, root=root, geo=geo, leaves=leaves, internal=internal,
                leaves0=leaves0, internal0=internal0, order=order, terms=terms)


def _centres(root, d, c):
    out = np.empty((len(d), 3), dtype=root["org"].dtype)
    for depth in np.unique(d):
        idx = np.nonzero(d == depth)[0]
        out[idx] = bounds(root, int(depth), c[idx])[2]
    return out


def locate(model, pts):
    """find_leaf for points (n, 3), converted to T: the leaf's index in leaf order; -1 outside the root box or NaN."""
    root = model["root"]
    T = root["T"]
    pts = np.asarray(pts).astype(root["org"].dtype).reshape(-1, 3)
    index = {(int(d), tuple(int(x) for x in c)): i for i, (d, c) in enumerate(zip(model["depth"], model["cell"]))}
    out = np.empty(len(pts), dtype=np.int64)
    top = root["org"] + root["size"]
    for i, p in enumerate(pts):
        if not ((p >= root["org"]) & (p <= top)).all():
            out[i] = -1
            continue
        d, c = 0, (0, 0, 0)
        while (d, c) in model["internal"]:
            ctr = bounds(root, d, np.array([c]))[2][0]
            c = tuple(2 * c[a] + (1 if p[a] >= ctr[a] else 0) for a in range(3))
            d += 1
        out[i] = index[(d, c)]
    return out


@functools.lru_cache(maxsize=None)
def model_run(name, dtype):
    """The case's model with the oracle's signed distance and the numpy law."""
    case = CASES[name]
    v, t = mesh_of(name, dtype)
    sp = spacing_of(name, dtype)
    return build(v, t, lambda p: law_h(sp, p), case["alpha"], case["ratio"])


@functools.lru_cache(maxsize=None)
def model_run_arrays(name, dtype):
    """The same through build_arrays; the only model of BIG_CASES["slab_fine"]."""
    case = case_of(name)
    v, t = mesh_of(name, dtype)
    sp = spacing_of(name, dtype)
    return build_arrays(v, t, lambda p: law_h(sp, p), case["alpha"], case["ratio"])


def locate_points(model):
    """Points that try find_leaf: every leaf centre; the child-splitting planes of the root and of a deepest internal box,
    where >= decides; the root's faces and corners; points outside the root and a NaN."""
    root = model["root"]
    T = root["T"]
    ctr = _centres(root, model["depth"], model["cell"])
    org, size = root["org"], root["size"]
    top = org + size
    pts = [ctr]
    d, c = max(model["internal"]) if model["internal"] else (0, (0, 0, 0))
    for dd, cc in ((0, (0, 0, 0)), (d, c)):
        lo, hi, m = (x[0] for x in bounds(root, dd, np.array([cc])))
        for a in range(3):
            p = np.array([m, m, m])
            p[1, a] = np.nextafter(m[a], T(-np.inf))
            p[2, a] = np.nextafter(m[a], T(np.inf))
            pts.append(p)
        pts.append(probe_points(lo[None], hi[None], PROBES)[0])
    pts.append(probe_points(org[None], top[None], PROBES)[0])
    out = np.array([org - T(1.0e-3) * size, top + T(1.0e-3) * size, [org[0], org[1], np.nextafter(top[2], T(np.inf))],
                    [np.nextafter(org[0], T(-np.inf)), org[1], org[2]], [np.nan, org[1], org[2]]], dtype=ctr.dtype)
    pts.append(out)
    return np.ascontiguousarray(np.concatenate(pts).astype(ctr.dtype))


# ---- the placements (include/wtp.h: wtp_node_place) ---------------------------------------------------------------------
PLACEMENTS = {"random": 0, "jittered": 1, "lattice": 2}
ST_INTERIOR, ST_CANDIDATES, ST_DEFICIT, ST_PICK_INTERIOR, ST_PICK_CANDIDATES, ST_PICK_DEFICIT = range(6)
_M64 = (1 << 64) - 1


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw(seed, stage, j, a):
    """r(stage, j, a) as a Python integer."""
    return _splitmix64(((seed << 40) + 3 * ((stage << 36) + int(j)) + a) & _M64)


def uniform(dtype, seed, stage, j, a):
    return dtype(np.float32(draw(seed, stage, j, a) >> 40) * np.float32(2.0 ** -24))


def grid_divisions(n):
    """The smallest g with g^3 >= n."""
    g = 1
    while g ** 3 < n:
        g += 1
    return g


def pick_table(F):
    """(cum, F_total) of integer shares F (uint64)."""
    cum = np.cumsum(F.astype(np.uint64), dtype=np.uint64)
    return cum, int(cum[-1]) if len(cum) else 0


def pick(cum, f_total, x):
    """The first leaf with cum_i > mulhi64(x, F_total)."""
    return int(np.searchsorted(cum, np.uint64((x * f_total) >> 64), side="right"))


def group_counts(w, W, member, count, seed, stage):
    """_allocate_counts_by_volume as the header states it: counts per leaf (zeros outside the group)."""
    counts = np.zeros(len(w), dtype=np.int64)
    if count < 1:
        return counts
    expected = float(count) * (w / W)
    base = np.floor(expected)
    counts += base.astype(np.int64)
    leftover = max(0, count - int(counts.sum()))
    cum, f_total = pick_table(np.floor((expected - base) * 4294967296.0).astype(np.uint64))
    if f_total == 0:
        cum, f_total = pick_table(member.astype(np.uint64))
    for t in range(leftover):
        counts[pick(cum, f_total, draw(seed, stage, t, 0))] += 1
    return counts


def leaf_points(model, i, n, j0, placement, seed, stage):
    """The n points of leaf i, the first of them being point j0 of its stage."""
    root = model["root"]
    dtype = root["org"].dtype
    T = dtype.type
    lo, hi, _ = (x[0] for x in bounds(root, int(model["depth"][i]), model["cell"][i][None]))
    e = hi - lo
    out = np.empty((n, 3), dtype=dtype)
    g = grid_divisions(n)
    for k in range(n):
        u = np.array([uniform(T, seed, stage, j0 + k, a) for a in range(3)], dtype=dtype) if placement != 2 else None
        if placement == 0:
            out[k] = lo + u * e
            continue
        cell = np.array([k % g, (k // g) % g, k // (g * g)]).astype(dtype)
        cs = e / T(g)
        cmin = lo + cell * cs
        out[k] = cmin + cs / T(2) if placement == 2 else cmin + u * cs
    return out


def group_points(model, counts, placement, seed, stage):
    xyz, leaf, j0 = [], [], 0
    for i in np.nonzero(counts)[0]:
        xyz.append(leaf_points(model, i, int(counts[i]), j0, placement, seed, stage))
        leaf.append(np.full(int(counts[i]), i, dtype=np.int64))
        j0 += int(counts[i])
    dtype = model["root"]["org"].dtype
    return (np.concatenate(xyz) if xyz else np.zeros((0, 3), dtype=dtype)), (np.concatenate(leaf) if leaf else np.zeros(0, dtype=np.int64))


def place(model, placement, max_points, oversampling, seed, inside_fn, W=None):
    """wtp_node_place.  W: the (W_int, W_ns) everything is defined from (the library's reported values), or None for the
    model's own sums.  inside_fn(points) -> bool per point (wtp_mesh_query's inside flag)."""
    placement = PLACEMENTS.get(placement, placement)
    w = model["terms"].astype(np.float64)
    interior, near = model["cls"] == INT, model["cls"] == BND
    w_int, w_ns = np.where(interior, w, 0.0), np.where(near, w, 0.0)
    W_int, W_ns = W if W is not None else (math.fsum(w_int), math.fsum(w_ns))
    dtype = model["root"]["org"].dtype
    info = dict(n_points=0, n_interior=0, n_candidates=0, n_accepted=0, n_deficit=0, W_int=W_int, W_ns=W_ns, placement=placement)
    if not W_int + W_ns > 0:
        return dict(xyz=np.zeros((0, 3), dtype=dtype), leaf=np.zeros(0, dtype=np.int64), info=info, candidates=None)
    n_int = int(np.rint(float(max_points) * (W_int / (W_int + W_ns))))
    n_ns = max_points - n_int
    n_cand = int(np.rint(float(n_ns) * oversampling))
    c_int = group_counts(w_int, W_int, interior, n_int, seed, ST_PICK_INTERIOR)
    assert c_int.sum() == n_int and not c_int[~interior].any()       # the weighted pick hands out exactly count
    xyz, leaf = group_points(model, c_int, placement, seed, ST_INTERIOR)
    c_ns = group_counts(w_ns, W_ns, near, n_cand, seed, ST_PICK_CANDIDATES)
    assert c_ns.sum() == n_cand and not c_ns[~near].any()
    cand, cleaf = group_points(model, c_ns, placement, seed, ST_CANDIDATES)
    inside = np.asarray(inside_fn(cand), dtype=bool) if len(cand) else np.zeros(0, dtype=bool)
    take = np.nonzero(inside)[0][:max_points - n_int]
    parts_x, parts_l = [xyz, cand[take]], [leaf, cleaf[take]]
    so_far = n_int + len(take)
    n_def = 0
    if so_far < max_points and W_int > 0:
        n_def = max_points - so_far
        cum, f_total = pick_table(np.floor((w_int / W_int) * 4294967296.0).astype(np.uint64))
        if f_total == 0:
            cum, f_total = pick_table(interior.astype(np.uint64))
        T = dtype.type
        dx, dl = np.empty((n_def, 3), dtype=dtype), np.empty(n_def, dtype=np.int64)
        for t in range(n_def):
            i = pick(cum, f_total, draw(seed, ST_PICK_DEFICIT, t, 0))
            lo, hi, _ = (x[0] for x in bounds(model["root"], int(model["depth"][i]), model["cell"][i][None]))
            u = np.array([uniform(T, seed, ST_DEFICIT, t, a) for a in range(3)], dtype=dtype)
            dx[t], dl[t] = lo + u * (hi - lo), i
        parts_x.append(dx), parts_l.append(dl)
    info.update(n_points=so_far + n_def, n_interior=n_int, n_candidates=n_cand, n_accepted=len(take), n_deficit=n_def)
    return dict(xyz=np.concatenate(parts_x), leaf=np.concatenate(parts_l), info=info, candidates=(cand, cleaf, inside))


def oracle_inside(name, dtype):
    v, t = mesh_of(name, dtype)
    return lambda p: oracle.mesh_query(v, t, p)["inside"]


def in_leaf(model, xyz, leaf):
    """Does every point lie in the closed box of the leaf named for it?"""
    root = model["root"]
    ok = np.ones(len(xyz), dtype=bool)
    for i in np.unique(leaf):
        lo, hi, _ = (x[0] for x in bounds(root, int(model["depth"][i]), model["cell"][i][None]))
        sel = leaf == i
        ok[sel] = ((xyz[sel] >= lo) & (xyz[sel] <= hi)).all(axis=1)
    return ok


def on_cell_centres(model, xyz, leaf):
    """Lattice points of whole leaves (every point of a leaf present): do they sit on the centres of the leaf's g^3 cells?"""
    root = model["root"]
    ok = np.ones(len(xyz), dtype=bool)
    for i in np.unique(leaf):
        lo, hi, _ = (x[0] for x in bounds(root, int(model["depth"][i]), model["cell"][i][None]))
        sel = leaf == i
        g = grid_divisions(int(sel.sum()))
        f = (xyz[sel].astype(F64) - lo) / ((hi - lo).astype(F64) / g) - 0.5
        ok[sel] = (np.abs(f - np.rint(f)) < 1e-3).all(axis=1) & (np.rint(f) >= 0).all(axis=1) & (np.rint(f) < g).all(axis=1)
    return ok


# ---- the same two models on arrays ------------------------------------------------------------------------------------
# build() and place() above are the definition.  Their sets of tuples and per-point Python integers cannot replay 3e5
# leaves or 1e6 points in a test's time; build_arrays() and place_arrays() follow the same words of include/wtp.h on
# numpy arrays and are proved equal to them, byte for byte, by test_node_tree_cases.py.
def box_code(d, c):
    """One uint64 per box (d[n], c[n, 3]): its Morton code at its own depth, a one behind it, zeros up to depth 20 (the
    library's key).  Distinct boxes have distinct codes."""
    d, c = np.asarray(d, dtype=np.int64), np.asarray(c, dtype=np.int64).reshape(-1, 3)
    m = _spread(c[:, 0]) | (_spread(c[:, 1]) << np.uint64(1)) | (_spread(c[:, 2]) << np.uint64(2))
    return ((m << np.uint64(1)) | np.uint64(1)) << (np.uint64(3) * (MAX_DEPTH - d).astype(np.uint64))


def _children(c):
    """(8 n, 3): the children of cells c (n, 3), each parent's eight together in child order."""
    m = np.array(_CORNERS, dtype=np.int64)
    return (2 * np.asarray(c, dtype=np.int64)[:, None, :] + m[None]).reshape(-1, 3)


def refine_arrays(root, geo, h_fn, alpha):
    """refine() level by level on arrays.  Returns (leaf depths, leaf cells, internal depths, internal cells, facts);
    facts["fronts"] = boxes looked at per level, facts["wanted"] = per level, which of them passed the size tests."""
    T = root["T"]
    eps = np.finfo(T).eps
    ld, lc, idp, ic, fronts, wanted = [], [], [], [], [], []
    c = np.zeros((1, 3), dtype=np.int64)
    touch_only, d = 0, 0
    while len(c):
        fronts.append(len(c))
        lo, hi, ctr = bounds(root, d, c)
        hb = h_box(root, d)
        h = np.asarray(h_fn(np.ascontiguousarray(ctr)), dtype=T)
        assert np.isfinite(h).all()
        size_ok = np.full(len(c), d < MAX_DEPTH and hb > root["absmin"]) & (h > eps) & (hb > T(alpha) * h)
        split = np.zeros(len(c), dtype=bool)
        idx = np.nonzero(size_ok)[0]
        wanted.append(idx)
        for i0 in range(0, len(idx), CHUNK):
            part = idx[i0:i0 + CHUNK]
            pts = probe_points(lo[part], hi[part], PROBES)
            k = geo.cls(pts.reshape(-1, 3), np.repeat(np.full(len(part), tol_of(root, d), dtype=T), 27)).reshape(-1, 27)
            seen = (k != EXT).any(axis=1)
            rest = part[~seen]
            touched = geo.touch(lo[rest], hi[rest]) if len(rest) else np.zeros(0, dtype=bool)
            split[part[seen]] = True
            split[rest[touched]] = True
            touch_only += int(touched.sum())
        ld.append(np.full(int((~split).sum()), d, dtype=np.int64)), lc.append(c[~split])
        idp.append(np.full(int(split.sum()), d, dtype=np.int64)), ic.append(c[split])
        c, d = _children(c[split]), d + 1
    return np.concatenate(ld), np.concatenate(lc), np.concatenate(idp), np.concatenate(ic), dict(touch_only=touch_only, fronts=fronts, wanted=wanted)


def needs_balancing_arrays(d, c, int_d, int_c):
    """needs_balancing() of every leaf (d[n], c[n, 3]): a face neighbour of its own depth is internal and has an internal
    child, which is to say that it is the parent of an internal box.  Set membership over sorted codes."""
    deep = int_d >= 1
    parents = np.unique(box_code(int_d[deep] - 1, int_c[deep] >> 1))
    out = np.zeros(len(d), dtype=bool)
    for a in range(3):
        for s in (-1, 1):
            nc = c.copy()
            nc[:, a] += s
            ok = (nc[:, a] >= 0) & (nc[:, a] < (np.int64(1) << d))
            out[ok] |= np.isin(box_code(d[ok], nc[ok]), parents)
    return out


def balance_arrays(root, ld, lc, idp, ic):
    """balance_jacobi() on arrays.  Returns (leaf depths, leaf cells, internal depths, internal cells, rounds, n_split,
    n_blocked)."""
    may = np.array([can_subdivide(root, d) for d in range(MAX_DEPTH + 1)], dtype=bool)
    rounds = n_split = n_blocked = 0
    while True:
        rounds += 1
        assert rounds <= 100
        want = needs_balancing_arrays(ld, lc, idp, ic)
        todo = want & may[ld]
        n_blocked += int(want.sum() - todo.sum())
        if not todo.any():
            return ld, lc, idp, ic, rounds, n_split, n_blocked
        idp, ic = np.concatenate([idp, ld[todo]]), np.concatenate([ic, lc[todo]])
        ld, lc = np.concatenate([ld[~todo], np.repeat(ld[todo] + 1, 8)]), np.concatenate([lc[~todo], _children(lc[todo])])
        n_split += int(todo.sum())


def finish(root, geo, spacing_fn, d, c, slices=1 << 19):
    """Leaf order, classes, h, the terms and the info's sums of the leaves (d, c), as build() ends; the classes in slices
    of at most `slices` boxes."""
    dtype = root["org"].dtype
    T = dtype.type
    o = np.argsort(morton_start(d, c), kind="stable")
    d, c = np.asarray(d, dtype=np.int32)[o], np.asarray(c, dtype=np.int32).reshape(-1, 3)[o]
    parts = [classify(root, geo, d[i:i + slices], c[i:i + slices]) for i in range(0, len(d), slices)]
    cls, vote, touched = (np.concatenate([p[k] for p in parts]) for k in range(3))
    ctr = _centres(root, d, c)
    hraw = np.asarray(spacing_fn(np.ascontiguousarray(ctr)), dtype=dtype)
    assert np.isfinite(hraw).all()
    h = np.maximum(hraw, np.sqrt(np.finfo(T).eps).astype(dtype))
    hb = (root["size"] / (np.int64(1) << np.arange(MAX_DEPTH + 1)).astype(dtype))[d]
    live = cls != EXT
    terms = ((hb * hb) * hb) / ((h * h) * h)
    return dict(depth=d, cell=c, cls=cls, vote=vote, touched=touched, h=h, hraw=hraw, terms=terms,
                integral=math.fsum(terms[live].astype(F64).tolist()), h_min=float(h[live].min()) if live.any() else 0.0)


def build_arrays(verts, tris, spacing_fn, alpha, ratio, sd_fn=None, bbox=None):
    """build() on arrays.  The result has no sets: internal boxes are model["internal_depth"], ["internal_cell"]."""
    dtype = verts.dtype
    geo = Geometry(verts, tris, sd_fn, bbox)
    root = root_of(geo.lo, geo.hi, dtype, ratio)
    ld0, lc0, id0, ic0, facts = refine_arrays(root, geo, spacing_fn, alpha)
    ld, lc, idp, ic, rounds, n_split, n_blocked = balance_arrays(root, ld0, lc0, id0, ic0)
    f = finish(root, geo, spacing_fn, ld, lc)
    d, cls = f["depth"], f["cls"]
    info = dict(n_leaves=len(d), n_interior=int((cls == INT).sum()), n_boundary=int((cls == BND).sum()),
                n_exterior=int((cls == EXT).sum()), n_boxes=len(ld) + len(idp), depth_max=int(d.max()),
                n_levels=int(d.max()) + 1, balance_rounds=rounds, integral=f["integral"], h_min=f["h_min"],
                origin=tuple(float(x) for x in root["org"]), root_size=float(root["size"]), absolute_min=float(root["absmin"]))
    facts.update(balance_splits=n_split, balance_blocked=n_blocked, demoted=int((f["touched"] & (f["vote"] != BND)).sum()),
                 demoted_interior=int((f["touched"] & (f["vote"] == INT)).sum()), depth_before_balance=int(ld0.max()))
    return dict(cell=f["cell"], depth=d, cls=cls, h=f["h"], info=info, facts=facts, root=root, geo=geo, terms=f["terms"],
                internal_depth=idp, internal_cell=ic, leaves0_depth=ld0, leaves0_cell=lc0)


def uniform_tree(verts, tris, h, depth, ratio, sd_fn=None, bbox=None):
    """The tree whose leaves are every cell of `depth`, under a constant spacing h, in closed form: no refinement is run.
    Leaves in Morton order, one balance round, classes from classify() in slices."""
    dtype = verts.dtype
    geo = Geometry(verts, tris, sd_fn, bbox)
    root = root_of(geo.lo, geo.hi, dtype, ratio)
    n = 8 ** depth
    code = np.arange(n, dtype=np.uint64)
    c = np.stack([_compact(code >> np.uint64(a)) for a in range(3)], axis=1).astype(np.int32)
    f = finish(root, geo, lambda p: np.full(len(p), dtype.type(h), dtype=dtype), np.full(n, depth, dtype=np.int32), c)
    assert np.array_equal(f["cell"], c)
    cls = f["cls"]
    info = dict(n_leaves=n, n_interior=int((cls == INT).sum()), n_boundary=int((cls == BND).sum()), n_exterior=int((cls == EXT).sum()),
                n_boxes=n + (n - 1) // 7, depth_max=depth, n_levels=depth + 1, balance_rounds=1, integral=f["integral"],
                h_min=f["h_min"], origin=tuple(float(x) for x in root["org"]), root_size=float(root["size"]),
                absolute_min=float(root["absmin"]))
    return dict(cell=c, depth=f["depth"], cls=cls, h=f["h"], info=info, root=root, geo=geo, terms=f["terms"])


def _compact(x):
    """Every third bit of x, from bit 0 (the inverse of _spread)."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0x1249249249249249)
    for s, m in ((2, 0x10C30C30C30C30C3), (4, 0x100F00F00F00F00F), (8, 0x1F0000FF0000FF), (16, 0x1F00000000FFFF), (32, 0x1FFFFF)):
        x = (x ^ (x >> np.uint64(s))) & np.uint64(m)
    return x


def leaf_bounds(model, idx):
    """(lo, hi) of the leaves idx[n] as bounds() computes them, one row per entry."""
    root = model["root"]
    dtype = root["org"].dtype
    hb = (root["size"] / (np.int64(1) << np.arange(MAX_DEPTH + 1)).astype(dtype))[model["depth"][idx]]
    lo = root["org"] + model["cell"][idx].astype(np.int64).astype(dtype) * hb[:, None]
    return lo, lo + hb[:, None]


def in_leaf_arrays(model, xyz, leaf):
    lo, hi = leaf_bounds(model, leaf)
    return ((xyz >= lo) & (xyz <= hi)).all(axis=1)


def zero_shares(model, group):
    """How many leaves of class `group` have the integer share floor(w / W 2^32) == 0, and how many leaves it has."""
    w = model["terms"].astype(np.float64)[model["cls"] == group]
    return int((np.floor((w / math.fsum(w)) * 4294967296.0) == 0).sum()), len(w)


def rows_in(a, b):
    """Per row of a (n, 3): is it, byte for byte, a row of b?  A 64-bit hash of the rows' words finds the few rows that
    may be (np.isin over integers); those are then compared as bytes, so the answer is exact."""
    def words(x):
        return np.ascontiguousarray(x).view(np.uint32).reshape(len(x), 3 * x.dtype.itemsize // 4).astype(np.uint64)

    def key(x):
        h = np.zeros(len(x), dtype=np.uint64)
        for col in words(x).T:
            h = splitmix64_arrays(h ^ col)
        return h

    assert a.dtype == b.dtype
    ka, kb = key(a), key(b)
    maybe = np.isin(ka, kb)
    out = np.zeros(len(a), dtype=bool)
    if maybe.any():
        have = {r.tobytes() for r in b[np.isin(kb, ka[maybe])]}
        out[np.nonzero(maybe)[0]] = [r.tobytes() in have for r in a[maybe]]
    return out


_U = np.uint64


def splitmix64_arrays(z):
    z = z + _U(0x9E3779B97F4A7C15)
    z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def draw_arrays(seed, stage, j, a):
    """r(stage, j, a) for j a uint64 array; sums and products wrap at 2^64 as the header's do."""
    return splitmix64_arrays(_U(seed << 40) + _U(3) * (_U(stage << 36) + np.asarray(j, dtype=np.uint64)) + _U(a))


def mulhi64(x, y):
    """floor(x y / 2^64) for a uint64 array x and one y < 2^64, by 32-bit halves."""
    lo32 = _U(0xFFFFFFFF)
    y = _U(y)
    x0, x1, y0, y1 = x & lo32, x >> _U(32), y & lo32, y >> _U(32)
    mid = x1 * y0 + ((x0 * y0) >> _U(32))
    mid2 = x0 * y1 + (mid & lo32)
    return x1 * y1 + (mid >> _U(32)) + (mid2 >> _U(32))


def uniform_arrays(dtype, seed, stage, j, a):
    return ((draw_arrays(seed, stage, j, a) >> _U(40)).astype(np.float32) * np.float32(2.0 ** -24)).astype(dtype)


def grid_divisions_arrays(n):
    """The smallest g with g^3 >= n, per entry of the int64 array n >= 1."""
    g = np.maximum(np.rint(np.cbrt(n.astype(F64))).astype(np.int64), 1)
    for _ in range(3):
        g = np.where(g ** 3 < n, g + 1, g)
    for _ in range(3):
        g = np.where((g - 1) ** 3 >= n, g - 1, g)
    assert ((g ** 3 >= n) & ((g - 1) ** 3 < n)).all()
    return g


def pick_arrays(cum, f_total, x):
    return np.searchsorted(cum, mulhi64(x, f_total), side="right")


def group_counts_arrays(w, W, member, count, seed, stage):
    counts = np.zeros(len(w), dtype=np.int64)
    if count < 1:
        return counts
    expected = float(count) * (w / W)
    base = np.floor(expected)
    counts += base.astype(np.int64)
    leftover = max(0, count - int(counts.sum()))
    cum, f_total = pick_table(np.floor((expected - base) * 4294967296.0).astype(np.uint64))
    if f_total == 0:
        cum, f_total = pick_table(member.astype(np.uint64))
    if leftover:
        picks = pick_arrays(cum, f_total, draw_arrays(seed, stage, np.arange(leftover, dtype=np.uint64), 0))
        counts += np.bincount(picks, minlength=len(w))
    return counts


def group_points_arrays(model, counts, placement, seed, stage):
    dtype = model["root"]["org"].dtype
    T = dtype.type
    cum = np.cumsum(counts)
    total = int(cum[-1]) if len(cum) else 0
    j = np.arange(total, dtype=np.int64)
    leaf = np.searchsorted(cum, j, side="right").astype(np.int64)
    lo, hi = leaf_bounds(model, leaf)
    e = hi - lo
    if placement != 2:
        u = np.stack([uniform_arrays(dtype, seed, stage, j, a) for a in range(3)], axis=1)
    if placement == 0:
        return lo + u * e, leaf
    n = counts[leaf]
    k = j - (cum[leaf] - n)
    g = grid_divisions_arrays(np.maximum(counts, 1))[leaf]
    cell = np.stack([k % g, (k // g) % g, k // (g * g)], axis=1).astype(dtype)
    cs = e / g.astype(dtype)[:, None]
    cmin = lo + cell * cs
    return (cmin + cs / T(2) if placement == 2 else cmin + u * cs), leaf


def place_arrays(model, placement, max_points, oversampling, seed, inside_fn, W=None):
    """place() on arrays: the same returns, byte for byte."""
    placement = PLACEMENTS.get(placement, placement)
    w = model["terms"].astype(np.float64)
    interior, near = model["cls"] == INT, model["cls"] == BND
    w_int, w_ns = np.where(interior, w, 0.0), np.where(near, w, 0.0)
    W_int, W_ns = W if W is not None else (math.fsum(w_int), math.fsum(w_ns))
    dtype = model["root"]["org"].dtype
    info = dict(n_points=0, n_interior=0, n_candidates=0, n_accepted=0, n_deficit=0, W_int=W_int, W_ns=W_ns, placement=placement)
    if not W_int + W_ns > 0:
        return dict(xyz=np.zeros((0, 3), dtype=dtype), leaf=np.zeros(0, dtype=np.int64), info=info, candidates=None)
    n_int = int(np.rint(float(max_points) * (W_int / (W_int + W_ns))))
    n_ns = max_points - n_int
    n_cand = int(np.rint(float(n_ns) * oversampling))
    c_int = group_counts_arrays(w_int, W_int, interior, n_int, seed, ST_PICK_INTERIOR)
    assert c_int.sum() == n_int and not c_int[~interior].any()
    xyz, leaf = group_points_arrays(model, c_int, placement, seed, ST_INTERIOR)
    c_ns = group_counts_arrays(w_ns, W_ns, near, n_cand, seed, ST_PICK_CANDIDATES)
    assert c_ns.sum() == n_cand and not c_ns[~near].any()
    cand, cleaf = group_points_arrays(model, c_ns, placement, seed, ST_CANDIDATES)
    inside = np.asarray(inside_fn(cand), dtype=bool) if len(cand) else np.zeros(0, dtype=bool)
    take = np.nonzero(inside)[0][:max_points - n_int]
    parts_x, parts_l = [xyz, cand[take]], [leaf, cleaf[take]]
    so_far = n_int + len(take)
    n_def = 0
    if so_far < max_points and W_int > 0:
        n_def = max_points - so_far
        share = np.floor((w_int / W_int) * 4294967296.0).astype(np.uint64)
        cum, f_total = pick_table(share)
        if f_total == 0:
            cum, f_total = pick_table(interior.astype(np.uint64))
        t = np.arange(n_def, dtype=np.uint64)
        dl = pick_arrays(cum, f_total, draw_arrays(seed, ST_PICK_DEFICIT, t, 0)).astype(np.int64)
        lo, hi = leaf_bounds(model, dl)
        u = np.stack([uniform_arrays(dtype, seed, ST_DEFICIT, t, a) for a in range(3)], axis=1)
        parts_x.append(lo + u * (hi - lo)), parts_l.append(dl)
    info.update(n_points=so_far + n_def, n_interior=n_int, n_candidates=n_cand, n_accepted=len(take), n_deficit=n_def)
    return dict(xyz=np.concatenate(parts_x), leaf=np.concatenate(parts_l), info=info, candidates=(cand, cleaf, inside),
                counts=(c_int, c_ns))
