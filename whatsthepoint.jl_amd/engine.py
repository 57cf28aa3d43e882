"""Thin host wrappers over the C ABI (include/wtp.h): one `Context` per GPU.

Everything here only marshals numpy arrays to libwtp; the algorithms live in csrc/.
There is deliberately no CPU implementation behind these calls.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _dtype_code(dt) -> int:
    dt = np.dtype(dt)
    if dt == np.float32:
        return L.WTP_F32
    if dt == np.float64:
        return L.WTP_F64
    raise L.WtpArgumentError(f"coordinates must be float32 or float64, got {dt}")


def _cloud(xyz):
    xyz = np.asarray(xyz)
    if xyz.ndim != 2 or xyz.shape[1] not in (2, 3):
        raise L.WtpArgumentError("coordinates must have shape (n, 2) or (n, 3)")
    if xyz.dtype not in (np.float32, np.float64):
        xyz = xyz.astype(np.float64)
    return np.ascontiguousarray(xyz)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """Owns the device buffers, stream and timers of one GPU (wtp_create / wtp_destroy)."""

    def __init__(self, device: int = 0):
        self._lib = L.load()
        h = C.c_void_p()
        dev = (C.c_int * 1)(device)
        rc = self._lib.wtp_create(dev, 1, C.byref(h))
        if rc != L.WTP_OK:
            L.check(None, rc)
        self._h = h
        self.device = device
        self._mesh_key = None   # identity of the mesh resident in this context (octree.py)
        self._loops_key = None  # (segments, dtype) of the boundary loops resident in this context (quadtree.py)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.wtp_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- KNNTopology / KNearestSearch (src/topology.jl:79-84, src/neighbors.jl) ---------
    def knn(self, xyz, k: int, include_self: bool = False, return_dist: bool = False):
        xyz = _cloud(xyz)
        n, dim = xyz.shape
        if k < 1 or k > n - (0 if include_self else 1):
            raise L.WtpArgumentError(f"k={k} needs k+1 <= n={n} points")
        idx = np.empty((n, k), dtype=np.int32)
        dist = np.empty((n, k), dtype=xyz.dtype) if return_dist else None
        rc = self._lib.wtp_knn(self._h, _vp(xyz), n, dim, _dtype_code(xyz.dtype), int(k), int(bool(include_self)),
                               _vp(idx), _vp(dist))
        L.check(self._h, rc)
        return (idx, dist) if return_dist else idx

    def knn_dev(self, d_xyz_ptr: int, n: int, dim: int, dtype, k: int, include_self: bool, d_idx_ptr: int,
                d_dist_ptr: int = 0):
        rc = self._lib.wtp_knn_dev(self._h, C.c_void_p(d_xyz_ptr), n, dim, _dtype_code(dtype), int(k),
                                   int(bool(include_self)), C.c_void_p(d_idx_ptr),
                                   C.c_void_p(d_dist_ptr) if d_dist_ptr else None)
        L.check(self._h, rc)

    # ---- RadiusTopology / BallSearch (src/topology.jl:91-97) -----------------------------
    def radius(self, xyz, r: float):
        """CSR stencils: (offsets int64[n+1], idx int32[nnz]); rows ascending (d2, index)."""
        xyz = _cloud(xyz)
        n, dim = xyz.shape
        # row lengths are scanned on the device; the offsets come back once and stay resident for the fill
        offsets = np.empty(n + 1, dtype=np.int64)
        rc = self._lib.wtp_radius_offsets(self._h, _vp(xyz), n, dim, _dtype_code(xyz.dtype), float(r), _vp(offsets))
        L.check(self._h, rc)
        idx = np.empty(max(int(offsets[-1]), 1), dtype=np.int32)
        rc = self._lib.wtp_radius_fill(self._h, None, _vp(idx))
        L.check(self._h, rc)
        return offsets, idx[: int(offsets[-1])]

    def radius_two_phase(self, xyz, r: float):
        """The caller-side scan of the C ABI's first form (wtp_radius_count -> offsets -> wtp_radius_fill)."""
        xyz = _cloud(xyz)
        n, dim = xyz.shape
        counts = np.empty(n, dtype=np.int32)
        rc = self._lib.wtp_radius_count(self._h, _vp(xyz), n, dim, _dtype_code(xyz.dtype), float(r), _vp(counts))
        L.check(self._h, rc)
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        idx = np.empty(max(int(offsets[-1]), 1), dtype=np.int32)
        rc = self._lib.wtp_radius_fill(self._h, _vp(offsets), _vp(idx))
        L.check(self._h, rc)
        return offsets, idx[: int(offsets[-1])]

    def radius_marks(self):
        """Diagnostic of the last radius count on this context (wtp_radius_marks): (marks uint8[n], info dict).
        marks: 0 = left to the fill phase, 1 = brick kernel row, 2 = row in the arena."""
        info = (C.c_double * 13)()
        L.check(self._h, self._lib.wtp_radius_marks(self._h, None, 0, info))  # n of the count, as the library holds it
        n = int(info[12])
        marks = np.empty(max(n, 1), dtype=np.uint8)
        L.check(self._h, self._lib.wtp_radius_marks(self._h, _vp(marks), len(marks), info))
        return marks[:n], dict(dense_used=bool(info[0]), rad_wave_only=int(info[1]), dense_hcap=int(info[2]),
                                          cells=(int(info[3]), int(info[4]), int(info[5])), cell_edge=float(info[6]),
                                          origin=(float(info[7]), float(info[8]), float(info[9])),
                                          arena_taken=int(info[10]), arena_cap=int(info[11]))

    # ---- repel -------------------------------------------------------------------------------
    def relax(self, snap, n_fixed: int, spacing, force, k: int, alpha_lo: float, alpha_max: float, device_ptr=None):
        return RelaxSession(self, snap, n_fixed, spacing, force, k, alpha_lo, alpha_max, device_ptr=device_ptr)

    # ---- variable spacing laws at arbitrary points (spacing.(points)) ---------------------------
    def spacing_eval(self, law: dict, xyz):
        xyz = _cloud(xyz)
        sd, keep = _law_desc(law, xyz.dtype, xyz.shape[1])
        out = np.empty(len(xyz), dtype=xyz.dtype)
        rc = self._lib.wtp_spacing_eval(self._h, C.byref(sd), _vp(xyz), len(xyz), xyz.shape[1], _dtype_code(xyz.dtype),
                                        _vp(out))
        L.check(self._h, rc)
        del keep
        return out

    # ---- isinside post-filter (src/repel.jl:90; src/isinside.jl) -------------------------------
    def isinside_greens(self, test, elem_xyz, elem_normal, elem_area, return_g: bool = False):
        """3-D: bool[n] (and g[n]) for test points against boundary elements (centroid, normal, area)."""
        test = _cloud(test)
        if test.shape[1] != 3:
            raise L.WtpArgumentError("the Green's-function test is 3-D")
        dt = test.dtype
        p = np.ascontiguousarray(elem_xyz, dtype=dt)
        nrm = np.ascontiguousarray(elem_normal, dtype=dt)
        a = np.ascontiguousarray(elem_area, dtype=dt).reshape(-1)
        if p.ndim != 2 or p.shape[1] != 3 or nrm.shape != p.shape or a.shape != (len(p),):
            raise L.WtpArgumentError("boundary elements need (m, 3) points, (m, 3) normals and m areas")
        inside = np.zeros(len(test), dtype=np.uint8)
        g = np.zeros(len(test), dtype=dt) if return_g else None
        rc = self._lib.wtp_isinside_greens(self._h, _vp(test), len(test), _vp(p), _vp(nrm), _vp(a), len(p),
                                           _dtype_code(dt), _vp(inside), _vp(g))
        L.check(self._h, rc)
        return (inside.astype(bool), g) if return_g else inside.astype(bool)

    def isinside_winding(self, test, poly, return_sum: bool = False):
        """2-D: bool[n] (and angle sums) for test points against an ordered, closed polygon."""
        test = _cloud(test)
        if test.shape[1] != 2:
            raise L.WtpArgumentError("the winding-number test is 2-D")
        dt = test.dtype
        poly = np.ascontiguousarray(poly, dtype=dt)
        if poly.ndim != 2 or poly.shape[1] != 2:
            raise L.WtpArgumentError("polygon must be (m, 2)")
        inside = np.zeros(len(test), dtype=np.uint8)
        s = np.zeros(len(test), dtype=dt) if return_sum else None
        rc = self._lib.wtp_isinside_winding(self._h, _vp(test), len(test), _vp(poly), len(poly), _dtype_code(dt),
                                            _vp(inside), _vp(s))
        L.check(self._h, rc)
        return (inside.astype(bool), s) if return_sum else inside.astype(bool)

    # ---- consumers of the rows -------------------------------------------------
    def pca_normals(self, xyz, k: int = 5):
        """compute_normals (src/normals.jl:15-46): (n, dim) unit normals, largest component positive."""
        xyz = _cloud(xyz)
        out = np.empty_like(xyz)
        rc = self._lib.wtp_pca_normals(self._h, _vp(xyz), len(xyz), xyz.shape[1], _dtype_code(xyz.dtype), int(k), _vp(out))
        L.check(self._h, rc)
        return out

    def gradient_limit(self, centers, h0, g: float, k: int = 12, tol: float = 1.0e-3, max_sweeps: int = 2000):
        """_gradient_limit_field on leaf centres (octree.jl:677-717): (limited field, sweeps applied)."""
        c = _cloud(centers)
        h0 = np.ascontiguousarray(h0, dtype=c.dtype).reshape(-1)
        if h0.shape != (len(c),):
            raise L.WtpArgumentError("h0 needs one value per centre")
        out = np.empty_like(h0)
        sw = C.c_int(0)
        rc = self._lib.wtp_gradient_limit(self._h, _vp(c), len(c), c.shape[1], _dtype_code(c.dtype), int(min(k, len(c))),
                                          _vp(h0), float(g), float(tol), int(max_sweeps), _vp(out), C.byref(sw))
        L.check(self._h, rc)
        return out, sw.value

    def knn_stats(self, xyz, k: int, h=None, coord_radius: float = 1.4, return_nn: bool = False, return_mean: bool = False):
        """The sums behind metrics / spacing_metrics / spacing_fidelity_metrics (src/metrics.jl:19-129), reduced on the
        device from the k-NN distance rows (wtp_knn_stats): a dict of the struct's fields.  k counts the point itself
        (KnearestSearch(cloud, k)), 2 <= k <= n.  h: None, one positive number, or n values (converted to float64).
        return_nn / return_mean add "nn" (n values of the cloud's dtype: the nearest-neighbour distances) and "mean"
        (n float64: the per-point mean distances); nothing else of size n, and never the (n, k) matrices, is copied."""
        xyz = _cloud(xyz)
        n, dim = xyz.shape
        hv, hc = None, 0.0
        if h is not None:
            if np.ndim(h) == 0:
                hc = float(h)
                if not hc > 0:
                    raise L.WtpArgumentError("a constant spacing must be > 0")
            else:
                hv = np.ascontiguousarray(h, dtype=np.float64).reshape(-1)
                if hv.shape != (n,):
                    raise L.WtpArgumentError("h needs one value per point")
        st = L.KnnStats()
        nn = np.empty(n, dtype=xyz.dtype) if return_nn else None
        mean = np.empty(n, dtype=np.float64) if return_mean else None
        rc = self._lib.wtp_knn_stats(self._h, _vp(xyz), n, dim, _dtype_code(xyz.dtype), int(k), _vp(hv), hc, float(coord_radius),
                                     C.byref(st), _vp(nn), _vp(mean))
        L.check(self._h, rc)
        out = {name: getattr(st, name) for name, _ in L.KnnStats._fields_}
        if return_nn:
            out["nn"] = nn
        if return_mean:
            out["mean"] = mean
        return out

    def knn_stats_dev(self, d_xyz_ptr: int, n: int, dim: int, dtype, k: int, d_h_ptr: int = 0, h_const: float = 0.0,
                      coord_radius: float = 1.4, d_nn_ptr: int = 0, d_mean_ptr: int = 0):
        """wtp_knn_stats_dev: the same over device arrays given as addresses (0 = absent); returns the struct's dict."""
        st = L.KnnStats()
        p = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        rc = self._lib.wtp_knn_stats_dev(self._h, C.c_void_p(d_xyz_ptr), n, dim, _dtype_code(dtype), int(k), p(d_h_ptr),
                                         float(h_const), float(coord_radius), C.byref(st), p(d_nn_ptr), p(d_mean_ptr))
        L.check(self._h, rc)
        return {name: getattr(st, name) for name, _ in L.KnnStats._fields_}

    @staticmethod
    def _graph_info(info):
        return {name: int(getattr(info, name)) for name, _ in L.NormalGraphInfo._fields_}

    def _cloud_and_normals(self, points, normals):
        xyz = _cloud(points)
        nrm = np.ascontiguousarray(normals, dtype=xyz.dtype)
        if nrm.shape != xyz.shape:
            raise L.WtpArgumentError("normals need the shape of the points")
        return xyz, nrm

    def orient_normals(self, points, normals, k: int, return_tree: bool = False):
        """The graph part of orient_normals! (src/normals.jl:75-161) on the device (wtp_orient_normals): returns
        (oriented normals as a new (n, dim) array of the cloud's dtype, info dict), with return_tree also the
        (n - n_components, 2) int32 edges {a < b} of the minimum spanning forest, sorted.  k counts the point itself,
        1 <= k <= n.  The rows never leave the device."""
        xyz, nrm = self._cloud_and_normals(points, normals)
        out = nrm.copy()
        n, dim = xyz.shape
        mst = np.empty((max(n - 1, 0), 2), dtype=np.int32) if return_tree else None
        info = L.NormalGraphInfo()
        rc = self._lib.wtp_orient_normals(self._h, _vp(xyz), n, dim, _dtype_code(xyz.dtype), int(k), _vp(out), _vp(mst),
                                          C.byref(info))
        L.check(self._h, rc)
        d = self._graph_info(info)
        if not return_tree:
            return out, d
        mst = mst[: n - d["n_components"]]
        return out, d, mst[np.lexsort((mst[:, 1], mst[:, 0]))]

    def orient_normals_dev(self, d_xyz_ptr: int, n: int, dim: int, dtype, k: int, d_normals_ptr: int, d_mst_ptr: int = 0):
        """wtp_orient_normals_dev: the same over device arrays given as addresses (d_mst_ptr 0 = absent); the normals
        are oriented in place, the info dict is returned."""
        info = L.NormalGraphInfo()
        rc = self._lib.wtp_orient_normals_dev(self._h, C.c_void_p(d_xyz_ptr), n, dim, _dtype_code(dtype), int(k),
                                              C.c_void_p(d_normals_ptr), C.c_void_p(d_mst_ptr) if d_mst_ptr else None,
                                              C.byref(info))
        L.check(self._h, rc)
        return self._graph_info(info)

    def normal_components(self, points, normals, k: int, angle: float):
        """The graph part of split_surface! (src/surface_operations.jl:58-94) on the device (wtp_normal_components):
        (labels, info dict); labels[i] is the smallest id in i's component of the row edges whose normals differ by
        less than `angle` radians."""
        xyz, nrm = self._cloud_and_normals(points, normals)
        n, dim = xyz.shape
        label = np.empty(n, dtype=np.int32)
        info = L.NormalGraphInfo()
        rc = self._lib.wtp_normal_components(self._h, _vp(xyz), _vp(nrm), n, dim, _dtype_code(xyz.dtype), int(k), float(angle),
                                             _vp(label), C.byref(info))
        L.check(self._h, rc)
        return label, self._graph_info(info)

    # ---- triangle-mesh geometry index (octree method of repel; src/octree/triangle_octree.jl) -----
    def mesh_set(self, vertices, triangles):
        """vertices (nv, 3) float32/float64 = the index's machine type; triangles (nt, 3) 0-based."""
        v = np.ascontiguousarray(vertices)
        if v.dtype not in (np.float32, np.float64):
            v = v.astype(np.float64)
        t = np.ascontiguousarray(triangles, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
            raise L.WtpArgumentError("mesh needs (nv, 3) vertices and (nt, 3) triangles")
        L.check(self._h, self._lib.wtp_mesh_set(self._h, _vp(v), len(v), _vp(t), len(t), _dtype_code(v.dtype)))
        self._mesh_key = (len(v), len(t), v.dtype)
        self._mesh_owner = None   # octree.py marks the TriangleOctree it uploaded
        self._node_tree_owner = None  # a new mesh drops the node tree (nodetree.py marks the NodeOctree it built)

    def mesh_clear(self):
        L.check(self._h, self._lib.wtp_mesh_clear(self._h))
        self._mesh_key = None
        self._mesh_owner = None
        self._node_tree_owner = None

    def mesh_face_normals(self):
        nt = self._mesh_key[1]
        out = np.empty((nt, 3), dtype=np.float64)
        L.check(self._h, self._lib.wtp_mesh_face_normals(self._h, _vp(out)))
        return out

    def mesh_bounds(self):
        out = np.empty(6, dtype=np.float64)
        L.check(self._h, self._lib.wtp_mesh_bounds(self._h, _vp(out)))
        return out[:3].copy(), out[3:].copy()

    def mesh_query(self, pts, offset: float = 0.0, want=("sd", "tri", "closest", "inside", "projected")):
        """Nearest-triangle queries for (n, 3) points; returns a dict with the requested outputs."""
        pts = _cloud(pts)
        if pts.shape[1] != 3:
            raise L.WtpArgumentError("mesh queries are 3-D")
        n, dt = len(pts), pts.dtype
        out = {}
        if "sd" in want:
            out["sd"] = np.empty(n, dtype=dt)
        if "tri" in want:
            out["tri"] = np.empty(n, dtype=np.int32)
        if "closest" in want:
            out["closest"] = np.empty((n, 3), dtype=dt)
        if "inside" in want:
            out["inside"] = np.zeros(n, dtype=np.uint8)
        if "projected" in want:
            out["projected"] = np.empty((n, 3), dtype=dt)
        rc = self._lib.wtp_mesh_query(self._h, _vp(pts), n, _dtype_code(dt), float(offset), _vp(out.get("sd")),
                                      _vp(out.get("tri")), _vp(out.get("closest")), _vp(out.get("inside")),
                                      _vp(out.get("projected")))
        L.check(self._h, rc)
        if "inside" in out:
            out["inside"] = out["inside"].astype(bool)
        return out

    # ---- graded Poisson-disk sampling of the mesh surface (src/surface_sampling.jl; wtp_mesh_sample) ----------
    def _mesh_dtype(self):
        return np.dtype(self._mesh_key[2]) if self._mesh_key else np.dtype(np.float64)

    def _sample_spacing(self, spacing):
        """wtp_spacing_desc for the sampler: a number (ConstantSpacing) or a device law's dict.  (desc, keepalive)"""
        if isinstance(spacing, dict):
            return _law_desc(spacing, self._mesh_dtype(), 3)
        sd = L.SpacingDesc()
        sd.kind, sd.constant = L.WTP_SPACING_CONSTANT, float(spacing)
        return sd, None

    def _out_arrays(self, n: int, want, spec):
        """Empty host arrays of n rows for the names of `spec` that `want` holds; spec: name -> dtype, None standing for
        the mesh's, and "xyz" being (n, 3)."""
        dt = self._mesh_dtype()
        return {k: np.empty((n, 3) if k == "xyz" else n, dtype=d or dt) for k, d in spec.items() if k in want}

    def mesh_sample(self, spacing, factor: float = 0.75, max_points: int = 10_000_000, stall_limit: int = 2000,
                    seed: int = 0, batch: int = 0, spacing_desc=None):
        """wtp_mesh_sample on the mesh of mesh_set: the serial dart thrower over the seeded stream, decided in batches on
        the device.  Returns the info dict; the samples stay on the device (mesh_sample_get).  spacing_desc: a ready
        L.SpacingDesc instead of `spacing`."""
        sd, keep = (spacing_desc, None) if spacing_desc is not None else self._sample_spacing(spacing)
        info = L.SampleInfo()
        rc = self._lib.wtp_mesh_sample(self._h, C.byref(sd), float(factor), int(max_points), int(stall_limit),
                                       C.c_uint64(int(seed)), int(batch), C.byref(info))
        L.check(self._h, rc)
        del keep
        return _info_dict(info)

    def mesh_sample_get(self, n: int, want=("xyz", "tri", "r", "dart")):
        """The n = info['n_points'] samples of the last mesh_sample as a dict of host arrays (mesh dtype)."""
        out = self._out_arrays(n, want, dict(xyz=None, tri=np.int32, r=None, dart=np.int64))
        rc = self._lib.wtp_mesh_sample_get(self._h, _vp(out.get("xyz")), _vp(out.get("tri")), _vp(out.get("r")),
                                           _vp(out.get("dart")))
        L.check(self._h, rc)
        return out

    def mesh_sample_get_dev(self, d_xyz_ptr: int = 0, d_tri_ptr: int = 0, d_r_ptr: int = 0):
        """wtp_mesh_sample_get_dev: the samples into device arrays given as addresses (0 = absent)."""
        rc = self._lib.wtp_mesh_sample_get_dev(self._h, C.c_void_p(d_xyz_ptr or None), C.c_void_p(d_tri_ptr or None),
                                               C.c_void_p(d_r_ptr or None))
        L.check(self._h, rc)

    def mesh_sample_darts(self, spacing, factor: float, seed: int, first: int, n: int):
        """wtp_mesh_sample_darts: darts first .. first + n - 1 as the sampler makes them: (xyz, tri, r)."""
        sd, keep = self._sample_spacing(spacing)
        dt = self._mesh_dtype()
        xyz, tri, r = np.empty((n, 3), dtype=dt), np.empty(n, dtype=np.int32), np.empty(n, dtype=dt)
        rc = self._lib.wtp_mesh_sample_darts(self._h, C.byref(sd), float(factor), C.c_uint64(int(seed)), int(first), int(n),
                                             _vp(xyz), _vp(tri), _vp(r))
        L.check(self._h, rc)
        del keep
        return xyz, tri, r

    # ---- graded Poisson-disk fill of the mesh's volume (discretize's Orthtree / :bridson placement; wtp_mesh_fill) ----
    def mesh_fill(self, spacing, factor: float = 0.75, seeds=None, max_points: int = 10_000_000, stall_limit: int = 2000,
                  seed: int = 0, batch: int = 0, spacing_desc=None):
        """wtp_mesh_fill on the mesh of mesh_set: the serial dart thrower over the seeded stream of the mesh's bounding
        box, decided in batches on the device.  seeds: (n, 3) points that occupy space from the start (converted to the
        mesh's dtype), or None.  Returns the info dict; the points stay on the device (mesh_fill_get)."""
        sd, keep = (spacing_desc, None) if spacing_desc is not None else self._sample_spacing(spacing)
        s = self._seed_rows(seeds)
        info = L.FillInfo()
        rc = self._lib.wtp_mesh_fill(self._h, C.byref(sd), float(factor), _vp(s), 0 if s is None else len(s), int(max_points),
                                     int(stall_limit), C.c_uint64(int(seed)), int(batch), C.byref(info))
        L.check(self._h, rc)
        del keep
        return _info_dict(info)

    def mesh_fill_get(self, n: int, want=("xyz", "r", "dart")):
        """The n = info['n_points'] points of the last mesh_fill as a dict of host arrays (mesh dtype)."""
        out = self._out_arrays(n, want, dict(xyz=None, r=None, dart=np.int64))
        rc = self._lib.wtp_mesh_fill_get(self._h, _vp(out.get("xyz")), _vp(out.get("r")), _vp(out.get("dart")))
        L.check(self._h, rc)
        return out

    def mesh_fill_get_dev(self, d_xyz_ptr: int = 0, d_r_ptr: int = 0):
        """wtp_mesh_fill_get_dev: the points into device arrays given as addresses (0 = absent)."""
        rc = self._lib.wtp_mesh_fill_get_dev(self._h, C.c_void_p(d_xyz_ptr or None), C.c_void_p(d_r_ptr or None))
        L.check(self._h, rc)

    def mesh_fill_darts(self, spacing, factor: float, seed: int, first: int, n: int):
        """wtp_mesh_fill_darts: darts first .. first + n - 1 as the fill makes them: (xyz, inside, r)."""
        sd, keep = self._sample_spacing(spacing)
        dt = self._mesh_dtype()
        xyz, inside, r = np.empty((n, 3), dtype=dt), np.zeros(n, dtype=np.uint8), np.empty(n, dtype=dt)
        rc = self._lib.wtp_mesh_fill_darts(self._h, C.byref(sd), float(factor), C.c_uint64(int(seed)), int(first), int(n),
                                           _vp(xyz), _vp(inside), _vp(r))
        L.check(self._h, rc)
        del keep
        return xyz, inside.astype(bool), r

    # ---- advancing-front fill of the mesh's volume (discretize's SlakKosec; wtp_mesh_front) ------------------------------
    def _seed_rows(self, seeds):
        if seeds is None or not len(seeds):
            return None
        s = np.ascontiguousarray(seeds, dtype=self._mesh_dtype())
        if s.ndim != 2 or s.shape[1] != 3:
            raise L.WtpArgumentError("seeds must have shape (n, 3)")
        return s

    def mesh_front(self, spacing, n: int = 10, seeds=None, max_points: int = 10_000_000, seed: int = 0, batch: int = 0,
                   spacing_desc=None):
        """wtp_mesh_front on the mesh of mesh_set: the serial advancing front over the seeded stream, n candidates per
        queue entry, decided in batches of parents on the device.  seeds: (m, 3) points, the head of the queue (converted
        to the mesh's dtype), or None.  Returns the info dict; the points stay on the device (mesh_front_get)."""
        sd, keep = (spacing_desc, None) if spacing_desc is not None else self._sample_spacing(spacing)
        s = self._seed_rows(seeds)
        info = L.FrontInfo()
        rc = self._lib.wtp_mesh_front(self._h, C.byref(sd), int(n), _vp(s), 0 if s is None else len(s), int(max_points),
                                      C.c_uint64(int(seed)), int(batch), C.byref(info))
        L.check(self._h, rc)
        del keep
        return _info_dict(info)

    def mesh_front_get(self, n: int, want=("xyz", "h", "cand", "parent")):
        """The n = info['n_points'] points of the last mesh_front as a dict of host arrays (mesh dtype): xyz, their own
        h, the candidate index each came from and its parent's queue index."""
        out = self._out_arrays(n, want, dict(xyz=None, h=None, cand=np.int64, parent=np.int32))
        rc = self._lib.wtp_mesh_front_get(self._h, _vp(out.get("xyz")), _vp(out.get("h")), _vp(out.get("cand")),
                                          _vp(out.get("parent")))
        L.check(self._h, rc)
        return out

    def mesh_front_get_dev(self, d_xyz_ptr: int = 0, d_h_ptr: int = 0):
        """wtp_mesh_front_get_dev: the points into device arrays given as addresses (0 = absent)."""
        rc = self._lib.wtp_mesh_front_get_dev(self._h, C.c_void_p(d_xyz_ptr or None), C.c_void_p(d_h_ptr or None))
        L.check(self._h, rc)

    def mesh_front_candidates(self, spacing, seed: int, parents, first_parent: int = 0, n: int = 10):
        """wtp_mesh_front_candidates: the n candidates each of the given parent positions, parent p standing for queue
        entry first_parent + p, as the front makes them: (xyz, inside, r), len(parents) * n rows."""
        sd, keep = self._sample_spacing(spacing)
        dt = self._mesh_dtype()
        par = np.ascontiguousarray(parents, dtype=dt).reshape(-1, 3)
        m = len(par) * int(n)
        xyz, inside, r = np.empty((m, 3), dtype=dt), np.zeros(m, dtype=np.uint8), np.empty(m, dtype=dt)
        rc = self._lib.wtp_mesh_front_candidates(self._h, C.byref(sd), C.c_uint64(int(seed)), _vp(par), len(par),
                                                 int(first_parent), int(n), _vp(xyz), _vp(inside), _vp(r))
        L.check(self._h, rc)
        del keep
        return xyz, inside.astype(bool), r

    # ---- boundary-loop index of a 2-D domain (src/octree/segment_quadtree.jl; wtp_loops_set) and its area fill -------
    def loops_set(self, loops):
        """loops: a list of (n_l, 2) arrays, each one closed loop in order (either orientation, closed or not); the
        first one's float32 / float64 dtype is the index's machine type."""
        loops = [np.asarray(l) for l in loops]
        if not loops or any(l.ndim != 2 or l.shape[1] != 2 for l in loops):
            raise L.WtpArgumentError("boundary loops must be a non-empty list of (n, 2) arrays")
        dt = loops[0].dtype if loops[0].dtype in (np.float32, np.float64) else np.dtype(np.float64)
        xy = np.ascontiguousarray(np.concatenate(loops, axis=0), dtype=dt)
        start = np.concatenate([[0], np.cumsum([len(l) for l in loops])]).astype(np.int64)
        self._loops_key = None
        self._loops_owner = None
        L.check(self._h, self._lib.wtp_loops_set(self._h, _vp(xy), len(xy), _vp(start), len(loops), _dtype_code(dt)))
        self._loops_key = (self.loops_bounds()[2], np.dtype(dt))

    def loops_clear(self):
        L.check(self._h, self._lib.wtp_loops_clear(self._h))
        self._loops_key = None
        self._loops_owner = None

    def loops_bounds(self):
        """(min xy, max xy, number of segments) of the resident loops."""
        out = np.empty(4, dtype=np.float64)
        ns = C.c_int64(0)
        L.check(self._h, self._lib.wtp_loops_bounds(self._h, _vp(out), C.byref(ns)))
        return out[:2].copy(), out[2:].copy(), int(ns.value)

    def loops_query(self, pts, want=("sd", "seg", "closest", "inside")):
        """Nearest-segment queries for (n, 2) points; returns a dict with the requested outputs."""
        pts = _cloud(pts)
        if pts.shape[1] != 2:
            raise L.WtpArgumentError("loop queries are 2-D")
        n, dt = len(pts), pts.dtype
        out = {}
        if "sd" in want:
            out["sd"] = np.empty(n, dtype=dt)
        if "seg" in want:
            out["seg"] = np.empty(n, dtype=np.int32)
        if "closest" in want:
            out["closest"] = np.empty((n, 2), dtype=dt)
        if "inside" in want:
            out["inside"] = np.zeros(n, dtype=np.uint8)
        rc = self._lib.wtp_loops_query(self._h, _vp(pts), n, _dtype_code(dt), _vp(out.get("sd")), _vp(out.get("seg")),
                                       _vp(out.get("closest")), _vp(out.get("inside")))
        L.check(self._h, rc)
        if "inside" in out:
            out["inside"] = out["inside"].astype(bool)
        return out

    def _loops_dtype(self):
        return self._loops_key[1] if self._loops_key else np.dtype(np.float64)

    def _area_spacing(self, spacing):
        if isinstance(spacing, dict):
            return _law_desc(spacing, self._loops_dtype(), 2)
        sd = L.SpacingDesc()
        sd.kind, sd.constant = L.WTP_SPACING_CONSTANT, float(spacing)
        return sd, None

    def loops_fill(self, spacing, factor: float = 0.75, seeds=None, max_points: int = 10_000_000, stall_limit: int = 2000,
                   seed: int = 0, batch: int = 0, spacing_desc=None):
        """wtp_loops_fill on the loops of loops_set: the serial dart thrower over the seeded stream of the loops' box,
        decided in batches on the device.  seeds: (n, 2) points that occupy space from the start (converted to the
        index's dtype), or None.  Returns the info dict; the points stay on the device (loops_fill_get)."""
        sd, keep = (spacing_desc, None) if spacing_desc is not None else self._area_spacing(spacing)
        s = None
        if seeds is not None and len(seeds):
            s = np.ascontiguousarray(seeds, dtype=self._loops_dtype())
            if s.ndim != 2 or s.shape[1] != 2:
                raise L.WtpArgumentError("seeds must have shape (n, 2)")
        info = L.FillInfo()
        rc = self._lib.wtp_loops_fill(self._h, C.byref(sd), float(factor), _vp(s), 0 if s is None else len(s), int(max_points),
                                      int(stall_limit), C.c_uint64(int(seed)), int(batch), C.byref(info))
        L.check(self._h, rc)
        del keep
        return _info_dict(info)

    def loops_fill_get(self, n: int, want=("xy", "r", "dart")):
        """The n = info['n_points'] points of the last loops_fill as a dict of host arrays (index dtype)."""
        dt = self._loops_dtype()
        spec = dict(xy=((n, 2), dt), r=(n, dt), dart=(n, np.int64))
        out = {k: np.empty(sh, dtype=d) for k, (sh, d) in spec.items() if k in want}
        rc = self._lib.wtp_loops_fill_get(self._h, _vp(out.get("xy")), _vp(out.get("r")), _vp(out.get("dart")))
        L.check(self._h, rc)
        return out

    def loops_fill_get_dev(self, d_xy_ptr: int = 0, d_r_ptr: int = 0):
        """wtp_loops_fill_get_dev: the points into device arrays given as addresses (0 = absent)."""
        rc = self._lib.wtp_loops_fill_get_dev(self._h, C.c_void_p(d_xy_ptr or None), C.c_void_p(d_r_ptr or None))
        L.check(self._h, rc)

    def loops_fill_darts(self, spacing, factor: float, seed: int, first: int, n: int):
        """wtp_loops_fill_darts: darts first .. first + n - 1 as the area fill makes them: (xy, inside, r)."""
        sd, keep = self._area_spacing(spacing)
        dt = self._loops_dtype()
        xy, inside, r = np.empty((n, 2), dtype=dt), np.zeros(n, dtype=np.uint8), np.empty(n, dtype=dt)
        rc = self._lib.wtp_loops_fill_darts(self._h, C.byref(sd), float(factor), C.c_uint64(int(seed)), int(first), int(n),
                                            _vp(xy), _vp(inside), _vp(r))
        L.check(self._h, rc)
        del keep
        return xy, inside.astype(bool), r

    # ---- spacing-driven node octree over the mesh (the Orthtree algorithm's tree; wtp_node_tree_*) -----------------------
    def node_tree_build(self, spacing, alpha: float = 2.0, node_min_ratio: float = 1.0e-6, spacing_desc=None):
        """wtp_node_tree_build on the mesh of mesh_set: refined by the spacing, balanced 2:1, leaves classified.  Returns
        the info dict (origin as a tuple); the tree stays on the device (node_tree_get, node_tree_locate)."""
        sd, keep = (spacing_desc, None) if spacing_desc is not None else self._sample_spacing(spacing)
        info = L.NodeTreeInfo()
        rc = self._lib.wtp_node_tree_build(self._h, C.byref(sd), float(alpha), float(node_min_ratio), C.byref(info))
        L.check(self._h, rc)
        del keep
        self._node_tree_owner = None
        out = _info_dict(info)
        out["origin"] = tuple(info.origin)
        return out

    def node_tree_get(self, n: int, want=("cell", "depth", "cls", "h")):
        """The n = info['n_leaves'] leaves in leaf order as a dict of host arrays: cell (n, 3) int32, depth int32,
        cls int8 (0 exterior, 1 boundary, 2 interior), h of the mesh's dtype."""
        spec = dict(cell=np.int32, depth=np.int32, cls=np.int8, h=self._mesh_dtype())
        out = {k: np.empty((n, 3) if k == "cell" else n, dtype=d) for k, d in spec.items() if k in want}
        rc = self._lib.wtp_node_tree_get(self._h, _vp(out.get("cell")), _vp(out.get("depth")), _vp(out.get("cls")),
                                         _vp(out.get("h")))
        L.check(self._h, rc)
        return out

    def node_tree_locate(self, pts):
        """wtp_node_tree_locate: the leaf (index in leaf order) of each of (n, 3) points, -1 outside the root box."""
        pts = _cloud(pts)
        if pts.shape[1] != 3:
            raise L.WtpArgumentError("the node tree is 3-D")
        out = np.empty(len(pts), dtype=np.int64)
        L.check(self._h, self._lib.wtp_node_tree_locate(self._h, _vp(pts), len(pts), _dtype_code(pts.dtype), _vp(out)))
        return out

    PLACEMENTS = {"random": 0, "jittered": 1, "lattice": 2}

    def node_place(self, placement, max_points: int, boundary_oversampling: float = 2.0, seed: int = 0):
        """wtp_node_place over the resident tree: placement "random" | "jittered" | "lattice" (or its code).  Returns the
        info dict; the points stay on the device (node_place_get)."""
        code = self.PLACEMENTS.get(placement, placement)
        if isinstance(code, str):
            raise L.WtpArgumentError("placement must be :random, :jittered, :lattice, or :bridson")
        info = L.NodePlaceInfo()
        rc = self._lib.wtp_node_place(self._h, int(code), int(max_points), float(boundary_oversampling), C.c_uint64(int(seed)),
                                      C.byref(info))
        L.check(self._h, rc)
        return _info_dict(info)

    def node_place_get(self, n: int, want=("xyz", "leaf")):
        """The n = info['n_points'] points of the last node_place: xyz (n, 3) of the mesh's dtype, leaf int64."""
        out = self._out_arrays(n, want, dict(xyz=None, leaf=np.int64))
        L.check(self._h, self._lib.wtp_node_place_get(self._h, _vp(out.get("xyz")), _vp(out.get("leaf"))))
        return out

    def node_place_get_dev(self, d_xyz_ptr: int = 0, d_leaf_ptr: int = 0):
        """wtp_node_place_get_dev: the points into device arrays given as addresses (0 = absent)."""
        L.check(self._h, self._lib.wtp_node_place_get_dev(self._h, C.c_void_p(d_xyz_ptr or None), C.c_void_p(d_leaf_ptr or None)))

    def node_tree_clear(self):
        self._node_tree_owner = None
        L.check(self._h, self._lib.wtp_node_tree_clear(self._h))

    def set_stream(self, stream_handle=None):
        """Run the library on a caller-owned HIP stream (handle as an int; 0 = the device's default
        stream, which is torch's current stream unless the caller switched); None = own stream."""
        ext = stream_handle is not None
        L.check(self._h, self._lib.wtp_set_stream(self._h, C.c_void_p(int(stream_handle or 0)), int(ext)))

    # ---- measurement ---------------------------------------------------------------------------
    # ---- the context's RCCL communicator (include/wtp.h: wtp_comm_*; one process per GPU) ----------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        L.check(self._h, self._lib.wtp_comm_unique_id(self._h, buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, nranks: int):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        L.check(self._h, self._lib.wtp_comm_init(self._h, buf, int(rank), int(nranks)))

    def comm_finalize(self):
        L.check(self._h, self._lib.wtp_comm_finalize(self._h))

    def comm_exchange_rows(self, peer_lo: int, peer_hi: int, send_lo_ptr: int, n_send_lo: int, send_hi_ptr: int,
                           n_send_hi: int, recv_lo_ptr: int, recv_hi_ptr: int, cap: int):
        """One round with the two neighbours along an axis (peer -1: none); device pointers to 16-byte rows.
        Returns the received row counts (lo, hi); the rows are ordered on the context's stream."""
        n_lo, n_hi = C.c_int64(0), C.c_int64(0)
        L.check(self._h, self._lib.wtp_comm_exchange_rows(
            self._h, int(peer_lo), int(peer_hi), C.c_void_p(send_lo_ptr or None), int(n_send_lo),
            C.c_void_p(send_hi_ptr or None), int(n_send_hi), C.c_void_p(recv_lo_ptr or None), C.c_void_p(recv_hi_ptr or None),
            int(cap), C.byref(n_lo), C.byref(n_hi)))
        return int(n_lo.value), int(n_hi.value)

    def comm_allreduce_stats(self, st: dict) -> dict:
        s = L.StepStats()
        for k, v in st.items():
            if hasattr(s, k):
                setattr(s, k, v)
        L.check(self._h, self._lib.wtp_comm_allreduce_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in L.StepStats._fields_}

    def timers(self):
        out = (C.c_double * 4)()
        L.check(self._h, self._lib.wtp_timers_get(self._h, out))
        return dict(hash_ms=out[0], sweep_ms=out[1], other_ms=out[2], sweep_launches=int(out[3]))

    def timers_reset(self):
        L.check(self._h, self._lib.wtp_timers_reset(self._h))

    def gen_uniform_dev(self, seed: int, first: int, n: int, dim: int, dtype, d_out_ptr: int):
        rc = self._lib.wtp_gen_uniform_dev(self._h, C.c_uint64(seed), first, n, dim, _dtype_code(dtype),
                                           C.c_void_p(d_out_ptr))
        L.check(self._h, rc)


def _info_dict(info):
    """A ctypes info struct as the dict the mesh_* runs return."""
    return {name: getattr(info, name) for name, _ in type(info)._fields_}


def _law_desc(law: dict, dtype, dim: int):
    """wtp_spacing_desc for a device-evaluated law: dict(kind=2|3, p0, p1, p2, boundary=(m, dim) array).
    Returns (desc, keepalive)."""
    b = np.ascontiguousarray(law["boundary"], dtype=dtype)
    if b.ndim != 2 or b.shape[1] != dim:
        raise L.WtpArgumentError(f"the spacing law's boundary points must be (m, {dim})")
    sd = L.SpacingDesc()
    sd.kind, sd.constant, sd.per_point = int(law["kind"]), 0.0, None
    sd.p0, sd.p1, sd.p2 = float(law["p0"]), float(law["p1"]), float(law.get("p2", 0.0))
    sd.boundary_xyz, sd.n_boundary = b.ctypes.data, len(b)
    return sd, b


def _stats_dict(s: L.StepStats):
    return dict(max_force=s.max_force, sum_u=s.sum_u, sum_u2=s.sum_u2, n_move=s.n_move, argmin_i=s.argmin_i,
                argmin_j=s.argmin_j, argmin_r=s.argmin_r, n_fallback=s.n_fallback, n_uncovered=s.n_uncovered,
                n_escaped=s.n_escaped)


class RelaxSession:
    """Device-resident state of one `_relax!` call (src/repel.jl:202-339): coordinates stay in
    HBM between sweeps; the host sees three scalars per iteration."""

    def __init__(self, ctx: Context, snap, n_fixed: int, spacing, force, k: int, alpha_lo: float, alpha_max: float,
                 device_ptr=None):
        """snap: host (n, dim) array — or, with device_ptr=(ptr, n, dim, dtype), a snapshot that is
        already resident on the context's GPU (bench / sharded driver)."""
        self.ctx = ctx
        self._lib = ctx._lib
        if device_ptr is None:
            snap = _cloud(snap)
            self.n, self.dim = snap.shape
            self.dtype = snap.dtype
        else:
            _, self.n, self.dim, dt = device_ptr
            self.dtype = np.dtype(dt)
        self.n_fixed = int(n_fixed)
        sd = L.SpacingDesc()
        self._sp_keep = None
        if np.isscalar(spacing):
            sd.kind, sd.constant, sd.per_point = 0, float(spacing), None
        elif isinstance(spacing, dict):  # a law the library evaluates itself (LogLike / BoundaryLayerSpacing)
            sd, self._sp_keep = _law_desc(spacing, self.dtype, self.dim)
        else:
            sp = np.ascontiguousarray(spacing, dtype=self.dtype)
            if sp.shape != (self.n,):
                raise L.WtpArgumentError("per-point spacing needs one value per snapshot point")
            self._sp_keep = sp
            sd.kind, sd.constant, sd.per_point = 1, 0.0, sp.ctypes.data
        fd = L.ForceDesc(int(force["kind"]), float(force["beta"]), float(force.get("u0", 1.0)),
                         float(force.get("gamma", 3.0)))
        if device_ptr is None:
            rc = self._lib.wtp_relax_init(ctx._h, _vp(snap), self.n, self.n_fixed, self.dim, _dtype_code(self.dtype),
                                          C.byref(sd), C.byref(fd), int(k), float(alpha_lo), float(alpha_max))
        else:
            rc = self._lib.wtp_relax_init_dev(ctx._h, C.c_void_p(device_ptr[0]), self.n, self.n_fixed, self.dim,
                                              _dtype_code(self.dtype), C.byref(sd), C.byref(fd), int(k),
                                              float(alpha_lo), float(alpha_max))
        L.check(ctx._h, rc)
        self._open = True

    def step(self, rebuild: bool = True):
        st = L.StepStats()
        L.check(self.ctx._h, self._lib.wtp_relax_step(self.ctx._h, int(bool(rebuild)), C.byref(st)))
        return _stats_dict(st)

    def run(self, n_iters: int, rebuild_every: int = 1):
        conv = np.zeros(max(n_iters, 1), dtype=np.float64)
        st = L.StepStats()
        L.check(self.ctx._h, self._lib.wtp_relax_run(self.ctx._h, int(n_iters), int(rebuild_every), _vp(conv),
                                                     C.byref(st)))
        return conv[:n_iters], _stats_dict(st)

    def run_async_free(self, n_iters: int, rebuild_every: int = 1):
        """n_iters sweeps with no read-back at all (bench inner loop)."""
        L.check(self.ctx._h, self._lib.wtp_relax_run(self.ctx._h, int(n_iters), int(rebuild_every), None, None))

    def run_until(self, max_iters: int, rebuild_every: int = 1, tol: float = 1e-6, stall_after: int = 50,
                  cv_target: float = 0.0):
        """The loop with the reference's stop rules evaluated on the device (src/repel.jl:305-334): returns
        (conv, reason, last stats); reason 0 max_iters, 1 tol, 2 cv_target (positions reverted), 3 stall."""
        conv = np.zeros(max(max_iters, 1), dtype=np.float64)
        st = L.StepStats()
        n_done, reason = C.c_int(0), C.c_int(0)
        L.check(self.ctx._h, self._lib.wtp_relax_run_until(self.ctx._h, int(max_iters), int(rebuild_every), float(tol),
                                                           int(stall_after), float(cv_target), _vp(conv), C.byref(n_done),
                                                           C.byref(reason), C.byref(st)))
        return conv[: n_done.value], int(reason.value), _stats_dict(st)

    def positions(self):
        out = np.empty((self.n - self.n_fixed, self.dim), dtype=self.dtype)
        L.check(self.ctx._h, self._lib.wtp_relax_get(self.ctx._h, _vp(out)))
        return out

    def positions_dev(self, d_out_ptr: int):
        """Movable points into device memory ((n - n_fixed) x dim of dtype)."""
        L.check(self.ctx._h, self._lib.wtp_relax_get_dev(self.ctx._h, C.c_void_p(d_out_ptr)))

    def point_data(self):
        m = self.n - self.n_fixed
        forces = np.empty(m, dtype=self.dtype)
        nn_dist = np.empty(m, dtype=self.dtype)
        nn_id = np.empty(m, dtype=np.int32)
        L.check(self.ctx._h, self._lib.wtp_relax_get_point_data(self.ctx._h, _vp(forces), _vp(nn_dist), _vp(nn_id)))
        return dict(forces=forces, nn_dist=nn_dist, nn_id=nn_id)

    def set_point(self, i: int, xyz):
        v = np.ascontiguousarray(xyz, dtype=self.dtype).reshape(self.dim)
        L.check(self.ctx._h, self._lib.wtp_relax_set(self.ctx._h, int(i), _vp(v)))

    def set_points(self, idx, xyz):
        """Place many movable points at once (indices strictly increasing)."""
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        v = np.ascontiguousarray(xyz, dtype=self.dtype).reshape(len(idx), self.dim)
        L.check(self.ctx._h, self._lib.wtp_relax_set_batch(self.ctx._h, _vp(idx), _vp(v), len(idx)))

    def revert(self):
        L.check(self.ctx._h, self._lib.wtp_relax_revert(self.ctx._h))

    def spacings(self):
        """The per-point spacings the session holds, snapshot order (src/repel.jl:209,251)."""
        out = np.empty(self.n, dtype=self.dtype)
        L.check(self.ctx._h, self._lib.wtp_relax_get_spacing(self.ctx._h, _vp(out)))
        return out

    def spacing_certs(self):
        """Diagnostic (wtp_relax_get_spacing_certs), device-evaluated laws only: per movable point the winning tree node
        of its last boundary search (-1: none yet), where it stood then and the bound that search left, and the winner's
        coordinates: dict(hint int32[m], x_ref (m, 3), lb [m], winner (m, 3)); winner rows are NaN where hint < 0."""
        m = self.n - self.n_fixed
        hint = np.empty(m, dtype=np.int32)
        cert = np.empty((m, 4), dtype=self.dtype)
        winner = np.full((m, 3), np.nan, dtype=self.dtype)
        L.check(self.ctx._h, self._lib.wtp_relax_get_spacing_certs(self.ctx._h, _vp(hint), _vp(cert), _vp(winner)))
        return dict(hint=hint, x_ref=cert[:, :3].copy(), lb=cert[:, 3].copy(), winner=winner)

    def set_spacing(self, spacing):
        sp = np.ascontiguousarray(spacing, dtype=self.dtype)
        if sp.shape != (self.n,):
            raise L.WtpArgumentError("per-point spacing needs one value per snapshot point")
        L.check(self.ctx._h, self._lib.wtp_relax_set_spacing(self.ctx._h, _vp(sp)))

    # ---- wall rule of the octree method (src/repel.jl:448-469) ----------------------------------
    def set_wall(self, n_boundary: int, offset_dist: float):
        """After every sweep: boundary points are re-projected onto the context's mesh, volume points
        that left the domain return to their previous position (stats['n_escaped'])."""
        L.check(self.ctx._h, self._lib.wtp_relax_set_wall(self.ctx._h, int(n_boundary), float(offset_dist)))

    def get_wall(self, clear_escaped: bool = False):
        m = self.n - self.n_fixed
        tri = np.empty(m, dtype=np.int32)
        is_bnd = np.empty(m, dtype=np.uint8)
        esc = np.empty(m, dtype=np.uint8)
        L.check(self.ctx._h, self._lib.wtp_relax_get_wall(self.ctx._h, _vp(tri), _vp(is_bnd), _vp(esc),
                                                          int(bool(clear_escaped))))
        return dict(tri=tri, is_bnd=is_bnd.astype(bool), escaped=esc.astype(bool))

    def query_knn(self, xyz, k: int, return_dist: bool = False):
        """k nearest snapshot points (of the last rebuild) of arbitrary positions: (nq, k) indices."""
        q = np.ascontiguousarray(np.atleast_2d(xyz), dtype=self.dtype)
        if q.shape[1] != self.dim:
            raise L.WtpArgumentError("queries must have the session's dimension")
        idx = np.empty((len(q), int(k)), dtype=np.int32)
        dist = np.empty((len(q), int(k)), dtype=self.dtype) if return_dist else None
        L.check(self.ctx._h, self._lib.wtp_relax_query_knn(self.ctx._h, _vp(q), len(q), int(k), _vp(idx), _vp(dist)))
        return (idx, dist) if return_dist else idx

    def set_wall_flags(self, is_bnd, tri):
        m = self.n - self.n_fixed
        b = np.ascontiguousarray(is_bnd, dtype=np.uint8)
        t = np.ascontiguousarray(tri, dtype=np.int32)
        if b.shape != (m,) or t.shape != (m,):
            raise L.WtpArgumentError("wall flags need one entry per movable point")
        L.check(self.ctx._h, self._lib.wtp_relax_set_wall_flags(self.ctx._h, _vp(b), _vp(t)))

    # ---- sharded sessions ------------------------------------------------------
    def layers_dev(self, axis: int, lo_in: float, hi_in: float, lo_out: float, hi_out: float, d_lo_ptr: int,
                   d_hi_ptr: int, cap: int):
        """Boundary layers of the movable points into device buffers of `cap` packed 4-vectors each;
        returns (n_lo, n_hi, n_stray_lo, n_stray_hi) — the true counts, also when they exceed cap."""
        cnt = (C.c_int64 * 4)()
        rc = self._lib.wtp_relax_layers_dev(self.ctx._h, int(axis), float(lo_in), float(hi_in), float(lo_out),
                                            float(hi_out), C.c_void_p(d_lo_ptr), C.c_void_p(d_hi_ptr), int(cap), cnt)
        L.check(self.ctx._h, rc)
        return tuple(int(c) for c in cnt)

    def step_layers(self, rebuild, axis, lo_in, hi_in, lo_out, hi_out, d_lo_ptr, d_hi_ptr, cap):
        """One sweep + the boundary layers of the positions it produced, one synchronisation for both:
        returns (stats, (n_lo, n_hi, n_stray_lo, n_stray_hi))."""
        st = L.StepStats()
        cnt = (C.c_int64 * 4)()
        rc = self._lib.wtp_relax_step_layers(self.ctx._h, int(bool(rebuild)), C.byref(st), int(axis), float(lo_in),
                                             float(hi_in), float(lo_out), float(hi_out), C.c_void_p(d_lo_ptr),
                                             C.c_void_p(d_hi_ptr), int(cap), cnt)
        L.check(self.ctx._h, rc)
        return _stats_dict(st), tuple(int(c) for c in cnt)

    def step_layers3(self, rebuild, axes_mask, lo_in3, hi_in3, lo_out3, hi_out3, d_lo_ptrs, d_hi_ptrs, cap):
        """step_layers along up to three axes (bit a of axes_mask), one synchronisation for everything:
        returns (stats, [(n_lo, n_hi, n_stray_lo, n_stray_hi)] * 3)."""
        st = L.StepStats()
        cnt = (C.c_int64 * 12)()
        d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
        p3 = lambda v: (C.c_void_p * 3)(*[C.c_void_p(int(x)) for x in v])
        rc = self._lib.wtp_relax_step_layers3(self.ctx._h, int(bool(rebuild)), C.byref(st), int(axes_mask), d3(lo_in3),
                                              d3(hi_in3), d3(lo_out3), d3(hi_out3), p3(d_lo_ptrs), p3(d_hi_ptrs), int(cap), cnt)
        L.check(self.ctx._h, rc)
        return _stats_dict(st), [tuple(int(cnt[4 * a + j]) for j in range(4)) for a in range(3)]

    def set_fixed_dev(self, d_fixed4_ptr: int, n_fixed_new: int):
        """Replace the fixed head of the snapshot by n_fixed_new packed 4-vectors in device memory."""
        rc = self._lib.wtp_relax_set_fixed_dev(self.ctx._h, C.c_void_p(d_fixed4_ptr) if n_fixed_new else None,
                                               int(n_fixed_new))
        L.check(self.ctx._h, rc)
        self.n += int(n_fixed_new) - self.n_fixed
        self.n_fixed = int(n_fixed_new)

    def set_coverage_box(self, lo3, hi3):
        """Block decompositions: the snapshot is complete inside the box lo3 .. hi3 (ends may be +-inf)."""
        lo = (C.c_double * 3)(*[float(v) for v in lo3])
        hi = (C.c_double * 3)(*[float(v) for v in hi3])
        L.check(self.ctx._h, self._lib.wtp_relax_set_coverage_box(self.ctx._h, lo, hi))

    def set_coverage(self, axis: int, lo: float = 0.0, hi: float = 0.0):
        """The snapshot is complete for lo <= coord[axis] <= hi (slab + ghost layers); sweeps report
        in n_uncovered the points whose neighbourhood reaches past it.  axis < 0: unlimited."""
        L.check(self.ctx._h, self._lib.wtp_relax_set_coverage(self.ctx._h, int(axis), float(lo), float(hi)))

    def close(self):
        if self._open and self.ctx._h:
            self._lib.wtp_relax_end(self.ctx._h)
        self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None or _default_ctx._h is None:
        _default_ctx = Context(0)
    return _default_ctx
