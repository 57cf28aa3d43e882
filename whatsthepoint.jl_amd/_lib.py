"""ctypes binding of libwtp.so (include/wtp.h).  Loading fails loudly: there is no CPU path."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# WTP_LIB selects another build of the same sources (A/B experiments); default: csrc/libwtp.so
SO_PATH = os.environ.get("WTP_LIB") or os.path.join(CSRC, "libwtp.so")

WTP_OK, WTP_ERR_ARG, WTP_ERR_OOM, WTP_ERR_HIP, WTP_ERR_STATE, WTP_ERR_NO_DEVICE, WTP_ERR_INTERNAL = range(7)
WTP_F32, WTP_F64 = 0, 1
WTP_SPACING_CONSTANT, WTP_SPACING_PER_POINT, WTP_SPACING_LOGLIKE, WTP_SPACING_BOUNDARY_LAYER = range(4)


class WtpError(RuntimeError):
    """Non-argument failure reported by libwtp (the Julia shim raises ErrorException)."""

    def __init__(self, code, msg):
        super().__init__(f"libwtp status {code}: {msg}")
        self.code = code


class WtpArgumentError(ValueError):
    """WTP_ERR_ARG: the reference throws ArgumentError for the same input (src/repel.jl:74)."""


class ForceDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("beta", C.c_double), ("u0", C.c_double), ("gamma", C.c_double)]


class SpacingDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("constant", C.c_double), ("per_point", C.c_void_p),
                ("p0", C.c_double), ("p1", C.c_double), ("p2", C.c_double),
                ("boundary_xyz", C.c_void_p), ("n_boundary", C.c_int64)]


class StepStats(C.Structure):
    _fields_ = [
        ("max_force", C.c_double), ("sum_u", C.c_double), ("sum_u2", C.c_double),
        ("n_move", C.c_int64), ("argmin_i", C.c_int64), ("argmin_j", C.c_int64),
        ("argmin_r", C.c_double), ("n_fallback", C.c_int64), ("n_uncovered", C.c_int64),
        ("n_escaped", C.c_int64),
    ]


class BlockDesc(C.Structure):
    _fields_ = [("rank", C.c_int32), ("nranks", C.c_int32), ("boxes", C.POINTER(C.c_double)),
                ("ghost_width", C.c_double), ("margin", C.c_double)]


class BlockInfo(C.Structure):
    _fields_ = [("n_owned", C.c_int64), ("n_ghost", C.c_int64), ("n_sent_rows", C.c_int64), ("n_recv_rows", C.c_int64),
                ("n_emigrated", C.c_int64), ("n_immigrated", C.c_int64), ("n_peers", C.c_int32), ("widened", C.c_int32),
                ("host_syncs", C.c_int32), ("redone", C.c_int32), ("ghost_width", C.c_double), ("overlapped", C.c_int32),
                ("reserved", C.c_int32)]


class BlockTopoInfo(C.Structure):
    _fields_ = [("width", C.c_double), ("n_ghost", C.c_int64), ("n_recv_rows", C.c_int64), ("n_peers", C.c_int32),
                ("widened", C.c_int32), ("host_syncs", C.c_int32), ("reserved", C.c_int32)]


class KnnStats(C.Structure):
    """struct wtp_knn_stats: the sums behind metrics / spacing_metrics / spacing_fidelity_metrics."""
    _fields_ = [("n", C.c_int64), ("k_eff", C.c_int32), ("has_spacing", C.c_int32),
                ("sum_mean", C.c_double), ("sum_std", C.c_double), ("sum_max", C.c_double), ("sum_min", C.c_double),
                ("nn_min", C.c_double), ("nn_max", C.c_double), ("nn_min_i", C.c_int64), ("nn_max_i", C.c_int64),
                ("sum_err", C.c_double), ("ssd_err", C.c_double), ("max_err", C.c_double),
                ("sum_u", C.c_double), ("ssd_u", C.c_double), ("sum_coord", C.c_int64)]


class NormalGraphInfo(C.Structure):
    """wtp_normal_graph_info: what wtp_orient_normals / wtp_normal_components report about the row graph."""
    _fields_ = [("n_edges", C.c_int64), ("n_components", C.c_int64), ("n_reached", C.c_int64), ("n_flipped", C.c_int64),
                ("start", C.c_int64), ("rounds", C.c_int32), ("host_syncs", C.c_int32)]


class SampleInfo(C.Structure):
    """wtp_sample_info: what wtp_mesh_sample reports about a run."""
    _fields_ = [("n_points", C.c_int64), ("n_darts", C.c_int64), ("batch", C.c_int64), ("stop_reason", C.c_int32),
                ("n_batches", C.c_int32), ("rounds_max", C.c_int32), ("host_syncs", C.c_int32),
                ("total_area", C.c_double), ("r_min", C.c_double), ("r_max", C.c_double)]


class FillInfo(C.Structure):
    """wtp_fill_info: what wtp_mesh_fill and wtp_loops_fill report about a run."""
    _fields_ = [("n_points", C.c_int64), ("n_darts", C.c_int64), ("n_inside", C.c_int64), ("n_seeds", C.c_int64),
                ("batch", C.c_int64), ("stop_reason", C.c_int32), ("n_batches", C.c_int32), ("rounds_max", C.c_int32),
                ("host_syncs", C.c_int32), ("bbox_volume", C.c_double), ("r_min", C.c_double), ("r_max", C.c_double)]


class FrontInfo(C.Structure):
    """wtp_front_info: what wtp_mesh_front reports about a run."""
    _fields_ = [("n_points", C.c_int64), ("n_parents", C.c_int64), ("n_candidates", C.c_int64), ("n_inside", C.c_int64),
                ("n_seeds", C.c_int64), ("batch", C.c_int64), ("stop_reason", C.c_int32), ("n_batches", C.c_int32),
                ("rounds_max", C.c_int32), ("host_syncs", C.c_int32), ("r_min", C.c_double), ("r_max", C.c_double)]


class NodeTreeInfo(C.Structure):
    """wtp_node_tree_info: what wtp_node_tree_build reports about the tree."""
    _fields_ = [("n_leaves", C.c_int64), ("n_interior", C.c_int64), ("n_boundary", C.c_int64), ("n_exterior", C.c_int64),
                ("n_boxes", C.c_int64), ("depth_max", C.c_int32), ("n_levels", C.c_int32), ("balance_rounds", C.c_int32),
                ("host_syncs", C.c_int32), ("integral", C.c_double), ("h_min", C.c_double), ("max_points_auto", C.c_int64),
                ("origin", C.c_double * 3), ("root_size", C.c_double), ("absolute_min", C.c_double)]


class NodePlaceInfo(C.Structure):
    """wtp_node_place_info: what wtp_node_place reports about a placement."""
    _fields_ = [("n_points", C.c_int64), ("n_interior", C.c_int64), ("n_candidates", C.c_int64), ("n_accepted", C.c_int64),
                ("n_deficit", C.c_int64), ("W_int", C.c_double), ("W_ns", C.c_double), ("placement", C.c_int32),
                ("host_syncs", C.c_int32)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                          C.POINTER(C.c_void_p), C.POINTER(C.c_int64))


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("allgather", ALLGATHER_FN), ("exchange", EXCHANGE_FN)]


# every symbol include/wtp.h declares: name -> (restype, argtypes)
_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
SIGNATURES = {
    "wtp_create": (_i, [C.POINTER(_i), _i, C.POINTER(_vp)]),
    "wtp_destroy": (_i, [_vp]),
    "wtp_last_error": (C.c_char_p, [_vp]),
    "wtp_version": (C.c_char_p, []),
    "wtp_knn": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp, _vp]),
    "wtp_knn_dev": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp, _vp]),
    "wtp_radius_count": (_i, [_vp, _vp, _i64, _i, _i, _d, _vp]),
    "wtp_radius_fill": (_i, [_vp, _vp, _vp]),
    "wtp_radius_offsets": (_i, [_vp, _vp, _i64, _i, _i, _d, _vp]),
    "wtp_radius_marks": (_i, [_vp, _vp, _i64, C.POINTER(_d)]),
    "wtp_relax_init": (_i, [_vp, _vp, _i64, _i64, _i, _i, C.POINTER(SpacingDesc), C.POINTER(ForceDesc), _i, _d, _d]),
    "wtp_relax_init_dev": (_i, [_vp, _vp, _i64, _i64, _i, _i, C.POINTER(SpacingDesc), C.POINTER(ForceDesc), _i, _d, _d]),
    "wtp_relax_step": (_i, [_vp, _i, C.POINTER(StepStats)]),
    "wtp_relax_run": (_i, [_vp, _i, _i, _vp, C.POINTER(StepStats)]),
    "wtp_relax_run_until": (_i, [_vp, _i, _i, _d, _i, _d, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(StepStats)]),
    "wtp_relax_get": (_i, [_vp, _vp]),
    "wtp_relax_get_dev": (_i, [_vp, _vp]),
    "wtp_relax_get_point_data": (_i, [_vp, _vp, _vp, _vp]),
    "wtp_relax_set": (_i, [_vp, _i64, _vp]),
    "wtp_relax_revert": (_i, [_vp]),
    "wtp_relax_set_batch": (_i, [_vp, _vp, _vp, _i64]),
    "wtp_relax_set_spacing": (_i, [_vp, _vp]),
    "wtp_relax_end": (_i, [_vp]),
    "wtp_relax_get_spacing": (_i, [_vp, _vp]),
    "wtp_relax_get_spacing_certs": (_i, [_vp, _vp, _vp, _vp]),
    "wtp_spacing_eval": (_i, [_vp, C.POINTER(SpacingDesc), _vp, _i64, _i, _i, _vp]),
    "wtp_pca_normals": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp]),
    "wtp_knn_stats": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _d, _d, C.POINTER(KnnStats), _vp, _vp]),
    "wtp_knn_stats_dev": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _d, _d, C.POINTER(KnnStats), _vp, _vp]),
    "wtp_orient_normals": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, C.POINTER(NormalGraphInfo)]),
    "wtp_orient_normals_dev": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, C.POINTER(NormalGraphInfo)]),
    "wtp_normal_components": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _d, _vp, C.POINTER(NormalGraphInfo)]),
    "wtp_gradient_limit": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _d, _d, _i, _vp, C.POINTER(_i)]),
    "wtp_mesh_set": (_i, [_vp, _vp, _i64, _vp, _i64, _i]),
    "wtp_mesh_clear": (_i, [_vp]),
    "wtp_mesh_face_normals": (_i, [_vp, _vp]),
    "wtp_mesh_bounds": (_i, [_vp, _vp]),
    "wtp_mesh_query": (_i, [_vp, _vp, _i64, _i, _d, _vp, _vp, _vp, _vp, _vp]),
    "wtp_mesh_sample": (_i, [_vp, C.POINTER(SpacingDesc), _d, _i64, _i64, C.c_uint64, _i64, C.POINTER(SampleInfo)]),
    "wtp_mesh_sample_get": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "wtp_mesh_sample_get_dev": (_i, [_vp, _vp, _vp, _vp]),
    "wtp_mesh_sample_darts": (_i, [_vp, C.POINTER(SpacingDesc), _d, C.c_uint64, _i64, _i64, _vp, _vp, _vp]),
    "wtp_mesh_fill": (_i, [_vp, C.POINTER(SpacingDesc), _d, _vp, _i64, _i64, _i64, C.c_uint64, _i64, C.POINTER(FillInfo)]),
    "wtp_mesh_fill_get": (_i, [_vp, _vp, _vp, _vp]),
    "wtp_mesh_fill_get_dev": (_i, [_vp, _vp, _vp]),
    "wtp_mesh_fill_darts": (_i, [_vp, C.POINTER(SpacingDesc), _d, C.c_uint64, _i64, _i64, _vp, _vp, _vp]),
    "wtp_mesh_front": (_i, [_vp, C.POINTER(SpacingDesc), _i64, _vp, _i64, _i64, C.c_uint64, _i64, C.POINTER(FrontInfo)]),
    "wtp_mesh_front_get": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "wtp_mesh_front_get_dev": (_i, [_vp, _vp, _vp]),
    "wtp_mesh_front_candidates": (_i, [_vp, C.POINTER(SpacingDesc), C.c_uint64, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "wtp_loops_set": (_i, [_vp, _vp, _i64, _vp, _i64, _i]),
    "wtp_loops_clear": (_i, [_vp]),
    "wtp_loops_bounds": (_i, [_vp, _vp, C.POINTER(_i64)]),
    "wtp_loops_query": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp, _vp]),
    "wtp_loops_fill": (_i, [_vp, C.POINTER(SpacingDesc), _d, _vp, _i64, _i64, _i64, C.c_uint64, _i64, C.POINTER(FillInfo)]),
    "wtp_loops_fill_get": (_i, [_vp, _vp, _vp, _vp]),
    "wtp_loops_fill_get_dev": (_i, [_vp, _vp, _vp]),
    "wtp_loops_fill_darts": (_i, [_vp, C.POINTER(SpacingDesc), _d, C.c_uint64, _i64, _i64, _vp, _vp, _vp]),
    "wtp_node_tree_build": (_i, [_vp, C.POINTER(SpacingDesc), _d, _d, C.POINTER(NodeTreeInfo)]),
    "wtp_node_tree_get": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "wtp_node_tree_locate": (_i, [_vp, _vp, _i64, _i, _vp]),
    "wtp_node_tree_clear": (_i, [_vp]),
    "wtp_node_place": (_i, [_vp, _i, _i64, _d, C.c_uint64, C.POINTER(NodePlaceInfo)]),
    "wtp_node_place_get": (_i, [_vp, _vp, _vp]),
    "wtp_node_place_get_dev": (_i, [_vp, _vp, _vp]),
    "wtp_relax_set_wall": (_i, [_vp, _i64, _d]),
    "wtp_relax_get_wall": (_i, [_vp, _vp, _vp, _vp, _i]),
    "wtp_relax_set_wall_flags": (_i, [_vp, _vp, _vp]),
    "wtp_relax_query_knn": (_i, [_vp, _vp, _i64, _i, _vp, _vp]),
    "wtp_isinside_greens": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _i, _vp, _vp]),
    "wtp_isinside_winding": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _vp, _vp]),
    "wtp_set_stream": (_i, [_vp, _vp, _i]),
    "wtp_relax_layers_dev": (_i, [_vp, _i, _d, _d, _d, _d, _vp, _vp, _i64, C.POINTER(_i64)]),
    "wtp_relax_set_fixed_dev": (_i, [_vp, _vp, _i64]),
    "wtp_relax_step_layers": (_i, [_vp, _i, C.POINTER(StepStats), _i, _d, _d, _d, _d, _vp, _vp, _i64, C.POINTER(_i64)]),
    "wtp_relax_step_layers3": (_i, [_vp, _i, C.POINTER(StepStats), _i, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_vp), C.POINTER(_vp), _i64,
                                    C.POINTER(_i64)]),
    "wtp_relax_set_coverage": (_i, [_vp, _i, _d, _d]),
    "wtp_relax_set_coverage_box": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "wtp_comm_unique_id": (_i, [_vp, _vp]),
    "wtp_comm_init": (_i, [_vp, _vp, _i, _i]),
    "wtp_comm_finalize": (_i, [_vp]),
    "wtp_comm_exchange_rows": (_i, [_vp, _i, _i, _vp, _i64, _vp, _i64, _vp, _vp, _i64, C.POINTER(_i64), C.POINTER(_i64)]),
    "wtp_comm_allreduce_stats": (_i, [_vp, C.POINTER(StepStats)]),
    "wtp_block_set_transport": (_i, [_vp, C.POINTER(Transport)]),
    "wtp_block_set_wall": (_i, [_vp, _vp, _i64]),
    "wtp_block_open": (_i, [_vp, C.POINTER(BlockDesc), _vp, _vp, _i64, C.POINTER(SpacingDesc), C.POINTER(ForceDesc), _i, _d, _d]),
    "wtp_block_step": (_i, [_vp, C.POINTER(StepStats), C.POINTER(BlockInfo)]),
    "wtp_block_run": (_i, [_vp, _i, _vp, C.POINTER(StepStats), C.POINTER(BlockInfo)]),
    "wtp_block_run_until": (_i, [_vp, _i, _d, _i, _d, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(StepStats)]),
    "wtp_block_get": (_i, [_vp, _vp, _vp, _i64, C.POINTER(_i64)]),
    "wtp_block_close": (_i, [_vp]),
    "wtp_block_grid": (_i, [_i, C.POINTER(_i)]),
    "wtp_block_morton_rank": (_i, [_i, _i, _i, C.POINTER(_i)]),
    "wtp_block_knn": (_i, [_vp, _i, _i, _vp, _vp, _i64, _i, _i, _d, _vp, _vp, C.POINTER(BlockTopoInfo)]),
    "wtp_block_knn_stats": (_i, [_vp, _i, _i, _vp, _vp, _i64, _i, _vp, _d, _d, _d, C.POINTER(KnnStats), _vp,
                                C.POINTER(BlockTopoInfo)]),
    "wtp_block_radius_offsets": (_i, [_vp, _i, _i, _vp, _vp, _i64, _d, _vp, C.POINTER(BlockTopoInfo)]),
    "wtp_block_radius_fill": (_i, [_vp, _vp]),
    "wtp_comm_exchange_peers": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_vp), C.POINTER(_i64)]),
    "wtp_comm_allgather_dev": (_i, [_vp, _vp, _vp, _i64]),
    "wtp_timers_get": (_i, [_vp, C.POINTER(_d)]),
    "wtp_timers_reset": (_i, [_vp]),
    "wtp_debug_diag": (_i, [_vp, C.POINTER(C.c_ulonglong)]),
    "wtp_gen_uniform_dev": (_i, [_vp, C.c_uint64, _i64, _i64, _i, _i, _vp]),
}

_lib = None


def build(verbose: bool = False) -> str:
    """Compile libwtp.so for gfx950 with hipcc (csrc/Makefile).  Works without a GPU."""
    res = subprocess.run(["make", "-C", CSRC, "-j4"], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libwtp.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    if verbose:
        print(res.stdout[-2000:])
    return SO_PATH


def load():
    """dlopen libwtp.so and bind every symbol of include/wtp.h (no compute is called)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 and a process
    # that maps the system copy first (through libwtp) leaves torch without devices ("No HIP GPUs
    # are available", observed).  Mapping torch's copy first makes both sides share it.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(ctx_handle, rc: int):
    if rc == WTP_OK:
        return
    msg = load().wtp_last_error(ctx_handle)
    msg = msg.decode("utf-8", "replace") if msg else ""
    if rc == WTP_ERR_ARG:
        raise WtpArgumentError(msg)
    raise WtpError(rc, msg)
