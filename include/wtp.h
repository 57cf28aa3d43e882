/*
 * wtp.h — C ABI of libwtp, the MI355X (gfx950) neighbour/stencil engine behind
 * WhatsThePoint.jl's `set_topology` / `repel` hot path.
 *
 * Every entry point below replaces the body of one reference function (citations are
 * relative to the reference checkout, JuliaMeshless/WhatsThePoint.jl v0.3.1).  The
 * reference has no FFI seam of its own: the seam is the set of Julia functions whose
 * bodies a maintainer swaps for `ccall`s (INTEGRATION.md shows the Julia side).
 *
 * Conventions
 *  - plain C, plain pointers and sizes; no exceptions or signals cross the ABI;
 *  - every function returns a wtp_status (0 = OK); wtp_last_error(ctx) gives the text;
 *  - host entry points (`xyz`, `idx_out`, ...) take HOST pointers, block until the
 *    result is on the host; `_dev` entry points take DEVICE pointers on the context's
 *    GPU and only enqueue + synchronise the context's stream;
 *  - coordinates are AoS `n x dim` contiguous (the in-memory layout of Julia's
 *    Vector{SVector{D,T}} / Vector{Point}, src/repel.jl:216), dim in {2,3};
 *  - indices are int32, 0-based, in the caller's (snapshot-global) numbering:
 *    boundary points first, then volume (src/cloud.jl:235-237);
 *  - canonical neighbour order: ascending (d2, index) with
 *    d2 = ((dx*dx + dy*dy) + dz*dz) evaluated in the cloud's float type, no FMA
 *    contraction; distances returned are sqrt(d2) in that type;
 *  - a context is not thread-safe (one caller at a time); several contexts may coexist.
 */
#ifndef WTP_H
#define WTP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wtp_ctx wtp_ctx;

typedef enum wtp_status {
    WTP_OK = 0,
    WTP_ERR_ARG = 1,      /* bad argument: the Julia shim maps it to ArgumentError (src/repel.jl:74) */
    WTP_ERR_OOM = 2,      /* device or host allocation failed */
    WTP_ERR_HIP = 3,      /* HIP runtime / kernel error */
    WTP_ERR_STATE = 4,    /* call out of order (e.g. relax_step before relax_init) */
    WTP_ERR_NO_DEVICE = 5,/* no usable gfx950 device: the library never falls back to a CPU path */
    WTP_ERR_INTERNAL = 6  /* a bound the algorithm guarantees was exceeded (wtp_mesh_sample's round limit): a defect */
} wtp_status;

typedef enum wtp_dtype { WTP_F32 = 0, WTP_F64 = 1 } wtp_dtype;

/* Force laws of src/repel_forces.jl:37,57-60,96-100,124-127 (u = r/s). */
typedef enum wtp_force_kind {
    WTP_FORCE_INVERSE_DISTANCE = 0,    /* 1/(u^2+beta)^2                       */
    WTP_FORCE_SPACING_EQUILIBRIUM = 1, /* (1-u^2)/(u^2+beta)^2                 */
    WTP_FORCE_CLIPPED_SPACING = 2,     /* max((u0^2-u^2)/(u^2+beta)^2, 0)  (default) */
    WTP_FORCE_STRONG_SPACING = 3       /* (1-u^2)/(u^2+beta)^gamma             */
} wtp_force_kind;

typedef struct wtp_force_desc {
    int32_t kind;  /* wtp_force_kind */
    double beta;   /* softening, > 0 */
    double u0;     /* support radius (clipped law only) */
    double gamma;  /* core strength (strong law only) */
} wtp_force_desc;

/* Spacing callables of src/discretization/spacings.jl invoked inside the sweep
 * (src/repel.jl:209,251,260). */
typedef enum wtp_spacing_kind {
    WTP_SPACING_CONSTANT = 0,  /* ConstantSpacing: spacings.jl:35-39 */
    WTP_SPACING_PER_POINT = 1, /* host-evaluated s[n] in snapshot order (any callable); refresh with
                                  wtp_relax_set_spacing */
    WTP_SPACING_LOGLIKE = 2,   /* LogLike: spacings.jl:67-72, p0 = base_size, p1 = growth_rate       */
    WTP_SPACING_BOUNDARY_LAYER = 3 /* BoundaryLayerSpacing: spacings.jl:121-133, p0 = at_wall,
                                  p1 = bulk, p2 = layer_thickness                                 */
} wtp_spacing_kind;

typedef struct wtp_spacing_desc {
    int32_t kind;            /* wtp_spacing_kind */
    double constant;         /* CONSTANT: the spacing (unitless, as ustrip gives it) */
    const void* per_point;   /* PER_POINT: host array of n values of the cloud's dtype */
    double p0, p1, p2;       /* LOGLIKE / BOUNDARY_LAYER parameters (unitless)          */
    const void* boundary_xyz;/* LOGLIKE / BOUNDARY_LAYER: host array, n_boundary x dim of the cloud's dtype:
                                the points the law measures its distance to (spacings.jl:17-28); they
                                are evaluated on the device at every point's current position, every
                                sweep (src/repel.jl:251,260) */
    int64_t n_boundary;
} wtp_spacing_desc;

/* Scalars the host-side stop logic of src/repel.jl:293-334 needs after one sweep. */
typedef struct wtp_step_stats {
    double max_force;  /* maximum(forces), forces[id] = |F|*s         (repel.jl:283,293) */
    double sum_u;      /* sum_i nn_dist[i]/spacings[i+n_fixed]        (repel.jl:374-386) */
    double sum_u2;     /* sum_i (nn_dist[i]/spacings[i+n_fixed])^2                        */
    int64_t n_move;    /* number of movable points the sums run over                     */
    int64_t argmin_i;  /* closest pair (repel.jl:396-403): snapshot-global index of the  */
    int64_t argmin_j;  /*   movable point with the smallest nn_dist, and its neighbour;  */
    double argmin_r;   /*   -1/-1/inf when n_move == 0                                    */
    int64_t n_fallback;/* queries that left the 27-cell fast path (diagnostic)           */
    int64_t n_uncovered;/* sharded sessions: queries whose neighbourhood reaches past the
                          covered range (wtp_relax_set_coverage); 0 when unlimited        */
    int64_t n_escaped; /* octree method: volume points the wall rule sent back this sweep
                          (repel.jl:466-467); 0 without wtp_relax_set_wall                */
} wtp_step_stats;

/* ---- lifetime ------------------------------------------------------------------ */

/* Create a context on one GPU (n_dev must be 1: multi-GPU runs use one context per
 * process/GPU, sharded by the host driver — SURVEY.md §8e). */
int wtp_create(const int* device_ordinals, int n_dev, wtp_ctx** out);
int wtp_destroy(wtp_ctx* ctx);
/* UTF-8 text of the last non-zero status on this context ("" if none).  ctx may be
 * NULL: then the text of the last failed wtp_create on this thread. */
const char* wtp_last_error(const wtp_ctx* ctx);
/* Library version string, for the binding's sanity check. */
const char* wtp_version(void);

/* ---- KNNTopology / KNearestSearch ------------------------------------------------ */

/* Replaces _build_knn_neighbors (src/topology.jl:79-84) and the KNearestSearch +
 * search/searchdists wrappers (src/neighbors.jl:1-21).
 * include_self = 0: row i = the k nearest OTHER points (self removed by index), as
 *                   set_topology stores them (k+1 query, first hit dropped);
 * include_self = 1: row i = the k nearest points including i itself (raw `search`
 *                   result: self first, test/neighbors.jl:54-56).
 * idx_out: n*k int32 (row-major); dist_out: n*k values of dtype, or NULL.
 * Errors: k < 1, or k > n - (include_self ? 0 : 1)  (the reference's kd-tree throws
 * for k+1 > n), dim not in {2,3}, n < 1. */
int wtp_knn(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k,
            int include_self, int32_t* idx_out, void* dist_out);
/* Same, device-resident input/output (bench and the sharded driver use this). */
int wtp_knn_dev(wtp_ctx* ctx, const void* d_xyz, int64_t n, int dim, int dtype, int k,
                int include_self, int32_t* d_idx_out, void* d_dist_out);

/* ---- RadiusTopology / BallSearch --------------------------------------------------- */

/* Replaces _build_radius_neighbors (src/topology.jl:91-97): all j != i with
 * d2(i,j) <= r*r (inclusive).  Two-phase CSR so the caller allocates exactly:
 * count fills counts_out[n]; the caller builds offsets[n+1] (exclusive scan, int64)
 * and calls fill, which writes rows sorted by ascending (d2, index) into idx_out.
 * fill refers to the cloud passed to the preceding count on the same context.  Every call that overwrites what the
 * count phase left on the context (wtp_knn* and what runs through it, the sharded topology, wtp_relax_init*) ends the
 * pair: a fill after it returns WTP_ERR_STATE; calls that keep buffers of their own (wtp_spacing_eval, wtp_isinside_*,
 * wtp_mesh_*) may come between the two. */
int wtp_radius_count(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype,
                     double r, int32_t* counts_out);
int wtp_radius_fill(wtp_ctx* ctx, const int64_t* offsets, int32_t* idx_out);
/* The same first phase with the exclusive scan done on the device: offsets_out[n+1] (int64) is what the
 * caller needs to allocate idx_out (offsets_out[n] entries); the offsets also stay resident, so the fill
 * that follows may pass offsets = NULL.  Saves the counts' trip to the host and the offsets' trip back.  */
int wtp_radius_offsets(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, double r,
                       int64_t* offsets_out);
/* Diagnostic, read-only: how the count phase disposed of each query of the cloud it was given.  Valid where
 * wtp_radius_fill is (after a count or offsets call on this context, WTP_ERR_STATE otherwise), before or after the fill.
 * marks_out[cap], cap >= n (WTP_ERR_ARG otherwise; NULL: only info_out is filled), by original id: 0 = left to the fill phase (the wave-per-query kernel, the serial kernel for rows beyond
 * 512), 1 = row of at most 32 ids parked by the lane-per-query brick kernel, 2 = row parked in the arena (by the
 * brick-staged dense kernel if info_out[0], else by the wave-per-query kernel).
 * info_out[13]: [0] the dense kernel ran, [1] the grid's rad_wave_only flag, [2] the dense kernel's LDS point area for
 * this dtype, [3..5] cells per axis, [6] cell edge, [7..9] grid origin (edge and origin exactly as the kernels use them),
 * [10] ids of the arena the dense kernel took (in pieces of 2048), [11] ids the arena holds (48 n), [12] n, the points of the cloud the count was given. */
int wtp_radius_marks(wtp_ctx* ctx, uint8_t* marks_out, int64_t cap, double* info_out);

/* ---- repel: _relax! ------------------------------------------------------------------ */

/* Replaces the setup of _relax! (src/repel.jl:207-241).  snap_xyz: the search snapshot,
 * n points, the first n_fixed static (the boundary wall), the tail movable.
 * k is the reference's `k` (self slot included: kk = min(k, n), repel.jl:208,259).
 * alpha_lo/alpha_max: step bounds (repel.jl:85,226). */
int wtp_relax_init(wtp_ctx* ctx, const void* snap_xyz, int64_t n, int64_t n_fixed, int dim,
                   int dtype, const wtp_spacing_desc* spacing, const wtp_force_desc* force,
                   int k, double alpha_lo, double alpha_max);

/* Same with the snapshot already on the context's GPU (spacing->per_point stays a host array). */
int wtp_relax_init_dev(wtp_ctx* ctx, const void* d_snap_xyz, int64_t n, int64_t n_fixed, int dim,
                       int dtype, const wtp_spacing_desc* spacing, const wtp_force_desc* force,
                       int k, double alpha_lo, double alpha_max);

/* One pass of src/repel.jl:244-293 plus the reductions of :293,374-403.
 * rebuild != 0 refreshes the search snapshot from the current positions first
 * (repel.jl:245-253); rebuild == 0 sweeps against the stale snapshot. */
int wtp_relax_step(wtp_ctx* ctx, int rebuild, wtp_step_stats* stats);

/* n_iters passes with no host round trip of coordinates; iteration i (0-based)
 * rebuilds iff i % rebuild_every == 0.  conv_out[n_iters] receives max_force per
 * iteration (may be NULL); last receives the final iteration's stats (may be NULL). */
int wtp_relax_run(wtp_ctx* ctx, int n_iters, int rebuild_every, double* conv_out,
                  wtp_step_stats* last);

/* The loop of `_relax!` WITH its stop rules (src/repel.jl:305-334), evaluated on the device after every sweep in the
 * reference's order: cv_target (positions are then reverted to p_old, :314), stall_after on the CV of d_NN / s
 * (:316-326), tol on max |F| s (:329-332).  Sweeps are enqueued in batches of 16 without any host round trip; once a
 * rule fires the rest of the batch does nothing, so the session ends in the state of the last iteration that ran.
 * The CV is evaluated from sums of u = d_NN / s and u^2 accumulated in DOUBLE (u itself is rounded in the cloud's
 * type).  The reference's `_dnn_cv` (src/repel.jl:374-386) sums serially in the cloud's type T: for Float64 clouds the
 * two agree to rounding and the loop stops at the reference's iteration (tests/test_gpu_stop_rules.py: same count,
 * reason and positions as the oracle's loop); for Float32 clouds a serial Float32 sum over >= 10^4 points carries
 * 1e-4 .. 1e-3 relative error in the variance — the size of the stall rule's own 1e-3 margin — so the reference's
 * stall / cv_target rule can fire at ANOTHER iteration than this one (which uses the better number).  tol is
 * unaffected (a maximum).  conv_out[0 .. *n_done) = max |F| s per sweep; *reason: 0 max_iters reached, 1 tol,
 * 2 cv_target, 3 stall.
 * Not for sessions with the octree wall rule (wtp_relax_set_wall), kicks, traces or a caller-evaluated spacing:
 * those need the host between two sweeps (wtp_relax_step).  */
int wtp_relax_run_until(wtp_ctx* ctx, int max_iters, int rebuild_every, double tol, int stall_after, double cv_target,
                        double* conv_out, int* n_done, int* reason, wtp_step_stats* last);

/* Current movable points, (n - n_fixed) x dim of dtype, snapshot order. */
int wtp_relax_get(wtp_ctx* ctx, void* xyz_out);
/* Same into device memory on the context's GPU (sharded driver: no host round trip). */
int wtp_relax_get_dev(wtp_ctx* ctx, void* d_xyz_out);
/* Per-point outputs of the last sweep, each n - n_fixed long (any may be NULL):
 * forces (|F|*s), nn_dist (dtype), nn_id (int32 snapshot-global, -1 if none). */
int wtp_relax_get_point_data(wtp_ctx* ctx, void* forces_out, void* nn_dist_out,
                             int32_t* nn_id_out);
/* Overwrite movable point i (0-based within the movable tail): _maybe_kick!'s write
 * (src/repel.jl:431). */
int wtp_relax_set(wtp_ctx* ctx, int64_t i, const void* xyz);
/* p .= p_old (src/repel.jl:314): undo the last sweep. */
int wtp_relax_revert(wtp_ctx* ctx);
/* wtp_relax_set for m movable points in one pass: idx strictly increasing, xyz m x dim of the session's
 * dtype (the deposition pass of the octree method may land thousands of points in one iteration).  */
int wtp_relax_set_batch(wtp_ctx* ctx, const int64_t* idx, const void* xyz, int64_t m);
/* Refresh the PER_POINT spacing array (n values, snapshot order; repel.jl:251). */
int wtp_relax_set_spacing(wtp_ctx* ctx, const void* spacing);
/* Release the relax state (device buffers stay pooled in the context). */
int wtp_relax_end(wtp_ctx* ctx);

/* The spacings the session currently holds, one value per snapshot point in snapshot order
 * (`spacings` of src/repel.jl:209,251 — the kick and the trace read it).  Host array of n values. */
int wtp_relax_get_spacing(wtp_ctx* ctx, void* spacing_out);

/* Diagnostic, read-only: what a session with a LOGLIKE / BOUNDARY_LAYER law keeps per movable point between sweeps so
 * that a point may skip its boundary search (WTP_ERR_STATE without a session or with any other spacing kind).  Host
 * arrays over the n - n_fixed movable points in movable order, any of them NULL:
 * hint_out[i]: index of the boundary-tree node that won the point's last search, -1 before the first;
 * cert_out[4 i ..]: x_ref (three coordinates, z = 0 in 2-D: where the point stood at its last search) and lb, a lower
 *   bound on the canonical d2 from x_ref to every boundary point other than the winner, in the session's dtype;
 * winner_xyz_out[3 i ..]: the coordinates of node hint_out[i] (left untouched where the hint is -1).
 * A search rewrites x_ref with the point's position at that sweep; a point whose certificate answered keeps its x_ref. */
int wtp_relax_get_spacing_certs(wtp_ctx* ctx, int32_t* hint_out, void* cert_out, void* winner_xyz_out);

/* A variable spacing law evaluated at arbitrary points (spacing.(points), e.g. the default
 * alpha = minimum(spacing.(to(cloud)))/20 of src/repel.jl:61, or the metrics): LOGLIKE /
 * BOUNDARY_LAYER descriptors only.  xyz: host n x dim of dtype, out: host n values.  The context caches one boundary
 * tree: while a relax session with a LOGLIKE / BOUNDARY_LAYER law is open, only that law's boundary (same points, dim and
 * dtype) may be evaluated here; any other returns WTP_ERR_STATE instead of replacing the tree under the session.  */
int wtp_spacing_eval(wtp_ctx* ctx, const wtp_spacing_desc* spacing, const void* xyz, int64_t n, int dim,
                     int dtype, void* out);

/* ---- isinside: the post-filter of the volume-only repel (src/repel.jl:90) -----------------
 * 3-D, replaces isinside(testpoint, cloud|boundary) + _greens (src/isinside.jl:86-106) for a whole
 * array of test points: g_i = sum_j ((area_j (x_i - p_j)) . n_j) / |x_i - p_j|^3 over the m boundary
 * elements (centroid p, unit normal n, area), inside_out[i] = (g_i < -2 pi); a test point that
 * coincides with an element gives NaN and is reported outside, as in the reference.  Host arrays:
 * test_xyz n x 3, elem_xyz / elem_normal m x 3, elem_area m, all of dtype; g_out n values or NULL.
 * g is evaluated with fused multiply-adds and a 1-ulp rsqrt: it agrees with a term-by-term
 * evaluation to ~1e-6 relative, so only points with |g + 2 pi| below that can flip.  */
int wtp_isinside_greens(wtp_ctx* ctx, const void* test_xyz, int64_t n, const void* elem_xyz,
                        const void* elem_normal, const void* elem_area, int64_t m, int dtype,
                        uint8_t* inside_out, void* g_out);
/* 2-D, replaces isinside(testpoint, pts) (src/isinside.jl:17-33): winding sum of the signed angles
 * around the ordered, closed polygon poly_xy (m x 2); inside iff |sum| >= 1e3 eps(dtype), or the
 * point coincides (r < 100 eps) with a polygon point.  The ordering check of
 * _validate_polygon_ordering (:36-69) is the caller's (it needs the polygon only).  m < 3 is an
 * argument error.  sum_out: n values or NULL.  */
int wtp_isinside_winding(wtp_ctx* ctx, const void* test_xy, int64_t n, const void* poly_xy, int64_t m,
                         int dtype, uint8_t* inside_out, void* sum_out);

/* ---- triangle-mesh geometry index: the octree method of repel --------
 * Replaces TriangleIndex(T, mesh) + the TriangleOctree queries repel makes
 * (src/octree/triangle_octree.jl:22-31,221-277; queries :71-99,532-607; src/repel.jl:522-537).
 * vertices: nv x 3 of dtype (the index's machine type T); triangles: nt x 3 int32, 0-based.
 * The library derives unit face normals and the angle-weighted edge / vertex pseudonormals
 * (keyed by exact coordinates, so triangle soup with duplicated vertices needs no welding) and
 * builds its own search tree; one mesh per context, replaced by the next call.  */
int wtp_mesh_set(wtp_ctx* ctx, const void* vertices, int64_t nv, const int32_t* triangles, int64_t nt,
                 int dtype);
int wtp_mesh_clear(wtp_ctx* ctx);
/* nt x 3 unit face normals (zero for degenerate triangles), as doubles.  */
int wtp_mesh_face_normals(wtp_ctx* ctx, double* normals_out);
/* {min xyz, max xyz} of the vertices, flat axes widened (_compute_bbox_raw, :279-291).  */
int wtp_mesh_bounds(wtp_ctx* ctx, double bbox_out[6]);
/* Per query point (host array n x 3 of dtype, converted once to the mesh's type as the reference's
 * seam does, results converted back); every output may be NULL:
 *   sd_out        signed distance, negative inside (_compute_signed_distance_octree, :583-607)
 *   tri_out       nearest triangle, 0-based; of equidistant triangles the smallest index
 *                 (the reference keeps whichever its octree traversal meets first: unpinned)
 *   closest_out   n x 3 closest point on that triangle (closest_point_on_triangle, geometric_utils.jl:68-136)
 *   inside_out    isinside(p, octree) (:97-99): inside the vertex bbox and sd < 0
 *   projected_out n x 3 _project_to_boundary(p, octree, offset) (src/repel.jl:522-537):
 *                 closest point - offset * face normal of the landing triangle  */
int wtp_mesh_query(wtp_ctx* ctx, const void* xyz, int64_t n, int dtype, double offset, void* sd_out,
                   int32_t* tri_out, void* closest_out, uint8_t* inside_out, void* projected_out);
/* Installs the wall rule _constrain_octree (src/repel.jl:448-469) on the current relax session:
 * after every sweep a boundary point is re-projected onto the mesh (offset_dist inward) and a
 * volume point that left the domain returns to its previous position and is flagged escaped
 * (stats.n_escaped counts them).  The first n_boundary movable points start as boundary points
 * (src/repel.jl:148).  The mesh must stay set until wtp_relax_end.  */
int wtp_relax_set_wall(wtp_ctx* ctx, int64_t n_boundary, double offset_dist);
/* Per movable point: landing triangle of its last projection (0-based, -1 never projected),
 * boundary membership, escaped flag (cleared by this read when clear_escaped != 0: the
 * deposition pass consumes it, src/repel.jl:486-487).  Outputs may be NULL.  */
int wtp_relax_get_wall(wtp_ctx* ctx, int32_t* tri_out, uint8_t* is_bnd_out, uint8_t* escaped_out,
                       int clear_escaped);
/* The k nearest snapshot points of arbitrary positions (nq x dim host array of the session's
 * dtype), searched in the structure of the last rebuild — the `tree` the sweep used: replaces
 * knn(tree, site, kq, true) of _deposit_escaped! (src/repel.jl:502).  idx_out: nq x k snapshot
 * indices (0-based), ascending (d2, index); dist_out: nq x k distances or NULL.  */
int wtp_relax_query_knn(wtp_ctx* ctx, const void* xyz, int64_t nq, int k, int32_t* idx_out, void* dist_out);
/* Writes membership and landing triangles back after the host-side deposition pass
 * (_deposit_escaped!, src/repel.jl:471-520, serial by design).  */
int wtp_relax_set_wall_flags(wtp_ctx* ctx, const uint8_t* is_bnd, const int32_t* tri);

/* ---- graded Poisson-disk sampling of the mesh surface ----
 * Replaces sample_surface(mesh, spacing; factor, max_points, stall_limit) / PointBoundary(mesh, spacing)
 * (src/surface_sampling.jl:34-118): dart throwing on the continuous surface under ||x_i - x_j|| >= min(r_i, r_j),
 * r = factor h(x).  The reference draws from rand(); here the darts are a seeded counter-based stream and the result is
 * DEFINED as the serial loop over that stream, so a run can be reproduced anywhere, bit for bit:
 *   Host, once, in double: area_t = sqrt((c_x^2 + c_y^2) + c_z^2) / 2 with c = (v2 - v1) x (v3 - v1) from the corners
 * converted to double (c_x = e_y g_z - e_z g_y, c_y = e_z g_x - e_x g_z, c_z = e_x g_y - e_y g_x); cum = their running
 * sum in triangle order; total_area = cum[nt - 1].
 *   Dart j = 0, 1, ... (64-bit) of seed s < 2^24: w_a = splitmix64((s << 40) + 3 j + a), a = 0, 1, 2 (the keys of
 * wtp_gen_uniform_dev).  Triangle, in double: x = ((w_0 >> 11) 2^-53) total_area; t = the first index with
 * cum[t] >= x, at most nt - 1.  In the mesh's type T, no contraction: u = T((w_1 >> 40) 2^-24), v = T((w_2 >> 40) 2^-24)
 * (wtp_gen_uniform_dev's values), su = sqrt(u), position c = ((1 - su) v1 + (su (1 - v)) v2) + (su v) v3 per component,
 * r = T(factor) h(c) with the spacing law evaluated at c in T (CONSTANT: h = T(constant)).
 *   Darts p and q conflict when ((dx^2 + dy^2) + dz^2) < m m, m = min(r_p, r_q), all in T.
 *   Run.  Darts are taken in order.  Before each dart the run ends if max_points darts have been accepted
 * (stop_reason 2) or the last stall_limit darts were all rejected (stop_reason 1); n_darts counts the darts taken.  A
 * dart is accepted iff it conflicts with no earlier accepted dart.  The samples are the accepted darts in dart order.
 * The device decides whole batches of darts at once (rounds of "decide every dart whose lower-numbered conflicting darts
 * are decided"); the result does not depend on the batch size, uses no floating-point atomics and does not depend on
 * arrival order: two calls return the same bits, and a smaller max_points returns a prefix.
 *   batch: darts per batch, 0 = the library chooses; it changes time only.  A spacing value that is not finite and > 0
 * at a dart the run takes is WTP_ERR_ARG naming the smallest such dart; such a dart is never sampled with.
 *   WTP_ERR_STATE: no mesh set; wtp_mesh_sample_get* before a successful wtp_mesh_sample; another boundary's law while a
 * relax session evaluates its own.  WTP_ERR_ARG: factor not finite or <= 0, stall_limit < 1, max_points < 1,
 * seed >= 2^24, batch < 0 or > 2^24, kind WTP_SPACING_PER_POINT, total_area not > 0, a bad spacing value.  WTP_ERR_INTERNAL: a
 * batch of B darts was not decided within B rounds (the algorithm's bound).  */
typedef struct wtp_sample_info {
    int64_t n_points, n_darts, batch;   /* batch: the size used in the last batch */
    int32_t stop_reason;                /* 1 stall_limit misses in a row, 2 max_points */
    int32_t n_batches, rounds_max, host_syncs;
    double total_area, r_min, r_max;    /* r over the samples */
} wtp_sample_info;
/* Samples the mesh of wtp_mesh_set; the result stays on the device until the next call / wtp_mesh_fill / wtp_mesh_front
 * (which share the buffers) / wtp_mesh_set / wtp_mesh_clear. */
int wtp_mesh_sample(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, int64_t max_points,
                    int64_t stall_limit, uint64_t seed, int64_t batch, wtp_sample_info* info);
/* n_points rows (xyz_out n x 3 and r_out of the mesh's dtype); every output may be NULL.  dart_out: the dart index each
 * sample came from.  */
int wtp_mesh_sample_get(wtp_ctx* ctx, void* xyz_out, int32_t* tri_out, void* r_out, int64_t* dart_out);
/* The same into device memory.  */
int wtp_mesh_sample_get_dev(wtp_ctx* ctx, void* d_xyz_out, int32_t* d_tri_out, void* d_r_out);
/* Read-out, no acceptance: darts first .. first + n - 1 as the rule above makes them (host outputs, may be NULL).  The
 * values are returned as computed, a spacing that is not > 0 included.  Leaves a resident sample untouched.  */
int wtp_mesh_sample_darts(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, uint64_t seed,
                          int64_t first, int64_t n, void* xyz_out, int32_t* tri_out, void* r_out);

/* ---- graded Poisson-disk fill of the mesh's volume ----------------------------------------------
 * Replaces the point placement of discretize(bnd, spacing; alg = Orthtree(mesh; spacing, placement = :bridson), max_points)
 * (src/discretization/algorithms/octree.jl:804-902): volume points under ||x_i - x_j|| >= min(r_i, r_j), r = factor h(x),
 * against each other and against the boundary points (the seeds).  The reference's advancing front is serial and draws
 * from rand(); here, as for the surface, the darts are a seeded counter-based stream over the mesh's bounding box and the
 * result is DEFINED as the serial loop over that stream.  All arithmetic is in the mesh's type T, no contraction:
 *   Dart j = 0, 1, ... (64-bit) of seed s < 2^24: w_a = splitmix64((s << 40) + 3 j + a), u_a = T(float(w_a >> 40) 2^-24)
 * (point j of wtp_gen_uniform_dev's dim-3 stream), position c_a = lo_a + u_a (hi_a - lo_a), a = 0, 1, 2, with {lo, hi} the
 * mesh's vertex bounding box as wtp_mesh_set holds it (wtp_mesh_bounds), in T.
 *   r = T(factor) h(c), the spacing law evaluated at c in T as wtp_mesh_sample does.  Kinds: CONSTANT, LOGLIKE,
 * BOUNDARY_LAYER.
 *   A dart is inside iff wtp_mesh_query's inside flag holds for c: in the box, closest-feature pseudonormal side < 0,
 * distance > 0.  Only an inside dart is a candidate; the spacing value of a dart that is not inside is never looked at.
 *   Points p and q conflict when ((dx^2 + dy^2) + dz^2) < m m, m = min(r_p, r_q).
 *   Seeds: n_seeds points (host, n_seeds x 3 of T; NULL / 0 for none), r = T(factor) h(seed) under the same law.  They
 * occupy space from the start, are never tested against each other, are not returned and may lie on or outside the box.
 *   Run.  Darts are taken in order.  Before each dart the run ends if max_points darts have been accepted (stop_reason 2)
 * or the last stall_limit darts were all rejected (stop_reason 1); n_darts counts the darts taken and n_inside those of
 * them that were inside.  A dart is accepted iff it is a candidate and conflicts with no seed and no earlier accepted dart;
 * any other dart is a miss, one outside the domain included.  The result is the accepted darts in dart order; it does not
 * depend on batch or on arrival order and uses no floating-point atomics: two calls return the same bits, and a smaller
 * max_points returns a prefix.  A run that ends with no point returns WTP_OK with n_points = 0.
 *   bbox_volume n_inside / n_darts is the run's own estimate of the domain's volume.  The stream is uniform over the box:
 * there is no thinning by h, no node octree and no max_growth limiter.  The 2-D fill is wtp_loops_fill below.
 *   WTP_ERR_ARG: a spacing value that is not finite and > 0 at a seed (naming the seed) or at an inside dart the run takes
 * (naming the smallest such dart; such a value at any other dart is no error); a seed coordinate that is not finite;
 * n_seeds < 0, or seeds NULL with n_seeds > 0; and every row of wtp_mesh_sample: factor, stall_limit, max_points, seed,
 * batch, kind WTP_SPACING_PER_POINT, a mesh of no area.  WTP_ERR_STATE and WTP_ERR_INTERNAL as for wtp_mesh_sample.
 *   State.  The surface sample and the volume fill share their device buffers: wtp_mesh_sample voids a resident fill and
 * wtp_mesh_fill a resident sample, once its arguments have passed, and the other's *_get* is WTP_ERR_STATE after that.  */
typedef struct wtp_fill_info {
    int64_t n_points, n_darts, n_inside, n_seeds, batch; /* batch: the size used in the last batch */
    int32_t stop_reason;                                 /* 1 stall_limit misses in a row, 2 max_points */
    int32_t n_batches, rounds_max, host_syncs;
    double bbox_volume, r_min, r_max;                    /* r over the accepted points (0 when there are none) */
} wtp_fill_info;
/* Fills the mesh of wtp_mesh_set; the result stays on the device until the next wtp_mesh_fill / wtp_mesh_sample /
 * wtp_mesh_set / wtp_mesh_clear.  seeds: host array of the mesh's dtype.  */
int wtp_mesh_fill(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, const void* seeds, int64_t n_seeds,
                  int64_t max_points, int64_t stall_limit, uint64_t seed, int64_t batch, wtp_fill_info* info);
/* n_points rows (xyz_out n x 3 and r_out of the mesh's dtype); every output may be NULL.  dart_out: the dart index each
 * point came from.  */
int wtp_mesh_fill_get(wtp_ctx* ctx, void* xyz_out, void* r_out, int64_t* dart_out);
/* The same into device memory.  */
int wtp_mesh_fill_get_dev(wtp_ctx* ctx, void* d_xyz_out, void* d_r_out);
/* Read-out, no acceptance: darts first .. first + n - 1 as the rule above makes them (host outputs, may be NULL); inside_out
 * one byte per dart.  r is returned as computed for every dart, a spacing that is not > 0 included.  Leaves a resident
 * sample or fill untouched.  */
int wtp_mesh_fill_darts(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, uint64_t seed, int64_t first,
                        int64_t n, void* xyz_out, uint8_t* inside_out, void* r_out);

/* ---- advancing-front fill of the mesh's volume ----------------------------------------------------
 * Replaces discretize(bnd, spacing; alg = SlakKosec(octree), max_points) (src/discretization/algorithms/slak_kosec.jl:72-123;
 * Slak & Kosec 2019): every point of a queue that starts as the boundary points throws n candidates onto the sphere of its
 * own spacing around it, and a candidate that is inside the domain and far enough from every point is appended to the
 * queue.  The reference loop is serial and draws from rand(); as for the sampler and the fill, the result is DEFINED as
 * the serial loop over a counter-based stream.  All arithmetic is in the mesh's type T, no contraction:
 *   Queue.  Entries q = 0 .. n_seeds - 1 are the seeds (host, n_seeds x 3 of T), in the order given; behind them the
 * accepted points in acceptance order: the queue is the accepted array with the seeds at its front.  Every entry has
 * h_q = T(h(x_q)), the spacing law evaluated at it in T as wtp_mesh_sample does (CONSTANT: T(constant)).  Kinds: CONSTANT,
 * LOGLIKE, BOUNDARY_LAYER.  There is no factor: the reference uses r = spacing(p).
 *   Candidate j = q n + s (64-bit), s = 0 .. n - 1, of parent q, seed < 2^24: w_a = splitmix64((seed << 40) + 2 j + a),
 * a = 0, 1; u = T(float(w_0 >> 40) 2^-24), v likewise from w_1.  Polar part z = 2 u - 1, rho = sqrt(1 - z z).  Azimuth
 * without libm, so that any IEEE machine agrees bit for bit: t = 8 v, o = floor(t), f = t - o, g = (o odd) ? 1 - f : f (all
 * exact), theta = g T(pi / 4), x = theta theta,
 *     s = theta (1 + x (S_1 + x (S_2 + ... + x S_9))),    c = 1 + x (C_1 + x (C_2 + ... + x C_9))      (Horner)
 * with S_k = T((-1)^k / (2k + 1)!), C_k = T((-1)^k / (2k)!), each the double quotient (n! is exact in double up to 19!)
 * rounded to T; (cos l, sin l) by octant o = 0 .. 7: (c, s) (s, c) (-s, c) (-c, s) (-c, -s) (-s, -c) (s, -c) (c, -s).
 * Direction d = (rho cos l, rho sin l, z), | |d| - 1 | <= 1.02 eps; position c_a = x_{q,a} + h_q d_a; test radius r_j = h_q.
 *   A candidate is inside iff wtp_mesh_query's inside flag holds for it, as in wtp_mesh_fill.
 *   Conflict is one-sided: candidate j conflicts with queue entry e iff ((dx^2 + dy^2) + dz^2) < r_j r_j.  The entry's own
 * h plays no part, and a candidate is never tested against its own parent (which sits at distance h_q (1 +- eps): the
 * reference's `> r` against a tree that still holds the parent is a coin toss on rounding).  Every other entry counts,
 * expanded or not: this is the published algorithm.  The reference rebuilds its search tree from the not yet expanded
 * seeds only, so later candidates are not tested against expanded boundary points; that is deliberately NOT reproduced.
 *   Run.  Parents are expanded in queue order, candidates in s order.  Before each candidate the run ends if max_points
 * points have been accepted (stop_reason 2).  A candidate is accepted iff it is inside and conflicts with no entry then in
 * the queue, and is appended.  The run ends with stop_reason 1 when every queue entry has been expanded (the normal end:
 * the front has died out).  n_candidates counts the candidates taken, n_inside those of them that were inside, n_parents
 * the parents of which a candidate was taken (ceil(n_candidates / n)).  The device decides the candidates of a range of
 * parents at once (batch parents per batch, 0 = the library chooses: every parent available; either way at most 2^20
 * candidates, i.e. 2^20 / n parents, at least one); the batch changes
 * time only, two calls return the same bits, and a smaller max_points returns a prefix.  n_seeds = 0 returns WTP_OK with
 * no points and stop_reason 1.
 *   WTP_ERR_ARG: n outside 1 .. 64; max_points < 1; seed >= 2^24; batch < 0 or > 2^24; kind WTP_SPACING_PER_POINT; a seed
 * coordinate that is not finite; n_seeds < 0, or seeds NULL with n_seeds > 0; n_seeds + max_points >= 2^31 - 1 (the queue
 * is indexed in int32; refused before the run starts); a spacing value that is not finite and > 0 at a seed (naming the
 * seed) or at an accepted point (naming the smallest such candidate index; such a point is never expanded); a mesh of no
 * area.  WTP_ERR_STATE and WTP_ERR_INTERNAL as for wtp_mesh_sample.
 *   State.  The front shares the sampler's buffers: it voids a resident sample or fill and is voided by wtp_mesh_sample and
 * wtp_mesh_fill, once the arguments have passed; each one's *_get* is WTP_ERR_STATE after that.  */
typedef struct wtp_front_info {
    int64_t n_points, n_parents, n_candidates, n_inside, n_seeds, batch; /* batch: parents in the last batch */
    int32_t stop_reason;                                                 /* 1 the front died out, 2 max_points */
    int32_t n_batches, rounds_max, host_syncs;
    double r_min, r_max;                                                 /* h over the accepted points (0 when there are none) */
} wtp_front_info;
/* Fills the mesh of wtp_mesh_set from the seeds; the result stays on the device until the next wtp_mesh_front /
 * wtp_mesh_fill / wtp_mesh_sample / wtp_mesh_set / wtp_mesh_clear.  seeds: host array of the mesh's dtype.  */
int wtp_mesh_front(wtp_ctx* ctx, const wtp_spacing_desc* spacing, int64_t n, const void* seeds, int64_t n_seeds,
                   int64_t max_points, uint64_t seed, int64_t batch, wtp_front_info* info);
/* n_points rows, the seeds not among them (xyz_out n x 3 and h_out of the mesh's dtype); every output may be NULL.
 * cand_out: the candidate index each point came from; parent_out: its parent's queue index (cand / n).  */
int wtp_mesh_front_get(wtp_ctx* ctx, void* xyz_out, void* h_out, int64_t* cand_out, int32_t* parent_out);
/* xyz and h into device memory.  */
int wtp_mesh_front_get_dev(wtp_ctx* ctx, void* d_xyz_out, void* d_h_out);
/* Read-out, no acceptance: the n candidates each of n_parents parent positions (host, n_parents x 3), parent p standing
 * for queue entry first_parent + p (0 <= first_parent <= 2^31), as the rule above makes them with h evaluated at the given
 * positions: xyz_out (n_parents n) x 3, inside_out one byte and r_out one value per candidate (host, may be NULL).  The
 * candidates of a parent whose h is not finite and > 0 are returned at the parent's position with that h.  Leaves a
 * resident result untouched.  */
int wtp_mesh_front_candidates(wtp_ctx* ctx, const wtp_spacing_desc* spacing, uint64_t seed, const void* parents_xyz,
                              int64_t n_parents, int64_t first_parent, int64_t n, void* xyz_out, uint8_t* inside_out,
                              void* r_out);

/* ---- boundary-loop geometry index of a 2-D domain ---------------------------------------------------
 * Replaces SegmentIndex(T, loops) + the SegmentQuadtree queries (src/octree/segment_quadtree.jl:115-238 and the queries
 * behind isinside): the 2-D twin of wtp_mesh_set / wtp_mesh_query.  xy: nv x 2 of dtype (the index's machine type T);
 * loop_start: n_loops + 1 offsets, loop l being rows [loop_start[l], loop_start[l + 1]) in order around the loop, either
 * orientation, explicitly closed (last vertex = first) or not.  One index per context, replaced by the next call.  The
 * host build, in T, term by term, no contraction:
 *   Dedup, per loop: tol = max(8 eps(T) diag, floatmin(T)), diag = sqrt(e_x^2 + e_y^2) of the loop's own bounding-box
 * extent e; a vertex with sqrt(dx^2 + dy^2) <= tol from the last kept one is dropped, then trailing vertices within tol of
 * the first.
 *   Validate: the shoelace area centred on the loop's first vertex o, sa = (sum over i in loop order of
 * (a_x b_y - b_x a_y), a = v_i - o, b = v_{i+1} - o) / 2; |sa| < max(T(1e-10) e_x e_y, 4 (T(n) eps(T)) (e_x^2 + e_y^2)) over the
 * cleaned loop's extent is WTP_ERR_ARG, as are fewer than 3 vertices before or after the dedup (both naming the loop),
 * n_loops < 1, a coordinate that is not finite and offsets that do not run upward from 0 to nv.
 *   Orient: depth = the number of OTHER cleaned loops that contain the loop's first vertex p by the even-odd crossing
 * rule (an edge a -> b with (a_y > p_y) != (b_y > p_y) crosses when a_x + ((p_y - a_y) / (b_y - a_y)) (b_x - a_x) > p_x); even
 * depth wants sa > 0 (counter-clockwise: an outer boundary), odd depth sa < 0 (a hole); a loop that disagrees is reversed.
 *   Segments: segment i of the concatenated oriented loops runs from vertex i to the next vertex of its loop, cyclically;
 * its normal is (d_y, -d_x) / sqrt(d_x^2 + d_y^2), out of the domain; a vertex's pseudonormal is the sum of its two segments'
 * normals.  The box is {min, max} over all vertices, a flat axis widened by max(100 eps(T), T(1e-10)) either way.
 * wtp_loops_set and wtp_loops_clear void a resident sample, fill or front, as wtp_mesh_set does.  */
int wtp_loops_set(wtp_ctx* ctx, const void* xy, int64_t nv, const int64_t* loop_start, int64_t n_loops, int dtype);
int wtp_loops_clear(wtp_ctx* ctx);
/* {min xy, max xy} as doubles and the number of segments; either may be NULL.  */
int wtp_loops_bounds(wtp_ctx* ctx, double bbox_out[4], int64_t* n_segments_out);
/* Per query point p (host array n x 2 of dtype, converted once to T, results converted back); every output may be NULL.
 * DEFINED as the brute-force minimum over the segments, in T, no contraction.  Per segment (a, b): ab = b - a,
 * den = ab_x^2 + ab_y^2, t = ((p - a)_x ab_x + (p - a)_y ab_y) / den; t <= 0: cp = a (feature: vertex a); t >= 1: cp = b
 * (vertex b); else cp = a + t ab per component (the segment itself); dv = p - cp, d2 = dv_x^2 + dv_y^2.  The nearest segment
 * is the smallest (d2, segment index) (the reference keeps whichever its traversal meets first: unpinned).  With n the
 * feature's normal (the segment's, or the vertex's pseudonormal), s = dv_x n_x + dv_y n_y:
 *   sd_out       +sqrt(d2) for s > 0, 0 for s == 0, -sqrt(d2) for s < 0: negative inside
 *   seg_out      the nearest segment, 0-based
 *   closest_out  n x 2, cp of that segment
 *   inside_out   p inside the box (no coordinate below lo or above hi) and sd < 0
 * WTP_ERR_ARG: a query coordinate that is not finite (checked on the host).  WTP_ERR_STATE: no index set.  */
int wtp_loops_query(wtp_ctx* ctx, const void* xy, int64_t n, int dtype, void* sd_out, int32_t* seg_out, void* closest_out,
                    uint8_t* inside_out);

/* ---- graded Poisson-disk fill of a 2-D domain's area -----------------------------------------------
 * Replaces the point placement of discretize(bnd2d, spacing) (_generate_bridson with N = 2,
 * src/discretization/algorithms/octree.jl:816-902): wtp_mesh_fill's contract with the z terms removed.  All arithmetic
 * is in the index's type T, no contraction:
 *   Dart j = 0, 1, ... (64-bit) of seed s < 2^24: w_a = splitmix64((s << 40) + 3 j + a), u_a = T(float(w_a >> 40) 2^-24),
 * a = 0, 1 (point j of wtp_gen_uniform_dev's dim-2 stream, which keeps the stride of 3), position c_a = lo_a + u_a (hi_a - lo_a)
 * with {lo, hi} the index's box (wtp_loops_bounds), in T.
 *   r = T(factor) h(c), the spacing law evaluated at (x, y) in T against boundary_xyz of n_boundary x 2.  Kinds: CONSTANT,
 * LOGLIKE, BOUNDARY_LAYER.
 *   A dart is inside iff wtp_loops_query's inside flag holds for c.  Only an inside dart is a candidate; the spacing value
 * of a dart that is not inside is never looked at.
 *   Points p and q conflict when (dx^2 + dy^2) < m m, m = min(r_p, r_q).
 *   Seeds: n_seeds points (host, n_seeds x 2 of T; NULL / 0 for none), r = T(factor) h(seed) under the same law.  They
 * occupy space from the start, are never tested against each other, are not returned and may lie on or outside the box.
 *   Run.  Darts are taken in order.  Before each dart the run ends if max_points darts have been accepted (stop_reason 2)
 * or the last stall_limit darts were all rejected (stop_reason 1); n_darts counts the darts taken and n_inside those of
 * them that were inside.  A dart is accepted iff it is a candidate and conflicts with no seed and no earlier accepted dart;
 * any other dart is a miss, one outside the domain included.  The result is the accepted darts in dart order; it does not
 * depend on batch or on arrival order and uses no floating-point atomics: two calls return the same bits, and a smaller
 * max_points returns a prefix.  A run that ends with no point returns WTP_OK with n_points = 0.
 *   info is a wtp_fill_info whose bbox_volume is the box's AREA: bbox_volume n_inside / n_darts is the run's own estimate
 * of the domain's area.  No thinning by h, no per-leaf placement, no node quadtree, no max_growth limiter.
 *   WTP_ERR_ARG: the rows of wtp_mesh_fill (a bad spacing value at a seed or at an inside dart the run takes, a seed
 * coordinate that is not finite, n_seeds, factor, stall_limit, max_points, seed, batch, kind WTP_SPACING_PER_POINT) but
 * for the mesh's area.  WTP_ERR_STATE: no loops set; wtp_loops_fill_get* without a resident area fill; another boundary's
 * law while a relax session evaluates its own.  WTP_ERR_INTERNAL as for wtp_mesh_sample.  The dtype is the index's.
 *   State.  The area fill shares the samplers' device buffers: once its arguments have passed it voids a resident sample,
 * fill or front, and each of those voids it; the wrong *_get* is WTP_ERR_STATE.  wtp_loops_set and wtp_loops_clear void
 * whatever is resident.  */
int wtp_loops_fill(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, const void* seeds, int64_t n_seeds,
                   int64_t max_points, int64_t stall_limit, uint64_t seed, int64_t batch, wtp_fill_info* info);
/* n_points rows (xy_out n x 2 and r_out of the index's dtype); every output may be NULL.  dart_out: the dart index each
 * point came from.  */
int wtp_loops_fill_get(wtp_ctx* ctx, void* xy_out, void* r_out, int64_t* dart_out);
/* The same into device memory.  */
int wtp_loops_fill_get_dev(wtp_ctx* ctx, void* d_xy_out, void* d_r_out);
/* Read-out, no acceptance: darts first .. first + n - 1 as the rule above makes them (host outputs, may be NULL): xy_out
 * n x 2, inside_out one byte per dart, r as computed for every dart.  Leaves a resident result of the index's dtype
 * untouched; one of the other dtype (a mesh's, where mesh and loops differ in type) is voided, for the buffers change type.  */
int wtp_loops_fill_darts(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, uint64_t seed, int64_t first,
                         int64_t n, void* xy_out, uint8_t* inside_out, void* r_out);

/* ---- spacing-driven node octree over the mesh ------------------------------------------------------
 * Replaces build_node_octree + classify_node_octree (src/octree/spacing_criterion.jl:88-215, src/octree/spatial_octree.jl)
 * and what the Orthtree algorithm reads off the tree: _estimate_volume_points, _bridson_h_min, _leaf_spacing_field
 * (src/discretization/algorithms/octree.jl:590-662) and find_leaf.  3-D, over the mesh of wtp_mesh_set, every term in the
 * mesh's type T, no contraction.  Classes are the reference's: 0 EXTERIOR, 1 BOUNDARY, 2 INTERIOR.
 *   Root (triangle_octree.jl:391-398) from wtp_mesh_bounds' {lo, hi}: centre = (lo + hi) T(0.5), half = ((hi - lo) T(0.5)) T(1.02),
 * origin = centre - half, top = centre + half, root_size = the largest of top_a - origin_a; diagonal = sqrt((e_x^2 + e_y^2) + e_z^2)
 * with e_a = (origin_a + root_size) - origin_a; absolute_min = diagonal T(node_min_ratio).
 *   Box (depth d, cell c), 0 <= c_a < 2^d (spatial_octree.jl:107-128): h_box = root_size / T(2^d), lo_a = origin_a + T(c_a) h_box,
 * hi_a = lo_a + h_box, centre_a = origin_a + (T(2 c_a + 1) h_box) / T(2).  The children of a box are the 8 boxes
 * (d + 1, 2 c + bits(m)), bit a of m along axis a.  Depth is capped at 20: a box at depth 20 is never subdivided (a stated
 * deviation, so that a leaf's key fits 64 bits).
 *   cls(p, tol) (classify_point, triangle_octree.jl:71-92): EXTERIOR if some p_a < lo_a - tol or p_a > hi_a + tol of the mesh's
 * vertex box (wtp_mesh_bounds); otherwise, with sd the signed distance wtp_mesh_query gives, BOUNDARY if |sd| <= tol, else
 * INTERIOR if sd < 0, else EXTERIOR.  The distance is exact, so there is no class cache.
 *   touch(box): some triangle's axis-aligned bounding box overlaps the closed box, both ends inclusive (_boxes_overlap); it
 * stands for any_leaf_overlapping over the reference's geometry tree and is the brute-force answer.
 *   Refinement (_subdivide_node_octree!), from the root: a box is subdivided iff d < 20, h_box > absolute_min,
 * h_local = h(centre) > eps(T), h_box > T(alpha) h_local, and it may contain interior: with tol = max(T(1e-8), h_box T(1e-6)),
 * some of the 27 probes of _box_probe_points (m = (lo + hi) / T(2) per axis; the point m, the 8 corners, the 6 face centres, the
 * 12 edge midpoints) has cls(p, tol) != EXTERIOR, or else touch(box).  h is the spacing law in T (CONSTANT: T(constant)).
 *   Balance (balance_octree! + needs_balancing): a leaf (d, c) is subdivided iff d < 20, h_box > absolute_min and for some face
 * direction the box (d, c +- e_a), if inside the root, is an internal box one of whose EIGHT children is internal.  Rounds
 * in which every leaf decides on the tree the round began with are repeated until one splits nothing; balance_rounds counts
 * them, that last one included.  Splitting only adds boxes, so the result is the reference's in-place fixed point.
 * WTP_ERR_INTERNAL if round 100 still splits.  (The size test can_subdivide never decides here: a neighbour's internal child
 * at depth d + 1 was subdivided, so h_box(d + 1) > absolute_min, and h_box(d) is larger still.  It is kept as the reference
 * has it.)
 *   Leaf class (_classify_leaf_conservative): cls at the box's centre and its 8 corners, tol as above: BOUNDARY if any is
 * BOUNDARY or they disagree, else their common class; then a leaf with touch(box) is BOUNDARY whatever the vote, since
 * INTERIOR leaves are trusted downstream without an inside test.
 *   Leaf order: ascending Morton key (x lowest bit) of the leaf's lower corner at depth 20; the index wtp_node_tree_locate
 * reports.  h of a leaf is max(h(centre), sqrt(eps(T))) (_leaf_spacing_field).
 *   info: the counts; n_boxes, internal boxes included; depth_max and n_levels = depth_max + 1; integral = the sum over the
 * non-exterior leaves of ((h_box h_box) h_box) / ((h h) h), each term in T, accumulated in double in an unspecified but
 * reproducible order; max_points_auto = ceil(1.5 integral) (_estimate_volume_points), INT64_MAX where that is 2^63 or more
 * (a leaf whose h was clamped can weigh 1e20 in Float64); h_min = the smallest h of a non-exterior
 * leaf (_bridson_h_min), 0 when there is none; host_syncs <= n_levels + balance_rounds + 4.  origin, root_size and
 * absolute_min, the root as held, have no counterpart in the reference's return values: they are an addition, so that a
 * caller can compute the leaves' boxes from their cells.
 *   Kinds: CONSTANT, LOGLIKE, BOUNDARY_LAYER.  WTP_ERR_ARG: kind WTP_SPACING_PER_POINT or unknown, alpha not finite or <= 0,
 * node_min_ratio not in (0, 1], a spacing value at a box or leaf centre that is NaN or infinite (a value <= eps(T) only
 * stops refinement, as in the reference), a tree of more than 2^28 leaves.  WTP_ERR_STATE: no mesh; another boundary's law
 * while a relax session evaluates its own.
 *   State.  The tree lives in buffers of its own: it voids no sample, fill or front and none of them voids it.
 * wtp_mesh_set and wtp_mesh_clear drop it, and so does a failed build.  */
typedef struct wtp_node_tree_info {
    int64_t n_leaves, n_interior, n_boundary, n_exterior, n_boxes;
    int32_t depth_max, n_levels, balance_rounds, host_syncs;
    double integral, h_min;
    int64_t max_points_auto;
    double origin[3], root_size, absolute_min; /* the root as held, T values as doubles */
} wtp_node_tree_info;
int wtp_node_tree_build(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double alpha, double node_min_ratio,
                        wtp_node_tree_info* info_out);
/* The n_leaves leaves in leaf order; every output may be NULL: cell_out n x 3, depth_out, class_out, h_out of the mesh's
 * dtype.  WTP_ERR_STATE without a tree.  */
int wtp_node_tree_get(wtp_ctx* ctx, int32_t* cell_out, int32_t* depth_out, int8_t* class_out, void* h_out);
/* find_leaf (spatial_octree.jl:223-234) for n host points (n x 3 of dtype, converted once to T): from the root, at every
 * internal box p_a >= centre_a picks the upper child along axis a.  leaf_out: the leaf's index in leaf order; -1 for a point
 * with some p_a < origin_a or p_a > origin_a + root_size, or not a number (the reference would index out of its tree).  */
int wtp_node_tree_locate(wtp_ctx* ctx, const void* xyz, int64_t n, int dtype, int64_t* leaf_out);
int wtp_node_tree_clear(wtp_ctx* ctx);

/* ---- per-leaf placements over the node octree -------------------------------------------------------
 * Replaces the :random, :jittered and :lattice placements of _discretize_volume (src/discretization/algorithms/octree.jl:
 * 325-458, 977-1039) over the resident tree.  The reference draws from rand(); here every draw is a seeded counter-based
 * value, so the result is DEFINED by the rules below and two calls return the same bits.  placement: 0 random, 1 jittered,
 * 2 lattice.  Leaves are named by their index in leaf order.
 *   Weights.  w_i = double(((h_box h_box) h_box) / ((h h) h)), the leaf's term of the integral, computed in T.  The INTERIOR
 * leaves form one group and the BOUNDARY leaves the other, each in leaf order; W_int and W_ns are the groups' sums of w in
 * double, in an unspecified but reproducible order.  They are reported, and everything below is defined from the reported
 * values.  W_int + W_ns <= 0 (no leaf in or on the domain): WTP_OK with n_points = 0.
 *   Split.  n_interior = round_half_even(double(max_points) (W_int / (W_int + W_ns))), n_ns = max_points - n_interior,
 * n_candidates = round_half_even(double(n_ns) boundary_oversampling), all in double.
 *   Draws.  key(stage, j, a) = (seed << 40) + 3 (stage 2^36 + j) + a modulo 2^64; r(stage, j, a) = splitmix64(key), the
 * function of wtp_gen_uniform_dev; u(stage, j, a) = T(float(r >> 40) 2^-24), its value.  Stages: 0 interior points,
 * 1 near-surface candidates, 2 deficit points, 3 the leftover picks of the interior counts, 4 those of the candidates'
 * counts, 5 the deficit's leaf picks.  Picks use a = 0.
 *   pick(F, x): with cum the inclusive running sums of the integers F_i over all leaves (F_i = 0 outside the group) and
 * F_total = cum of the last leaf, the first leaf i with cum_i > mulhi64(x, F_total) (the high 64 bits of the product).
 * If F_total = 0, F_i = 1 for every leaf of the group instead: the uniform rule of the reference's fill(inv(n)) branch.
 *   Counts of a group for `count` points (_allocate_counts_by_volume), with W the group's reported sum: expected_i =
 * double(count) (w_i / W), base_i = floor(expected_i), leftover = max(0, count - sum base_i), F_i = floor((expected_i -
 * base_i) 2^32) as an integer; count_i = base_i + the number of t < leftover with pick(F, r(stage, t, 0)) = i.  The
 * counts add up to `count` exactly (to sum base_i if that is larger, which needs rounding to conspire and is not
 * expected).  A group of no leaves gets count 0 by the split.
 *   Points of a leaf with count n, in T, {lo, hi} the leaf's box as the tree computes it, e = hi - lo per axis.  The leaf's
 * k-th point (k < n) has the global index j = (the counts of the leaves before it) + k within its stage.  Random:
 * lo_a + u(stage, j, a) e_a.  Jittered and lattice: g = the smallest integer with g^3 >= n; cell = e / T(g); the point's cell
 * is c = (k mod g, (k / g) mod g, k / g^2) (the first n of CartesianIndices, first axis fastest); cell_min_a = lo_a +
 * T(c_a) cell_a; lattice: cell_min_a + cell_a / T(2); jittered: cell_min_a + u(stage, j, a) cell_a.
 *   Result, in this order.  (1) The n_interior interior points (stage 0), with no inside test.  (2) Of the n_candidates
 * near-surface candidates (stage 1), those whose wtp_mesh_query inside flag holds, in candidate order, as long as the
 * result holds fewer than max_points; n_accepted counts them.  (3) If the result is still short and W_int > 0, n_deficit =
 * max_points - (n_interior + n_accepted) more points: point t lies in the leaf pick(F, r(5, t, 0)) with F_i =
 * floor((w_i / W_int) 2^32) over the interior leaves, at lo_a + u(2, t, a) e_a.  With W_int > 0 the result has exactly
 * max_points points; without an interior leaf it may have fewer, with n_deficit = 0.
 *   WTP_ERR_ARG: a bad placement code, max_points < 1 or > 2^31, boundary_oversampling not finite or <= 0 or so large that
 * n_candidates exceeds 2^31, seed >= 2^24.  WTP_ERR_STATE: no mesh, no tree; wtp_node_place_get* without a placement.
 *   State.  The placement lives in buffers of its own beside the tree's: it voids no sample, fill or front and none voids
 * it.  A tree build (successful or not), wtp_node_tree_clear, wtp_mesh_set and wtp_mesh_clear drop it.  */
typedef struct wtp_node_place_info {
    int64_t n_points, n_interior, n_candidates, n_accepted, n_deficit;
    double W_int, W_ns;
    int32_t placement, host_syncs;
} wtp_node_place_info;
int wtp_node_place(wtp_ctx* ctx, int placement, int64_t max_points, double boundary_oversampling, uint64_t seed,
                   wtp_node_place_info* info_out);
/* n_points rows: xyz_out n x 3 of the mesh's dtype, leaf_out each point's leaf; either may be NULL.  */
int wtp_node_place_get(wtp_ctx* ctx, void* xyz_out, int64_t* leaf_out);
/* The same into device memory.  */
int wtp_node_place_get_dev(wtp_ctx* ctx, void* d_xyz_out, int64_t* d_leaf_out);

/* ---- consumers of the k-NN rows ------------------------------------
 * Replaces compute_normals(points; k) / update_normals! (src/normals.jl:15-69): per point the
 * eigenvector of the smallest eigenvalue of the covariance of its k nearest points (self
 * included, KNearestSearch(points, k)), unit length.  eigen() leaves the sign open (the
 * reference fixes it afterwards with orient_normals!); here the component of largest
 * magnitude is positive.  normals_out: n x dim of dtype.  2 <= k <= n.  */
int wtp_pca_normals(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, void* normals_out);
/* Replaces _gradient_limit_field (src/discretization/algorithms/octree.jl:677-717) on the
 * leaf centres: k-NN graph (self included, distances) + min-plus Jacobi sweeps
 * h[i] <- min(h[i], min_j h[j] + g d_ij) until the largest relative change of a sweep is
 * below tol or max_sweeps ran.  h0 / h_out: n values of dtype; sweeps_out: sweeps applied.  */
int wtp_gradient_limit(wtp_ctx* ctx, const void* centers, int64_t n, int dim, int dtype, int k, const void* h0,
                       double g, double tol, int max_sweeps, void* h_out, int* sweeps_out);

/* The reductions of metrics / spacing_metrics / spacing_fidelity_metrics (src/metrics.jl:19-129) over the k-NN distance
 * rows, on the device: the search of KNearestSearch(cloud, k) (k counts the point itself, 2 <= k <= n), then one pass
 * over the n x k distances where the search left them.  Slot 0 of a row (the point itself, or a coincident twin at
 * distance 0) is dropped as x[2][2:end] does; the statistics cover the k_eff = k - 1 slots behind it.  Per point, in
 * double and in slot order: mean_i, the two-pass sample deviation std_i (NaN for k_eff = 1, as Julia's std of one
 * value), max_i and min_i = nn_i (slot 1); with a spacing h_i also e_i = |mean_i - h_i| / h_i, u_i = nn_i / h_i and
 * c_i = #{slots with d <= coord_radius h_i}.  The struct holds their sums over the cloud (divide by n), the extremes
 * of nn_i with the smallest index that attains each, and the sums of squared deviations of e and u from their means
 * (sample variance = ssd / (n - 1)), merged from per-block (count, sum, M2) triples.  The reduction order is fixed and
 * uses no floating-point atomics: two calls on the same cloud return the same bits; no sum chains more than 4096
 * additions.  Without a spacing has_spacing = 0 and the fields from sum_err on are zero.  (The struct shares its name
 * with the call, as stat does: it has a tag and no typedef, so write `struct wtp_knn_stats`.)  */
struct wtp_knn_stats {
    int64_t n; int32_t k_eff; int32_t has_spacing;
    double sum_mean, sum_std, sum_max, sum_min;   /* divide by n for metrics()' avg/std/max/min */
    double nn_min, nn_max; int64_t nn_min_i, nn_max_i; /* separation, fill */
    double sum_err, ssd_err, max_err;             /* e_i; ssd = sum of squared deviations from the mean */
    double sum_u, ssd_u;                          /* u_i = nn_i / h_i */
    int64_t sum_coord;
};
/* xyz: host n x dim of dtype.  h: n host doubles, each finite and > 0 (checked on the device: WTP_ERR_ARG names the
 * first offending index), or NULL; with h == NULL a h_const > 0 is the spacing of every point and h_const <= 0 means no
 * spacing.  out: host.  nn_out (n of dtype) and mean_out (n doubles): host arrays or NULL.  The call copies back the
 * struct and those two arrays, never the n x k matrices.  Like every call that runs the k-NN search (wtp_knn,
 * wtp_pca_normals, ...) it ends a pending wtp_radius_count / wtp_radius_fill pair; WTP_ERR_STATE while a relax session
 * is open.  */
int wtp_knn_stats(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, const double* h, double h_const,
                  double coord_radius, struct wtp_knn_stats* out, void* nn_out, double* mean_out);
/* The same with d_xyz, d_h, d_nn_out and d_mean_out in device memory; out stays a host struct.  */
int wtp_knn_stats_dev(wtp_ctx* ctx, const void* d_xyz, int64_t n, int dim, int dtype, int k, const double* d_h,
                      double h_const, double coord_radius, struct wtp_knn_stats* out, void* d_nn_out, double* d_mean_out);

/* The graph part of orient_normals! (src/normals.jl:75-161) and split_surface! (src/surface_operations.jl:58-94), on the
 * device: the search of KNearestSearch(points, k) (k counts the point itself, 1 <= k <= n), whose rows stay where the
 * search left them, then rounds of component merging over those rows.
 *   Edge set.  As the reference builds it: for every row, src = slot 0 and dst = slots 1..k-1.  Slot 0 is the point
 * itself or the coincident twin that sorts first; the row is followed, the row's own index is not substituted.  The
 * graph is undirected and simple: an edge exists if either row names it (both directions give the same weight bits).
 *   wtp_orient_normals.  Weight w = (1 - |((nx nx' + ny ny') + nz nz')|) + 100 eps(T) in the cloud's type T, term by
 * term; weights compare as IEEE values (w < 0 is legal: normals may be a little longer than 1).  The forest is the
 * unique minimum spanning forest under the total order (w, a, b), a < b the endpoint ids, which is what Kruskal over the
 * edges sorted stably by w after de-duplication by a n + b gives.  The start is the first index that attains the largest
 * last coordinate; it is flipped if its normal's last component is < 0.  Every other vertex of the start's component is
 * flipped iff the number of tree edges (u, v) with n_u . n_v < 0 (input normals; a dot of exactly 0 is not negative) on
 * its path to the start is odd, XOR the start's own flip: what the reference's walk does, in any walk order.  Vertices
 * of other components come back untouched, bit for bit.  k = 1 or n = 1: no edges, only the start rule.  The result is
 * unique, uses no floating-point atomics and does not depend on arrival order: two calls return the same bits.
 *   mst_out (or NULL): room for n - 1 pairs {a, b}, a < b; the first n - n_components pairs are the forest's edges, in
 * any order (sort them to compare); the rest is not written.
 *   wtp_normal_components.  Keeps an edge iff |_angle(n_src, n_dst)| < angle, _angle as in src/utils.jl:18-23 evaluated
 * in double from the normals converted to double (2-D: atan2(cross, dot), signed; 3-D: atan2(|cross|, dot)).
 * label_out[i] is the smallest id in i's component of the kept edges.  The device's atan2 may differ from a host's in the
 * last ulps: only edges whose angle is within 1e-12 rad of the threshold can be decided differently.
 *   A normal with a non-finite component is WTP_ERR_ARG naming the first such index (checked on the device; nothing has
 * been written then).  Like every call that runs the k-NN search these calls end a pending wtp_radius_count /
 * wtp_radius_fill pair; WTP_ERR_STATE while a relax or block session is open.  Termination is a device flag read back
 * once per batch of 4 rounds, the last of which only finds nothing left to merge: the graph part synchronises
 * ceil((rounds + 1) / 4) + 1 times (twice for k = 1), which info (or NULL) reports with the rounds.  */
typedef struct wtp_normal_graph_info {
    int64_t n_edges;       /* distinct undirected edges of the row graph                                        */
    int64_t n_components;  /* connected components of that graph (orient) / of the kept edges (components)      */
    int64_t n_reached;     /* orient: vertices in the start's component                                         */
    int64_t n_flipped;     /* orient: normals whose sign changed                                                */
    int64_t start;         /* orient: argmax of the last coordinate, smallest index among equals (else -1)      */
    int32_t rounds;        /* Boruvka / hooking rounds that merged something                                    */
    int32_t host_syncs;    /* host synchronisations of the graph part (the search's own are not counted)        */
} wtp_normal_graph_info;
/* xyz: host n x dim of dtype; normals_inout: host n x dim of dtype, oriented in place; mst_out: host or NULL.  */
int wtp_orient_normals(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, void* normals_inout,
                       int32_t* mst_out, wtp_normal_graph_info* info);
/* The same with d_xyz, d_normals_inout and d_mst_out in device memory; info stays a host struct.  */
int wtp_orient_normals_dev(wtp_ctx* ctx, const void* d_xyz, int64_t n, int dim, int dtype, int k, void* d_normals_inout,
                           int32_t* d_mst_out, wtp_normal_graph_info* info);
/* xyz, normals: host n x dim of dtype (normals are not changed); label_out: n host int32.  */
int wtp_normal_components(wtp_ctx* ctx, const void* xyz, const void* normals, int64_t n, int dim, int dtype, int k,
                          double angle, int32_t* label_out, wtp_normal_graph_info* info);

/* ---- sharded sessions (no counterpart in the reference) --------------
 * One rank sweeps one spatial slab.  Its session's fixed head is the ghost layer received
 * from the neighbouring ranks, its movable tail the points it owns.  The two calls below
 * keep such a session resident across iterations: only the layers cross the boundary.  */

/* Run the library on a caller-owned HIP stream (e.g. the stream RCCL's results are ordered
 * on) instead of the context's own: external = 1 lends hip_stream (NULL is the device's
 * default stream), external = 0 restores the context's stream.  Device pointers handed to
 * the *_dev entry points must be ready in the order of the stream in use.  */
int wtp_set_stream(wtp_ctx* ctx, void* hip_stream, int external);

/* Boundary layers of the movable points at their current positions, as packed 4-vectors
 * {x, y, z, bits(movable index)} (dtype of the session) in device memory:
 *   d_lo4  <- points with coord[axis] <  lo_in      counts[0]
 *   d_hi4  <- points with coord[axis] >= hi_in      counts[1]
 * and, counted only, the strays: coord < lo_out -> counts[2], coord >= hi_out -> counts[3].
 * Order within a layer is deterministic (slot order of the last rebuild).  At most `cap`
 * points are written per layer; counts report the true sizes.  */
int wtp_relax_layers_dev(wtp_ctx* ctx, int axis, double lo_in, double hi_in, double lo_out, double hi_out,
                         void* d_lo4, void* d_hi4, int64_t cap, int64_t counts[4]);

/* wtp_relax_step followed by wtp_relax_layers_dev on the positions it produced, with one read-back
 * and one synchronisation for both: the layers of iteration i+1 come home with the statistics of
 * iteration i.  */
int wtp_relax_step_layers(wtp_ctx* ctx, int rebuild, wtp_step_stats* stats, int axis, double lo_in, double hi_in,
                          double lo_out, double hi_out, void* d_lo4, void* d_hi4, int64_t cap, int64_t counts[4]);

/* The same for a block decomposition: layers along up to three axes (bit a of axes_mask set), all with the one
 * read-back.  counts[4*a .. 4*a+3] as above; d_lo4[a] / d_hi4[a] hold `cap` rows each.  */
int wtp_relax_step_layers3(wtp_ctx* ctx, int rebuild, wtp_step_stats* stats, int axes_mask, const double lo_in[3],
                           const double hi_in[3], const double lo_out[3], const double hi_out[3], void* const d_lo4[3],
                           void* const d_hi4[3], int64_t cap, int64_t counts[12]);

/* ---- the context owns an RCCL communicator ---------------------------------------------------
 * One process per GPU, one context per process.  With these four calls and the wtp_relax_*_dev / *_layers3 /
 * set_fixed_dev / set_coverage_box entry points a caller without torch.distributed (the Julia side) runs the block
 * decomposition of DESIGN.md §7b through the C ABI alone; INTEGRATION.md lists the loop.  librccl is opened with dlopen
 * at the first call, so single-GPU users never load it.  No counterpart in the reference (it has no multi-GPU path). */
#define WTP_COMM_ID_BYTES 128
/* Rank 0 creates the id (ncclGetUniqueId); the caller carries the 128 bytes to the other ranks (MPI, a file, ...). */
int wtp_comm_unique_id(wtp_ctx* ctx, void* id_out);
/* Collective over all ranks: ncclCommInitRank on the context's device. */
int wtp_comm_init(wtp_ctx* ctx, const void* id, int rank, int nranks);
int wtp_comm_finalize(wtp_ctx* ctx);
/* One point-to-point round with the low and the high neighbour along an axis (peer = rank, or -1 for none).  Rows are
 * 16 bytes — the packed {x, y, z, w} fp32 rows wtp_relax_step_layers3 fills and wtp_relax_set_fixed_dev takes.  The
 * counts travel first, then the rows, all on the context's stream: on return the received counts are known on the
 * host and the rows are stream-ordered (the next launch on this context sees them).  d_recv_* hold `cap` rows; if a
 * peer sends more, the rows are dropped, the counts are still returned and the call fails with WTP_ERR_ARG (nobody
 * is left hanging).  Every rank that names a peer must be named by that peer in the same call. */
int wtp_comm_exchange_rows(wtp_ctx* ctx, int peer_lo, int peer_hi, const void* d_send_lo, int64_t n_send_lo,
                           const void* d_send_hi, int64_t n_send_hi, void* d_recv_lo, void* d_recv_hi, int64_t cap,
                           int64_t* n_recv_lo, int64_t* n_recv_hi);
/* The global view of a sweep, in place: maximum of max_force; sums of sum_u, sum_u2, n_move, n_fallback, n_uncovered,
 * n_escaped — what the stop rules of `_relax!` (src/repel.jl:293,305-334) and the ghost-width check read.  argmin_r
 * becomes the global minimum; argmin_i / argmin_j stay local indices on the rank that holds it and become -1 elsewhere. */
int wtp_comm_allreduce_stats(wtp_ctx* ctx, wtp_step_stats* stats);

/* ---- the whole sharded iteration behind the boundary ------------------------------------------------
 * wtp_block_* run one rank's share of a multi-GPU repel: what `_relax!`'s loop body (src/repel.jl:243-334) becomes when
 * the cloud is cut into the cells of an orthtree partition, one cell (an axis-aligned box) per rank.  The caller hands
 * over its owned points and every rank's box once, then calls wtp_block_step once per iteration — ghost exchange,
 * migration, hash, sweep, the global statistics and the ghost-width check all happen inside:
 *
 *   exchange   ONE grouped point-to-point round with every spatially adjacent rank (ncclSend/ncclRecv inside one
 *              group: faces, edges and corners directly, 7 peers for 2 x 2 x 2 octants, one xGMI link each).  Row counts
 *              are known beforehand: they rode with the previous iteration's statistics, so no host round trip sits
 *              between the counts and the rows.
 *   ghosts     rank q receives every foreign point within ghost_width + margin of its box; they become the fixed
 *              head of the local snapshot (searched, never moved, never counted).
 *   migration  a point that strayed more than `margin` past its owner's box travels in the same round, straight to
 *              the rank whose box holds it (64-bit global ids travel along); the sender keeps it as a ghost for
 *              this iteration.
 *   sweep      hash + sweep of [ghosts ; owned] (wtp_relax_step's kernels), then, from the positions it produced, the
 *              rows and counts of the NEXT exchange.
 *   statistics one all-gather per iteration carries {the step's statistics, the next row counts}; every rank reduces
 *              the gathered statistics in rank order (a fixed order: the global sums are reproducible).  This is the
 *              iteration's only host synchronisation.
 *   coverage   the sweep counts the queries whose support reaches past the box the snapshot is complete for; if any rank
 *              reports one, all ranks undo the step, widen the ghost layer by 1.5x and repeat it.
 * fp32, 3-D; constant spacing or a device-evaluated law (LOGLIKE / BOUNDARY_LAYER: ghosts need no spacing, only queries
 * do).  Needs wtp_comm_init (the context's RCCL communicator) or a caller-supplied transport.  */
typedef struct wtp_block_desc {
    int32_t rank, nranks;
    const double* boxes;  /* nranks x 6: {lo x, lo y, lo z, hi x, hi y, hi z} of every rank's box, half-open [lo, hi);
                             the boxes tile space (outer ends +-inf); identical on every rank                       */
    double ghost_width;   /* w: at least the largest support u0 * s of a query near a face (checked, widened on demand) */
    double margin;        /* lazy migration: a point changes owner once it is this far outside its box; < 0: w / 4  */
} wtp_block_desc;

typedef struct wtp_block_info {
    int64_t n_owned, n_ghost;   /* this rank, in the iteration just done                                         */
    int64_t n_sent_rows, n_recv_rows; /* ghost rows of the iteration's exchange (16 bytes each)                  */
    int64_t n_emigrated, n_immigrated;
    int32_t n_peers;            /* ranks this rank exchanges with                                                 */
    int32_t widened;            /* times the ghost layer was widened so far                                       */
    int32_t host_syncs;         /* host synchronisations this call made (1 in steady state)                       */
    int32_t redone;             /* 1 if the step was undone and repeated with a wider layer                       */
    double ghost_width;         /* current w                                                                      */
    int32_t overlapped;         /* 1 if the owned points were ranked into the cells while the ghost rows travelled */
    int32_t reserved;
} wtp_block_info;

/* Optional transport in place of the context's RCCL communicator (MPI without GPU awareness, tests with several ranks
 * on one GPU): host buffers only; the library stages through the host around the callbacks.  All ranks call in step. */
typedef struct wtp_transport {
    void* user;
    /* every rank contributes `bytes` bytes; recv holds nranks * bytes, rank-major */
    int (*allgather)(void* user, const void* send, void* recv, int64_t bytes);
    /* message j goes to and comes from rank peers[j] (send_bytes[j] / recv_bytes[j] may be 0) */
    int (*exchange)(void* user, int n_msgs, const int* peers, const void* const* send, const int64_t* send_bytes,
                    void* const* recv, const int64_t* recv_bytes);
} wtp_transport;
int wtp_block_set_transport(wtp_ctx* ctx, const wtp_transport* t); /* NULL: back to RCCL */

/* The boundary wall of the volume-only repel (src/repel.jl:75-87) for the NEXT wtp_block_open on this context:
 * d_wall_xyz n_wall x 3 fp32 on the context's GPU, the SAME array (same order) on every rank; n_wall = 0 clears it.
 * Copied; the caller's array is free on return.  WTP_ERR_STATE while a block session is open.
 * Every rank keeps the wall points inside its coverage box (its box grown by ghost_width + margin, the box of
 * wtp_relax_set_coverage_box) as the leading part of its snapshot's fixed head: searched, never moved, never sent,
 * migrated, counted in n_move or returned by wtp_block_get; selected again on every widening.  One rank whose box
 * holds the whole wall runs the session of wtp_relax_init([wall ; owned], n_fixed = n_wall): same positions.  */
int wtp_block_set_wall(wtp_ctx* ctx, const void* d_wall_xyz, int64_t n_wall);

/* d_owned_xyz: n_owned x 3 fp32 on the context's GPU; d_gid: n_owned int64 global ids (device).  spacing / force / k /
 * alpha as wtp_relax_init.  Collective: every rank calls it.  */
int wtp_block_open(wtp_ctx* ctx, const wtp_block_desc* desc, const void* d_owned_xyz, const int64_t* d_gid,
                   int64_t n_owned, const wtp_spacing_desc* spacing, const wtp_force_desc* force, int k,
                   double alpha_lo, double alpha_max);
/* One iteration; stats = the GLOBAL view (max / sums over all ranks), on every rank.  The closest pair argmin_i /
 * argmin_j / argmin_r is numbered as the snapshot of the assembled cloud [wall ; volume]: wall point k is k, the volume
 * point with global id g is n_wall + g (without a wall: g).  Of equally close pairs the one with the smallest argmin_i.
 * argmin_j is -1 if it is a ghost whose global id is 2^32 - 1 or more (ghost rows carry 32 bits of it).  info may be
 * NULL.  */
int wtp_block_step(wtp_ctx* ctx, wtp_step_stats* stats, wtp_block_info* info);
/* n_iters iterations; conv_out[n_iters] = global max |F| s per iteration (may be NULL).  */
int wtp_block_run(wtp_ctx* ctx, int n_iters, double* conv_out, wtp_step_stats* last, wtp_block_info* info);
/* The reference's stop rules on the global statistics (src/repel.jl:305-334, same order as wtp_relax_run_until): every
 * rank sees the same numbers, so all stop at the same iteration.  */
int wtp_block_run_until(wtp_ctx* ctx, int max_iters, double tol, int stall_after, double cv_target, double* conv_out,
                        int* n_done, int* reason, wtp_step_stats* last);
/* Owned points now: *n_owned of them; d_xyz_out (n x 3 fp32) and d_gid_out (int64) are device buffers of at least
 * `cap` entries, either may be NULL (then only the count is returned).  */
int wtp_block_get(wtp_ctx* ctx, void* d_xyz_out, int64_t* d_gid_out, int64_t cap, int64_t* n_owned);
int wtp_block_close(wtp_ctx* ctx);
/* Host-only helpers (no GPU): the block grid px x py x pz for nranks (as cubic as possible, larger factors on later
 * axes) and the Morton rank of block (ix, iy, iz) — the orthtree's leaf order along its Z-curve, so neighbouring ranks
 * are spatial neighbours (src/octree/spatial_octree.jl:283 `find_leaf` is the reference's only use of that order). */
int wtp_block_grid(int nranks, int p_out[3]);
int wtp_block_morton_rank(int ix, int iy, int iz, const int p[3]);
/* ---- sharded set_topology ("same decomposition, no iteration; output stays sharded") ----------------
 * KNNTopology / RadiusTopology rows (src/topology.jl:79-97) of a cloud that stays split across ranks, e.g. what
 * wtp_block_get leaves behind after a block repel (call wtp_block_get, wtp_block_close, then these).  Every rank holds
 * its owned points and their global ids; the assembled cloud is cloud[gid[i]] = xyz[i] on the rank that owns point i,
 * so the gids of all ranks together are exactly 0 .. N_total - 1 (N_total < 2^31).  Per call and rank:
 *   1. one all-gather of {owned count, bounding box of the owned points, gid range and fingerprint, status, arguments}:
 *      every check that needs global knowledge (k against N_total, k <= 128, gids in range and each owned once, the same
 *      k / r everywhere, a NULL output with n_owned > 0, a busy context) runs on the gathered words, so ALL RANKS
 *      RETURN THE SAME STATUS and none is left waiting in a collective.  A rank's region is the bounding box of its own
 *      points (no caller-supplied box: points a lazy migration left outside their box cost ghosts, never correctness).
 *   2. ghosts: rank r sends rank q every owned point inside q's box grown by q's own width w_q (inclusive, fp32
 *      thresholds rounded outward), 16-byte rows {x, y, z, bits(gid)}, in one grouped exchange whose row counts
 *      reached every rank in an all-gather first.
 *   3. the local set [owned + ghosts] is laid out in ascending gid order, so the search's (d², index) order IS the
 *      single-GPU (d², gid) order: ties inside a row and at the k-th place resolve as on one GPU.
 *   4. the single-context k-NN / radius kernels search the local set.
 *   5. row i is complete if its k-th d² (radius: r²) lies strictly below the squared distance to the nearest face of
 *      the rank's box grown by w_q, with a margin for the fp32 rounding of d²; a face beyond the global bounding box
 *      counts as infinitely far.  If any rank has an incomplete row, every such rank widens w_q by 1.5x and all redo
 *      2-5.  Radius: w_q is r rounded outward, so the first round completes every row.
 * Rows carry GLOBAL ids and equal, bit for bit, the rows wtp_knn / wtp_radius_fill return for the assembled cloud;
 * distances too.  fp32, 3-D.  Collective; uses the context's RCCL communicator (wtp_comm_init with the same rank /
 * nranks) or wtp_block_set_transport's callbacks.  WTP_ERR_STATE while a relax or block session is open on the
 * context.  */
typedef struct wtp_block_topo_info {
    double  width;        /* ghost width this rank ended with                                                  */
    int64_t n_ghost;      /* foreign points in this rank's local set                                           */
    int64_t n_recv_rows;  /* rows received in the last exchange                                                */
    int32_t n_peers;      /* ranks this rank received from in the last round                                   */
    int32_t widened;      /* widening rounds (all ranks report the same number)                                */
    int32_t host_syncs;   /* host synchronisations this call made                                              */
    int32_t reserved;
} wtp_block_topo_info;

/* Collective.  Rows of this rank's owned points, in the caller's order: row i equals wtp_knn's row of point gid[i] of
 * the assembled cloud, in global ids.  d_xyz: n_owned x 3 fp32 (device), d_gid: n_owned int64 (device); n_owned may
 * be 0.  width <= 0: the library estimates a first width from each rank's point count and box.  d_idx_out:
 * n_owned x k int64 (device); d_dist_out: n_owned x k fp32 (device) or NULL; info may be NULL.  */
int wtp_block_knn(wtp_ctx* ctx, int rank, int nranks, const void* d_xyz, const int64_t* d_gid, int64_t n_owned, int k,
                  int include_self, double width, int64_t* d_idx_out, float* d_dist_out, wtp_block_topo_info* info);
/* Collective first phase of the sharded RadiusTopology.  d_offsets_out: n_owned + 1 int64 (device; exclusive scan of
 * this rank's row lengths, caller order).  The rows are computed here and kept on the context for the fill.  */
int wtp_block_radius_offsets(wtp_ctx* ctx, int rank, int nranks, const void* d_xyz, const int64_t* d_gid, int64_t n_owned,
                             double r, int64_t* d_offsets_out, wtp_block_topo_info* info);
/* Local second phase: d_idx_out (device, offsets[n_owned] int64) gets the rows in global ids, each sorted ascending by
 * (d², gid): equal to wtp_radius_fill's rows of the assembled cloud.  WTP_ERR_STATE without a preceding
 * wtp_block_radius_offsets on this context.  */
int wtp_block_radius_fill(wtp_ctx* ctx, int64_t* d_idx_out);
/* Collective.  wtp_knn_stats of the assembled cloud without assembling it: every rank searches its rows as
 * wtp_block_knn does (include_self = 1, distances into an internal buffer), reduces its owned rows on the device, and one
 * more all-gather carries each rank's partial struct; every rank merges the partials in rank order ((count, sum, M2)
 * triples for the variances), so `out` is the global view, the same bytes on every rank.  nn_min_i / nn_max_i are
 * global ids, ties to the smaller gid.  A rank with n_owned = 0 contributes the neutral element.  2 <= k <= N_total
 * (k counts the point itself).  d_h: n_owned device doubles in the caller's order or NULL (then h_const as in
 * wtp_knn_stats); the ranks that own points must agree on whether there is a spacing.  d_nn_out: n_owned fp32 (device)
 * or NULL.  A bad argument on any rank, a bad spacing value included, is WTP_ERR_ARG on all of them.  */
int wtp_block_knn_stats(wtp_ctx* ctx, int rank, int nranks, const void* d_xyz, const int64_t* d_gid, int64_t n_owned, int k,
                        const double* d_h, double h_const, double coord_radius, double width, struct wtp_knn_stats* out,
                        float* d_nn_out, wtp_block_topo_info* info);
/* Grouped point-to-point primitive of the exchange, exposed for callers that drive their own iteration: message j is
 * sent to and received from rank peers[j], rows of 16 bytes, device buffers, stream-ordered on the context's stream.
 * Counts must agree on both sides (ncclSend/ncclRecv semantics).  peers[j] may equal the caller's own rank. */
int wtp_comm_exchange_peers(wtp_ctx* ctx, int n_msgs, const int* peers, const void* const* d_send, const int64_t* n_send,
                            void* const* d_recv, const int64_t* n_recv);
/* All-gather of `bytes` bytes per rank between device buffers on the context's stream (bytes a multiple of 8). */
int wtp_comm_allgather_dev(wtp_ctx* ctx, const void* d_send, void* d_recv, int64_t bytes);

/* Coverage of a sharded session: the caller guarantees that the snapshot holds every point of
 * the global cloud with lo <= coord[axis] <= hi (its slab plus the ghost layers; an end may be
 * +-inf).  A sweep then counts in stats.n_uncovered the movable points whose answer needs more:
 * a k-th neighbour (compact-support sweep: the law's support u0*s, or the nearest neighbour)
 * farther away than the nearer end of that range — so the caller can widen the layer and redo
 * the step (wtp_relax_revert).  axis < 0: unlimited (default).  */
int wtp_relax_set_coverage(wtp_ctx* ctx, int axis, double lo, double hi);
/* The same for a block decomposition (orthtree cells, 2 x 2 x 2 octants on 8 GPUs): the snapshot
 * holds every point of the global cloud inside the box lo[a] <= coord[a] <= hi[a] (the rank's block plus the
 * ghost layers received from its face, edge and corner neighbours; ends may be +-inf).  */
int wtp_relax_set_coverage_box(wtp_ctx* ctx, const double lo[3], const double hi[3]);

/* Replace the fixed head of the snapshot by n_fixed_new points (packed 4-vectors in device
 * memory, 4th component ignored).  Movable indices are unchanged; the next wtp_relax_step
 * rebuilds.  Constant spacing or a device-evaluated law (LOGLIKE / BOUNDARY_LAYER: the law is evaluated at the
 * movable points only, so the new head needs no spacing values); not with a PER_POINT array.  */
int wtp_relax_set_fixed_dev(wtp_ctx* ctx, const void* d_fixed4, int64_t n_fixed_new);

/* ---- measurement hooks (bench.py, profiles/) -------------------------------------- */

/* Device time (ms, HIP events on the context's stream) spent in each phase since the
 * last reset: [0] hash build, [1] neighbour sweep (dominant kernel), [2] fallback +
 * reductions, [3] sweep-kernel launches counted.  */
int wtp_timers_get(wtp_ctx* ctx, double out[4]);
int wtp_timers_reset(wtp_ctx* ctx);
/* Diagnostic builds only (-DWTP_DIAG=1): per-phase wave-cycle sums of the sweep kernel since the last
 * call ([0..6] phases, [7] waves); release builds return zeros.  tools/exp_diag.py. */
int wtp_debug_diag(wtp_ctx* ctx, unsigned long long out[16]);

/* Synthetic workload generator of SURVEY.md §8d, written straight into device memory:
 * value(i, axis) = (splitmix64(seed*2^40 + 3*(first+i) + axis) >> 40) * 2^-24.
 * d_out: n x dim of dtype on the context's GPU.  (bench.py / sharded driver only.) */
int wtp_gen_uniform_dev(wtp_ctx* ctx, uint64_t seed, int64_t first, int64_t n, int dim, int dtype,
                        void* d_out);

#ifdef __cplusplus
}
#endif
#endif /* WTP_H */
