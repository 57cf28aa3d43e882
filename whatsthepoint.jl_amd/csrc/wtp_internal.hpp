// wtp_internal.hpp — shared types of libwtp (gfx950 only; no portability layer).
//
// Data layout in HBM:
//   Pt<T>      one point = {x, y, z, bits(id)} : float4 (16 B) / double4 (32 B).  One 16-B
//              (or 2x16-B) coalesced access moves a whole point; the id rides along so the
//              counting sort permutes nothing else.
//   cell_start int32[ncells+1]  exclusive scan of per-cell counts (row-major cz,cy,cx).
//   Points of one cell are contiguous, cells of one x-row are contiguous.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/wtp.h"

namespace wtp {

// ---- point record ---------------------------------------------------------------------------
template <typename T> struct PtOf;
template <> struct PtOf<float> { using type = float4; };
template <> struct PtOf<double> { using type = double4; };
template <typename T> using Pt = typename PtOf<T>::type;

using KnnStats = struct ::wtp_knn_stats; // (the C name is also the call's: see include/wtp.h)

// One call for both dtypes: f(float{}) for WTP_F32, f(double{}) for WTP_F64; f takes `auto t` and works on T = decltype(t).
template <typename F> inline auto by_dtype(int dtype, F&& f) { return dtype == WTP_F32 ? f(float{}) : f(double{}); }

__host__ __device__ inline float id_to_w(float, int32_t id) { return __builtin_bit_cast(float, id); }
__host__ __device__ inline double id_to_w(double, int32_t id) {
    return __builtin_bit_cast(double, (int64_t)id);
}
__host__ __device__ inline int32_t w_to_id(float w) { return __builtin_bit_cast(int32_t, w); }
__host__ __device__ inline int32_t w_to_id(double w) {
    return (int32_t)__builtin_bit_cast(int64_t, w);
}

// ---- uniform grid (device resident; written by grid_setup_kernel) ------------------------------
// Cell of coordinate v on axis a: clamp((int)floor((v - org[a]) * inv_c), 0, n[a]-1).
// Points outside the box (repel has no wall inside the sweep) pile into the edge cells; the
// exactness radius treats those cells as unbounded outward.
template <typename T> struct Grid {
    T org[3];
    T c;      // cell edge
    T inv_c;  // 1/c
    T margin; // c * 2^-8: covers the rounding of the cell map (n[a] <= 4096 enforced)
    int32_t n[3];
    int32_t ncells;
    int32_t nb[3];   // bricks per axis
    int32_t nbricks;
    int32_t dim;
    int32_t npts;
    int32_t rad_wave_only; // RadiusTopology builds: rows are expected to outgrow the brick kernel's 32 entries — the wave kernel serves every query
    int32_t pad_;
};

constexpr int kMaxAxisCells = 4096;

// Brick geometry of the fast path: one workgroup sweeps BX x BY x BZ cells, staging the
// (BX+2)(BY+2)(BZ+2) halo in LDS.
constexpr int BX = 4, BY = 4, BZ = 4;
constexpr int HX = BX + 2, HY = BY + 2, HZ = BZ + 2;
constexpr int HCELLS = HX * HY * HZ;
// RadiusTopology: a brick whose halo holds more points than this (~7.4 per cell) has rows beyond the lane-per-query
// kernel's 32 entries (a row is ~4.06 cells' worth of points): it belongs to the dense kernel, or to the wave kernel
constexpr int kRadDenseMin = 1600;
constexpr int kBrickThreads = 256;
constexpr int kRadArenaPerPoint = 48; // RadiusTopology: ids of the count phase's arena per point of the cloud (radius_count_t, wtp_topology.hip)
// partial-reduction slots: [0, brick_partials()) brick blocks, then kWavePartials, then kGenericPartials
constexpr int kWavePartials = 4096;    // wave-per-query kernel blocks
constexpr int kGenericPartials = 1024; // serial last-resort kernel blocks
int brick_partials();
constexpr int kGenericKMax = 128; // largest k the library accepts (generic kernel's list)

// ---- tuned search constants (measured) ------------------------------------------------
constexpr double kGammaCap = 1.0;       // first filter radius of the topology kernels, in cell edges (round 2: 1.08 -> 1.0, fewer ring prunes)
constexpr double kGammaCapSweep = 0.96; // the same for the sweep with explicit k-selection (4.28 -> 3.55 ms at 10 M)
constexpr double kTnnFrac = 0.8;        // CS sweeps: measured optimum between candidate volume and isolated-query hand-backs (0.9: 1.55 ms, 0.8: 1.44, 0.7: 1.69 per 10 M step)
constexpr double kRhoCs2 = 1.0;         // target points per cell of the round-2 compact-support sweep (the support floor usually binds)
constexpr double kRhoKsel = 1.2;        // points per cell of the wtp_ksel.hip grids at k + self = 22 (scales with k)
constexpr double kCapKsel = 40.0;       // points the first filter ball of wtp_ksel.hip is expected to hold at k + self = 22
constexpr int kGridReuseMax = 7;        // rebuilds of a relax session that may reuse a grid

// ---- per-block partial reductions of one sweep -------------------------------------------------
struct Partial {
    double max_force;
    double sum_u;
    double sum_u2;
    double argmin_r;   // +inf when empty
    int64_t argmin_i;  // snapshot-global id of the movable point (ties: lowest id)
    int64_t argmin_j;
    int64_t n_move;
};

// The 64-byte counter block of a search (ctx->fb_count; the float copy's in F64Stage::cnt): cleared with one memset before
// the kernels count in it, read and zeroed again, all 16 words, by a step's final reduction (reduce_partials_block).
// SearchArgs hands the kernels the address of each word.
struct StepCounters {
    int32_t brick_handbacks, pad1_; // [0] queries the brick kernels hand to the wave kernel (SearchArgs::fb_count)
    int32_t nn_count, pad3_;        // [2] wtp_cs2.hip: queries whose nearest neighbour the follow-up kernel still has to find
    int32_t wave_handbacks, pad5_;  // [4] queries the wave kernel hands to the serial one (SearchArgs::fb2_count)
    int32_t ball_count, pad7_;      // [6] what the ball kernel leaves for the exact path
    int32_t uncovered, pad9_[3];    // [8] sharded sessions: queries whose neighbourhood reaches past the covered range
    int32_t escaped, pad13_[3];     // [12] octree wall rule: movable points that left the mesh in this sweep
};
static_assert(sizeof(StepCounters) == 64 && offsetof(StepCounters, escaped) == 48, "16 words: the reduction zeroes exactly these");

// RadiusTopology's counter block (RadiusState::pos), cleared by every count phase
struct RadCursor {
    unsigned long long arena_next; // [0, 8) next free id of the arena (wtp_radb.hip takes pieces of it)
    int32_t bricks_listed;         // [8, 12) bricks listed for the dense kernel
    int32_t dense_queries;         // [12, 16) diagnostics: queries the dense kernel served (WTP_DEBUG prints it)
};
static_assert(sizeof(RadCursor) == 16, "wtp_radb.hip addresses these words by offset");

struct ForceParams {
    int32_t kind;
    double beta, u0, gamma;
};

// ---- kernel parameter blocks -------------------------------------------------------------------
template <typename T> struct SearchArgs {
    const Grid<T>* grid;
    const Pt<T>* snap;         // sorted snapshot (search structure)
    const int32_t* cell_start; // ncells+1
    const Pt<T>* query;        // query positions, slot-aligned with snap (== snap when fresh)
    int32_t n;
    int32_t k;                 // neighbours wanted (relax: kk incl. self slot)
    int32_t include_self;      // topology: 1 = raw search result, 0 = self removed by index
    // topology outputs (row = original id)
    int32_t* idx_out;
    T* dist_out;
    // relax
    Pt<T>* out;                // new positions, slot order
    T* forces;                 // slot order
    T* nn_dist;
    int32_t* nn_id;
    const T* spacing_pp;       // per-point spacing by original id, or nullptr
    T spacing_const;
    T alpha_lo, alpha_max;
    T beta, u0, gamma;
    int32_t force_kind;
    int32_t n_fixed;
    Partial* partials;         // [n_partials]
    int32_t n_partials;
    // blocks each sweep kernel was launched with = partial slots it wrote (set by the launchers):
    // brick [0, used_brick), wave [brick_partials(), +used_wave), serial [n_partials - kGenericPartials, +used_generic)
    int32_t used_brick, used_wave, used_generic;
    // RadiusTopology through the brick kernel: r^2, row lengths out (count phase) or row starts in (fill phase)
    T radius2;
    int32_t* rad_counts;
    const int64_t* rad_offsets;
    int32_t rad_fill;
    int32_t* rad_tmp;          // count phase, fp32 brick kernel: the sorted row of every query it serves (32 ids each) is parked here,
    uint8_t* rad_done;         // and the query marked (1), so that the fill phase copies rows instead of searching again (or nullptr)
    int32_t* rad_arena;        // count phase, wave kernel: ranked rows of any length, bump-allocated (mark 2, start in rad_arena_off)
    int64_t* rad_arena_off;
    unsigned long long* rad_arena_pos;
    int64_t rad_arena_cap;
    int32_t* rad_bricks;       // bricks listed for the dense kernel (at most one per point)
    int32_t rad_dense;         // > 0: the brick-staged wave-per-query kernel (wtp_radb.hip) takes the bricks whose halo holds more than kRadDenseMin and at most this many points
    // fallback work list
    int32_t* fb_list;
    int32_t* fb_count;
    int32_t* fb2_list;         // second level: wave kernel -> serial kernel
    int32_t* fb2_count;
    int32_t* nn_list;          // round-2 sweep: queries whose nearest neighbour the follow-up kernel still has to find
    int32_t* nn_count;
    int32_t* ball_list;        // what the ball kernel (variable-spacing hand-backs) leaves for the exact path, and its count
    int32_t* ball_count;
    const int32_t* stop;       // wtp_relax_run_until: non-zero once a stop rule has fired; later sweeps of the batch do nothing
    // sharded sessions: the snapshot is complete only for cover_lo <= coord[cover_axis] <= cover_hi;
    // queries whose neighbourhood reaches past that range are counted (wtp_relax_set_coverage)
    int32_t cover_axis;        // -1: unlimited; 0..2: a slab along that axis; 3: the box cover_lo3 .. cover_hi3
    T cover_lo, cover_hi;
    T cover_lo3[3], cover_hi3[3];
    int32_t* uncovered;
    // tunables
    T gamma_cap;               // initial filter radius cap, in cell edges
    float cap_count;           // k-selection kernels: points the first filter ball is expected to hold (0: fixed gamma_cap * c)
    T tnn_frac;                // CS sweeps: nearest-neighbour margin of the ring, in cell edges (kTnnFrac)
    int32_t brick_hcap;        // LDS point capacity for the brick kernel (0 = default)
    int32_t cs2_bx;            // > 0: brick length (own cells along x) of the round-2 compact-support sweep (wtp_cs2.hip)
    const uint8_t* brick_dead; // wtp_cs2.hip, variable spacing: bricks whose points all went to the ball kernel's list already (cs2_dead_kernel), or nullptr
    int32_t brick_dead_cap;
    int32_t cs2_chunked;       // wtp_cs2.hip: runs longer than the hit masks are taken in chunks (variable spacing, several points per cell)
    int32_t counters_cleared;  // topology calls: the caller cleared fb_count / fb2_count (one StepCounters block) itself
    int32_t fb_r0;             // first block radius (cells) of the exact path for hand-backs; 0: the default (2: the 27 cells failed already)
    int32_t ksel_bx;           // > 0: the grid was built for the k-selection kernels of wtp_ksel.hip; largest brick length along x
    unsigned long long* diag;  // -DWTP_DIAG builds: per-phase wave-cycle sums (8 slots), else unused
};

// ---- device buffer with capacity: grown by ensure(), freed with its owner ------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
        o.p = nullptr;
        o.cap = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() {
        if (p) hipFree(p);
    }
};

// Input view of a hash build whose input array still holds stale fixed points and has the new
// ones appended: entry i is dropped when i < n_old and its id < fixed_old; kept entries below
// n_old get id + id_shift (fixed head resized), entries from n_old on keep their id.
struct HashView {
    bool active = false;
    int64_t n_in = 0;    // entries in the input array
    int64_t n_old = 0;   // entries of the previous snapshot (stale fixed points among them)
    int32_t fixed_old = 0;
    int32_t id_shift = 0;
};

// One hash build (build_hash in wtp_hash.hip): from the Pt array `in` the sorted `out`, cell_start and the grid.  The
// constructor takes what every build names; the rest reads as what the caller sets, on top of these defaults.
template <typename T> struct HashBuild {
    const Pt<T>* in;
    Pt<T>* out;
    int64_t n;                   // points of the structure (a view may read them from a longer input array)
    int dim;
    int k;                       // scales the target occupancy
    double radius = 0.0;         // > 0: cell edge >= radius (RadiusTopology)
    double rho_direct = 0.0;     // > 0: the caller fixes the occupancy (points per cell) instead
    double min_cell = 0.0;       // floor of the cell edge (the force law's support)
    double cell_scale = 1.0;     // measured cell scale (GridTune::scale)
    HashView view;               // inactive: `in` holds exactly the n points
    bool keep_grid = false;      // keep the previous Grid (no bounding-box pass): the relax session's rebuilds
    bool canonical = true;       // order each cell by id (dirty marks, canon_kernel); false where rows are ordered by (d2, id) explicitly
    const double* box = nullptr; // clip the bounding box to this device box {lo xyz, hi xyz} (GridTune::clipped)
    HashBuild(const Pt<T>* in_, Pt<T>* out_, int64_t n_, int dim_, int k_) : in(in_), out(out_), n(n_), dim(dim_), k(k_) {}
    int64_t n_in() const { return view.active ? view.n_in : n; } // entries of the input array
};

// Part of a hash build issued ahead of time (block driver: while the ghost rows of the iteration travel): the old
// snapshot's entries [0, n_old) of `in` are already ranked into the cell counts.  One-shot; build_hash takes it over only
// when it matches the build it is asked for (prerank_matches in wtp_hash.hip), otherwise it zeroes the counts and ranks
// everything itself.
struct Prerank {
    bool valid = false;
    const void* in = nullptr;
    int64_t n_old = 0;
    int32_t fixed_old = 0;
    bool canonical = true; // dirty marks written
    const void *cnt = nullptr, *cr = nullptr, *dirty = nullptr;
};

// Measured tuning of a grid (build_hash_tuned, ksel_tune in wtp_tune.hip): the key it was measured for and what was measured.
// The topology calls keep one per context; a relax session keeps one for its own grid (only `valid` of the key: measured
// once per session) and one for the float copy of its Float64 sweeps.
struct GridTune {
    bool loose = false;      // Float64 sweeps: a cloud within 5 % of n fits, and a scale measured on a clipped box is kept (build_grid_cached)
    bool valid = false;
    bool clipped = false;    // the measured grid lies over a quantile box (find_robust_box, in ctx->box_dev): the rebuilds of a relax session clip to it
    int64_t n = 0;
    int dim = 0, kq = 0;     // kq: neighbours sought per query (self included)
    bool ksel = false;       // the grid was built for the k-selection kernels of wtp_ksel.hip
    double scale = 1.0;      // cell scale: < 1 when the occupied cells hold more than the box average
    double rho = 0;          // occupancy the grid was built with (the k-selection pick, ksel_pick_rho)
    int bx = 0, hcap = 0;    // wtp_ksel.hip: brick length along x and LDS point area (0: not measured)
};

// The kernels of a relax sweep on a fresh snapshot, chosen at every rebuild (sweep_route in wtp_relax.hip).  A stale snapshot
// (rebuild_every > 1) sends every query through the ball kernel on the routes that have one, else to the exact path.
enum class SweepRoute {
    Exact,    // wave-per-query and serial kernels for every query
    Select,   // fp32: brick_kernel<1,21|0,0>, explicit k-selection on 4 x 4 x 4 bricks (wtp_brick.hip)
    Ksel,     // fp32 3-D: ksel_kernel on the x-slowest layout (wtp_ksel.hip); Select until its geometry is measured
    Cs,       // fp32 2-D ClippedSpacingForce: brick_kernel<1,0,1> over cells that cover the law's support
    Cs2,      // fp32 3-D ClippedSpacingForce: cs2_kernel (wtp_cs2.hip)
    Cs64,     // fp64 ClippedSpacingForce: brick_cs_kernel<double> (wtp_brick64.hip), the ball kernel for wide supports
    Cs64Wave, // the same with WTP_BALL64=0: wide supports and stale snapshots go to the exact path
    Ball,     // a stale snapshot on Cs, Cs2 or Cs64: every query through the ball kernel (per step, never a session's route)
    F64Ksel,  // fp64 3-D k-nearest laws: fp32 candidates, exact re-ranking (wtp_sweep64.hip)
};

struct RelaxState {
    bool active = false;
    int64_t n = 0, n_fixed = 0;
    int dim = 3, dtype = 0, k = 0;
    int k_req = 0;           // k as requested (k = min(k_req, n) follows n when the fixed head is swapped)
    int spacing_kind = 0;
    double spacing_const = 0, alpha_lo = 0, alpha_max = 0;
    ForceParams force{};
    int bufS = -1, bufP = -1, bufOld = -1; // indices into pts[3]
    bool have_tree = false;
    bool can_revert = false;
    bool have_point_data = false;
    double spacing_max = 0;  // largest spacing value (host-side max of the per-point array)
    int brick_hcap = 0;      // LDS point capacity of the sweep's brick kernel (0 = not chosen yet)
    GridTune tune;           // cell scale (and, for the k-selection sweep, occupancy and brick geometry) measured on the first rebuild
    int grid_age = 0;             // rebuilds since the grid (bounding box, cell edge) was last computed
    int sweeps_since_rebuild = 0; // every sweep moves a point by at most its spacing (src/repel.jl:286-289)
    bool moved_by_hand = false;   // wtp_relax_set since the last rebuild: that bound is gone
    double spacing_typ = 0;  // mean spacing over the snapshot (floor of the compact-support cell edge)
    SweepRoute route = SweepRoute::Exact; // the sweep's kernels, chosen at the last rebuild
    bool cs_disabled = false; // measured on the first rebuild: support cells would be over-full, use the k-selection sweep
    double cs2_rho = 0;      // points per cell the sweep's bricks were sized for (cs2_tune)
    int cs2_bx = 0;          // > 0: the round-2 compact-support sweep (wtp_cs2.hip) with bricks of this many cells along x
    int64_t tuned_fixed = 0; // fixed points the grid / brick geometry was measured with (a swapped head re-measures when it differs by > 5 % of n)
    double sp_p0 = 0, sp_p1 = 0, sp_p2 = 0; // LOGLIKE / BOUNDARY_LAYER parameters
    HashView pending;        // wtp_relax_set_fixed_dev left its work to the next rebuild (see there)
    int64_t shard_extra = 0; // extra capacity of the point buffers once the fixed head gets replaced
    int64_t aux_off = 0;     // device-evaluated spacing laws: sp_hint / sp_cert are stored at [id - aux_off] (a swapped fixed head shifts the movable ids, not the entries)
    int swap_target = -1;    // relax_swap_begin .. relax_swap_commit (wtp_block.hip: migration)
    bool shard_grid_reuse = false; // block sessions: the grid is kept across a swapped ghost head (points outside it pile into edge cells, which every search treats as unbounded outward)
    int64_t grid_fixed = -1;       // fixed points the current grid's bounding box was computed with
    GridTune f64k_tune{/*loose=*/true}; // fp64 sweeps through fp32 candidates: the float copy's grid
    bool wall_active = false; // octree method: _constrain_octree runs after every sweep (wtp_relax_set_wall)
    double wall_offset = 0;   // inward nudge of a projected boundary point (src/repel.jl:143)
    int64_t wall_nm = 0;      // movable points the wall arrays are sized for
    int cover_axis = -1;     // sharded session: snapshot complete for cover_lo <= coord[axis] <= cover_hi
    double cover_lo = 0, cover_hi = 0;
    double cover_lo3[3] = {0, 0, 0}, cover_hi3[3] = {0, 0, 0}; // cover_axis == 3: a box (ends may be +-inf)
};

// ---- groups of wtp_ctx's fields ------------------------------------------------------------------------------------
// radius two-phase state (wtp_radius_count / wtp_radius_offsets, then wtp_radius_fill)
struct RadiusState {
    int64_t n = 0;
    int dim = 0, dtype = 0;
    double r = 0;
    int64_t nnz = 0;
    bool valid = false;
    bool offsets_dev = false; // wtp_radius_offsets left the CSR offsets in dist_out (device): fill may take them from there
    DevBuf pos;               // counter block: one RadCursor
    DevBuf bricks;            // the dense kernel's brick list
    bool dense_attr[2] = {false, false}; // wtp_radb.hip: the kernel's LDS size has been declared (fp32, fp64)
    bool dense_used = false;  // the count phase ran the dense kernel: the fill phase's wave kernel works from the hand-back list
    DevBuf tmp, done;         // RadiusTopology: rows parked by the count phase (32 ids per query), one byte per query
    DevBuf arena, arena_off;  // ... and the wave kernel's rows (any length), their starts; the bump counter sits behind the starts
};

// triangle mesh of the octree method (wtp_mesh.hip): bounding-volume tree nodes, pseudonormals
struct MeshState {
    DevBuf nodes, pn, io;
    int64_t nt = 0;
    int dtype = -1;
    double bbox[6] = {0, 0, 0, 0, 0, 0};
    double scale = 0;
    std::vector<double> face_host; // unit face normals (the returned boundary's normals, src/repel.jl:614)
    DevBuf wall_flags, wall_tri;   // per movable point: is_bnd | escaped (+ counter), landing triangle
    DevBuf wall_hint;              // per movable point: tree node of its nearest triangle at the last sweep
    DevBuf cls;                    // inside/outside class per cell of a uniform grid over the mesh bbox
    bool cls_ready = false;
    int cls_dim[3] = {0, 0, 0};
    double cls_cell = 0;
    DevBuf corners, cum;           // wtp_mesh_sample: nt x 9 corner coordinates (mesh dtype), running area sums (double), triangle order
    double total_area = 0;         // cum[nt - 1]
};

// closed boundary loops of a 2-D domain (wtp_loops.hip): search-tree nodes over the oriented segments, with the feature
// normals the sign needs in every node
struct LoopsState {
    DevBuf nodes, io;
    int64_t ns = 0;                        // segments (= vertices of the cleaned loops); 0: no index
    int dtype = -1;
    double bbox[4] = {0, 0, 0, 0};         // {min xy, max xy} (_compute_bbox_raw_2d)
    double scale = 0;                      // largest |coordinate| of the box
};

// What a sampler run needs to know of its domain, passed down from the entry point: the box the cell map lies over (and
// the fill's darts are drawn from), the index's dtype, its dimension (rows are {x, y, z, r} either way; dim 2 keeps
// z = 0 and a box whose third axis is [0, 0]) and which inside test a fill launches.
struct SampleDomain {
    double lo[3], hi[3];
    int dtype, dim;
    bool loops;                            // launch_loops_inside instead of launch_mesh_inside
};

// Poisson-disk surface sampling (wtp_sample.hip; its streams: wtp_sample_streams.hip): the accepted samples and their cell
// table stay on the device between wtp_mesh_sample and the wtp_mesh_sample_get* calls; the batch buffers are reused by
// every batch and by the dart read-out.  wtp_mesh_fill and wtp_mesh_front run in the same buffers (their seeds at the
// front of the accepted array), so one result is resident at a time.
enum class SampleKind { none, sample, fill, front, area };
struct SampleState {
    SampleKind kind = SampleKind::none; // the run whose result of the current mesh is resident; fill's and front's lie
                                   // behind n_seeds seed rows, and front's `dart` holds candidate indices
    int front_per = 0;             // candidates per parent of a resident front
    int64_t n_seeds = 0;
    int dtype = -1;
    int64_t n = 0, cap = 0;        // samples held, rows the arrays below have room for
    DevBuf pts, tri, dart, next;   // per sample: {x, y, z, r} (Pt), parent triangle, dart index, next sample of its cell
    DevBuf table;                  // open addressing over 64-bit cell keys: [keys ; heads], tsz slots each
    int64_t tsz = 0;
    int64_t bcap = 0;              // darts the batch buffers have room for
    DevBuf b_xyz, b_h, b_pts, b_tri, b_st, b_next, b_pos, b_last, b_table, b_blk;
    DevBuf b_in;                   // wtp_mesh_fill: the domain test's flag per dart
    int64_t b_tsz = 0;
    DevBuf ctl;                    // one SampleCtl
};

// A run's control block on the device: the kernels of a batch update it, the host reads it once per group of rounds.
constexpr int kSampleGroup = 8;    // rounds per group
struct SampleCtl {
    unsigned long long bad;        // smallest dart index with a bad spacing value (~0: none)
    unsigned long long rmin, rmax; // bits of the smallest / largest r (as double) a range pass saw
    long long n;                   // samples accepted so far
    long long miss;                // rejected darts in a row so far
    long long n_darts;             // darts taken so far
    int32_t stopped;               // 0 running, 1 the run ended, 3 a dart the run took has a bad spacing value
    int32_t reason;
    int32_t end;                   // batch-local index of the first dart the run does not take (INT_MAX: none)
    int32_t n_new;                 // samples the batch appended
    int32_t und[kSampleGroup];     // darts left undecided by each round of the group
    unsigned long long n_inside;   // wtp_mesh_fill: darts taken so far that were inside the mesh
};

// spacing-driven node octree over the mesh (wtp_node_tree.hip): the leaves as one array of 64-bit keys, always in leaf
// (Morton) order: a split puts the 8 children where their parent stood.  Everything else is scratch of a build or a
// read-out; nothing here is shared with the samplers.
struct NodeTreeState {
    bool valid = false;
    int dtype = -1;
    int64_t n = 0;                 // leaves
    int cur = 0;                   // keys[cur] holds them
    DevBuf keys[2], front[2];      // leaf keys; positions of the boxes the current level decides on
    DevBuf cnt, off, scan_tmp;     // boxes each leaf turns into (1 or 8), their exclusive scan
    DevBuf ctr, h, tol, lohi;      // per box of a pass: centre, h(centre), probe tolerance, {lo, hi}
    DevBuf flag, need, touch;      // per box of a pass: passed the size tests / split; wants the touch walk; its answer
    DevBuf pts, pcls;              // a chunk's probe points and their classes
    DevBuf cls, hout;              // per leaf: class, max(h(centre), sqrt(eps))
    DevBuf red;                    // counters and the integral's block partials
    DevBuf io;                     // wtp_node_tree_locate: points in, leaves out
    wtp_node_tree_info info{};
    // wtp_node_place: the resident placement (points, each point's leaf) and the scratch of a run
    bool placed = false;
    DevBuf p_xyz, p_leaf;          // the result: n x 3 of the tree's dtype, int64 leaves
    DevBuf p_w, p_cnt, p_cum, p_f, p_fcum, p_tile; // per leaf: weights of both groups, counts, their sums, F, its sums; scan tiles
    DevBuf p_cand, p_cleaf, p_in;  // candidates, their leaves, their inside flags
    wtp_node_place_info pinfo{};
};

struct KdTree {
    DevBuf nodes;      // variable spacings: kd-tree over the boundary points (heap order)
    int64_t m = 0;     // nodes in it; the key below identifies the boundary it was built from
    uint64_t key = 0;
    int dim = 0, dtype = -1;
};

struct Timers {
    bool timing = false;      // per-phase event pairs around every step: off until wtp_timers_reset asks for them (6 event records per step are a third of a small cloud's step)
    bool timing_forced = false; // WTP_TIMING in the environment decides, wtp_timers_reset does not
    double t_hash = 0, t_sweep = 0, t_other = 0;
    int64_t n_sweep_launches = 0;
    std::vector<hipEvent_t> ev_pool;
    struct Span { int a, b, kind; };
    std::vector<Span> spans;
    int ev_used = 0;
    int ev_last_end = -1;     // the event that closed the latest span: the next span starts from it (no second record)
};

// fp64 sweeps through fp32 candidates (wtp_sweep64.hip): the session's grid, cell table and box parked while the float
// copy's are built and searched; the fp64 points and their session slots in the float copy's order; the search's own
// lists and their counter block (a StepCounters)
struct F64Stage {
    DevBuf grid_b, cell_start_b, box_b, s64, slot, lists, cnt;
};

// How this rank reaches the others (wtp_comm.hip): the caller's host callbacks (wtp_block_set_transport) or, without them,
// the context's RCCL communicator.  The block driver and the sharded topology both go through transport_ready,
// transport_allgather and transport_exchange below.
struct Transport {
    bool host = false;                         // wtp_block_set_transport gave callbacks
    wtp_transport tr{};
    std::vector<unsigned char> hbuf_a, hbuf_b; // host staging around the callbacks: rows out, rows in
    DevBuf gbuf;                               // an all-gather through RCCL: [this rank's words ; every rank's]
};

// a device region of 16-byte rows that messages of a grouped exchange lie in
struct RowRegion {
    void* d;
    int64_t rows;
};

// The reference's stop rules (`_relax!`, src/repel.jl:305-334) for one run: on the device for wtp_relax_run_until
// (ctx->stop_state), on the host for wtp_block_run_until.  best_cv starts at +inf (typemax(U), src/repel.jl:238).
struct StopState {
    int32_t stopped, reason, n_done, last_impr;
    double best_cv;
};

// One sweep's statistics (sweep number iter1, from 1) under the rules, in the reference's order: cv_target (the caller
// then reverts p to p_old), the stall counter on the CV of d_NN / s, the tolerance on max |F| s.  reason: 1 tol,
// 2 cv_target, 3 stall.
__host__ __device__ inline void stop_rules_apply(StopState& s, const wtp_step_stats& st, int iter1, double tol, int stall_after,
                                                 double cv_target) {
    if (s.stopped) return;
    s.n_done = iter1;
    const double conv = st.max_force;
    if ((stall_after > 0 || cv_target > 0) && st.n_move > 0) {
        const double n = (double)st.n_move, mu = st.sum_u / n;
        const double var = st.sum_u2 / n - mu * mu;
        const double cv = sqrt(var > 0.0 ? var : 0.0) / mu; // _dnn_cv, src/repel.jl:374-386
        if (cv_target > 0 && cv <= cv_target) {
            s.stopped = 1;
            s.reason = 2;
            return;
        }
        if (stall_after > 0) {
            if (cv < s.best_cv * (1 - 1.0e-3)) {
                s.best_cv = cv;
                s.last_impr = iter1;
            } else if (iter1 - s.last_impr >= stall_after) {
                s.stopped = 1;
                s.reason = 3;
                return;
            }
        }
    }
    if (conv < tol) {
        s.stopped = 1;
        s.reason = 1;
    }
}

} // namespace wtp

struct wtp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;     // the stream every launch goes to
    hipStream_t own_stream = nullptr; // created with the context; `stream` unless wtp_set_stream lent another
    std::string err;
    int sm_count = 256;
    // switches, read from the environment by wtp_create only
    double rho = 9.0;          // WTP_RHO: points per cell of the k = 21 selection grids (round 2: 8 -> 9, fewer hand-backs; measured)
    int force_generic = 0;     // WTP_FORCE_GENERIC=1: the exact wave / serial path for everything (sums in the reference's order)
    int full_select = 0;       // WTP_FULL_SELECT=1: never use the compact-support sweep
    int ksel = 1;              // WTP_KSEL=0: the round-1 k-selection kernels (4 x 4 x 4 bricks, wtp_brick.hip) instead of wtp_ksel.hip
    int ball64 = 1;            // WTP_BALL64=0: Float64 variable-spacing hand-backs straight to the wave kernel
    int f64_ksel = 1;          // WTP_F64_KSEL=0: Float64 sweeps of the k-nearest laws on the exact wave-per-query path
    int radius_dense = 1;      // WTP_RADIUS_DENSE=0: RadiusTopology without the brick-staged kernel for long rows (wtp_radb.hip)
    int block_overlap = 1;     // WTP_BLOCK_OVERLAP=0: block sessions rank the owned points into the cells after the ghost rows arrive, not while they travel
    bool debug = false;        // WTP_DEBUG: hand-back counts and brick geometry on stderr
    bool debug_kd = false;     // WTP_DEBUG_KD: node visits of the spacing law's tree walk on stderr
    size_t cs2_smem = 0;       // launch attributes of cs2_kernel cached per context
    const void* cs2_fn = nullptr; // (and the variant they belong to)
    int cs2_occ = 0;
    // (kernel, dynamic LDS bytes) -> blocks per CU, per CONTEXT: the dynamic-LDS attribute and the occupancy are
    // properties of a kernel on one device, and several contexts (devices) may live in one process
    std::map<std::pair<const void*, size_t>, int> launch_cache;
    // topology calls: the grid tuning of the last call, reused for a cloud of the same size (knn_dev_t; knn_dev_f64 for the
    // fp32 candidate search of fp64 calls)
    wtp::GridTune knn_tune, knn64_tune;
    // pooled device buffers
    wtp::DevBuf pts[3];        // Pt arrays
    wtp::DevBuf raw_in;        // AoS staging of host input
    wtp::DevBuf cell_of, rank_of, cell_cnt, cell_start, scan_tmp;
    wtp::DevBuf grid, bbox_part, occ;
    wtp::DevBuf box_dev;       // robust box {lo xyz, hi xyz} (doubles) + histogram scratch behind it
    wtp::DevBuf idx_out, dist_out, counts_out;
    wtp::DevBuf cand_idx, cand_dist, f32_pts; // fp64 topology: fp32 candidate lists and the float copy of the cloud
    wtp::F64Stage f64k;
    wtp::DevBuf forces, nn_dist, nn_id, spacing_pp;
    wtp::DevBuf partials, stats, fb_list, fb_count, fb2_list, fb2_count, nn_list;
    wtp::RadiusState rad;
    wtp::DevBuf brick_dead;    // wtp_cs2.hip, variable spacing: one byte per brick (cs2_dead_kernel)
    wtp::Prerank prerank;             // wtp_hash.hip: prerank_old_snapshot
    int64_t preranked_builds = 0;     // hash builds that took a first half over
    hipStream_t comm_stream = nullptr; // transport_exchange: the grouped round runs here while the caller's work runs on `stream`
    hipEvent_t ev_comm_a = nullptr, ev_comm_b = nullptr;
    bool hash_scratch_clean = false;  // cell counts and dirty map are all-zero (every completed build leaves them so)
    bool counters_clean = false;      // the counter block (StepCounters in fb_count) is all-zero (the step's final reduction leaves it so)
    wtp::DevBuf stop_state;           // wtp_relax_run_until: {stopped, reason, n_done, last_impr, best_cv} on the device
    const int32_t* stop_dev = nullptr; // its first word while such a run is enqueued, else NULL (kernels then never look)
    wtp::DevBuf scratch;       // misc (relax_get staging, radius rows)
    wtp::DevBuf kstats;        // wtp_knn_stats: block partials, the result, the first bad spacing index
    wtp::DevBuf ngraph;        // wtp_orient_normals / wtp_normal_components: components, per-component minima, control block
    wtp::DevBuf diag;          // diagnostic builds only
    wtp::DevBuf ins_in, ins_elems, ins_partial, ins_out; // isinside filter
    wtp::MeshState mesh;
    wtp::LoopsState loops;
    wtp::SampleState sample;
    wtp::NodeTreeState ntree;
    wtp::DevBuf sp_hint;       // variable spacings: nearest tree node of each snapshot point at the last sweep
    wtp::KdTree kd;
    int64_t n_syncs = 0;       // host synchronisations of the context's stream so far (wtp_block_info.host_syncs counts with it)
    void* block = nullptr;     // wtp::BlockState (wtp_block.hip): this rank's share of a block-decomposed repel
    void* block_topo = nullptr; // wtp::TopoState (wtp_block_topo.hip): buffers of the sharded KNN / radius rows
    void* comm = nullptr;      // ncclComm_t (wtp_comm.hip); rank and size of the communicator
    int comm_rank = 0, comm_size = 0;
    wtp::Transport transport;  // callbacks in place of the communicator, and the staging either one needs (wtp_comm.hip)
    wtp::DevBuf comm_scratch;
    wtp::DevBuf sp_cert;       // device-evaluated spacing laws: per point, where it stood at its last tree walk and the bound that walk left (wtp_spacing.hip)
    void* host_pinned = nullptr;
    size_t host_pinned_cap = 0;
    wtp::RelaxState relax;
    wtp::Timers timers;
};

namespace wtp {

inline StepCounters* step_counters(wtp_ctx* ctx) { return (StepCounters*)ctx->fb_count.p; } // the context's counter block

// ---- wtp_context.hip: error plumbing, the buffer pool, timing spans, the entry points' argument checks ---------
int fail(wtp_ctx* ctx, int code, const std::string& msg);
int sync(wtp_ctx* ctx);        // the host waits for the context's stream (counted in n_syncs)
size_t tsize(int dtype);       // bytes of a coordinate
size_t pt_size(int dtype);     // bytes of a Pt record
int check_cloud(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype);
int check_idle(wtp_ctx* ctx);  // no relax session holds the context's buffers
int check_k(wtp_ctx* ctx, int64_t n, int k, int include_self);
int ensure_pinned(wtp_ctx* ctx, size_t bytes); // the context's page-locked staging block, at least this large
#define WTP_HIP(ctx, call)                                                                    \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ::wtp::fail(ctx, e_ == hipErrorOutOfMemory ? WTP_ERR_OOM : WTP_ERR_HIP,    \
                               std::string(#call) + ": " + hipGetErrorString(e_));            \
    } while (0)

int ensure(wtp_ctx* ctx, DevBuf& b, size_t bytes);
template <typename T> Pt<T>* pts_of(wtp_ctx* ctx, int i) { return (Pt<T>*)ctx->pts[i].p; } // point buffer i as Pt<T>
int need_session(wtp_ctx* ctx, const char* entry); // guard of the relax entry points: a context with an active session
// sets the kernel's dynamic-LDS limit once per (context, kernel, size) and returns the blocks per CU it can hold
int launch_occupancy_of(wtp_ctx* ctx, const void* fn, int threads, size_t smem);

// timing spans: kind 0 hash, 1 sweep, 2 other
int span_begin(wtp_ctx* ctx, int kind);
void span_end(wtp_ctx* ctx, int span);
void spans_collect(wtp_ctx* ctx);

// ---- wtp_tune.hip: measured grids (see GridTune) and the owner of the context's grid ----------------------------
template <typename T> int build_hash_tuned(wtp_ctx* ctx, GridTune& t, HashBuild<T> b, Grid<T>* hg_out, double* rho_eff_out);
template <typename T> int ksel_tune(wtp_ctx* ctx, GridTune& t, HashBuild<T> b, Grid<T>& hg, double& rho_eff);
template <typename T> int build_grid_cached(wtp_ctx* ctx, GridTune& t, HashBuild<T> b, bool ksel);
template <typename T>
void init_search(SearchArgs<T>& a, const wtp_ctx* ctx, const Pt<T>* snap, const Pt<T>* query, int64_t n, int k, int include_self);
double ksel_rho_for(int kq);
double ksel_cap_count(int kq);
int cs2_tune(wtp_ctx* ctx, RelaxState& r, const Grid<float>& hg, double rho_eff);
void grid_taken(wtp_ctx* ctx); // a call is about to build, or has built, its hash on ctx->grid: what others left there is void

// ---- wtp_topology.hip: the Float64 candidate stage, shared with the session's fp64 sweep ------------------------
int f64_candidates(wtp_ctx* ctx, const double4* pts, int64_t n, int dim, int kc, GridTune& t, SearchArgs<float>& b, int& sp,
                   const double** org4_out, const std::function<int(float4*)>& relabel);

// ---- wtp_spacing.hip: the spacing laws' host side (wtp_relax_init, wtp_spacing_eval) -----------------------------
bool spacing_on_device(int kind);
int check_spacing_law(wtp_ctx* ctx, const wtp_spacing_desc* s);
int ensure_kd(wtp_ctx* ctx, const wtp_spacing_desc* s, int dim, int dtype); // the kd-tree over the law's boundary, cached per context

// ---- wtp_relax.hip -------------------------------------------------------------------------------------------------
int flush_pending(wtp_ctx* ctx); // materialise a pending fixed head (every entry point that reads P calls it first)

// ---- launch wrappers (implemented per translation unit) ----------------------------------------
// hash build (HashBuild above) into ctx->grid, ctx->cell_start and b.out
template <typename T> int build_hash(wtp_ctx* ctx, const HashBuild<T>& b);
// the first half of the build `next` ahead of time (ctx->prerank): its view's old snapshot ranked into the kept grid
template <typename T> int prerank_old_snapshot(wtp_ctx* ctx, const HashBuild<T>& next);
// occupancy of the cells of grid g (the one in ctx->cell_start): d_out3 = [sum cnt^2, sum cnt, max cnt]
template <typename T> int launch_occupancy(wtp_ctx* ctx, const Grid<T>* g, unsigned long long* d_out3);
template <typename T> int launch_sum(wtp_ctx* ctx, const T* d_v, int64_t n, double* d_out);
int launch_offsets_scan(wtp_ctx* ctx, const int32_t* d_cnt, int64_t n, int64_t* d_tmp, int64_t* d_off);
size_t offsets_scan_tmp_bytes(int64_t n);
// per-axis coordinate histograms over d_range = {lo xyz, hi xyz}: 3 x 1024 bins
template <typename T>
int launch_axis_hist(wtp_ctx* ctx, const Pt<T>* pts, int64_t n, int dim, const double* d_range, unsigned int* d_hist);

template <typename T>
int load_points(wtp_ctx* ctx, const T* d_xyz, Pt<T>* out, int64_t n, int dim);

// blocks of a grid-stride launch: ceil(n / threads), clamped to [1, cap]
inline int grid_for(int64_t n, int threads, int cap) {
    int64_t b = (n + threads - 1) / threads;
    if (b < 1) b = 1;
    return (int)(b > cap ? cap : b);
}
template <typename T> int launch_topology(wtp_ctx* ctx, SearchArgs<T>& a);
// fp32 sweep on 4 x 4 x 4 bricks (wtp_brick.hip), compact-support (cs) or explicit k-selection; hand-backs land in a.fb_list
int launch_brick_sweep(wtp_ctx* ctx, SearchArgs<float>& a, bool cs);
// fp64 compact-support brick sweep (wtp_brick64.hip); hand-backs land in a.fb_list
template <typename T> int launch_brick_cs(wtp_ctx* ctx, SearchArgs<T>& a);
// exact paths: wave-per-query (list = fb_list or all points), then the serial kernel on fb2_list
template <typename T> int launch_wave_topology(wtp_ctx* ctx, SearchArgs<T>& a, bool all);
template <typename T> int launch_wave_sweep(wtp_ctx* ctx, SearchArgs<T>& a, bool all);
template <typename T>
int launch_wave_radius_count(wtp_ctx* ctx, SearchArgs<T>& a, T r, int32_t* d_counts, const int32_t* list,
                             const int32_t* list_count);
template <typename T>
int launch_wave_radius_fill(wtp_ctx* ctx, SearchArgs<T>& a, T r, const int64_t* d_offsets, int32_t* d_idx,
                            const int32_t* list, const int32_t* list_count);
template <typename T> int launch_generic_topology(wtp_ctx* ctx, SearchArgs<T>& a, bool all);
template <typename T> int launch_query_knn(wtp_ctx* ctx, SearchArgs<T>& a, const T* d_xyz, int dim, Pt<T>* d_packed);
template <typename T> int launch_generic_sweep(wtp_ctx* ctx, SearchArgs<T>& a, bool all);
inline int total_partials() { return brick_partials() + kWavePartials + kGenericPartials; }
int launch_brick_radius(wtp_ctx* ctx, SearchArgs<float>& a);
// round-2 compact-support sweep (wtp_cs2.hip)
int launch_cs2(wtp_ctx* ctx, SearchArgs<float>& a);
int launch_cs2_followup(wtp_ctx* ctx, SearchArgs<float>& a);
int debug_kd_steps(unsigned long long out[2]); // -DWTP_DIAG builds: node visits / wave-walks of the spacing law's tree walk since the last call
int launch_cs_ball(wtp_ctx* ctx, SearchArgs<float>& a, int32_t* rest_list, int32_t* rest_count);
int launch_cs2_census(wtp_ctx* ctx, int BX, unsigned int* d_out513);
int launch_cs2_dead(wtp_ctx* ctx, SearchArgs<float>& a, uint8_t* d_dead, int dead_cap);
int cs2_max_bx();
// wtp_ksel.hip: k-selection on the x-slowest layout (fp32, 3-D, k + self <= ksel_kmax())
int launch_ksel_topology(wtp_ctx* ctx, SearchArgs<float>& a);
int launch_ksel_sweep(wtp_ctx* ctx, SearchArgs<float>& a);
int ksel_max_bx();
int ksel_kmax();
template <typename T>
int launch_radius_count(wtp_ctx* ctx, SearchArgs<T>& a, T r, int32_t* d_counts);
template <typename T>
int launch_radius_fill(wtp_ctx* ctx, SearchArgs<T>& a, T r, const int64_t* d_offsets,
                       int32_t* d_idx);
int launch_reduce_partials(wtp_ctx* ctx, const Partial* parts, int n_parts, int used_brick, int used_wave,
                           int used_generic, const int32_t* fb_count, const int32_t* uncovered,
                           const int32_t* escaped, wtp_step_stats* d_stats_slot);
// consumers of the rows (wtp_consumers.hip)
template <typename T>
int launch_pca_normals(wtp_ctx* ctx, const T* d_xyz, int64_t n, int dim, const int32_t* d_rows, int k, T* d_out);
template <typename T>
int launch_minplus_batch(wtp_ctx* ctx, const int32_t* d_rows, const T* d_dist, int64_t n, int k, double g, double tol,
                         T* d_h0, T* d_h1, int first, int sweeps, unsigned long long* d_state);
// the metrics' reductions over the distance rows (wtp_stats.hip): result and first bad spacing index land in d_tmp
size_t knn_stats_tmp_bytes(int64_t n);
template <typename T>
int launch_knn_stats(wtp_ctx* ctx, const T* d_dist, int64_t n, int k, const double* d_h, double h_const, int has_spacing,
                     double coord_radius, const int64_t* d_gid, T* d_nn_out, double* d_mean_out, void* d_tmp,
                     const KnnStats** d_result_out, const unsigned long long** d_bad_out);
// wtp_topology.hip: the reduction of device rows into a host struct, shared with the sharded call (wtp_block_topo.hip)
int knn_stats_spacing(const void* h, double h_const, double coord_radius, const char** why);
int knn_stats_rows(wtp_ctx* ctx, const void* d_dist, int64_t n, int k, int dtype, const double* d_h, double h_const,
                   int has_spacing, double coord_radius, const int64_t* d_gid, void* d_nn_out, double* d_mean_out,
                   KnnStats* out, int64_t* bad_out);
void knn_stats_merge(KnnStats& a, const KnnStats& b); // a <- a merged with b (host; the kernels' own rule)
KnnStats knn_stats_neutral();
// the graph part of orient_normals! / split_surface! (wtp_normal_graph.hip): prep, `rounds` rounds from round `first`
// (components in bufs[r & 1] before round r), and the flips / labels with the counts; d_ctl: normal_graph_ctl_bytes()
size_t normal_graph_ctl_bytes();
template <typename T>
int launch_normal_graph_prep(wtp_ctx* ctx, const T* d_xyz, const T* d_nrm, const int32_t* d_rows, int64_t n, int dim, int k,
                             int orient, double angle, uint32_t* d_cur, uint8_t* d_keep, unsigned long long* d_ctl);
template <typename T>
int launch_normal_graph_rounds(wtp_ctx* ctx, const T* d_nrm, const int32_t* d_rows, int64_t n, int dim, int k, int orient,
                               const uint8_t* d_keep, uint32_t* d_buf0, uint32_t* d_buf1, unsigned long long* d_best_w,
                               unsigned long long* d_best_e, int32_t* d_mst_out, int first, int rounds,
                               unsigned long long* d_ctl);
template <typename T>
int launch_normal_graph_apply(wtp_ctx* ctx, T* d_nrm, int64_t n, int dim, const uint32_t* d_cur, int32_t* d_label_out,
                              unsigned long long* d_ctl);
// wtp_sample.hip: a new or cleared mesh voids the resident sample
void sample_invalidate(wtp_ctx* ctx);
// The host-level seam between wtp_sample.hip, which decides a batch from the batch buffers, and wtp_sample_streams.hip,
// which fills them.  Of wtp_sample.hip: the batch buffers for B points; rows {x, y, z, r} into xyz and r (NULL: absent).
constexpr int kSmThreads = 256;
inline int sm_stride_grid(int64_t n) { return grid_for(n, kSmThreads, 8192); }
template <typename T> int ensure_batch(wtp_ctx* ctx, int64_t B);
template <typename T> int sample_unpack(wtp_ctx* ctx, const void* pts, int64_t n, T* d_xyz, T* d_r);
// the first two of every `stride` values of src into xy (n x 2): Pt rows (stride 4) or the batch's xyz (stride 3)
template <typename T> int sample_unpack_xy(wtp_ctx* ctx, const T* src, int stride, int64_t n, T* d_xy);
// Of wtp_sample_streams.hip: a batch of darts or candidates, the seeds, the front's own-h pass, the streams' read-outs.
template <typename T>
int enqueue_darts(wtp_ctx* ctx, const SampleDomain& dom, const wtp_spacing_desc* sp, double factor, uint64_t seed, int64_t first,
                  int64_t n, bool fill);
template <typename T>
int enqueue_candidates(wtp_ctx* ctx, uint64_t seed, const Pt<T>* parents, int64_t par0, int64_t first, int64_t B, int per);
template <typename T>
int fill_seeds(wtp_ctx* ctx, const wtp_spacing_desc* sp, double factor, const T* seeds, int64_t ns, int dim);
template <typename T> int front_own_h(wtp_ctx* ctx, const wtp_spacing_desc* sp, int64_t n, int64_t n_new);
template <typename T>
int sample_darts(wtp_ctx* ctx, const SampleDomain& dom, const wtp_spacing_desc* sp, double factor, uint64_t seed, int64_t first,
                 int64_t n, bool fill, T* xyz_out, int32_t* tri_out, uint8_t* inside_out, T* r_out);
template <typename T>
int front_candidates(wtp_ctx* ctx, const wtp_spacing_desc* sp, uint64_t seed, const T* parents, int64_t np, int64_t first_parent,
                     int per, T* xyz_out, uint8_t* inside_out, T* r_out);
// wtp_mesh_query's inside flag for n device points of the mesh's own type (wtp_mesh.hip): the domain test of wtp_mesh_fill
template <typename T> int launch_mesh_inside(wtp_ctx* ctx, const T* d_xyz, int64_t n, uint8_t* d_inside);
// classify_point's class (0 exterior, 1 boundary, 2 interior) of n device points of the mesh's own type (wtp_mesh.hip);
// point i takes the tolerance d_tol[i / per] and is skipped, its class left unwritten, where d_need[i / per] == 0
template <typename T>
int launch_mesh_point_class(wtp_ctx* ctx, const T* d_xyz, int64_t n, const T* d_tol, int per, const uint8_t* d_need,
                            uint8_t* d_cls);
// does some triangle's bounding box overlap the closed box d_lohi[6 i ..] = {lo, hi}?  Boxes with d_need[i] == 0 are skipped
template <typename T>
int launch_mesh_box_touch(wtp_ctx* ctx, const T* d_lohi, int64_t n, const uint8_t* d_need, uint8_t* d_touch);
// wtp_node_tree.hip: a new or cleared mesh drops the node tree
void node_tree_invalidate(wtp_ctx* ctx);
// wtp_loops_query's inside flag for n device rows of 3 columns (z ignored) of the index's own type (wtp_loops.hip): the
// domain test of wtp_loops_fill
template <typename T> int launch_loops_inside(wtp_ctx* ctx, const T* d_xyz, int64_t n, uint8_t* d_inside);
// the mesh's inside/outside class grid with cells of about `cell` (kept if one about as fine exists), and the number of
// cells such a grid has: one exact test each, which launch_mesh_inside then saves every point of a one-sided cell
int mesh_ensure_classes(wtp_ctx* ctx, double cell);
int64_t mesh_class_cells(const wtp_ctx* ctx, double cell);
// wall rule of the octree method (wtp_mesh.hip)
template <typename TP>
int launch_mesh_constrain(wtp_ctx* ctx, const Pt<TP>* old, Pt<TP>* cur, int64_t n, int64_t n_fixed, double offset,
                          const uint8_t* is_bnd, uint8_t* escaped, int32_t* tri_idx, int32_t* hint, int32_t* n_escaped);
template <typename T>
int launch_unpermute(wtp_ctx* ctx, const Pt<T>* pts, int64_t n, int64_t n_fixed, int dim, T* d_xyz_out);
template <typename T>
int launch_unpermute_point_data(wtp_ctx* ctx, const Pt<T>* pts, int64_t n, int64_t n_fixed,
                                const T* forces, const T* nn_dist, const int32_t* nn_id,
                                T* forces_o, T* nn_dist_o, int32_t* nn_id_o);
template <typename T>
int launch_set_points(wtp_ctx* ctx, Pt<T>* pts, int64_t n, const int32_t* d_ids, int64_t m, int dim, const T* d_v);
template <typename T>
int launch_set_point(wtp_ctx* ctx, Pt<T>* pts, int64_t n, int32_t id, int dim, const T* d_xyz3);
template <typename T>
int launch_gen_uniform(wtp_ctx* ctx, uint64_t seed, int64_t first, int64_t n, int dim, T* d_out);
// variable spacing laws on the device (wtp_spacing.hip)
template <typename T> size_t kd_bytes(int64_t m);
template <typename T> void kd_build_host(const T* xyz, int64_t m, int dim, void* out);
template <typename T>
int launch_spacing_eval(wtp_ctx* ctx, const T* d_xyz, int64_t n, int dim, const void* d_nodes, int64_t m, int kind,
                        double p0, double p1, double p2, T* d_out);
template <typename T>
int launch_spacing_session(wtp_ctx* ctx, const Pt<T>* pts, int64_t n, int64_t first_id, const void* d_nodes, int64_t m,
                           int kind, double p0, double p1, double p2, T* d_spacing_pp, int32_t* d_hint,
                           const int32_t* d_cell_start = nullptr, const void* d_grid = nullptr, void* d_cert = nullptr);
// per-block bounding boxes of a Float64 cloud into ctx->bbox_part (wtp_hash.hip)
int launch_bbox64(wtp_ctx* ctx, const double4* pts, int64_t n, int* nparts);
// wtp_sweep64.hip: the Float64 candidate stage of fp64 topology and of fp64 sweeps of the k-nearest laws
int launch_origin(wtp_ctx* ctx, const double4* pts, int64_t n, double* d_org4);
int launch_to_local_f32(wtp_ctx* ctx, const double4* in, int64_t n, const double* d_org4, float4* out);
int launch_relabel_slots(wtp_ctx* ctx, const double4* raw, float4* sorted32, double4* sorted64, int32_t* sslot, int64_t n);
int launch_refine_f64(wtp_ctx* ctx, const double4* raw, const int32_t* cand, const float* cdist, int64_t n, int kc, int k,
                      int include_self, const double* d_org4, int32_t* idx_out, double* dist_out, int32_t* fail_list,
                      int32_t* fail_count);
int launch_refine_f64_slots(wtp_ctx* ctx, const double4* sorted, const int32_t* cand, const float* cdist, int64_t n, int kc, int k,
                            int include_self, const double* d_org4, int32_t* idx_out, double* dist_out, int32_t* fail_list,
                            int32_t* fail_count);
int launch_refine_sweep_f64(wtp_ctx* ctx, SearchArgs<double>& a, const double4* s64, const int32_t* sslot, const int32_t* cand,
                            const float* cdist, const double* d_org4);
// isinside post-filter (wtp_inside.hip)
int isinside_chunks(wtp_ctx* ctx, int64_t n, int64_t m, int points_per_block);
int isinside_greens_ppb();
int isinside_winding_ppb();
size_t isinside_elem_bytes(int dtype);
template <typename T>
int launch_isinside_greens(wtp_ctx* ctx, const T* d_test, int64_t n, const T* d_p, const T* d_nrm, const T* d_area,
                           int64_t m, void* d_elems, int chunks, T* d_partial, T* d_g, uint8_t* d_inside);
template <typename T>
int launch_isinside_winding(wtp_ctx* ctx, const T* d_test, int64_t n, const T* d_poly, int64_t m, int chunks,
                            T* d_partial, int32_t* d_coincident, T* d_sum, uint8_t* d_inside);
// sharded sessions: boundary layers of the movable points / replacement of the fixed head
int layer_blocks(int64_t n);
template <typename T>
int launch_layers(wtp_ctx* ctx, const Pt<T>* pts, int64_t n, int64_t n_fixed, int axis, double lo_in, double hi_in,
                  double lo_out, double hi_out, Pt<T>* d_lo, Pt<T>* d_hi, int64_t cap, int2* d_blk, int32_t* d_totals,
                  bool slot_ordered, double reach);
template <typename T> int launch_append_fixed(wtp_ctx* ctx, const Pt<T>* d_src, int64_t n, Pt<T>* d_dst);
// block decomposition (wtp_block.hip) <-> session internals (wtp_relax.hip)
int relax_step_enqueue(wtp_ctx* ctx, int rebuild, wtp_step_stats* d_slot); // one sweep, statistics into a device slot, no synchronisation
int relax_swap_begin(wtp_ctx* ctx, int64_t n_move_new, void** d_buf_out);  // a free point buffer for a replaced movable set ...
int relax_swap_commit(wtp_ctx* ctx, int64_t n_move_new);                   // ... which becomes the session's P (no fixed head, tuning kept)
int relax_set_fixed_dev_impl(wtp_ctx* ctx, const void* d_fixed4, int64_t n_fixed_new, bool keep_alive);
// wtp_comm.hip: the transport of the block driver and the sharded topology (see Transport); `who` leads the error texts.
// A caller's transport, or a communicator of this rank and size (one rank needs neither)
int transport_ready(wtp_ctx* ctx, int rank, int nranks, const std::string& who);
// every rank's `nwords` 8-byte words (device or host memory) into the host array all[nranks * nwords], rank-major
int transport_allgather(wtp_ctx* ctx, int nranks, const void* mine, bool on_device, int64_t* all, int64_t nwords, const char* who);
// One grouped round, messages as wtp_comm_exchange_peers takes them; a host transport stages whole regions (send[r] /
// recv[r], r < n_regions) through the host.  meanwhile(ctx, arg), if given, enqueues work on the context's stream that
// runs while the rows travel.
int transport_exchange(wtp_ctx* ctx, int n_msgs, const int* peers, const void* const* d_send, const int64_t* n_send,
                       void* const* d_recv, const int64_t* n_recv, int n_regions, const RowRegion* send, const RowRegion* recv,
                       int (*meanwhile)(wtp_ctx*, void*), void* arg, const char* who);
template <typename T> int launch_radius_dense(wtp_ctx* ctx, SearchArgs<T>& a, T r, int32_t* d_counts); // wtp_radb.hip
template <typename T> int radius_dense_hcap();
int launch_cs_all_slots(wtp_ctx* ctx, int32_t* list, int32_t n, int32_t* count); // wtp_cs2.hip: list = 0 .. n-1, *count = n
int launch_cs_ball64(wtp_ctx* ctx, SearchArgs<double>& a, int32_t* rest_list, int32_t* rest_count); // wtp_ball64.hip
int relax_prerank(wtp_ctx* ctx, int64_t n_fixed_new); // first half of the next rebuild's hash, ahead of wtp_relax_set_fixed_dev (see wtp_relax.hip)
void block_destroy(wtp_ctx* ctx);                                          // frees ctx->block (wtp_destroy)
// sharded topology (wtp_block_topo.hip) <-> block driver (wtp_block.hip) and the single-context searches (wtp_topology.hip)
void block_topo_destroy(wtp_ctx* ctx);                                     // frees ctx->block_topo (wtp_destroy)
bool block_session_open(wtp_ctx* ctx);                                     // a wtp_block_open session is active
int launch_blk_scan(wtp_ctx* ctx, int32_t* span_counts, int64_t nspans, int ncol, int32_t* totals); // column scan of per-span counts
int topo_knn_local(wtp_ctx* ctx, const float* d_xyz, int64_t n, int k, int include_self, int32_t* d_idx, float* d_dist);
// radius rows of a device fp32 3-D cloud: counts -> d_off (n + 1, exclusive scan) -> rows into *d_idx (grown to fit); *nnz
int topo_radius_local(wtp_ctx* ctx, const float* d_xyz, int64_t n, double r, int32_t* d_counts, int64_t* d_off, DevBuf& d_idx,
                      int64_t* nnz);
template <typename T>
int launch_refix(wtp_ctx* ctx, const Pt<T>* in, int64_t n_old, int64_t n_fixed_old, int64_t n_fixed_new,
                 const Pt<T>* d_fixed_new, Pt<T>* out, int32_t* d_counter);

} // namespace wtp
