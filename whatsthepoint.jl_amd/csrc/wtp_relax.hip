// wtp_relax.hip — the relax session of include/wtp.h: the body of _relax!'s loop (src/repel.jl:243-334) as init, route
// choice, rebuild and step, and the calls that read or replace the session's points.  The calls that drive the steps
// (step, run, run_until, step + layers) are in wtp_relax_run.hip.
#include <cstdlib>
#include <cstring>

#include "wtp_internal.hpp"

using namespace wtp;

#define WTP_API extern "C"

static double host_max(const void* v, int64_t n, int dtype) {
    double m = 0;
    if (dtype == WTP_F64) {
        const double* p = (const double*)v;
        for (int64_t i = 0; i < n; ++i) m = p[i] > m ? p[i] : m;
    } else {
        const float* p = (const float*)v;
        for (int64_t i = 0; i < n; ++i) m = p[i] > m ? p[i] : m;
    }
    return m;
}

// upper bound of a law's values (sizes the compact-support grid; need not be attained)
static double spacing_law_max(const wtp_spacing_desc* s) {
    if (s->kind == WTP_SPACING_LOGLIKE) return s->p0;
    return s->p0 > s->p1 ? s->p0 : s->p1;
}

// ---- repel ------------------------------------------------------------------------------------------
static int pick_free(const RelaxState& r, int avoid_a, int avoid_b) {
    for (int i = 0; i < 3; ++i)
        if (i != avoid_a && i != avoid_b) return i;
    (void)r;
    return 0;
}

// Materialise a pending input view (wtp_relax_set_fixed_dev below): stale fixed points dropped, the
// appended ones moved to the head, ids renumbered.  Every entry point that reads P calls this first;
// the usual consumer, the next rebuild, never needs it.
int wtp::flush_pending(wtp_ctx* ctx) {
    RelaxState& r = ctx->relax;
    if (!r.pending.active) return WTP_OK;
    int rc;
    const int t = pick_free(r, r.bufP, -1);
    if ((rc = ensure(ctx, ctx->pts[t], pt_size(r.dtype) * (size_t)(r.n + r.shard_extra)))) return rc;
    if ((rc = ensure(ctx, ctx->scratch, 64))) return rc;
    const HashView v = r.pending;
    rc = by_dtype(r.dtype, [&](auto tt) {
        using T = decltype(tt);
        const Pt<T>* P = pts_of<T>(ctx, r.bufP);
        return launch_refix<T>(ctx, P, v.n_old, v.fixed_old, r.n_fixed, P + v.n_old, pts_of<T>(ctx, t), (int32_t*)ctx->scratch.p);
    });
    if (rc) return rc;
    r.bufP = t;
    r.pending.active = false;
    return WTP_OK;
}

static int relax_init_impl(wtp_ctx* ctx, const void* snap_xyz, bool on_device, int64_t n, int64_t n_fixed, int dim,
                           int dtype, const wtp_spacing_desc* spacing, const wtp_force_desc* force, int k,
                           double alpha_lo, double alpha_max) {
    int rc = check_cloud(ctx, snap_xyz, n, dim, dtype);
    if (rc) return rc;
    if (n_fixed < 0 || n_fixed > n) return fail(ctx, WTP_ERR_ARG, "n_fixed must be in [0, n]");
    if (!spacing || !force) return fail(ctx, WTP_ERR_ARG, "spacing/force descriptor is NULL");
    if (k < 1) return fail(ctx, WTP_ERR_ARG, "k must be >= 1");
    if (force->kind < 0 || force->kind > 3) return fail(ctx, WTP_ERR_ARG, "unknown force kind");
    if (!(force->beta > 0)) return fail(ctx, WTP_ERR_ARG, "force beta must be > 0");
    if (spacing->kind == WTP_SPACING_CONSTANT) {
        if (!(spacing->constant > 0)) return fail(ctx, WTP_ERR_ARG, "constant spacing must be > 0");
    } else if (spacing->kind == WTP_SPACING_PER_POINT) {
        if (!spacing->per_point) return fail(ctx, WTP_ERR_ARG, "per_point spacing array is NULL");
    } else if (spacing_on_device(spacing->kind)) {
        if ((rc = check_spacing_law(ctx, spacing))) return rc;
    } else {
        return fail(ctx, WTP_ERR_ARG, "unknown spacing kind");
    }
    if (!(alpha_lo >= 0) || !(alpha_max >= alpha_lo)) return fail(ctx, WTP_ERR_ARG, "need 0 <= alpha_lo <= alpha_max");
    const int kk = (int64_t)k < n ? k : (int)n; // kk = min(k, length(snap)), src/repel.jl:208
    if (kk > kGenericKMax) return fail(ctx, WTP_ERR_ARG, "k > 128 is not supported");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    RelaxState& r = ctx->relax;
    r = RelaxState{};
    grid_taken(ctx); // the session's rebuilds hash into the context's grid
    for (int i = 0; i < 2; ++i)
        if ((rc = ensure(ctx, ctx->pts[i], pt_size(dtype) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->raw_in, ts * (size_t)n * dim))) return rc;
    if ((rc = ensure(ctx, ctx->forces, ts * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->nn_dist, ts * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->nn_id, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_count, sizeof(StepCounters)))) return rc;
    ctx->counters_clean = false; // (this call counts in the block; the next sweep clears it itself)
    if ((rc = ensure(ctx, ctx->fb2_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb2_count, 64))) return rc;
    const int n_partials = total_partials();
    if ((rc = ensure(ctx, ctx->partials, sizeof(Partial) * (size_t)n_partials))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->raw_in.p, snap_xyz, ts * (size_t)n * dim,
                                on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return load_points<T>(ctx, (const T*)ctx->raw_in.p, pts_of<T>(ctx, 0), n, dim);
    });
    if (rc) return rc;
    if (spacing->kind == WTP_SPACING_PER_POINT) {
        if ((rc = ensure(ctx, ctx->spacing_pp, ts * (size_t)n))) return rc;
        WTP_HIP(ctx, hipMemcpyAsync(ctx->spacing_pp.p, spacing->per_point, ts * (size_t)n, hipMemcpyHostToDevice,
                                    ctx->stream));
    }
    if (spacing_on_device(spacing->kind)) {
        // spacings = spacing.(snap) (src/repel.jl:209): every snapshot point once, the wall included
        if ((rc = ensure_kd(ctx, spacing, dim, dtype))) return rc;
        if ((rc = ensure(ctx, ctx->spacing_pp, ts * (size_t)n))) return rc;
        if ((rc = ensure(ctx, ctx->sp_hint, sizeof(int32_t) * (size_t)n))) return rc;
        WTP_HIP(ctx, hipMemsetAsync(ctx->sp_hint.p, 0xFF, sizeof(int32_t) * (size_t)n, ctx->stream)); // -1: no hint
        if ((rc = ensure(ctx, ctx->sp_cert, 4 * ts * (size_t)n))) return rc;
        WTP_HIP(ctx, hipMemsetAsync(ctx->sp_cert.p, 0xFF, 4 * ts * (size_t)n, ctx->stream)); // no certificate yet
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return launch_spacing_session<T>(ctx, pts_of<T>(ctx, 0), n, 0, ctx->kd.nodes.p, ctx->kd.m, spacing->kind,
                                             spacing->p0, spacing->p1, spacing->p2, (T*)ctx->spacing_pp.p,
                                             (int32_t*)ctx->sp_hint.p, nullptr, nullptr, ctx->sp_cert.p);
        });
        if (rc) return rc;
    }
    if ((rc = sync(ctx))) return rc;
    r.active = true;
    r.n = n;
    r.n_fixed = n_fixed;
    r.dim = dim;
    r.dtype = dtype;
    r.k = kk;
    r.k_req = k;
    r.spacing_kind = spacing->kind;
    r.spacing_const = spacing->constant;
    r.spacing_max = spacing->constant;
    if (spacing->kind == WTP_SPACING_PER_POINT) r.spacing_max = host_max(spacing->per_point, n, dtype);
    if (spacing_on_device(spacing->kind)) {
        r.spacing_max = spacing_law_max(spacing);
        r.sp_p0 = spacing->p0;
        r.sp_p1 = spacing->p1;
        r.sp_p2 = spacing->p2;
    }
    r.alpha_lo = alpha_lo;
    r.alpha_max = alpha_max;
    r.force.kind = force->kind;
    r.force.beta = force->beta;
    r.force.u0 = force->u0;
    r.force.gamma = force->gamma;
    r.bufP = 0;
    r.bufS = -1;
    r.bufOld = -1;
    return WTP_OK;
}

WTP_API int wtp_relax_init(wtp_ctx* ctx, const void* snap_xyz, int64_t n, int64_t n_fixed, int dim, int dtype,
                           const wtp_spacing_desc* spacing, const wtp_force_desc* force, int k, double alpha_lo,
                           double alpha_max) {
    return relax_init_impl(ctx, snap_xyz, false, n, n_fixed, dim, dtype, spacing, force, k, alpha_lo, alpha_max);
}

WTP_API int wtp_relax_init_dev(wtp_ctx* ctx, const void* d_snap_xyz, int64_t n, int64_t n_fixed, int dim, int dtype,
                               const wtp_spacing_desc* spacing, const wtp_force_desc* force, int k,
                               double alpha_lo, double alpha_max) {
    return relax_init_impl(ctx, d_snap_xyz, true, n, n_fixed, dim, dtype, spacing, force, k, alpha_lo, alpha_max);
}

// The session's grid, cell table and box trade places with the float copy's (relax_f64_ksel_sweep): what the float copy
// builds and measures — a quantile box among it, in its own coordinates — stays in its own buffers.
static void swap_float_copy_grid(wtp_ctx* ctx) {
    std::swap(ctx->grid, ctx->f64k.grid_b);
    std::swap(ctx->cell_start, ctx->f64k.cell_start_b);
    std::swap(ctx->box_dev, ctx->f64k.box_b);
}

// Float64 sweep of a k-nearest law on a fresh snapshot (wtp_sweep64.hip): candidates from the fp32 k-selection kernels on a
// float copy of the snapshot with its own grid — the session's grid, cell table and box are parked meanwhile and come back
// untouched for the exact path —, exact re-ranking + force sum + step per query; what is not certified is left in a.fb_list.
// *sp: the hash span it opens is closed and the search span left open.
static int relax_f64_ksel_sweep(wtp_ctx* ctx, SearchArgs<double>& a, int* sp) {
    RelaxState& r = ctx->relax;
    const int64_t n = r.n;
    const int kc = 24;
    int rc;
    if ((rc = ensure(ctx, ctx->f64k.s64, sizeof(double4) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->f64k.slot, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->f64k.lists, sizeof(int32_t) * 2 * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->f64k.cnt, sizeof(StepCounters)))) return rc;
    StepCounters* counters = (StepCounters*)ctx->f64k.cnt.p; // the float copy's own block
    const double4* snap = (const double4*)a.snap; // the sorted snapshot (fresh: the queries are its points)
    SearchArgs<float> b{};
    b.fb_list = (int32_t*)ctx->f64k.lists.p;
    b.fb_count = &counters->brick_handbacks;
    b.fb2_list = (int32_t*)ctx->f64k.lists.p + n;
    b.fb2_count = &counters->wave_handbacks;
    b.stop = ctx->stop_dev;
    b.diag = a.diag;
    *sp = span_begin(ctx, 0);
    WTP_HIP(ctx, hipMemsetAsync(counters, 0, sizeof(StepCounters), ctx->stream));
    b.counters_cleared = 1;
    swap_float_copy_grid(ctx);
    const double* org4 = nullptr;
    rc = f64_candidates(ctx, snap, n, 3, kc, r.f64k_tune, b, *sp, &org4, [&](float4* sorted32) {
        return launch_relabel_slots(ctx, snap, sorted32, (double4*)ctx->f64k.s64.p, (int32_t*)ctx->f64k.slot.p, n);
    });
    // the session's structures again (the float copy's stay where they are until the next sweep overwrites them)
    swap_float_copy_grid(ctx);
    if (rc) return rc;
    return launch_refine_sweep_f64(ctx, a, (const double4*)ctx->f64k.s64.p, (const int32_t*)ctx->f64k.slot.p,
                                   (const int32_t*)ctx->cand_idx.p, (const float*)ctx->cand_dist.p, org4);
}

// Will the next rebuild keep its grid (no bounding-box pass) for a head of n_fixed_next points?  head_swapped: it reads a
// replaced fixed head (HashView).  relax_rebuild decides by it, relax_prerank guesses by it ahead of the ghost rows.
static bool grid_reusable(const RelaxState& r, int64_t n_fixed_next, bool head_swapped) {
    const bool head_ok = !head_swapped || (r.shard_grid_reuse && r.grid_fixed > 0 &&
                                           std::llabs((long long)(n_fixed_next - r.grid_fixed)) * 10 <= (long long)r.grid_fixed + 640);
    return r.grid_age < kGridReuseMax && !r.moved_by_hand && head_ok && !r.tune.clipped;
}

// The brick geometry of the round-2 sweep (and which queries its bricks hand to the exact path, whose sums round
// differently) was measured on the cloud of the first rebuild: a head that changes the cloud by more than 5 % has it
// measured again, so that a resident session keeps equalling a fresh one bit for bit.
static bool head_remeasures(const RelaxState& r, int64_t n_fixed_new) {
    const int64_t n_new = r.n - r.n_fixed + n_fixed_new;
    return r.cs2_bx > 0 && std::llabs((long long)(n_fixed_new - r.tuned_fixed)) * 20 > (long long)n_new;
}

// The route of a session's sweeps, from the session and the switches; relax_step_t decides at every rebuild (a swapped head
// changes n and k), and once more with cs_disabled set when the first rebuild finds the support cells over-full.
template <typename T> static SweepRoute sweep_route(const wtp_ctx* ctx, const RelaxState& r) {
    if (ctx->force_generic) return SweepRoute::Exact;
    // ClippedSpacingForce (the reference default): cells only have to cover the law's support u0*s and the nearest-neighbour
    // radius, so they can be smaller than the k-NN cells — unless WTP_FULL_SELECT=1 asks for the explicit k-selection on
    // every query (both give the same output)
    const bool clipped = r.force.kind == WTP_FORCE_CLIPPED_SPACING;
    if (clipped && r.k >= 2 && r.k < 32 && !ctx->full_select && !r.cs_disabled) {
        if (sizeof(T) == 8) return ctx->ball64 ? SweepRoute::Cs64 : SweepRoute::Cs64Wave;
        return r.dim == 3 ? SweepRoute::Cs2 : SweepRoute::Cs;
    }
    if (sizeof(T) == 8) {
        // Float64, a k-nearest law, 3-D: candidates from the fp32 k-selection kernels.  (ClippedSpacingForce keeps its
        // compact-support kernels: measured through this route on the graded 10 M-point cloud, 39 ms per iteration against
        // 20 — the k-selection grid hands a quarter of a graded cloud's queries back)
        const bool f64k = r.dim == 3 && ctx->ksel && ctx->f64_ksel && !clipped && r.k >= 2 && r.k <= 22 && r.n >= 4096;
        return f64k ? SweepRoute::F64Ksel : SweepRoute::Exact;
    }
    if (r.k >= 32) return SweepRoute::Exact; // beyond the brick kernels' lists
    // every other law, WTP_FULL_SELECT=1 and over-full support cells: the explicit k-selection — on the x-slowest layout of
    // wtp_ksel.hip where that applies
    const bool ksel = r.dim == 3 && ctx->ksel && r.k >= 2 && r.k <= ksel_kmax() && r.n >= 4096;
    return ksel ? SweepRoute::Ksel : SweepRoute::Select;
}

static bool route_cs(SweepRoute s) {
    return s == SweepRoute::Cs || s == SweepRoute::Cs2 || s == SweepRoute::Cs64 || s == SweepRoute::Cs64Wave;
}
// the ball kernel takes the route's supports wider than a cell and every query of a stale snapshot
static bool route_ball(SweepRoute s) { return s == SweepRoute::Cs || s == SweepRoute::Cs2 || s == SweepRoute::Cs64; }

// The session's hash builds for its route: occupancy (points per cell, 0: the k-NN default) and smallest cell edge
struct RouteGrid { double rho, min_cell; };
static RouteGrid route_grid(const wtp_ctx* ctx, const RelaxState& r) {
    if (r.route == SweepRoute::Ksel) return {r.tune.valid && r.tune.bx > 0 ? r.tune.rho : ksel_rho_for(r.k), 0.0};
    if (!route_cs(r.route)) return {0.0, 0.0};
    // round-2 sweep (wtp_cs2.hip): the nearest neighbour comes from the support or from a per-wave follow-up, so the cells
    // only cover the support: rho ~ 1.  The other compact-support kernels: rho ~ 3.5 instead of ~8, 2.3x fewer candidates.
    const bool cs2 = r.route == SweepRoute::Cs2;
    // The cells cover the law's support u0*s.  With a variable spacing the cell edge follows the spacing a typical point
    // asks for (the mean over points, which the dense regions dominate), not the largest one: the few points whose support
    // is wider than that are handed to the exact path, instead of everybody's cells being 64x over-full.
    // (constant spacing: c - margin = c (1 - 1/256) must reach u0 s, 1.01 does; variable: 10 % headroom over the mean)
    const double cell_f = (cs2 && r.spacing_kind == WTP_SPACING_CONSTANT) ? 1.01 : 1.1;
    return {cs2 ? kRhoCs2 : 3.5 * (ctx->rho / 9.0),
            cell_f * r.force.u0 * (r.spacing_typ < r.spacing_max ? r.spacing_typ : r.spacing_max)};
}

// What this step's sweep runs: the session's route on a fresh snapshot; on a stale one the ball kernel for every query where
// the route has one, else the exact path.
static SweepRoute step_route(const RelaxState& r, bool fresh) {
    if (!fresh) return route_ball(r.route) ? SweepRoute::Ball : SweepRoute::Exact;
    // a grid measured for another route (a head swap took n past 4096, or k below 32) left this one without its brick
    // geometry: the explicit k-selection on 4 x 4 x 4 bricks, in Float64 the exact path
    const bool measured = r.route == SweepRoute::Ksel ? r.tune.bx > 0 : !route_cs(r.route) || r.brick_hcap > 0;
    if (measured) return r.route;
    return r.route == SweepRoute::Cs64 || r.route == SweepRoute::Cs64Wave ? SweepRoute::Exact : SweepRoute::Select;
}

static int ball_pass(wtp_ctx* ctx, SearchArgs<float>& a) { return launch_cs_ball(ctx, a, a.ball_list, a.ball_count); }
static int ball_pass(wtp_ctx* ctx, SearchArgs<double>& a) { return launch_cs_ball64(ctx, a, a.ball_list, a.ball_count); }

// One relax sweep along the step's route (ball: with the ball kernel for supports wider than a cell): span 1 around the
// route's own kernels, span 2 around the exact path for what they hand back.  The caller cleared the counter block; partial
// slots need no clearing: the reduction reads only the slots this step's launches write (a.used_*).
template <typename T> static int launch_sweep(wtp_ctx* ctx, SearchArgs<T>& a, SweepRoute route, bool ball) {
    constexpr bool f32 = sizeof(T) == 4;
    ctx->timers.n_sweep_launches += 1;
    int rc = WTP_OK, sp = -1;
    switch (route) {
    case SweepRoute::Exact:
    case SweepRoute::Ball:
        sp = span_begin(ctx, 1);
        if (route == SweepRoute::Ball) {
            // A stale snapshot (rebuild_every > 1, src/repel.jl:245) and the default law: the query has moved away from its
            // snapshot entry, so the brick kernels (queries = the staged points) do not apply, but the ball kernel's argument
            // does — the support ball around the point where it is NOW, searched in the block that provably holds it, at
            // most k points in it — with eight lanes per query instead of the wave kernel's 64 (10.5 -> see DESIGN.md).
            rc = launch_cs_all_slots(ctx, a.fb_list, a.n, a.fb_count);
            if (!rc) rc = ball_pass(ctx, a);
        }
        if (!rc) rc = launch_generic_sweep<T>(ctx, a, route == SweepRoute::Exact);
        span_end(ctx, sp);
        return rc;
    case SweepRoute::F64Ksel:
        if constexpr (!f32) rc = relax_f64_ksel_sweep(ctx, a, &sp);
        break;
    case SweepRoute::Ksel:
        sp = span_begin(ctx, 1);
        if constexpr (f32) rc = launch_ksel_sweep(ctx, a);
        a.fb_r0 = 3; // its hand-backs failed at the 5^3 cells around the query
        break;
    case SweepRoute::Select:
    case SweepRoute::Cs:
    case SweepRoute::Cs2:
        sp = span_begin(ctx, 1);
        if constexpr (f32) {
            if (route == SweepRoute::Cs2 && ball) {
                // variable spacing: bricks that would hand every point back are found first and passed over (wtp_cs2.hip)
                const int dead_cap = (int)(ctx->cell_start.cap / sizeof(int32_t) / 4 + 4096);
                rc = ensure(ctx, ctx->brick_dead, (size_t)dead_cap);
                if (!rc) rc = launch_cs2_dead(ctx, a, (uint8_t*)ctx->brick_dead.p, dead_cap);
                a.brick_dead = (const uint8_t*)ctx->brick_dead.p;
                a.brick_dead_cap = dead_cap;
            }
            if (!rc) rc = route == SweepRoute::Cs2 ? launch_cs2(ctx, a) : launch_brick_sweep(ctx, a, route == SweepRoute::Cs);
        }
        break;
    case SweepRoute::Cs64:
    case SweepRoute::Cs64Wave:
        sp = span_begin(ctx, 1);
        if constexpr (!f32) {
            rc = launch_brick_cs<double>(ctx, a);
            if (!rc && ball) rc = ball_pass(ctx, a); // supports wider than a cell (wtp_ball64.hip), before the exact path
        }
        break;
    }
    span_end(ctx, sp);
    if (rc) return rc;
    sp = span_begin(ctx, 2);
    if constexpr (f32) {
        if (route == SweepRoute::Cs2) rc = launch_cs2_followup(ctx, a); // nearest neighbour of the queries the bricks left open
        if (!rc && ball) rc = ball_pass(ctx, a); // hand-backs whose support outgrew their cell, ball by ball (wtp_cs2.hip)
    }
    if (!rc) rc = launch_generic_sweep<T>(ctx, a, false);
    span_end(ctx, sp);
    return rc;
}

// The session's hash build of the snapshot `in` (n points, k neighbours; read through `view` when a replaced fixed head waits
// behind it) into `out`, on its route's grid with the measured cell scale and clipped box.  The Float64 candidate route orders
// every sum by (d2, index) explicitly, on the exact path behind it too: no canonical-order pass (0.37 ms per 10 M Float64
// points) — except in the builds that measure the grid.
template <typename T>
static HashBuild<T> relax_request(const wtp_ctx* ctx, const RelaxState& r, const Pt<T>* in, Pt<T>* out, int64_t n, int k,
                                  const HashView& view, bool keep_grid) {
    const RouteGrid g = route_grid(ctx, r);
    HashBuild<T> b(in, out, n, r.dim, k);
    b.rho_direct = g.rho;
    b.min_cell = g.min_cell;
    b.cell_scale = r.tune.scale;
    b.view = view;
    b.keep_grid = keep_grid;
    b.canonical = !r.tune.valid || r.route != SweepRoute::F64Ksel;
    b.box = r.tune.clipped ? (const double*)ctx->box_dev.p : nullptr;
    return b;
}

// Snapshot tail <- p, tree rebuilt (src/repel.jl:245-253): the route for the snapshot as it stands, P (through the replaced
// fixed head waiting in it, wtp_relax_set_fixed_dev) hashed into a free buffer — on the session's first rebuild with a
// measured grid —, and the session's bookkeeping of its grid.
template <typename T> static int relax_rebuild(wtp_ctx* ctx) {
    RelaxState& r = ctx->relax;
    int rc;
    const int t = pick_free(r, r.bufP, -1);
    if ((rc = ensure(ctx, ctx->pts[t], sizeof(Pt<T>) * (size_t)(r.n + r.shard_extra)))) return rc;
    int sp = span_begin(ctx, 0);
    grid_taken(ctx); // (have_tree comes back below, once the build has gone through)
    r.route = sweep_route<T>(ctx, r);
    if (r.spacing_typ <= 0) { // once per session: the spacing a typical point asks for
        r.spacing_typ = r.spacing_const;
        if (r.spacing_kind != WTP_SPACING_CONSTANT) {
            if ((rc = ensure(ctx, ctx->occ, 64))) return rc;
            if ((rc = ensure_pinned(ctx, 1024))) return rc;
            if ((rc = launch_sum<T>(ctx, (const T*)ctx->spacing_pp.p, r.n, (double*)ctx->occ.p))) return rc;
            WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, ctx->occ.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            if ((rc = sync(ctx))) return rc;
            r.spacing_typ = ((const double*)ctx->host_pinned)[0] / (double)r.n; // the mean (mean + sigma measured only slower)
            if (!(r.spacing_typ > 0)) r.spacing_typ = r.spacing_max;
        }
    }
    const Pt<T>* in = pts_of<T>(ctx, r.bufP);
    Pt<T>* out = pts_of<T>(ctx, t);
    if (!r.tune.valid) { // once per session: measured cell edge, LDS point area sized from the real grid
        double rho_eff = 0;
        Grid<T> hg;
        HashBuild<T> b = relax_request<T>(ctx, r, in, out, r.n, r.k, r.pending, false);
        if ((rc = build_hash_tuned<T>(ctx, r.tune, b, &hg, &rho_eff))) return rc;
        // A spacing far coarser than the cloud (the reference's own tests repel 46 786 face centres 0.22 apart
        // with a spacing of 3): cells that cover the law's support then hold hundreds of points, every support
        // ball holds more than k of them and each query would go to the exact path one by one.  Such a session
        // takes the k-selection sweep on cells sized for the k-th neighbour instead (same results).  Only when
        // the crowded points are themselves queries: a dense FIXED wall around a few movable points is served
        // well by the support cells (their balls hold few points), and badly by small cells (the movable
        // points' k-th neighbour is many cells away).
        if (route_cs(r.route) && rho_eff > (r.route == SweepRoute::Cs2 ? 5.0 : 4.0 * b.rho_direct) && 2 * r.n_fixed < r.n) {
            r.cs_disabled = true;
            r.route = sweep_route<T>(ctx, r);
            b = relax_request<T>(ctx, r, in, out, r.n, r.k, r.pending, false);
            if ((rc = build_hash_tuned<T>(ctx, r.tune, b, &hg, &rho_eff))) return rc;
        }
        r.cs2_bx = 0;
        if (r.route == SweepRoute::Cs2) {
            Grid<float> hgf;
            memcpy(&hgf, &hg, sizeof(hgf)); // T == float here
            if ((rc = cs2_tune(ctx, r, hgf, rho_eff))) return rc;
        } else if (route_cs(r.route)) {
            int hc = (int)(HCELLS * rho_eff * 1.15) + 128;
            hc = (hc + 63) / 64 * 64;
            r.brick_hcap = hc < 640 ? 640 : (hc > 2560 ? 2560 : hc);
        }
        if (r.route == SweepRoute::Ksel && (rc = ksel_tune<T>(ctx, r.tune, b, hg, rho_eff))) return rc;
        r.tune.valid = true;
        r.tuned_fixed = r.n_fixed;
        r.grid_fixed = r.n_fixed;
        r.grid_age = 0;
    } else {
        // The bounding box moves by at most a spacing per sweep: it is recomputed every few rebuilds only
        // (and always after a point was placed by hand, a fixed head was swapped, or with a clipped box).
        // A block session swaps its ghost head every iteration; the layer keeps its place and, nearly, its size, so the
        // box of the last full pass still fits (what sticks out is clamped into edge cells: exact, as for a moved point).
        const bool reuse = grid_reusable(r, r.n_fixed, r.pending.active);
        r.grid_age = reuse ? r.grid_age + 1 : 0;
        if (!reuse) r.grid_fixed = r.n_fixed;
        rc = build_hash<T>(ctx, relax_request<T>(ctx, r, in, out, r.n, r.k, r.pending, reuse));
    }
    span_end(ctx, sp);
    if (rc) return rc;
    r.pending.active = false;
    r.bufS = t;
    r.bufP = t;
    r.have_tree = true;
    r.sweeps_since_rebuild = 0;
    r.moved_by_hand = false;
    return WTP_OK;
}

template <typename T> static int relax_step_t(wtp_ctx* ctx, int rebuild, wtp_step_stats* d_slot) {
    RelaxState& r = ctx->relax;
    int rc;
    if (!r.have_tree || r.pending.active) rebuild = 1; // the reference builds its first tree in the setup (src/repel.jl:218)
    if (rebuild && (rc = relax_rebuild<T>(ctx))) return rc;
    if (spacing_on_device(r.spacing_kind)) {
        // s = spacing(x_i) at the point's current position (src/repel.jl:251 on rebuilds, :260 in every
        // sweep): the movable tail is re-evaluated before each sweep, the wall keeps its setup values
        int sps = span_begin(ctx, 2);
        // (the slot order of P is the sorted order of the last rebuild: the grid groups the points of a wave compactly)
        rc = launch_spacing_session<T>(ctx, (const Pt<T>*)ctx->pts[r.bufP].p, r.n, r.n_fixed, ctx->kd.nodes.p, ctx->kd.m,
                                       r.spacing_kind, r.sp_p0, r.sp_p1, r.sp_p2, (T*)ctx->spacing_pp.p,
                                       (int32_t*)ctx->sp_hint.p - r.aux_off, r.have_tree ? (const int32_t*)ctx->cell_start.p : nullptr,
                                       ctx->grid.p, (Pt<T>*)ctx->sp_cert.p - r.aux_off);
        span_end(ctx, sps);
        if (rc) return rc;
    }
    const bool fresh = (r.bufS == r.bufP);
    const int o = pick_free(r, r.bufS, r.bufP);
    if ((rc = ensure(ctx, ctx->pts[o], sizeof(Pt<T>) * (size_t)(r.n + r.shard_extra)))) return rc;
    SearchArgs<T> a{};
    init_search(a, ctx, (const Pt<T>*)ctx->pts[r.bufS].p, (const Pt<T>*)ctx->pts[r.bufP].p, r.n, r.k, 1);
    a.out = (Pt<T>*)ctx->pts[o].p;
    a.forces = (T*)ctx->forces.p;
    a.nn_dist = (T*)ctx->nn_dist.p;
    a.nn_id = (int32_t*)ctx->nn_id.p;
    a.spacing_pp = r.spacing_kind != WTP_SPACING_CONSTANT ? (const T*)ctx->spacing_pp.p : nullptr;
    a.spacing_const = (T)r.spacing_const;
    a.alpha_lo = (T)r.alpha_lo;
    a.alpha_max = (T)r.alpha_max;
    a.beta = (T)r.force.beta;
    a.u0 = (T)r.force.u0;
    a.gamma = (T)r.force.gamma;
    a.force_kind = r.force.kind;
    a.n_fixed = (int32_t)r.n_fixed;
    a.partials = (Partial*)ctx->partials.p;
    a.n_partials = total_partials();
    StepCounters* counters = step_counters(ctx); // one block, cleared once per sweep
    a.fb_list = (int32_t*)ctx->fb_list.p;
    a.fb_count = &counters->brick_handbacks;
    a.fb2_list = (int32_t*)ctx->fb2_list.p;
    a.fb2_count = &counters->wave_handbacks;
    a.stop = ctx->stop_dev;
    a.nn_count = &counters->nn_count;
    const SweepRoute route = step_route(r, fresh);
    // the session's route keeps the ball kernel's list: supports wider than a cell, and every query of a stale snapshot
    const bool ball = route_ball(r.route) && (!fresh || r.spacing_kind != WTP_SPACING_CONSTANT);
    if (ball || route == SweepRoute::Cs2) {
        if ((rc = ensure(ctx, ctx->nn_list, sizeof(int32_t) * (size_t)r.n))) return rc;
        if (sizeof(T) == 4) a.nn_list = (int32_t*)ctx->nn_list.p; // wtp_cs2.hip: the follow-up kernel's list
        if (ball) { // the follow-up kernel has consumed the list by the time the ball kernel refills it
            a.ball_list = (int32_t*)ctx->nn_list.p;
            a.ball_count = &counters->ball_count;
        }
    }
    if ((rc = ensure(ctx, ctx->diag, 128))) return rc;
    a.diag = (unsigned long long*)ctx->diag.p;
    // the grid the session's route was built for (the exact path's kernels receive it too), and the first filter radius
    a.brick_hcap = route_cs(r.route) ? r.brick_hcap : (r.route == SweepRoute::Ksel ? r.tune.hcap : 0);
    a.cs2_bx = route_cs(r.route) ? r.cs2_bx : 0;
    a.cs2_chunked = (r.spacing_kind != WTP_SPACING_CONSTANT || r.cs2_rho > 1.6) ? 1 : 0;
    a.ksel_bx = r.route == SweepRoute::Ksel ? r.tune.bx : 0;
    if (r.route == SweepRoute::Ksel) a.cap_count = (float)ksel_cap_count(r.k);
    if (route == SweepRoute::Select || route == SweepRoute::Cs || route == SweepRoute::Cs2) {
        a.gamma_cap = (T)kGammaCapSweep;
        a.cap_count = (float)(4.18879 * kGammaCapSweep * kGammaCapSweep * kGammaCapSweep * ctx->rho * (a.k + 1) / 22.0);
    }
    if (route == SweepRoute::Cs64 || route == SweepRoute::Cs64Wave) a.gamma_cap = (T)kGammaCap;
    a.tnn_frac = (T)kTnnFrac;
    a.cover_axis = r.cover_axis;
    a.cover_lo = (T)r.cover_lo;
    a.cover_hi = (T)r.cover_hi;
    for (int ax = 0; ax < 3; ++ax) {
        a.cover_lo3[ax] = (T)r.cover_lo3[ax];
        a.cover_hi3[ax] = (T)r.cover_hi3[ax];
    }
    a.uncovered = &counters->uncovered;
    if (!ctx->counters_clean) WTP_HIP(ctx, hipMemsetAsync(counters, 0, sizeof(StepCounters), ctx->stream));
    ctx->counters_clean = false; // (set again by the step's final reduction, which zeroes the block after reading it)
    a.used_brick = a.used_wave = a.used_generic = 0;
    if ((rc = launch_sweep<T>(ctx, a, route, ball && route_ball(route)))) return rc;
    int sp = span_begin(ctx, 2);
    if (r.wall_active) { // p[id] = constrain(id, x_i, x_i + disp) (src/repel.jl:290): the octree wall rule
        char* wf = (char*)ctx->mesh.wall_flags.p;
        rc = launch_mesh_constrain<T>(ctx, a.query, a.out, r.n, r.n_fixed, r.wall_offset, (const uint8_t*)wf,
                                      (uint8_t*)wf + r.wall_nm, (int32_t*)ctx->mesh.wall_tri.p, (int32_t*)ctx->mesh.wall_hint.p,
                                      &counters->escaped);
        if (rc) return rc;
    }
    rc = launch_reduce_partials(ctx, a.partials, a.n_partials, a.used_brick, a.used_wave, a.used_generic, a.fb_count,
                                a.uncovered, r.wall_active ? &counters->escaped : nullptr, d_slot);
    span_end(ctx, sp);
    if (rc) return rc;
    r.bufOld = r.bufP; // p_old (src/repel.jl:244)
    r.bufP = o;
    r.can_revert = true;
    r.have_point_data = true;
    r.sweeps_since_rebuild += 1;
    return WTP_OK;
}

static int relax_step_any(wtp_ctx* ctx, int rebuild, wtp_step_stats* d_slot) {
    return by_dtype(ctx->relax.dtype, [&](auto t) { return relax_step_t<decltype(t)>(ctx, rebuild, d_slot); });
}
int wtp::relax_step_enqueue(wtp_ctx* ctx, int rebuild, wtp_step_stats* d_slot) { return relax_step_any(ctx, rebuild, d_slot); }

// The block driver knows, before the ghost rows of an iteration have arrived, how many there will be.  When the rebuild that
// follows is going to keep its grid (grid_reusable, as in relax_rebuild), the snapshot's own entries are ranked into the
// cells right away, on the context's stream, while the rows travel on another; build_hash then ranks the appended head
// only.  The guess is the request relax_rebuild will form once wtp_relax_set_fixed_dev has appended the head (the same
// view, n and k); a wrong guess costs one wasted pass, never a wrong result (build_hash checks what it finds).
int wtp::relax_prerank(wtp_ctx* ctx, int64_t n_fixed_new) {
    RelaxState& r = ctx->relax;
    ctx->prerank.valid = false;
    if (!r.active || !r.tune.valid || !r.have_tree || r.pending.active) return WTP_OK;
    if (!grid_reusable(r, n_fixed_new, true) || head_remeasures(r, n_fixed_new)) return WTP_OK;
    const int64_t n_new = r.n - r.n_fixed + n_fixed_new;
    if (ctx->pts[r.bufP].cap < pt_size(r.dtype) * (size_t)(r.n + n_fixed_new)) return WTP_OK; // (the head would be rewritten, not appended)
    const int k = (int64_t)r.k_req < n_new ? r.k_req : (int)n_new;
    HashView view;
    view.active = true;
    view.n_in = r.n + n_fixed_new;
    view.n_old = r.n;
    view.fixed_old = (int32_t)r.n_fixed;
    view.id_shift = (int32_t)(n_fixed_new - r.n_fixed);
    return by_dtype(r.dtype, [&](auto t) {
        using T = decltype(t);
        return prerank_old_snapshot<T>(ctx, relax_request<T>(ctx, r, pts_of<T>(ctx, r.bufP), nullptr, n_new, k, view, true));
    });
}

// The movable set of a session is replaced as a whole (block decomposition: points migrated in and out).  The caller
// writes the new points {x, y, z, bits(index)} into the buffer relax_swap_begin hands out and commits: the session then
// holds exactly these points, no fixed head, no tree — but keeps what it measured (cell scale, brick geometry, typical
// spacing), so the next rebuild costs one hash build, not a tuning pass.
int wtp::relax_swap_begin(wtp_ctx* ctx, int64_t n_move_new, void** d_buf_out) {
    RelaxState& r = ctx->relax;
    if (!r.active || r.pending.active) return fail(ctx, WTP_ERR_STATE, "relax_swap_begin: no session, or a pending fixed head");
    if (n_move_new < 1 || n_move_new > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "relax_swap_begin: bad point count");
    const int t = pick_free(r, r.bufP, -1);
    int rc;
    if ((rc = ensure(ctx, ctx->pts[t], pt_size(r.dtype) * (size_t)(n_move_new + r.shard_extra)))) return rc;
    r.swap_target = t;
    *d_buf_out = ctx->pts[t].p;
    return WTP_OK;
}

int wtp::relax_swap_commit(wtp_ctx* ctx, int64_t n_move_new) {
    RelaxState& r = ctx->relax;
    if (!r.active || r.swap_target < 0) return fail(ctx, WTP_ERR_STATE, "relax_swap_commit without relax_swap_begin");
    const size_t ts = tsize(r.dtype);
    int rc;
    if (spacing_on_device(r.spacing_kind)) { // hints and certificates belonged to the old set: every point walks once
        if ((rc = ensure(ctx, ctx->spacing_pp, ts * (size_t)n_move_new))) return rc;
        if ((rc = ensure(ctx, ctx->sp_hint, sizeof(int32_t) * (size_t)n_move_new))) return rc;
        if ((rc = ensure(ctx, ctx->sp_cert, 4 * ts * (size_t)n_move_new))) return rc;
        WTP_HIP(ctx, hipMemsetAsync(ctx->sp_hint.p, 0xFF, sizeof(int32_t) * (size_t)n_move_new, ctx->stream));
        WTP_HIP(ctx, hipMemsetAsync(ctx->sp_cert.p, 0xFF, 4 * ts * (size_t)n_move_new, ctx->stream));
        r.aux_off = 0;
    }
    r.bufP = r.swap_target;
    r.swap_target = -1;
    r.n = n_move_new;
    r.n_fixed = 0;
    r.k = (int64_t)r.k_req < n_move_new ? r.k_req : (int)n_move_new;
    r.bufS = -1;
    r.bufOld = -1;
    r.have_tree = false;
    r.can_revert = false;
    r.have_point_data = false;
    r.moved_by_hand = true; // (the kept grid's bounding box is not this set's)
    return WTP_OK;
}

// the movable points of P in index order into d_out (device)
static int unpermute_p(wtp_ctx* ctx, void* d_out) {
    const RelaxState& r = ctx->relax;
    return by_dtype(r.dtype, [&](auto t) {
        using T = decltype(t);
        return launch_unpermute<T>(ctx, pts_of<T>(ctx, r.bufP), r.n, r.n_fixed, r.dim, (T*)d_out);
    });
}

WTP_API int wtp_relax_get(wtp_ctx* ctx, void* xyz_out) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    RelaxState& r = ctx->relax;
    if (!xyz_out) return fail(ctx, WTP_ERR_ARG, "xyz_out is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = flush_pending(ctx))) return rc;
    const int64_t n_move = r.n - r.n_fixed;
    if (n_move == 0) return WTP_OK;
    const size_t bytes = tsize(r.dtype) * (size_t)n_move * r.dim;
    if ((rc = ensure(ctx, ctx->scratch, bytes))) return rc;
    if ((rc = unpermute_p(ctx, ctx->scratch.p))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(xyz_out, ctx->scratch.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_relax_get_dev(wtp_ctx* ctx, void* d_xyz_out) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    RelaxState& r = ctx->relax;
    if (!d_xyz_out) return fail(ctx, WTP_ERR_ARG, "xyz_out is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = flush_pending(ctx))) return rc;
    if (r.n - r.n_fixed == 0) return WTP_OK;
    if ((rc = unpermute_p(ctx, d_xyz_out))) return rc;
    return sync(ctx);
}

WTP_API int wtp_relax_get_point_data(wtp_ctx* ctx, void* forces_out, void* nn_dist_out, int32_t* nn_id_out) {
    if (!ctx) return WTP_ERR_ARG;
    RelaxState& r = ctx->relax;
    if (!r.active || !r.have_point_data || r.bufOld < 0)
        return fail(ctx, WTP_ERR_STATE, "wtp_relax_get_point_data needs a completed wtp_relax_step");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n_move = r.n - r.n_fixed;
    if (n_move == 0) return WTP_OK;
    const size_t ts = tsize(r.dtype);
    int rc;
    if ((rc = ensure(ctx, ctx->scratch, (2 * ts + 4) * (size_t)n_move))) return rc;
    char* base = (char*)ctx->scratch.p;
    void* fo = base;
    void* no = base + ts * n_move;
    int32_t* io = (int32_t*)(base + 2 * ts * n_move);
    // per-point arrays are in the slot order of the sweep's query buffer (== bufOld)
    rc = by_dtype(r.dtype, [&](auto t) {
        using T = decltype(t);
        return launch_unpermute_point_data<T>(ctx, pts_of<T>(ctx, r.bufOld), r.n, r.n_fixed, (const T*)ctx->forces.p,
                                              (const T*)ctx->nn_dist.p, (const int32_t*)ctx->nn_id.p, (T*)fo, (T*)no, io);
    });
    if (rc) return rc;
    if (forces_out) WTP_HIP(ctx, hipMemcpyAsync(forces_out, fo, ts * n_move, hipMemcpyDeviceToHost, ctx->stream));
    if (nn_dist_out) WTP_HIP(ctx, hipMemcpyAsync(nn_dist_out, no, ts * n_move, hipMemcpyDeviceToHost, ctx->stream));
    if (nn_id_out) WTP_HIP(ctx, hipMemcpyAsync(nn_id_out, io, 4 * (size_t)n_move, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

// P may alias the snapshot (fresh tree): moving points by hand must not move the tree's copy, so P gets its own buffer first
static int own_p(wtp_ctx* ctx, const char* entry) {
    RelaxState& r = ctx->relax;
    if (r.bufP != r.bufS) return WTP_OK;
    const int t = pick_free(r, r.bufS, r.can_revert ? r.bufOld : -1);
    if (t == r.bufS) return fail(ctx, WTP_ERR_STATE, std::string("no free buffer for ") + entry);
    const size_t bytes = pt_size(r.dtype) * (size_t)r.n;
    int rc;
    if ((rc = ensure(ctx, ctx->pts[t], bytes))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->pts[t].p, ctx->pts[r.bufP].p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    if (r.bufOld == t) r.can_revert = false;
    r.bufP = t;
    return WTP_OK;
}

WTP_API int wtp_relax_set(wtp_ctx* ctx, int64_t i, const void* xyz) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    RelaxState& r = ctx->relax;
    if (!xyz) return fail(ctx, WTP_ERR_ARG, "xyz is NULL");
    if (i < 0 || i >= r.n - r.n_fixed) return fail(ctx, WTP_ERR_ARG, "movable point index out of range");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = flush_pending(ctx))) return rc;
    const size_t ts = tsize(r.dtype);
    if ((rc = ensure(ctx, ctx->scratch, 64))) return rc;
    if ((rc = own_p(ctx, __func__))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->scratch.p, xyz, ts * r.dim, hipMemcpyHostToDevice, ctx->stream));
    const int32_t id = (int32_t)(i + r.n_fixed);
    r.moved_by_hand = true;
    rc = by_dtype(r.dtype, [&](auto t) {
        using T = decltype(t);
        return launch_set_point<T>(ctx, pts_of<T>(ctx, r.bufP), r.n, id, r.dim, (const T*)ctx->scratch.p);
    });
    if (rc) return rc;
    return sync(ctx);
}

// Many movable points placed at once (the deposition pass of the octree method lands a whole layer of
// escapees in one iteration): idx ascending, strictly increasing; one pass over the snapshot.
WTP_API int wtp_relax_set_batch(wtp_ctx* ctx, const int64_t* idx, const void* xyz, int64_t m) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    RelaxState& r = ctx->relax;
    if (m < 0) return fail(ctx, WTP_ERR_ARG, "m must be >= 0");
    if (m == 0) return WTP_OK;
    if (!idx || !xyz) return fail(ctx, WTP_ERR_ARG, "NULL array");
    std::vector<int32_t> ids((size_t)m);
    for (int64_t j = 0; j < m; ++j) {
        if (idx[j] < 0 || idx[j] >= r.n - r.n_fixed) return fail(ctx, WTP_ERR_ARG, "movable point index out of range");
        if (j > 0 && idx[j] <= idx[j - 1]) return fail(ctx, WTP_ERR_ARG, "indices must be strictly increasing");
        ids[(size_t)j] = (int32_t)(idx[j] + r.n_fixed);
    }
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = flush_pending(ctx))) return rc;
    const size_t ts = tsize(r.dtype);
    const size_t o_v = (sizeof(int32_t) * (size_t)m + 255) / 256 * 256;
    if ((rc = ensure(ctx, ctx->scratch, o_v + ts * (size_t)m * r.dim))) return rc;
    if ((rc = own_p(ctx, __func__))) return rc;
    char* b = (char*)ctx->scratch.p;
    WTP_HIP(ctx, hipMemcpyAsync(b, ids.data(), sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    WTP_HIP(ctx, hipMemcpyAsync(b + o_v, xyz, ts * (size_t)m * r.dim, hipMemcpyHostToDevice, ctx->stream));
    r.moved_by_hand = true;
    rc = by_dtype(r.dtype, [&](auto t) {
        using T = decltype(t);
        return launch_set_points<T>(ctx, pts_of<T>(ctx, r.bufP), r.n, (const int32_t*)b, m, r.dim, (const T*)(b + o_v));
    });
    if (rc) return rc;
    return sync(ctx); // also keeps `ids` alive until the copy has run
}

WTP_API int wtp_relax_revert(wtp_ctx* ctx) {
    if (!ctx) return WTP_ERR_ARG;
    RelaxState& r = ctx->relax;
    if (!r.active || !r.can_revert || r.bufOld < 0)
        return fail(ctx, WTP_ERR_STATE, "wtp_relax_revert needs a wtp_relax_step to undo");
    r.bufP = r.bufOld; // p .= p_old (src/repel.jl:314)
    r.can_revert = false;
    return WTP_OK;
}

WTP_API int wtp_relax_set_spacing(wtp_ctx* ctx, const void* spacing) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    RelaxState& r = ctx->relax;
    if (r.spacing_kind != WTP_SPACING_PER_POINT) return fail(ctx, WTP_ERR_STATE, "spacing is not PER_POINT");
    if (!spacing) return fail(ctx, WTP_ERR_ARG, "spacing is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    WTP_HIP(ctx, hipMemcpyAsync(ctx->spacing_pp.p, spacing, tsize(r.dtype) * (size_t)r.n, hipMemcpyHostToDevice,
                                ctx->stream));
    r.spacing_max = host_max(spacing, r.n, r.dtype);
    return sync(ctx);
}

WTP_API int wtp_relax_get_spacing(wtp_ctx* ctx, void* spacing_out) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    RelaxState& r = ctx->relax;
    if (!spacing_out) return fail(ctx, WTP_ERR_ARG, "spacing_out is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(r.dtype);
    if (r.spacing_kind == WTP_SPACING_CONSTANT) {
        for (int64_t i = 0; i < r.n; ++i) {
            if (r.dtype == WTP_F32) ((float*)spacing_out)[i] = (float)r.spacing_const;
            else ((double*)spacing_out)[i] = r.spacing_const;
        }
        return WTP_OK;
    }
    WTP_HIP(ctx, hipMemcpyAsync(spacing_out, ctx->spacing_pp.p, ts * (size_t)r.n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

template <typename T>
static int relax_query_knn_t(wtp_ctx* ctx, const void* xyz, int64_t nq, int k, int32_t* idx_out, void* dist_out) {
    RelaxState& r = ctx->relax;
    const size_t o_q = (sizeof(T) * (size_t)nq * r.dim + 255) / 256 * 256;
    int rc;
    if ((rc = ensure(ctx, ctx->scratch, o_q + sizeof(Pt<T>) * (size_t)nq))) return rc;
    if ((rc = ensure(ctx, ctx->idx_out, sizeof(int32_t) * (size_t)nq * k))) return rc;
    if (dist_out && (rc = ensure(ctx, ctx->dist_out, sizeof(T) * (size_t)nq * k))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->scratch.p, xyz, sizeof(T) * (size_t)nq * r.dim, hipMemcpyHostToDevice, ctx->stream));
    SearchArgs<T> a{};
    init_search(a, ctx, (const Pt<T>*)ctx->pts[r.bufS].p, nullptr, nq, k, 0);
    a.idx_out = (int32_t*)ctx->idx_out.p;
    a.dist_out = dist_out ? (T*)ctx->dist_out.p : nullptr;
    int sp = span_begin(ctx, 2);
    rc = launch_query_knn<T>(ctx, a, (const T*)ctx->scratch.p, r.dim, (Pt<T>*)((char*)ctx->scratch.p + o_q));
    span_end(ctx, sp);
    if (rc) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(idx_out, ctx->idx_out.p, sizeof(int32_t) * (size_t)nq * k, hipMemcpyDeviceToHost, ctx->stream));
    if (dist_out)
        WTP_HIP(ctx, hipMemcpyAsync(dist_out, ctx->dist_out.p, sizeof(T) * (size_t)nq * k, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_relax_query_knn(wtp_ctx* ctx, const void* xyz, int64_t nq, int k, int32_t* idx_out, void* dist_out) {
    if (!ctx) return WTP_ERR_ARG;
    RelaxState& r = ctx->relax;
    if (!r.active || !r.have_tree || r.bufS < 0 || r.pending.active)
        return fail(ctx, WTP_ERR_STATE, "wtp_relax_query_knn needs a session that has swept at least once");
    if (nq < 0 || nq > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "bad nq");
    if (k < 1 || k > r.n || k > kGenericKMax) return fail(ctx, WTP_ERR_ARG, "k must be in 1..min(n, 128)");
    if (nq == 0) return WTP_OK;
    if (!xyz || !idx_out) return fail(ctx, WTP_ERR_ARG, "NULL array");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    return by_dtype(r.dtype, [&](auto t) { return relax_query_knn_t<decltype(t)>(ctx, xyz, nq, k, idx_out, dist_out); });
}

WTP_API int wtp_relax_end(wtp_ctx* ctx) {
    if (!ctx) return WTP_ERR_ARG;
    ctx->relax = RelaxState{};
    return WTP_OK;
}

// (keep_alive: the caller's array stays valid until the copy has run in stream order — the block driver's own pool)
int wtp::relax_set_fixed_dev_impl(wtp_ctx* ctx, const void* d_fixed4, int64_t n_fixed_new, bool keep_alive) {
    int rc = need_session(ctx, "wtp_relax_set_fixed_dev");
    if (rc) return rc;
    RelaxState& r = ctx->relax;
    if (r.spacing_kind == WTP_SPACING_PER_POINT)
        return fail(ctx, WTP_ERR_STATE, "wtp_relax_set_fixed_dev: not with a caller-evaluated (PER_POINT) spacing array");
    if (n_fixed_new < 0 || (n_fixed_new > 0 && !d_fixed4)) return fail(ctx, WTP_ERR_ARG, "bad fixed-point array");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = flush_pending(ctx))) return rc; // two calls in a row: the first one's view is materialised
    const int64_t n_move = r.n - r.n_fixed, n_new = n_move + n_fixed_new;
    if (n_new < 1) return fail(ctx, WTP_ERR_ARG, "the snapshot would be empty");
    if (n_new > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "n exceeds the int32 index space");
    const size_t ts = tsize(r.dtype);
    const size_t ptsz = pt_size(r.dtype);
    // from now on the point buffers keep room for a replaced head next to the old one
    const int64_t extra = n_fixed_new + n_fixed_new / 4 + 4096;
    if (extra > r.shard_extra) r.shard_extra = extra;
    if ((rc = ensure(ctx, ctx->forces, ts * (size_t)n_new))) return rc;
    if ((rc = ensure(ctx, ctx->nn_dist, ts * (size_t)n_new))) return rc;
    if ((rc = ensure(ctx, ctx->nn_id, sizeof(int32_t) * (size_t)n_new))) return rc;
    if ((rc = ensure(ctx, ctx->fb_list, sizeof(int32_t) * (size_t)n_new))) return rc;
    if ((rc = ensure(ctx, ctx->fb2_list, sizeof(int32_t) * (size_t)n_new))) return rc;
    if ((rc = ensure(ctx, ctx->scratch, 64))) return rc;
    if (spacing_on_device(r.spacing_kind)) {
        // The law is evaluated at the movable points before every sweep (src/repel.jl:260) and nobody reads a fixed
        // point's spacing, so the new head needs no values: the array only has to hold n_new entries.  Hints and
        // certificates stay where they are, addressed by movable index (aux_off follows the head's size).
        if ((rc = ensure(ctx, ctx->spacing_pp, ts * (size_t)n_new))) return rc; // (contents: rewritten before the next sweep)
        r.aux_off += n_fixed_new - r.n_fixed;
    }
    const bool fits = ctx->pts[r.bufP].cap >= ptsz * (size_t)(r.n + n_fixed_new);
    if (fits) {
        // No pass over the cloud: the new head is appended behind the old snapshot and the NEXT hash
        // build reads the array through a view that drops the stale fixed points and renumbers the
        // rest (HashView; 0.16 ms per iteration saved at 11 M points against rewriting the array).
        if (n_fixed_new > 0) {
            rc = by_dtype(r.dtype, [&](auto t) {
                using T = decltype(t);
                return launch_append_fixed<T>(ctx, (const Pt<T>*)d_fixed4, n_fixed_new, pts_of<T>(ctx, r.bufP) + r.n);
            });
            if (rc) return rc;
        }
        r.pending.active = true;
        r.pending.n_old = r.n;
        r.pending.n_in = r.n + n_fixed_new;
        r.pending.fixed_old = (int32_t)r.n_fixed;
        r.pending.id_shift = (int32_t)(n_fixed_new - r.n_fixed);
    } else { // first call of a session (buffers sized for the plain snapshot): rewrite once
        const int t = pick_free(r, r.bufP, -1);
        if ((rc = ensure(ctx, ctx->pts[t], ptsz * (size_t)(n_new + r.shard_extra)))) return rc;
        rc = by_dtype(r.dtype, [&](auto tt) {
            using T = decltype(tt);
            return launch_refix<T>(ctx, pts_of<T>(ctx, r.bufP), r.n, r.n_fixed, n_fixed_new, (const Pt<T>*)d_fixed4,
                                   pts_of<T>(ctx, t), (int32_t*)ctx->scratch.p);
        });
        if (rc) return rc;
        r.bufP = t;
    }
    if (head_remeasures(r, n_fixed_new)) r.tune.valid = false; // the next rebuild measures the grid again
    r.n = n_new;
    r.n_fixed = n_fixed_new;
    r.k = (int64_t)r.k_req < n_new ? r.k_req : (int)n_new;
    r.bufS = -1;
    r.bufOld = -1;
    r.have_tree = false;
    r.can_revert = false;
    r.have_point_data = false;
    // the caller's array must outlive the copy: on a lent stream that is stream order, else wait
    return (ctx->stream == ctx->own_stream && !keep_alive) ? sync(ctx) : WTP_OK;
}

WTP_API int wtp_relax_set_fixed_dev(wtp_ctx* ctx, const void* d_fixed4, int64_t n_fixed_new) {
    return relax_set_fixed_dev_impl(ctx, d_fixed4, n_fixed_new, false);
}

WTP_API int wtp_relax_set_coverage(wtp_ctx* ctx, int axis, double lo, double hi) {
    if (int rc = need_session(ctx, __func__)) return rc;
    RelaxState& r = ctx->relax;
    if (axis >= r.dim) return fail(ctx, WTP_ERR_ARG, "axis must be < dim (negative: unlimited)");
    if (axis >= 0 && !(lo <= hi)) return fail(ctx, WTP_ERR_ARG, "need lo <= hi");
    r.cover_axis = axis < 0 ? -1 : axis;
    r.cover_lo = lo;
    r.cover_hi = hi;
    return WTP_OK;
}

WTP_API int wtp_relax_set_coverage_box(wtp_ctx* ctx, const double lo[3], const double hi[3]) {
    if (!ctx || !lo || !hi) return WTP_ERR_ARG;
    if (int rc = need_session(ctx, __func__)) return rc;
    RelaxState& r = ctx->relax;
    for (int ax = 0; ax < 3; ++ax) {
        if (!(lo[ax] <= hi[ax])) return fail(ctx, WTP_ERR_ARG, "need lo <= hi on every axis");
        r.cover_lo3[ax] = lo[ax];
        r.cover_hi3[ax] = hi[ax];
    }
    r.cover_axis = 3;
    return WTP_OK;
}
