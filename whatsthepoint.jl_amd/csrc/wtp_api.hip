// wtp_api.hip — the C ABI of include/wtp.h: context, buffer pool, host<->device staging and
// the call sequences that replace _build_knn_neighbors / _build_radius_neighbors
// (src/topology.jl:79-97) and the body of _relax!'s loop (src/repel.jl:243-334).
// No CPU fallback exists: without a usable gfx950 device wtp_create fails.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "wtp_internal.hpp"

namespace wtp {

static thread_local std::string g_create_err;

int fail(wtp_ctx* ctx, int code, const std::string& msg) {
    if (ctx)
        ctx->err = msg;
    else
        g_create_err = msg;
    return code;
}

int ensure(wtp_ctx* ctx, DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return WTP_OK;
    if (b.p) {
        hipFree(b.p);
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 16 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError(); // clear sticky OOM
        e = hipMalloc(&b.p, bytes);
        want = bytes;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(ctx, WTP_ERR_OOM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
    }
    b.cap = want;
    return WTP_OK;
}

int launch_occupancy_of(wtp_ctx* ctx, const void* fn, int threads, size_t smem) {
    const auto key = std::make_pair(fn, smem);
    auto it = ctx->launch_cache.find(key);
    if (it != ctx->launch_cache.end()) return it->second;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    int occ = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, threads, smem);
    if (e != hipSuccess || occ < 1) occ = 1;
    ctx->launch_cache[key] = occ;
    return occ;
}

int ensure_pinned(wtp_ctx* ctx, size_t bytes) {
    if (ctx->host_pinned_cap >= bytes) return WTP_OK;
    if (ctx->host_pinned) hipHostFree(ctx->host_pinned);
    ctx->host_pinned = nullptr;
    ctx->host_pinned_cap = 0;
    WTP_HIP(ctx, hipHostMalloc(&ctx->host_pinned, bytes, hipHostMallocDefault));
    ctx->host_pinned_cap = bytes;
    return WTP_OK;
}

// ---- timing spans -----------------------------------------------------------------------------
static int take_event(wtp_ctx* ctx) {
    if (ctx->ev_used == (int)ctx->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return -1;
        ctx->ev_pool.push_back(e);
    }
    return ctx->ev_used++;
}

// Spans of a step follow each other without a gap (hash | sweep | follow-ups | reduction | next hash ...), so the
// event that closes one opens the next: one record per span instead of two (an event record costs ~4 us of stream
// time; eight per step were a third of a 50 k-point step).  Work enqueued between two spans counts for the later one.
int span_begin(wtp_ctx* ctx, int kind) {
    if (!ctx->timing) return -1;
    if (ctx->spans.size() > 8192) spans_collect(ctx); // bounded pool; costs one sync
    int a = ctx->ev_last_end;
    if (a < 0) {
        a = take_event(ctx);
        if (a < 0) return -1;
        hipEventRecord(ctx->ev_pool[a], ctx->stream);
    }
    const int b = take_event(ctx);
    if (b < 0) return -1;
    ctx->spans.push_back({a, b, kind});
    return (int)ctx->spans.size() - 1;
}

void span_end(wtp_ctx* ctx, int span) {
    if (span < 0) return;
    hipEventRecord(ctx->ev_pool[ctx->spans[span].b], ctx->stream);
    ctx->ev_last_end = ctx->spans[span].b;
}

void spans_collect(wtp_ctx* ctx) {
    ctx->ev_last_end = -1; // the pool is recycled below (and a caller that reads the timers has synchronised: a gap)
    if (ctx->spans.empty()) return;
    hipStreamSynchronize(ctx->stream);
    for (auto& s : ctx->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev_pool[s.a], ctx->ev_pool[s.b]) == hipSuccess) {
            if (s.kind == 0) ctx->t_hash += ms;
            else if (s.kind == 1) ctx->t_sweep += ms;
            else ctx->t_other += ms;
        }
    }
    ctx->spans.clear();
    ctx->ev_used = 0;
}

static int sync(wtp_ctx* ctx) {
    ctx->ev_last_end = -1; // the host waits here: whatever it does next is not part of a span
    ctx->n_syncs += 1;
    WTP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WTP_OK;
}

static size_t tsize(int dtype) { return dtype == WTP_F64 ? 8 : 4; }
static size_t pt_size(int dtype) { return by_dtype(dtype, [](auto t) { return sizeof(Pt<decltype(t)>); }); }

int need_session(wtp_ctx* ctx, const char* entry) {
    if (!ctx) return WTP_ERR_ARG;
    if (!ctx->relax.active) return fail(ctx, WTP_ERR_STATE, std::string(entry) + " before wtp_relax_init");
    return WTP_OK;
}

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

static int check_cloud(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype) {
    if (!ctx) return WTP_ERR_ARG;
    if (!xyz) return fail(ctx, WTP_ERR_ARG, "xyz is NULL");
    if (n < 1) return fail(ctx, WTP_ERR_ARG, "n must be >= 1");
    if (n > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "n exceeds the int32 index space");
    if (dim != 2 && dim != 3) return fail(ctx, WTP_ERR_ARG, "dim must be 2 or 3");
    if (dtype != WTP_F32 && dtype != WTP_F64) return fail(ctx, WTP_ERR_ARG, "dtype must be WTP_F32 or WTP_F64");
    return WTP_OK;
}

// ---- hash with a measured cell edge ------------------------------------------------------------------
// build_hash sizes its cells from the box average n / volume.  That is right for a cloud that fills
// its box evenly and wrong for graded clouds (a 64x density contrast puts ~85 points into every wall
// cell), for surface clouds and for boxes stretched by a few outliers: the occupied cells then hold
// far more points than intended, halos overflow the LDS and whole bricks drop to the slow exact
// path (measured: 157 ms instead of ~2 ms per iteration on a 1 M-point graded cloud).  So the
// first build of a session / call measures the occupancy the POINTS see (sum cnt^2 / sum cnt, = rho + 1
// for a Poisson cloud) and shrinks the cell edge until that matches the target; at most 3 builds,
// one small read-back each.  Floors (radius, the force law's support) stay in force.
static double hash_target_rho(const wtp_ctx* ctx, int dim, int k, double rho_direct) {
    if (rho_direct > 0) return rho_direct < 1.0 ? 1.0 : rho_direct;
    const double r = (dim == 3 ? 0.381 : 0.436) * (double)(k > 0 ? k : 21) * (ctx->rho / 8.0);
    return r < 1.0 ? 1.0 : r;
}

// Quantile box: when a few far outliers stretch the bounding box so much that even the finest grid
// the caps allow (4096 cells per axis, 8 n cells) leaves the bulk of the cloud in a handful of cells,
// the grid is laid over the bulk only.  Per-axis histograms are zoomed (<= 4 rounds of 1024 bins)
// onto the range that holds all but 0.05 % of the points on either side; points outside are clamped
// into the edge cells, which every search treats as unbounded outward — results stay exact.
template <typename T>
static int find_robust_box(wtp_ctx* ctx, const Pt<T>* in, int64_t n, int dim, const Grid<T>& hg) {
    int rc;
    const size_t hist_bytes = sizeof(unsigned int) * 3 * 1024;
    if ((rc = ensure(ctx, ctx->box_dev, 64 + hist_bytes))) return rc;
    if ((rc = ensure_pinned(ctx, 64 + hist_bytes))) return rc;
    double box[6];
    for (int a = 0; a < 3; ++a) {
        box[a] = (double)hg.org[a];
        box[3 + a] = (double)hg.org[a] + (double)hg.n[a] * (double)hg.c;
    }
    const uint64_t tail = (uint64_t)(n / 2000) + 1; // 0.05 % per side
    for (int round = 0; round < 4; ++round) {
        memcpy(ctx->host_pinned, box, sizeof(box));
        WTP_HIP(ctx, hipMemcpyAsync(ctx->box_dev.p, ctx->host_pinned, sizeof(box), hipMemcpyHostToDevice, ctx->stream));
        unsigned int* d_hist = (unsigned int*)((char*)ctx->box_dev.p + 64);
        if ((rc = launch_axis_hist<T>(ctx, in, n, dim, (const double*)ctx->box_dev.p, d_hist))) return rc;
        WTP_HIP(ctx, hipMemcpyAsync((char*)ctx->host_pinned + 64, d_hist, hist_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
        const unsigned int* h = (const unsigned int*)((const char*)ctx->host_pinned + 64);
        bool shrunk = false;
        for (int a = 0; a < dim; ++a) {
            const double w = (box[3 + a] - box[a]) / 1024.0;
            if (!(w > 0)) continue;
            uint64_t run = 0;
            int b_lo = 0, b_hi = 1023;
            for (int b = 0; b < 1024; ++b) {
                run += h[a * 1024 + b];
                if (run >= tail) { b_lo = b; break; }
            }
            run = 0;
            for (int b = 1023; b >= 0; --b) {
                run += h[a * 1024 + b];
                if (run >= tail) { b_hi = b; break; }
            }
            if (b_hi < b_lo) b_hi = b_lo;
            const double nlo = box[a] + w * b_lo, nhi = box[a] + w * (b_hi + 1);
            if ((nhi - nlo) < 0.5 * (box[3 + a] - box[a])) shrunk = true;
            box[a] = nlo;
            box[3 + a] = nhi;
        }
        if (!shrunk) break;
    }
    memcpy(ctx->host_pinned, box, sizeof(box));
    WTP_HIP(ctx, hipMemcpyAsync(ctx->box_dev.p, ctx->host_pinned, sizeof(box), hipMemcpyHostToDevice, ctx->stream));
    return sync(ctx);
}

// Measured build b: the cell scale into t.scale (from 1), the occupancy asked for into t.rho and whether the grid lies over a
// quantile box into t.clipped; the grid of the last build and the occupancy its points see into *hg_out / *rho_eff_out.
template <typename T>
static int build_hash_tuned(wtp_ctx* ctx, GridTune& t, HashBuild<T> b, Grid<T>* hg_out, double* rho_eff_out) {
    const double target = hash_target_rho(ctx, b.dim, b.k, b.rho_direct);
    double scale = 1.0;
    double prev_c = -1;
    int rc;
    if ((rc = ensure(ctx, ctx->occ, 64))) return rc;
    if ((rc = ensure_pinned(ctx, 16384))) return rc;
    t.clipped = false; // every tuned build starts from the true bounding box
    b.keep_grid = false;
    for (int round = 0; round < 3; ++round) {
        b.cell_scale = scale;
        b.box = t.clipped ? (const double*)ctx->box_dev.p : nullptr;
        if ((rc = build_hash<T>(ctx, b))) return rc;
        if ((rc = launch_occupancy<T>(ctx, (const Grid<T>*)ctx->grid.p, (unsigned long long*)ctx->occ.p))) return rc;
        char* hp = (char*)ctx->host_pinned;
        WTP_HIP(ctx, hipMemcpyAsync(hp, ctx->occ.p, 24, hipMemcpyDeviceToHost, ctx->stream));
        WTP_HIP(ctx, hipMemcpyAsync(hp + 64, ctx->grid.p, sizeof(Grid<T>), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
        const unsigned long long* o = (const unsigned long long*)hp;
        const double rho_eff = o[1] ? (double)o[0] / (double)o[1] : 1.0;
        Grid<T> hg;
        memcpy(&hg, hp + 64, sizeof(hg));
        *rho_eff_out = rho_eff;
        *hg_out = hg;
        const double excess = (rho_eff - 1.0) / target;
        // the caps on the cell count bind (4096 per axis / 8 n) and the cells are still far over-full:
        // the box is stretched by outliers — lay the grid over the bulk and start over, once
        const bool capped = hg.n[0] >= kMaxAxisCells || hg.n[1] >= kMaxAxisCells || hg.n[2] >= kMaxAxisCells ||
                            (double)hg.ncells > 6.0 * (double)b.n;
        if (excess > 4.0 && capped && !t.clipped) {
            if ((rc = find_robust_box<T>(ctx, b.in, b.n, b.dim, hg))) return rc;
            t.clipped = true;
            scale = 1.0;
            prev_c = -1;
            round = -1;
            continue;
        }
        if (!(excess > 1.6) || round == 2) break;
        if (prev_c > 0 && !((double)hg.c < prev_c * 0.999)) break; // a floor binds: shrinking changes nothing
        prev_c = (double)hg.c;
        double f = std::cbrt(1.15 / excess); // occupancy ~ c^3 (c^2 on surfaces: the next round catches up)
        if (f < 0.3) f = 0.3;
        scale *= f;
        if (scale < 0.02) scale = 0.02;
    }
    t.scale = scale;
    t.rho = b.rho_direct;
    return WTP_OK;
}

// ---- topology -----------------------------------------------------------------------------------
// Expected cost per query of the bricks of wtp_ksel.hip over `cols` columns of rho_cell points per cell, for the cheapest
// split of the columns into bricks of equal length along x (its length in *bx_out): a brick costs one round of the 256
// lanes, two when its Q own points (Poisson) exceed them
static double ksel_brick_cost(int cols, double rho_cell, int* bx_out = nullptr) {
    int bx = ksel_max_bx();
    double best = 1e300;
    for (int nbx = 1; nbx <= cols; ++nbx) {
        const int b = (cols + nbx - 1) / nbx;
        if (b > ksel_max_bx()) continue;
        const double q = 4.0 * rho_cell * b;
        const double p2 = 0.5 * std::erfc((256.0 - q) / std::sqrt(2.0 * (q > 1 ? q : 1)));
        const double cost = (1.0 + p2 + (q > 512.0 ? 100.0 : 0.0)) / q;
        if (cost < best) {
            best = cost;
            bx = b;
        }
        if (b < 8) break;
    }
    if (bx_out) *bx_out = bx;
    return best;
}

// Brick geometry of wtp_ksel.hip from the measured grid: the brick length along x that puts ~224 queries on the 256
// lanes (four own cells per column; the denser of the box average and the occupancy the points see), and the LDS
// point area for its halo of 36 cells per column plus five standard deviations.
static void ksel_geometry(wtp_ctx* ctx, double n, double ncells, int n0, double rho_eff, int* bx_out, int* hcap_out) {
    double rho_cell = ncells > 0 ? n / ncells : 1.0;
    if (rho_eff - 1.0 > rho_cell) rho_cell = rho_eff - 1.0;
    if (rho_cell < 0.05) rho_cell = 0.05;
    int bx;
    ksel_brick_cost(n0, rho_cell, &bx);
    bx = bx < 8 ? (n0 < 8 ? (n0 > 0 ? n0 : 1) : 8) : bx;
    const double halo = 36.0 * (bx + 4) * rho_cell;
    int hc = (int)(halo + 5.0 * std::sqrt(halo)) + 32;
    hc = (hc + 63) / 64 * 64;
    *bx_out = bx;
    *hcap_out = hc < 512 ? 512 : (hc > 3072 ? 3072 : hc);
    if (ctx->debug)
        fprintf(stderr, "[wtp] ksel geometry: rho_cell %.3f (box average %.3f), %d columns -> bricks of %d, LDS point area %d\n",
                rho_cell, ncells > 0 ? n / ncells : 0.0, n0, *bx_out, *hcap_out);
}
// The occupancy (points per cell) that serves THIS cloud best, between 1.08 and 1.26 times k/22: the x axis holds a whole
// number of equal bricks, so the lane fill of a brick steps with the number of columns (at 10 M points 1.2 leaves bricks of
// 41 columns, 77 % of the lanes; 1.1 fills 90 %).  Model per query: (one brick round, two with probability p2) / Q own
// points, times the round's cost (a scan in proportion to the occupancy on top of a fixed part), plus the hand-backs that
// grow as the provable radius 2c shrinks.  `n0`, `c`: the grid just built with occupancy rho_cur.
static double ksel_pick_rho(double n, double ncells, int n0, double rho_cur, double rho_eff) {
    double fill_cur = ncells > 0 ? n / ncells : rho_cur; // points per cell, box average
    if (rho_eff - 1.0 > fill_cur) fill_cur = rho_eff - 1.0;
    double best = 1e300, best_rho = rho_cur;
    for (double f = 0.90; f <= 1.051; f += 0.0125) { // candidate occupancy = f * rho_cur
        if (rho_cur * f > 1.27) continue;                 // (a run of 173 cells must fit the 256 slots of the hit masks)
        const double edge = std::cbrt(f);                 // cell edge relative to the current one
        const int cols = (int)(((double)n0 - 0.5) / edge) + 1;
        const double cost_b = ksel_brick_cost(cols, fill_cur * f);
        const double round = 0.63 + 0.37 * f;                       // per-round work: fixed part + scan
        const double handback = 1.0 + 0.20 * (1.0 - f) / 0.1 * 0.1;   // ~2 % more total time per 10 % less occupancy
        const double cost = cost_b * round * handback;
        if (cost < best) {
            best = cost;
            best_rho = rho_cur * f;
        }
    }
    return best_rho;
}

// occupancy of the wtp_ksel.hip grid for kq = k + self: in proportion to kq (the cell edge follows r_k), capped where a run of
// 173 cells still fits the 256 slots of the hit masks
static double ksel_rho_for(int kq) {
    const double rho = kRhoKsel * (double)kq / 22.0;
    return rho > 1.26 ? 1.26 : rho;
}
// points the first filter ball is expected to hold: k + self plus the same number of standard deviations as
// kCapKsel leaves at 22
static double ksel_cap_count(int kq) {
    return (double)kq + (kCapKsel - 22.0) / std::sqrt(22.0) * std::sqrt((double)kq);
}

// The k-selection layout of build b on the grid just measured (hg, with rho_eff the occupancy its points see): the occupancy
// whose grid fills the bricks' lanes best — one more measured build when the pick moves t.rho by more than 1 % — and the
// brick geometry of the final grid, into t.
template <typename T>
static int ksel_tune(wtp_ctx* ctx, GridTune& t, HashBuild<T> b, Grid<T>& hg, double& rho_eff) {
    const double pick = ksel_pick_rho((double)b.n, (double)hg.ncells, hg.n[0], t.rho, rho_eff);
    int rc;
    if (std::fabs(pick - t.rho) > 0.01 * t.rho) {
        b.rho_direct = pick;
        if ((rc = build_hash_tuned<T>(ctx, t, b, &hg, &rho_eff))) return rc;
    }
    ksel_geometry(ctx, (double)b.n, (double)hg.ncells, hg.n[0], rho_eff, &t.bx, &t.hcap);
    return WTP_OK;
}

// The grid of build b (b.k: neighbours sought per query, self included) with the tuning cached in t.  When t was measured
// for this cloud size, dim, k and layout (the usual case: rebuild_topology! on the same points) it is one build_hash on the
// full box: no occupancy passes, no host synchronisation.  The tuning only affects speed, never the result.  Otherwise the
// grid is measured (build_hash_tuned, then ksel_tune on the k-selection layout) and stored with its key.
template <typename T> static int build_grid_cached(wtp_ctx* ctx, GridTune& t, HashBuild<T> b, bool ksel) {
    // (loose: a Float64 session's cloud changes size with every swapped head; an exact match would measure again each sweep)
    const int64_t slack = t.loose ? b.n / 20 : 0;
    if (t.valid && t.dim == b.dim && t.kq == b.k && t.ksel == ksel && std::llabs((long long)(b.n - t.n)) <= slack) {
        b.rho_direct = t.rho;
        b.cell_scale = t.scale;
        return build_hash<T>(ctx, b);
    }
    t.valid = false;
    double rho_eff = 0;
    Grid<T> hg;
    b.rho_direct = ksel ? ksel_rho_for(b.k) : 0.0;
    int rc = build_hash_tuned<T>(ctx, t, b, &hg, &rho_eff);
    if (!rc && ksel) rc = ksel_tune<T>(ctx, t, b, hg, rho_eff);
    if (rc) return rc;
    t.n = b.n;
    t.dim = b.dim;
    t.kq = b.k;
    t.ksel = ksel;
    // A clipped box belongs to this very cloud: a topology call never reuses its scale on the full box a hit builds.  (loose:
    // kept, as a Float64 session has always kept it — measuring again would cost three builds and host reads per sweep.)
    t.valid = t.loose || !t.clipped;
    return WTP_OK;
}

// the seven leading fields of a search; the rest stays as the caller has it
template <typename T>
static void init_search(SearchArgs<T>& a, const wtp_ctx* ctx, const Pt<T>* snap, const Pt<T>* query, int64_t n, int k,
                        int include_self) {
    a.grid = (const Grid<T>*)ctx->grid.p;
    a.snap = snap;
    a.query = query;
    a.cell_start = (const int32_t*)ctx->cell_start.p;
    a.n = (int32_t)n;
    a.k = k;
    a.include_self = include_self;
}

template <typename T>
static int knn_dev_t(wtp_ctx* ctx, const T* d_xyz, int64_t n, int dim, int k, int include_self,
                     int32_t* d_idx, T* d_dist) {
    int rc;
    if ((rc = ensure(ctx, ctx->pts[0], sizeof(Pt<T>) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->pts[1], sizeof(Pt<T>) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_count, 64))) return rc;
    ctx->counters_clean = false; // (this call counts in the block; the next sweep clears it itself)
    if ((rc = ensure(ctx, ctx->fb2_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb2_count, 64))) return rc;
    Pt<T>* raw = (Pt<T>*)ctx->pts[0].p;
    Pt<T>* sorted = (Pt<T>*)ctx->pts[1].p;
    int sp = span_begin(ctx, 0);
    if ((rc = load_points<T>(ctx, d_xyz, raw, n, dim))) return rc;
    // neighbours sought per query inside the structure: k others + self
    const int kq = include_self ? k : k + 1;
    // fp32 3-D clouds with k + self <= 24 (the reference's k = 21 among them): the x-slowest layout of wtp_ksel.hip —
    // cells of ~1.2 points, the k nearest inside the 5 x 5 x 5 block around the query's cell
    const bool ksel = sizeof(T) == 4 && dim == 3 && ctx->ksel && !ctx->force_generic && kq <= ksel_kmax() && n >= 4096;
    HashBuild<T> b(raw, sorted, n, dim, kq);
    b.canonical = false; // rows are ordered by (d2, id) explicitly (canon_kernel: 0.3 of a 1.1 ms KNN call on unsorted input)
    if ((rc = build_grid_cached<T>(ctx, ctx->knn_tune, b, ksel))) return rc;
    span_end(ctx, sp);
    SearchArgs<T> a{};
    init_search(a, ctx, sorted, sorted, n, k, include_self);
    a.idx_out = d_idx;
    a.dist_out = d_dist;
    a.fb_list = (int32_t*)ctx->fb_list.p;
    a.fb_count = (int32_t*)ctx->fb_count.p;
    a.fb2_list = (int32_t*)ctx->fb2_list.p;
    // one 64-byte counter block, cleared once: [0] hand-backs of the brick kernel, [4] of the wave kernel
    a.fb2_count = (int32_t*)ctx->fb_count.p + 4;
    WTP_HIP(ctx, hipMemsetAsync(ctx->fb_count.p, 0, 64, ctx->stream));
    a.counters_cleared = 1;
    if ((rc = ensure(ctx, ctx->diag, 128))) return rc;
    a.diag = (unsigned long long*)ctx->diag.p; // (written by -DWTP_DIAG builds only)
    if (ksel) {
        a.ksel_bx = ctx->knn_tune.bx;
        a.brick_hcap = ctx->knn_tune.hcap;
        a.cap_count = (float)ksel_cap_count(kq);
    }
    sp = span_begin(ctx, 1);
    rc = launch_topology<T>(ctx, a);
    span_end(ctx, sp);
    if (!rc && ctx->debug) { // hand-backs of the brick kernel to the exact path
        int32_t h[2] = {0, 0};
        hipMemcpyAsync(&h[0], a.fb_count, 4, hipMemcpyDeviceToHost, ctx->stream);
        hipMemcpyAsync(&h[1], a.fb2_count, 4, hipMemcpyDeviceToHost, ctx->stream);
        hipStreamSynchronize(ctx->stream);
        fprintf(stderr, "[wtp] knn n=%lld k=%d: %d queries to the wave kernel, %d to the serial one\n", (long long)n, k, h[0], h[1]);
    }
    ctx->n_sweep_launches += 1;
    ctx->relax.have_tree = false; // pts[] reused
    ctx->rad_valid = false;
    return rc;
}

// fp32 k-nearest candidates of a double4 cloud (knn_dev_f64, relax_f64_ksel_sweep; kernels in wtp_sweep64.hip): the cloud
// (w = its row) moved to its own origin (*org4_out) and rounded to float, hashed with the tuning cached in t, relabel(sorted32)
// run on the sorted float copy, then the kc nearest per query (self included) into cand_idx / cand_dist, on the x-slowest
// layout of wtp_ksel.hip where that applies (3-D, kc <= 24).  `b` comes with the caller's counter block; `sp`, the caller's
// hash span, is closed and the search span left open.
template <typename Relabel>
static int f64_candidates(wtp_ctx* ctx, const double4* pts, int64_t n, int dim, int kc, GridTune& t, SearchArgs<float>& b,
                          int& sp, const double** org4_out, Relabel relabel) {
    int rc;
    if ((rc = ensure(ctx, ctx->f32_pts, 2 * sizeof(float4) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->cand_idx, sizeof(int32_t) * (size_t)n * kc))) return rc;
    if ((rc = ensure(ctx, ctx->cand_dist, sizeof(float) * (size_t)n * kc))) return rc;
    if ((rc = ensure(ctx, ctx->occ, 64))) return rc;
    float4* raw32 = (float4*)ctx->f32_pts.p;
    float4* sorted32 = raw32 + n;
    double* org4 = (double*)ctx->occ.p + 4; // behind the occupancy counters
    *org4_out = org4;
    if ((rc = launch_origin(ctx, pts, n, org4))) return rc;
    if ((rc = launch_to_local_f32(ctx, pts, n, org4, raw32))) return rc;
    const bool ksel = dim == 3 && ctx->ksel && kc <= ksel_kmax() && n >= 4096;
    HashBuild<float> hb(raw32, sorted32, n, dim, kc);
    hb.canonical = false; // rows are ordered by (d2, id) explicitly: no canonical-order pass
    rc = build_grid_cached<float>(ctx, t, hb, ksel);
    if (!rc) rc = relabel(sorted32);
    if (rc) return rc;
    span_end(ctx, sp);
    sp = span_begin(ctx, 1);
    init_search(b, ctx, sorted32, sorted32, n, kc, 1);
    b.idx_out = (int32_t*)ctx->cand_idx.p;
    b.dist_out = (float*)ctx->cand_dist.p;
    if (ksel) {
        b.ksel_bx = t.bx;
        b.brick_hcap = t.hcap;
        b.cap_count = (float)ksel_cap_count(kc);
    }
    return launch_topology<float>(ctx, b);
}

// fp64 clouds, KNNTopology: Float64 is the reference's default type, and the exact wave-per-query
// path costs 16 ns per query.  Faster and still exact: search CANDIDATES in fp32 (the cloud moved to
// its own origin and rounded to float; the k+2 nearest per query through the fp32 brick kernel),
// re-rank them in exact fp64, and certify per query that nothing outside the candidate list can
// belong to the answer (refine_f64_kernel).  Queries that fail the certificate — coincident
// clusters larger than the list, clouds whose extent/spacing ratio exhausts float — take the exact
// path.  Returns 1 in *done when it handled the call.
static int knn_dev_f64(wtp_ctx* ctx, const double* d_xyz, int64_t n, int dim, int k, int include_self, int32_t* d_idx,
                       double* d_dist, bool* done) {
    *done = false;
    const int kq = include_self ? k : k + 1;
    // two candidates beyond the kq wanted: the certificate needs ONE whose fp32 distance clears the exact
    // kq-th by more than the rounding bound (gaps between consecutive neighbour distances are ~1e-2 of
    // the distance, the bound ~1e-6), and longer lists overflow the brick kernel's 64-entry ring
    int kc = kq + 2;
    if ((int64_t)kc > n) kc = (int)n;
    if (ctx->force_generic || kc > 31) return WTP_OK; // beyond the fp32 brick kernel's list length: exact path
    int rc;
    if ((rc = ensure(ctx, ctx->pts[0], sizeof(double4) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->pts[1], sizeof(double4) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_count, 64))) return rc;
    ctx->counters_clean = false; // (this call counts in the block; the next sweep clears it itself)
    if ((rc = ensure(ctx, ctx->fb2_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb2_count, 64))) return rc;
    double4* raw64 = (double4*)ctx->pts[0].p;
    int sp = span_begin(ctx, 0);
    if ((rc = load_points<double>(ctx, d_xyz, raw64, n, dim))) return rc;
    // k = 21 without self (kc = 24): search and re-ranking in slot order (see refine_f64_slots_kernel)
    const bool slots = kc == 24;
    double4* slot64 = (double4*)ctx->pts[1].p;
    SearchArgs<float> a{};
    a.fb_list = (int32_t*)ctx->fb_list.p;
    a.fb_count = (int32_t*)ctx->fb_count.p;
    a.fb2_list = (int32_t*)ctx->fb2_list.p;
    a.fb2_count = (int32_t*)ctx->fb2_count.p;
    const double* org4 = nullptr;
    rc = f64_candidates(ctx, raw64, n, dim, kc, ctx->knn64_tune, a, sp, &org4, [&](float4* sorted32) {
        return slots ? launch_relabel_slots(ctx, raw64, sorted32, slot64, nullptr, n) : WTP_OK;
    });
    if (rc) return rc;
    // kept: the next fp32 call measures its cloud afresh, not with a scale measured before this call on a cloud of that size
    ctx->knn_tune.valid = false;
    if (slots)
        rc = launch_refine_f64_slots(ctx, slot64, a.idx_out, a.dist_out, n, kc, k, include_self, org4, d_idx, d_dist,
                                     (int32_t*)ctx->fb_list.p, (int32_t*)ctx->fb_count.p);
    else
        rc = launch_refine_f64(ctx, raw64, a.idx_out, a.dist_out, n, kc, k, include_self, org4, d_idx, d_dist,
                               (int32_t*)ctx->fb_list.p, (int32_t*)ctx->fb_count.p);
    span_end(ctx, sp);
    if (rc) return rc;
    ctx->n_sweep_launches += 1;
    ctx->relax.have_tree = false;
    ctx->rad_valid = false;
    if ((rc = ensure_pinned(ctx, 64))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, ctx->fb_count.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    const int32_t n_fail = *(const int32_t*)ctx->host_pinned;
    if (n_fail > 0) { // exact fp64 path for the uncertified queries: wave kernel over their ids, fp64 grid
        double4* sorted64 = (double4*)ctx->pts[1].p;
        HashBuild<double> hb(raw64, sorted64, n, dim, kq);
        hb.canonical = false; // rows are ordered by (d2, id) explicitly: no canonical-order pass (0.5 ms on unsorted input)
        if ((rc = build_hash<double>(ctx, hb))) return rc;
        SearchArgs<double> b{};
        init_search(b, ctx, sorted64, raw64, n, k, include_self); // list entries are ids: raw64[id] is the query, its w the id
        b.idx_out = d_idx;
        b.dist_out = d_dist;
        b.fb_list = (int32_t*)ctx->fb_list.p;
        b.fb_count = (int32_t*)ctx->fb_count.p;
        b.fb2_list = (int32_t*)ctx->fb2_list.p;
        b.fb2_count = (int32_t*)ctx->fb2_count.p;
        if ((rc = launch_generic_topology<double>(ctx, b, false))) return rc;
    }
    *done = true;
    return WTP_OK;
}

static int check_idle(wtp_ctx* ctx) {
    if (ctx->relax.active)
        return fail(ctx, WTP_ERR_STATE,
                    "context holds a relax session (its buffers are live): call wtp_relax_end or use another context");
    return WTP_OK;
}

static int check_k(wtp_ctx* ctx, int64_t n, int k, int include_self) {
    if (k < 1) return fail(ctx, WTP_ERR_ARG, "k must be >= 1");
    if ((int64_t)k > n - (include_self ? 0 : 1))
        return fail(ctx, WTP_ERR_ARG, "k exceeds the number of available neighbours (k+1 > n)");
    if (k > kGenericKMax) return fail(ctx, WTP_ERR_ARG, "k > 128 is not supported");
    return WTP_OK;
}

} // namespace wtp

using namespace wtp;

#define WTP_API extern "C"

WTP_API const char* wtp_version(void) { return "wtp-mi355x 0.1.0 (gfx950)"; }

WTP_API const char* wtp_last_error(const wtp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

WTP_API int wtp_create(const int* device_ordinals, int n_dev, wtp_ctx** out) {
    if (!out) return fail(nullptr, WTP_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (n_dev != 1)
        return fail(nullptr, WTP_ERR_ARG, "one context drives one GPU: create one context per process/GPU");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        (void)hipGetLastError();
        return fail(nullptr, WTP_ERR_NO_DEVICE, "no HIP device visible (libwtp has no CPU path)");
    }
    int dev = device_ordinals ? device_ordinals[0] : 0;
    if (dev < 0 || dev >= count) return fail(nullptr, WTP_ERR_ARG, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return fail(nullptr, WTP_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, WTP_ERR_NO_DEVICE,
                    std::string("device is ") + prop.gcnArchName + ", libwtp is built for gfx950 only");
    if (hipSetDevice(dev) != hipSuccess) return fail(nullptr, WTP_ERR_HIP, "hipSetDevice failed");
    wtp_ctx* ctx = new wtp_ctx();
    ctx->device = dev;
    ctx->sm_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return fail(nullptr, WTP_ERR_HIP, "hipStreamCreate failed");
    }
    ctx->stream = ctx->own_stream;
    if (const char* e = getenv("WTP_RHO")) ctx->rho = atof(e) > 0 ? atof(e) : ctx->rho;
    if (const char* e = getenv("WTP_FORCE_GENERIC")) ctx->force_generic = atoi(e);
    if (const char* e = getenv("WTP_FULL_SELECT")) ctx->full_select = atoi(e);
    if (const char* e = getenv("WTP_KSEL")) ctx->ksel = atoi(e);
    if (const char* e = getenv("WTP_BALL64")) ctx->ball64 = atoi(e);
    if (const char* e = getenv("WTP_F64_KSEL")) ctx->f64_ksel = atoi(e);
    if (const char* e = getenv("WTP_RADIUS_DENSE")) ctx->radius_dense = atoi(e);
    if (const char* e = getenv("WTP_BLOCK_OVERLAP")) ctx->block_overlap = atoi(e);
    ctx->debug = getenv("WTP_DEBUG") != nullptr;
    ctx->debug_kd = getenv("WTP_DEBUG_KD") != nullptr;
    if (const char* e = getenv("WTP_TIMING")) {
        ctx->timing = atoi(e) != 0;
        ctx->timing_forced = true;
    }
    *out = ctx;
    return WTP_OK;
}

WTP_API int wtp_destroy(wtp_ctx* ctx) {
    if (ctx) block_destroy(ctx);
    if (ctx) block_topo_destroy(ctx);
    if (!ctx) return WTP_OK;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    wtp_comm_finalize(ctx);
    if (ctx->host_pinned) hipHostFree(ctx->host_pinned);
    for (auto e : ctx->ev_pool) hipEventDestroy(e);
    if (ctx->ev_comm_a) hipEventDestroy(ctx->ev_comm_a);
    if (ctx->ev_comm_b) hipEventDestroy(ctx->ev_comm_b);
    if (ctx->comm_stream) hipStreamDestroy(ctx->comm_stream);
    hipStreamDestroy(ctx->own_stream);
    delete ctx; // (frees the device buffers)
    return WTP_OK;
}

// The k-NN dispatch of a device cloud: fp32 through knn_dev_t; fp64 through fp32 candidates and exact re-ranking
// (knn_dev_f64), else the exact fp64 path.
static int knn_on_device(wtp_ctx* ctx, const void* d_xyz, int64_t n, int dim, int dtype, int k, int include_self,
                         int32_t* d_idx, void* d_dist) {
    bool done = false;
    int rc = dtype == WTP_F64 ? knn_dev_f64(ctx, (const double*)d_xyz, n, dim, k, include_self, d_idx, (double*)d_dist, &done)
                              : WTP_OK;
    if (rc || done) return rc;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return knn_dev_t<T>(ctx, (const T*)d_xyz, n, dim, k, include_self, d_idx, (T*)d_dist);
    });
}

// rows and, if wanted, distances of a host cloud, left in ctx->idx_out / dist_out (the cloud in ctx->raw_in)
static int knn_rows_on_device(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, int include_self,
                              bool want_dist) {
    const size_t ts = tsize(dtype);
    int rc;
    if ((rc = ensure(ctx, ctx->raw_in, ts * (size_t)n * dim))) return rc;
    if ((rc = ensure(ctx, ctx->idx_out, sizeof(int32_t) * (size_t)n * k))) return rc;
    if (want_dist && (rc = ensure(ctx, ctx->dist_out, ts * (size_t)n * k))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->raw_in.p, xyz, ts * (size_t)n * dim, hipMemcpyHostToDevice, ctx->stream));
    return knn_on_device(ctx, ctx->raw_in.p, n, dim, dtype, k, include_self, (int32_t*)ctx->idx_out.p,
                         want_dist ? ctx->dist_out.p : nullptr);
}

WTP_API int wtp_knn_dev(wtp_ctx* ctx, const void* d_xyz, int64_t n, int dim, int dtype, int k, int include_self,
                int32_t* d_idx_out, void* d_dist_out) {
    int rc = check_cloud(ctx, d_xyz, n, dim, dtype);
    if (rc) return rc;
    if ((rc = check_k(ctx, n, k, include_self))) return rc;
    if ((rc = check_idle(ctx))) return rc;
    if (!d_idx_out) return fail(ctx, WTP_ERR_ARG, "idx_out is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = knn_on_device(ctx, d_xyz, n, dim, dtype, k, include_self, d_idx_out, d_dist_out))) return rc;
    return sync(ctx);
}

WTP_API int wtp_knn(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, int include_self,
            int32_t* idx_out, void* dist_out) {
    int rc = check_cloud(ctx, xyz, n, dim, dtype);
    if (rc) return rc;
    if ((rc = check_k(ctx, n, k, include_self))) return rc;
    if ((rc = check_idle(ctx))) return rc;
    if (!idx_out) return fail(ctx, WTP_ERR_ARG, "idx_out is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    if ((rc = knn_rows_on_device(ctx, xyz, n, dim, dtype, k, include_self, dist_out != nullptr))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(idx_out, ctx->idx_out.p, sizeof(int32_t) * (size_t)n * k, hipMemcpyDeviceToHost,
                                ctx->stream));
    if (dist_out)
        WTP_HIP(ctx, hipMemcpyAsync(dist_out, ctx->dist_out.p, ts * (size_t)n * k, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

// ---- consumers of the rows ------------------------------------------------------
WTP_API int wtp_pca_normals(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, void* normals_out) {
    int rc = check_cloud(ctx, xyz, n, dim, dtype);
    if (rc) return rc;
    if (k < 2) return fail(ctx, WTP_ERR_ARG, "k must be >= 2 (a covariance needs two points)");
    if ((rc = check_k(ctx, n, k, 1))) return rc;
    if ((rc = check_idle(ctx))) return rc;
    if (!normals_out) return fail(ctx, WTP_ERR_ARG, "normals_out is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    if ((rc = knn_rows_on_device(ctx, xyz, n, dim, dtype, k, 1, false))) return rc;
    if ((rc = ensure(ctx, ctx->scratch, ts * (size_t)n * dim))) return rc;
    int sp = span_begin(ctx, 2);
    rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_pca_normals<T>(ctx, (const T*)ctx->raw_in.p, n, dim, (const int32_t*)ctx->idx_out.p, k, (T*)ctx->scratch.p);
    });
    span_end(ctx, sp);
    if (rc) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(normals_out, ctx->scratch.p, ts * (size_t)n * dim, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_gradient_limit(wtp_ctx* ctx, const void* centers, int64_t n, int dim, int dtype, int k, const void* h0,
                               double g, double tol, int max_sweeps, void* h_out, int* sweeps_out) {
    int rc = check_cloud(ctx, centers, n, dim, dtype);
    if (rc) return rc;
    if ((rc = check_k(ctx, n, k, 1))) return rc;
    if ((rc = check_idle(ctx))) return rc;
    if (!h0 || !h_out) return fail(ctx, WTP_ERR_ARG, "NULL array");
    if (max_sweeps < 0) return fail(ctx, WTP_ERR_ARG, "max_sweeps must be >= 0");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    if ((rc = knn_rows_on_device(ctx, centers, n, dim, dtype, k, 1, true))) return rc;
    const size_t o1 = (ts * (size_t)n + 255) / 256 * 256;
    if ((rc = ensure(ctx, ctx->scratch, 2 * o1 + 64))) return rc;
    char* b = (char*)ctx->scratch.p;
    unsigned long long* st = (unsigned long long*)(b + 2 * o1);
    WTP_HIP(ctx, hipMemcpyAsync(b, h0, ts * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    WTP_HIP(ctx, hipMemsetAsync(st, 0, 64, ctx->stream));
    if ((rc = ensure_pinned(ctx, 64))) return rc;
    unsigned long long* hst = (unsigned long long*)ctx->host_pinned;
    hst[0] = hst[1] = 0;
    int sp = span_begin(ctx, 2);
    for (int first = 0; first < max_sweeps && !hst[0];) { // batches: one read-back per 16 sweeps
        const int batch = max_sweeps - first < 16 ? max_sweeps - first : 16;
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return launch_minplus_batch<T>(ctx, (const int32_t*)ctx->idx_out.p, (const T*)ctx->dist_out.p, n, k, g, tol, (T*)b,
                                           (T*)(b + o1), first, batch, st);
        });
        if (rc) return rc;
        WTP_HIP(ctx, hipMemcpyAsync(hst, st, 16, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
        first += batch;
    }
    span_end(ctx, sp);
    const int applied = (int)hst[1];
    if (sweeps_out) *sweeps_out = applied;
    WTP_HIP(ctx, hipMemcpyAsync(h_out, b + ((applied & 1) ? o1 : 0), ts * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

// ---- RadiusTopology ------------------------------------------------------------------------------
template <typename T> static int radius_count_t(wtp_ctx* ctx, int64_t n, int dim, double r, int32_t* d_counts) {
    int rc;
    if ((rc = ensure(ctx, ctx->pts[0], sizeof(Pt<T>) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->pts[1], sizeof(Pt<T>) * (size_t)n))) return rc;
    Pt<T>* raw = (Pt<T>*)ctx->pts[0].p;
    Pt<T>* sorted = (Pt<T>*)ctx->pts[1].p;
    int sp = span_begin(ctx, 0);
    if ((rc = load_points<T>(ctx, (const T*)ctx->raw_in.p, raw, n, dim))) return rc;
    HashBuild<T> b(raw, sorted, n, dim, 0);
    b.radius = r > 0 ? r : 1e-300;
    b.canonical = false; // rows are ordered by (d2, id) explicitly
    if ((rc = build_hash<T>(ctx, b))) return rc;
    span_end(ctx, sp);
    SearchArgs<T> a{};
    init_search(a, ctx, sorted, sorted, n, 0, 0);
    if ((rc = ensure(ctx, ctx->fb_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_count, 64))) return rc;
    ctx->counters_clean = false; // (this call counts in the block; the next sweep clears it itself)
    a.fb_list = (int32_t*)ctx->fb_list.p; // queries the brick kernel hands back to the wave kernel
    a.fb_count = (int32_t*)ctx->fb_count.p;
    // fp32: the brick kernel parks the rows it finds (32 ids per query) and marks the query, so that wtp_radius_fill copies
    // them instead of running the whole search a second time (128 B per point of scratch)
    if ((rc = ensure(ctx, ctx->rad_done, (size_t)n + 64))) return rc;
    WTP_HIP(ctx, hipMemsetAsync(ctx->rad_done.p, 0, (size_t)n, ctx->stream));
    a.rad_done = (uint8_t*)ctx->rad_done.p;
    if (sizeof(T) == 4 && !ctx->force_generic) { // the brick kernel's rows: 32 ids per query
        if ((rc = ensure(ctx, ctx->rad_tmp, sizeof(int32_t) * 32 * (size_t)n))) return rc;
        a.rad_tmp = (int32_t*)ctx->rad_tmp.p;
    }
    // the wave kernel's rows (any length up to its list), where it serves every query (fp64; fp32 grids whose rows are
    // expected to outgrow the brick kernel, Grid::rad_wave_only; WTP_FORCE_GENERIC=1): an arena of 48 ids per point,
    // shared out evenly among the waves; a row that does not fit any more is simply searched again by the fill phase.
    // (For the hand-backs of the fp32 brick kernel it buys nothing: measured 2.07 -> 2.14 ms per graded 1 M cloud —
    // ranking in the count phase costs what it saves in the fill phase; the kernel decides by the grid's flag.)
    const int64_t arena_cap = (int64_t)kRadArenaPerPoint * n;
    if ((rc = ensure(ctx, ctx->rad_arena, sizeof(int32_t) * (size_t)arena_cap))) return rc;
    if ((rc = ensure(ctx, ctx->rad_arena_off, sizeof(int64_t) * (size_t)(n + 2)))) return rc;
    a.rad_arena = (int32_t*)ctx->rad_arena.p;
    a.rad_arena_off = (int64_t*)ctx->rad_arena_off.p;
    if ((rc = ensure(ctx, ctx->rad_pos, 64))) return rc;
    WTP_HIP(ctx, hipMemsetAsync(ctx->rad_pos.p, 0, 16, ctx->stream));
    if ((rc = ensure(ctx, ctx->rad_bricks, sizeof(int32_t) * (size_t)(n + 64)))) return rc;
    a.rad_bricks = (int32_t*)ctx->rad_bricks.p;
    a.rad_arena_pos = (unsigned long long*)ctx->rad_pos.p; // the dense kernel takes pieces of the arena (wtp_radb.hip)
    a.rad_arena_cap = arena_cap;
    sp = span_begin(ctx, 1);
    rc = launch_radius_count<T>(ctx, a, (T)r, d_counts);
    ctx->rad_dense_used = a.rad_dense > 0;
    span_end(ctx, sp);
    if (!rc && a.rad_dense > 0 && ctx->debug) {
        int32_t h[4] = {0, 0, 0, 0};
        WTP_HIP(ctx, hipMemcpyAsync(h, ctx->rad_pos.p, 16, hipMemcpyDeviceToHost, ctx->stream));
        WTP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "[wtp] radius, dense kernel: %d bricks, %d of %lld queries, %lld ids parked\n", h[2], h[3], (long long)n,
                (long long)(((unsigned long long)(uint32_t)h[1] << 32) | (uint32_t)h[0]));
    }
    return rc;
}

template <typename T> static int radius_fill_t(wtp_ctx* ctx, const int64_t* d_off, int32_t* d_idx) {
    SearchArgs<T> a{};
    init_search(a, ctx, (const Pt<T>*)ctx->pts[1].p, (const Pt<T>*)ctx->pts[1].p, ctx->rad_n, 0, 0);
    a.fb2_list = (int32_t*)ctx->fb2_list.p;
    a.fb2_count = (int32_t*)ctx->fb2_count.p;
    a.fb_list = (int32_t*)ctx->fb_list.p; // ensured by the count phase
    a.fb_count = (int32_t*)ctx->fb_count.p;
    // the rows the count phase of this very cloud parked (rad_valid guards the pair of calls)
    a.rad_tmp = sizeof(T) == 4 && !ctx->force_generic ? (int32_t*)ctx->rad_tmp.p : nullptr;
    a.rad_done = (uint8_t*)ctx->rad_done.p;
    a.rad_arena = (int32_t*)ctx->rad_arena.p;
    a.rad_arena_off = (int64_t*)ctx->rad_arena_off.p;
    a.rad_arena_cap = (int64_t)kRadArenaPerPoint * ctx->rad_n;
    a.rad_dense = ctx->rad_dense_used ? 1 : 0; // (the hand-back list of the count phase is what is left to search)
    int sp = span_begin(ctx, 1);
    int rc = launch_radius_fill<T>(ctx, a, (T)ctx->rad_r, d_off, d_idx);
    span_end(ctx, sp);
    return rc;
}

// wtp_radius_count and wtp_radius_offsets: counts of a host cloud on the device, handed back as they are or, with
// `offsets`, as CSR offsets (exclusive scan on the device: the counts never cross the bus and the offsets stay resident
// for the fill)
static int radius_count_call(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, double r, bool offsets, void* out) {
    int rc = check_cloud(ctx, xyz, n, dim, dtype);
    if (rc) return rc;
    if (!(r >= 0) || !std::isfinite(r)) return fail(ctx, WTP_ERR_ARG, "radius must be finite and >= 0");
    if (!out) return fail(ctx, WTP_ERR_ARG, offsets ? "offsets_out is NULL" : "counts_out is NULL");
    if ((rc = check_idle(ctx))) return rc;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    ctx->rad_valid = false;
    ctx->rad_offsets_dev = false;
    ctx->relax.have_tree = false;
    if ((rc = ensure(ctx, ctx->raw_in, ts * (size_t)n * dim))) return rc;
    if ((rc = ensure(ctx, ctx->counts_out, sizeof(int32_t) * (size_t)n))) return rc;
    if (offsets && (rc = ensure(ctx, ctx->dist_out, sizeof(int64_t) * (size_t)(n + 1)))) return rc; // offsets live here until the fill
    WTP_HIP(ctx, hipMemcpyAsync(ctx->raw_in.p, xyz, ts * (size_t)n * dim, hipMemcpyHostToDevice, ctx->stream));
    rc = by_dtype(dtype, [&](auto t) { return radius_count_t<decltype(t)>(ctx, n, dim, r, (int32_t*)ctx->counts_out.p); });
    if (rc) return rc;
    if (offsets) {
        // (radius_count_t uses scratch for nothing; the scan's tile sums go there)
        if ((rc = ensure(ctx, ctx->scratch, offsets_scan_tmp_bytes(n)))) return rc;
        int sp = span_begin(ctx, 2);
        rc = launch_offsets_scan(ctx, (const int32_t*)ctx->counts_out.p, n, (int64_t*)ctx->scratch.p, (int64_t*)ctx->dist_out.p);
        span_end(ctx, sp);
        if (rc) return rc;
        WTP_HIP(ctx, hipMemcpyAsync(out, ctx->dist_out.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost,
                                    ctx->stream));
    } else {
        WTP_HIP(ctx, hipMemcpyAsync(out, ctx->counts_out.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    }
    if ((rc = sync(ctx))) return rc;
    ctx->rad_n = n;
    ctx->rad_dim = dim;
    ctx->rad_dtype = dtype;
    ctx->rad_r = r;
    ctx->rad_valid = true;
    ctx->rad_offsets_dev = offsets;
    if (offsets) ctx->rad_nnz = ((const int64_t*)out)[n];
    return WTP_OK;
}

WTP_API int wtp_radius_count(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, double r, int32_t* counts_out) {
    return radius_count_call(ctx, xyz, n, dim, dtype, r, false, counts_out);
}

WTP_API int wtp_radius_offsets(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, double r,
                               int64_t* offsets_out) {
    return radius_count_call(ctx, xyz, n, dim, dtype, r, true, offsets_out);
}

WTP_API int wtp_radius_fill(wtp_ctx* ctx, const int64_t* offsets, int32_t* idx_out) {
    if (!ctx) return WTP_ERR_ARG;
    if (!ctx->rad_valid) return fail(ctx, WTP_ERR_STATE, "wtp_radius_fill needs a preceding wtp_radius_count");
    if (!offsets && !ctx->rad_offsets_dev)
        return fail(ctx, WTP_ERR_ARG, "offsets is NULL (only wtp_radius_offsets leaves them on the device)");
    const int64_t n = ctx->rad_n;
    if (offsets) {
        if (offsets[0] != 0) return fail(ctx, WTP_ERR_ARG, "offsets[0] must be 0");
        for (int64_t i = 0; i < n; ++i)
            if (offsets[i + 1] < offsets[i]) return fail(ctx, WTP_ERR_ARG, "offsets must be non-decreasing");
    }
    const int64_t nnz = offsets ? offsets[n] : ctx->rad_nnz;
    if (nnz > 0 && !idx_out) return fail(ctx, WTP_ERR_ARG, "idx_out is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(ctx->rad_dtype);
    int rc;
    if ((rc = ensure(ctx, ctx->idx_out, sizeof(int32_t) * (size_t)(nnz + 1)))) return rc;
    if ((rc = ensure(ctx, ctx->scratch, ts * (size_t)(nnz + 1)))) return rc;
    if ((rc = ensure(ctx, ctx->dist_out, sizeof(int64_t) * (size_t)(n + 1)))) return rc; // offsets staging
    if ((rc = ensure(ctx, ctx->fb2_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb2_count, 64))) return rc;
    if (offsets)
        WTP_HIP(ctx, hipMemcpyAsync(ctx->dist_out.p, offsets, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice,
                                    ctx->stream));
    rc = by_dtype(ctx->rad_dtype,
                  [&](auto t) { return radius_fill_t<decltype(t)>(ctx, (const int64_t*)ctx->dist_out.p, (int32_t*)ctx->idx_out.p); });
    if (rc) return rc;
    if (nnz > 0)
        WTP_HIP(ctx, hipMemcpyAsync(idx_out, ctx->idx_out.p, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost,
                                    ctx->stream));
    return sync(ctx);
}

// Diagnostic of the pair above: the count phase's mark per query, which kernels stood in front, and the grid they ran on.
// Copies only; no kernel is launched.
WTP_API int wtp_radius_marks(wtp_ctx* ctx, uint8_t* marks_out, int64_t cap, double* info_out) {
    if (!ctx) return WTP_ERR_ARG;
    if (!ctx->rad_valid) return fail(ctx, WTP_ERR_STATE, "wtp_radius_marks needs a preceding wtp_radius_count");
    if (!info_out) return fail(ctx, WTP_ERR_ARG, "info_out is NULL");
    const int64_t n = ctx->rad_n;
    if (marks_out && cap < n) return fail(ctx, WTP_ERR_ARG, "marks_out holds fewer than n marks (info_out[12] of a call with marks_out = NULL)");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if (marks_out && n > 0) WTP_HIP(ctx, hipMemcpyAsync(marks_out, ctx->rad_done.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return by_dtype(ctx->rad_dtype, [&](auto t) {
        using T = decltype(t);
        Grid<T> g;
        unsigned long long taken = 0;
        WTP_HIP(ctx, hipMemcpyAsync(&g, ctx->grid.p, sizeof(g), hipMemcpyDeviceToHost, ctx->stream));
        WTP_HIP(ctx, hipMemcpyAsync(&taken, ctx->rad_pos.p, sizeof(taken), hipMemcpyDeviceToHost, ctx->stream));
        int rc = sync(ctx);
        if (rc) return rc;
        info_out[0] = ctx->rad_dense_used ? 1 : 0;
        info_out[1] = g.rad_wave_only;
        info_out[2] = radius_dense_hcap<T>();
        for (int a = 0; a < 3; ++a) {
            info_out[3 + a] = g.n[a];
            info_out[7 + a] = (double)g.org[a];
        }
        info_out[6] = (double)g.c;
        info_out[10] = (double)taken;
        info_out[11] = (double)((int64_t)kRadArenaPerPoint * n);
        info_out[12] = (double)n;
        return (int)WTP_OK;
    });
}

// ---- the sharded topology's local searches (wtp_block_topo.hip): the kernels of wtp_knn_dev / wtp_radius_* on the
// rank's gid-ordered local set, fp32 3-D, on the device; the caller has checked the context is idle
int wtp::topo_knn_local(wtp_ctx* ctx, const float* d_xyz, int64_t n, int k, int include_self, int32_t* d_idx, float* d_dist) {
    return knn_dev_t<float>(ctx, d_xyz, n, 3, k, include_self, d_idx, d_dist);
}

int wtp::topo_radius_local(wtp_ctx* ctx, const float* d_xyz, int64_t n, double r, int32_t* d_counts, int64_t* d_off,
                           DevBuf& d_idx, int64_t* nnz) {
    int rc;
    ctx->rad_valid = false; // (wtp_radius_fill has nothing to continue from: the rows go to the caller's buffers)
    ctx->rad_offsets_dev = false;
    ctx->relax.have_tree = false;
    if ((rc = ensure(ctx, ctx->raw_in, sizeof(float) * 3 * (size_t)n))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->raw_in.p, d_xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = radius_count_t<float>(ctx, n, 3, r, d_counts))) return rc;
    if ((rc = ensure(ctx, ctx->scratch, offsets_scan_tmp_bytes(n)))) return rc;
    if ((rc = launch_offsets_scan(ctx, d_counts, n, (int64_t*)ctx->scratch.p, d_off))) return rc;
    if ((rc = ensure_pinned(ctx, 64))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, d_off + n, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    *nnz = *(const int64_t*)ctx->host_pinned;
    if ((rc = ensure(ctx, d_idx, sizeof(int32_t) * (size_t)(*nnz + 1)))) return rc;
    if ((rc = ensure(ctx, ctx->fb2_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb2_count, 64))) return rc;
    ctx->rad_n = n;
    ctx->rad_dim = 3;
    ctx->rad_dtype = WTP_F32;
    ctx->rad_r = r;
    return radius_fill_t<float>(ctx, d_off, (int32_t*)d_idx.p);
}

// ---- variable spacings: kd-tree over the law's boundary points, cached per context -----------------
static bool spacing_on_device(int kind) { return kind == WTP_SPACING_LOGLIKE || kind == WTP_SPACING_BOUNDARY_LAYER; }

static int check_spacing_law(wtp_ctx* ctx, const wtp_spacing_desc* s) {
    if (!s->boundary_xyz || s->n_boundary < 1)
        return fail(ctx, WTP_ERR_ARG, "boundary_points must be non-empty"); // spacings.jl:61-62,106-107
    if (s->n_boundary > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "n_boundary exceeds the int32 index space");
    if (s->kind == WTP_SPACING_BOUNDARY_LAYER && !(s->p2 > 0))
        return fail(ctx, WTP_ERR_ARG, "layer_thickness must be positive"); // spacings.jl:108-109
    return WTP_OK;
}

static int ensure_kd(wtp_ctx* ctx, const wtp_spacing_desc* s, int dim, int dtype) {
    const size_t ts = tsize(dtype);
    const size_t bytes = ts * (size_t)s->n_boundary * dim;
    uint64_t h = 1469598103934665603ull; // FNV-1a over the coordinates: same boundary -> same tree
    const unsigned char* b = (const unsigned char*)s->boundary_xyz;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    if (ctx->kd_m == s->n_boundary && ctx->kd_key == h && ctx->kd_dim == dim && ctx->kd_dtype == dtype) return WTP_OK;
    const size_t kdsz = by_dtype(dtype, [&](auto t) { return kd_bytes<decltype(t)>(s->n_boundary); });
    int rc;
    if ((rc = ensure(ctx, ctx->kd_nodes, kdsz))) return rc;
    std::vector<char> host(kdsz);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        kd_build_host<T>((const T*)s->boundary_xyz, s->n_boundary, dim, host.data());
    });
    WTP_HIP(ctx, hipMemcpyAsync(ctx->kd_nodes.p, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = sync(ctx))) return rc; // `host` dies with this scope
    ctx->kd_m = s->n_boundary;
    ctx->kd_key = h;
    ctx->kd_dim = dim;
    ctx->kd_dtype = dtype;
    return WTP_OK;
}

// upper bound of a law's values (sizes the compact-support grid; need not be attained)
static double spacing_law_max(const wtp_spacing_desc* s) {
    if (s->kind == WTP_SPACING_LOGLIKE) return s->p0;
    return s->p0 > s->p1 ? s->p0 : s->p1;
}

// ---- repel ------------------------------------------------------------------------------------------
static int flush_pending(wtp_ctx* ctx); // defined with wtp_relax_set_fixed_dev

static int pick_free(const RelaxState& r, int avoid_a, int avoid_b) {
    for (int i = 0; i < 3; ++i)
        if (i != avoid_a && i != avoid_b) return i;
    (void)r;
    return 0;
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
    ctx->rad_valid = false;
    for (int i = 0; i < 2; ++i)
        if ((rc = ensure(ctx, ctx->pts[i], pt_size(dtype) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->raw_in, ts * (size_t)n * dim))) return rc;
    if ((rc = ensure(ctx, ctx->forces, ts * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->nn_dist, ts * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->nn_id, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_count, 64))) return rc;
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
            return launch_spacing_session<T>(ctx, pts_of<T>(ctx, 0), n, 0, ctx->kd_nodes.p, ctx->kd_m, spacing->kind,
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

// Brick geometry of the round-2 compact-support sweep (wtp_cs2.hip), from a census of the grid just built:
// the brick length BX is set so that 97 % of the non-empty bricks hold at most ~244 queries (one round of
// the 256-thread workgroup) and the LDS point area so that 99.9 % of the halos fit; the rest takes a second
// round / the exact path.  Two or three tiny launches and read-backs, once per session.
static int cs2_tune(wtp_ctx* ctx, RelaxState& r, const Grid<float>& hg, double rho_eff) {
    int rc;
    if ((rc = ensure(ctx, ctx->occ, 513 * sizeof(unsigned int)))) return rc;
    if ((rc = ensure_pinned(ctx, 16384))) return rc;
    const double cells = (double)hg.n[0] * hg.n[1] * hg.n[2];
    double rho_est = cells > 0 ? (double)r.n / cells : 1.0;
    if (rho_eff - 1.0 > rho_est) rho_est = rho_eff - 1.0;
    if (rho_est < 0.25) rho_est = 0.25;
    const int bx_max = hg.n[0] < cs2_max_bx() ? (hg.n[0] < 1 ? 1 : hg.n[0]) : cs2_max_bx();
    auto clampbx = [&](double v) {
        int b = (int)(v + 0.5);
        return b < 2 ? (bx_max < 2 ? bx_max : 2) : (b > bx_max ? bx_max : b);
    };
    r.cs2_rho = rho_est;
    int bx = clampbx(220.0 / (4.0 * rho_est));
    int q97 = 0, h999 = 0;
    for (int it = 0; it < 4; ++it) {
        if ((rc = launch_cs2_census(ctx, bx, (unsigned int*)ctx->occ.p))) return rc;
        WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, ctx->occ.p, 513 * sizeof(unsigned int), hipMemcpyDeviceToHost,
                                    ctx->stream));
        if ((rc = sync(ctx))) return rc;
        const unsigned int* h = (const unsigned int*)ctx->host_pinned;
        const double nb = (double)h[512];
        auto quant = [&](int base, double frac, int width) {
            double run = 0;
            for (int b = 0; b < 256; ++b) {
                run += h[base + b];
                if (run >= frac * nb) return (b + 1) * width;
            }
            return 256 * width;
        };
        q97 = nb > 0 ? quant(0, 0.97, 2) : 0;
        h999 = nb > 0 ? quant(256, 0.999, 8) : 0;
        if (nb <= 0) break;
        // queries: aim at 236 for the 97th percentile; halo: at most ~1060 points (four workgroups per CU)
        double f = 1.0;
        if (q97 > 248 || q97 < 216) f = 236.0 / (double)q97;
        if (h999 * f > 1060.0) f = 1060.0 / (double)h999;
        const int nbx = clampbx(bx * f);
        if (nbx == bx || it == 3) break;
        bx = nbx;
    }
    // equal bricks along x: n[0] = 214 cells cut into bricks of 51 leaves a fifth brick of 10 cells that pays the
    // whole per-brick setup for a fifth of the work.  Cut the row into equal parts instead — as few as the two
    // limits (one round of the workgroup for 97 % of the bricks, the LDS point area) allow.
    if (hg.n[0] > bx && q97 > 0) {
        int best = 0;
        for (int parts = hg.n[0] / bx > 1 ? hg.n[0] / bx : 1; parts <= (hg.n[0] + bx - 1) / bx; ++parts) {
            const int bxc = (hg.n[0] + parts - 1) / parts;
            if (bxc > bx_max) continue;
            const double grow = (double)bxc / (double)bx;
            if (q97 * grow <= 254.0 && h999 * grow <= 1100.0) {
                best = bxc;
                h999 = (int)(h999 * grow) + 1;
                break; // the fewest parts that fit
            }
        }
        if (!best) {
            const int parts = (hg.n[0] + bx - 1) / bx;
            best = (hg.n[0] + parts - 1) / parts;
        }
        bx = best;
    }
    int hc = (int)(h999 * 1.05) + 48;
    hc = (hc + 63) / 64 * 64;
    r.brick_hcap = hc < 256 ? 256 : (hc > 1920 ? 1920 : hc);
    r.cs2_bx = bx;
    if (ctx->debug)
        fprintf(stderr, "[wtp] cs2 geometry: BX=%d hcap=%d (q97=%d h999=%d rho_est=%.3f grid %dx%dx%d c=%g)\n", bx,
                r.brick_hcap, q97, h999, rho_est, hg.n[0], hg.n[1], hg.n[2], (double)hg.c);
    return WTP_OK;
}

// The session's grid, cell table and box trade places with the float copy's (relax_f64_ksel_sweep): what the float copy
// builds and measures — a quantile box among it, in its own coordinates — stays in its own buffers.
static void swap_float_copy_grid(wtp_ctx* ctx) {
    std::swap(ctx->grid, ctx->grid_b);
    std::swap(ctx->cell_start, ctx->cell_start_b);
    std::swap(ctx->box_dev, ctx->box_b);
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
    if ((rc = ensure(ctx, ctx->f64k_s64, sizeof(double4) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->f64k_slot, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->f64k_lists, sizeof(int32_t) * 2 * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->f64k_cnt, 64))) return rc;
    const double4* snap = (const double4*)a.snap; // the sorted snapshot (fresh: the queries are its points)
    SearchArgs<float> b{};
    b.fb_list = (int32_t*)ctx->f64k_lists.p;
    b.fb_count = (int32_t*)ctx->f64k_cnt.p;
    b.fb2_list = (int32_t*)ctx->f64k_lists.p + n;
    b.fb2_count = (int32_t*)ctx->f64k_cnt.p + 4;
    b.stop = ctx->stop_dev;
    b.diag = a.diag;
    *sp = span_begin(ctx, 0);
    WTP_HIP(ctx, hipMemsetAsync(ctx->f64k_cnt.p, 0, 64, ctx->stream));
    b.counters_cleared = 1;
    swap_float_copy_grid(ctx);
    const double* org4 = nullptr;
    rc = f64_candidates(ctx, snap, n, 3, kc, r.f64k_tune, b, *sp, &org4, [&](float4* sorted32) {
        return launch_relabel_slots(ctx, snap, sorted32, (double4*)ctx->f64k_s64.p, (int32_t*)ctx->f64k_slot.p, n);
    });
    // the session's structures again (the float copy's stay where they are until the next sweep overwrites them)
    swap_float_copy_grid(ctx);
    if (rc) return rc;
    return launch_refine_sweep_f64(ctx, a, (const double4*)ctx->f64k_s64.p, (const int32_t*)ctx->f64k_slot.p,
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
    ctx->n_sweep_launches += 1;
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
        rc = launch_spacing_session<T>(ctx, (const Pt<T>*)ctx->pts[r.bufP].p, r.n, r.n_fixed, ctx->kd_nodes.p, ctx->kd_m,
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
    a.fb_list = (int32_t*)ctx->fb_list.p;
    a.fb_count = (int32_t*)ctx->fb_count.p;
    a.fb2_list = (int32_t*)ctx->fb2_list.p;
    // one 64-byte counter block, cleared once per sweep: [0] hand-backs of the brick kernel,
    // [4] of the wave kernel, [8] uncovered queries
    a.fb2_count = (int32_t*)ctx->fb_count.p + 4;
    a.stop = ctx->stop_dev;
    a.nn_count = (int32_t*)ctx->fb_count.p + 2;
    const SweepRoute route = step_route(r, fresh);
    // the session's route keeps the ball kernel's list: supports wider than a cell, and every query of a stale snapshot
    const bool ball = route_ball(r.route) && (!fresh || r.spacing_kind != WTP_SPACING_CONSTANT);
    if (ball || route == SweepRoute::Cs2) {
        if ((rc = ensure(ctx, ctx->nn_list, sizeof(int32_t) * (size_t)r.n))) return rc;
        if (sizeof(T) == 4) a.nn_list = (int32_t*)ctx->nn_list.p; // wtp_cs2.hip: the follow-up kernel's list
        if (ball) { // the follow-up kernel has consumed the list by the time the ball kernel refills it
            a.ball_list = (int32_t*)ctx->nn_list.p;
            a.ball_count = (int32_t*)ctx->fb_count.p + 6;
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
    a.uncovered = (int32_t*)ctx->fb_count.p + 8;
    if (!ctx->counters_clean) WTP_HIP(ctx, hipMemsetAsync(ctx->fb_count.p, 0, 64, ctx->stream));
    ctx->counters_clean = false; // (set again by the step's final reduction, which zeroes the block after reading it)
    a.used_brick = a.used_wave = a.used_generic = 0;
    if ((rc = launch_sweep<T>(ctx, a, route, ball && route_ball(route)))) return rc;
    int sp = span_begin(ctx, 2);
    if (r.wall_active) { // p[id] = constrain(id, x_i, x_i + disp) (src/repel.jl:290): the octree wall rule
        char* wf = (char*)ctx->wall_flags.p;
        rc = launch_mesh_constrain<T>(ctx, a.query, a.out, r.n, r.n_fixed, r.wall_offset, (const uint8_t*)wf,
                                      (uint8_t*)wf + r.wall_nm, (int32_t*)ctx->wall_tri.p, (int32_t*)ctx->wall_hint.p,
                                      (int32_t*)ctx->fb_count.p + 12);
        if (rc) return rc;
    }
    rc = launch_reduce_partials(ctx, a.partials, a.n_partials, a.used_brick, a.used_wave, a.used_generic, a.fb_count,
                                a.uncovered, r.wall_active ? (const int32_t*)ctx->fb_count.p + 12 : nullptr, d_slot);
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

// After a sweep into ctx->stats: its statistics (none wanted: just the synchronisation) and the four layer totals of every
// axis a < n_axes that enqueue_layers was asked for (d_tot[a] != NULL; counts 0 otherwise), one read-back for all.
static int read_step(wtp_ctx* ctx, wtp_step_stats* stats, int n_axes = 0, int32_t* const* d_tot = nullptr,
                     int64_t* counts = nullptr) {
    if (!stats) return sync(ctx);
    const size_t off = (sizeof(wtp_step_stats) + 63) / 64 * 64;
    int rc;
    if ((rc = ensure_pinned(ctx, n_axes ? off + 64 * n_axes : sizeof(wtp_step_stats)))) return rc;
    char* h = (char*)ctx->host_pinned;
    WTP_HIP(ctx, hipMemcpyAsync(h, ctx->stats.p, sizeof(wtp_step_stats), hipMemcpyDeviceToHost, ctx->stream));
    for (int ax = 0; ax < n_axes; ++ax)
        if (d_tot[ax])
            WTP_HIP(ctx, hipMemcpyAsync(h + off + 64 * ax, d_tot[ax], 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    memcpy(stats, h, sizeof(wtp_step_stats));
    for (int ax = 0; ax < n_axes; ++ax)
        for (int j = 0; j < 4; ++j) counts[4 * ax + j] = d_tot[ax] ? ((const int32_t*)(h + off + 64 * ax))[j] : 0;
    return WTP_OK;
}

WTP_API int wtp_relax_step(wtp_ctx* ctx, int rebuild, wtp_step_stats* stats) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, ctx->stats, sizeof(wtp_step_stats)))) return rc;
    if ((rc = relax_step_any(ctx, rebuild, (wtp_step_stats*)ctx->stats.p))) return rc;
    return read_step(ctx, stats);
}

WTP_API int wtp_relax_run(wtp_ctx* ctx, int n_iters, int rebuild_every, double* conv_out, wtp_step_stats* last) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    if (rebuild_every < 1) return fail(ctx, WTP_ERR_ARG, "rebuild_every must be >= 1"); // src/repel.jl:74
    if (n_iters < 0) return fail(ctx, WTP_ERR_ARG, "n_iters must be >= 0");
    if (n_iters == 0) return WTP_OK;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, ctx->stats, sizeof(wtp_step_stats) * (size_t)n_iters))) return rc;
    wtp_step_stats* d = (wtp_step_stats*)ctx->stats.p;
    for (int i = 0; i < n_iters; ++i)
        if ((rc = relax_step_any(ctx, (i % rebuild_every) == 0, d + i))) return rc;
    if (conv_out || last) {
        if ((rc = ensure_pinned(ctx, sizeof(wtp_step_stats) * (size_t)n_iters))) return rc;
        WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, d, sizeof(wtp_step_stats) * (size_t)n_iters,
                                    hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
        const wtp_step_stats* h = (const wtp_step_stats*)ctx->host_pinned;
        if (conv_out)
            for (int i = 0; i < n_iters; ++i) conv_out[i] = h[i].max_force;
        if (last) *last = h[n_iters - 1];
        return WTP_OK;
    }
    return sync(ctx);
}

// ---- stop rules on the device (src/repel.jl:305-334) -----------------------------------------------------------
// After every sweep of a batch one thread applies the reference's rules, in the reference's order, to that sweep's
// statistics: cv_target (the caller then reverts p to p_old), the stall counter on the CV of d_NN / s, the tolerance
// on max |F| s.  Once a rule fires, every kernel of the later iterations of the batch that would touch the session's
// state returns at once (SearchArgs::stop / ctx->stop_dev), so the state is that of the stopping iteration.
struct StopState {
    int32_t stopped, reason, n_done, last_impr;
    double best_cv;
};
__global__ void stop_rules_kernel(const wtp_step_stats* __restrict__ st, StopState* __restrict__ s, int iter1, double tol,
                                  int stall_after, double cv_target) {
    if (s->stopped) return;
    s->n_done = iter1;
    const double conv = st->max_force;
    if ((stall_after > 0 || cv_target > 0) && st->n_move > 0) {
        const double n = (double)st->n_move, mu = st->sum_u / n;
        const double var = st->sum_u2 / n - mu * mu;
        const double cv = sqrt(var > 0.0 ? var : 0.0) / mu; // _dnn_cv, src/repel.jl:374-386
        if (cv_target > 0 && cv <= cv_target) {
            s->stopped = 1;
            s->reason = 2;
            return;
        }
        if (stall_after > 0) {
            if (cv < s->best_cv * (1 - 1.0e-3)) {
                s->best_cv = cv;
                s->last_impr = iter1;
            } else if (iter1 - s->last_impr >= stall_after) {
                s->stopped = 1;
                s->reason = 3;
                return;
            }
        }
    }
    if (conv < tol) {
        s->stopped = 1;
        s->reason = 1;
    }
}

WTP_API int wtp_relax_run_until(wtp_ctx* ctx, int max_iters, int rebuild_every, double tol, int stall_after,
                                double cv_target, double* conv_out, int* n_done_out, int* reason_out,
                                wtp_step_stats* last) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    RelaxState& r = ctx->relax;
    if (rebuild_every < 1) return fail(ctx, WTP_ERR_ARG, "rebuild_every must be >= 1"); // src/repel.jl:74
    if (max_iters < 0) return fail(ctx, WTP_ERR_ARG, "max_iters must be >= 0");
    if (r.wall_active) return fail(ctx, WTP_ERR_STATE, "wtp_relax_run_until: the octree wall rule steps through wtp_relax_step");
    if (n_done_out) *n_done_out = 0;
    if (reason_out) *reason_out = 0;
    if (max_iters == 0) return WTP_OK;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, ctx->stats, sizeof(wtp_step_stats) * (size_t)max_iters))) return rc;
    if ((rc = ensure(ctx, ctx->stop_state, 64))) return rc;
    if ((rc = ensure_pinned(ctx, 64 + sizeof(wtp_step_stats) * (size_t)max_iters))) return rc;
    StopState h0{};
    h0.best_cv = __builtin_huge_val(); // typemax(U), src/repel.jl:238
    memcpy(ctx->host_pinned, &h0, sizeof(h0));
    WTP_HIP(ctx, hipMemcpyAsync(ctx->stop_state.p, ctx->host_pinned, sizeof(h0), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = sync(ctx))) return rc; // (the pinned block is reused for the read-backs below)
    wtp_step_stats* d = (wtp_step_stats*)ctx->stats.p;
    StopState* ds = (StopState*)ctx->stop_state.p;
    const int kBatch = 16; // sweeps enqueued between two looks at the stop state
    std::vector<RelaxState> hist;
    hist.reserve((size_t)kBatch);
    int done = 0, reason = 0;
    ctx->stop_dev = &ds->stopped;
    for (int i0 = 0; i0 < max_iters && !reason; i0 += kBatch) {
        const int i1 = i0 + kBatch < max_iters ? i0 + kBatch : max_iters;
        hist.clear();
        for (int i = i0; i < i1; ++i) {
            if ((rc = relax_step_any(ctx, (i % rebuild_every) == 0, d + i))) {
                ctx->stop_dev = nullptr;
                return rc;
            }
            hist.push_back(r); // what the host believes after this sweep (buffer roles, grid age, ...)
            hipLaunchKernelGGL(stop_rules_kernel, dim3(1), dim3(1), 0, ctx->stream, d + i, ds, i + 1, tol, stall_after, cv_target);
        }
        WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, ds, sizeof(StopState), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) {
            ctx->stop_dev = nullptr;
            return rc;
        }
        StopState hs;
        memcpy(&hs, ctx->host_pinned, sizeof(hs));
        done = hs.n_done;
        if (hs.stopped) {
            reason = hs.reason;
            r = hist[(size_t)(done - 1 - i0)]; // the sweeps after the stop did nothing: forget that they were enqueued
        }
    }
    ctx->stop_dev = nullptr;
    if (reason == 2) { // cv_target: p .= p_old (src/repel.jl:314)
        if ((rc = wtp_relax_revert(ctx))) return rc;
    }
    if (conv_out || last) {
        WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, d, sizeof(wtp_step_stats) * (size_t)done, hipMemcpyDeviceToHost,
                                    ctx->stream));
        if ((rc = sync(ctx))) return rc;
        const wtp_step_stats* hst = (const wtp_step_stats*)ctx->host_pinned;
        if (conv_out)
            for (int i = 0; i < done; ++i) conv_out[i] = hst[i].max_force;
        if (last && done > 0) *last = hst[done - 1];
    }
    if (n_done_out) *n_done_out = done;
    if (reason_out) *reason_out = reason;
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

WTP_API int wtp_spacing_eval(wtp_ctx* ctx, const wtp_spacing_desc* spacing, const void* xyz, int64_t n, int dim,
                             int dtype, void* out) {
    int rc = check_cloud(ctx, xyz, n, dim, dtype);
    if (rc) return rc;
    if (!spacing || !out) return fail(ctx, WTP_ERR_ARG, "spacing/out is NULL");
    if (!spacing_on_device(spacing->kind))
        return fail(ctx, WTP_ERR_ARG, "wtp_spacing_eval evaluates LOGLIKE / BOUNDARY_LAYER descriptors");
    if ((rc = check_spacing_law(ctx, spacing))) return rc;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    if ((rc = ensure_kd(ctx, spacing, dim, dtype))) return rc;
    if ((rc = ensure(ctx, ctx->ins_in, ts * (size_t)n * dim))) return rc;
    if ((rc = ensure(ctx, ctx->ins_out, ts * (size_t)n))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->ins_in.p, xyz, ts * (size_t)n * dim, hipMemcpyHostToDevice, ctx->stream));
    rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_spacing_eval<T>(ctx, (const T*)ctx->ins_in.p, n, dim, ctx->kd_nodes.p, ctx->kd_m, spacing->kind,
                                      spacing->p0, spacing->p1, spacing->p2, (T*)ctx->ins_out.p);
    });
    if (rc) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(out, ctx->ins_out.p, ts * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_relax_end(wtp_ctx* ctx) {
    if (!ctx) return WTP_ERR_ARG;
    ctx->relax = RelaxState{};
    return WTP_OK;
}

// ---- isinside post-filter (src/repel.jl:90) ------------------------------------------------------------
static size_t align256(size_t b) { return (b + 255) / 256 * 256; }

WTP_API int wtp_isinside_greens(wtp_ctx* ctx, const void* test_xyz, int64_t n, const void* elem_xyz,
                                const void* elem_normal, const void* elem_area, int64_t m, int dtype,
                                uint8_t* inside_out, void* g_out) {
    if (!ctx) return WTP_ERR_ARG;
    if (dtype != WTP_F32 && dtype != WTP_F64) return fail(ctx, WTP_ERR_ARG, "dtype must be WTP_F32 or WTP_F64");
    if (n < 0 || m < 1) return fail(ctx, WTP_ERR_ARG, "need n >= 0 test points and m >= 1 boundary elements");
    if (n > 2000000000LL || m > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "n or m exceeds the int32 index space");
    if (n == 0) return WTP_OK;
    if (!test_xyz || !elem_xyz || !elem_normal || !elem_area || !inside_out)
        return fail(ctx, WTP_ERR_ARG, "NULL array");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    const int chunks = isinside_chunks(ctx, n, m, isinside_greens_ppb());
    // ins_in: [test n*3 | p m*3 | normal m*3 | area m]; ins_out: [g n | inside n]
    const size_t o_p = align256(ts * n * 3), o_n = o_p + align256(ts * m * 3), o_a = o_n + align256(ts * m * 3);
    int rc;
    if ((rc = ensure(ctx, ctx->ins_in, o_a + ts * m))) return rc;
    if ((rc = ensure(ctx, ctx->ins_elems, isinside_elem_bytes(dtype) * (size_t)m))) return rc;
    if ((rc = ensure(ctx, ctx->ins_partial, ts * (size_t)n * chunks))) return rc;
    if ((rc = ensure(ctx, ctx->ins_out, align256(ts * n) + (size_t)n))) return rc;
    char* in = (char*)ctx->ins_in.p;
    char* out = (char*)ctx->ins_out.p;
    WTP_HIP(ctx, hipMemcpyAsync(in, test_xyz, ts * n * 3, hipMemcpyHostToDevice, ctx->stream));
    WTP_HIP(ctx, hipMemcpyAsync(in + o_p, elem_xyz, ts * m * 3, hipMemcpyHostToDevice, ctx->stream));
    WTP_HIP(ctx, hipMemcpyAsync(in + o_n, elem_normal, ts * m * 3, hipMemcpyHostToDevice, ctx->stream));
    WTP_HIP(ctx, hipMemcpyAsync(in + o_a, elem_area, ts * m, hipMemcpyHostToDevice, ctx->stream));
    uint8_t* d_inside = (uint8_t*)(out + align256(ts * n));
    int sp = span_begin(ctx, 2);
    rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_isinside_greens<T>(ctx, (const T*)in, n, (const T*)(in + o_p), (const T*)(in + o_n), (const T*)(in + o_a),
                                         m, ctx->ins_elems.p, chunks, (T*)ctx->ins_partial.p, (T*)out, d_inside);
    });
    span_end(ctx, sp);
    if (rc) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(inside_out, d_inside, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (g_out) WTP_HIP(ctx, hipMemcpyAsync(g_out, out, ts * n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_isinside_winding(wtp_ctx* ctx, const void* test_xy, int64_t n, const void* poly_xy, int64_t m,
                                 int dtype, uint8_t* inside_out, void* sum_out) {
    if (!ctx) return WTP_ERR_ARG;
    if (dtype != WTP_F32 && dtype != WTP_F64) return fail(ctx, WTP_ERR_ARG, "dtype must be WTP_F32 or WTP_F64");
    if (m < 3) return fail(ctx, WTP_ERR_ARG, "need at least 3 points to define a polygon"); // src/isinside.jl:38-43
    if (n < 0 || n > 2000000000LL || m > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "bad n or m");
    if (n == 0) return WTP_OK;
    if (!test_xy || !poly_xy || !inside_out) return fail(ctx, WTP_ERR_ARG, "NULL array");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    const int chunks = isinside_chunks(ctx, n, m, isinside_winding_ppb());
    const size_t o_p = align256(ts * n * 2);
    int rc;
    if ((rc = ensure(ctx, ctx->ins_in, o_p + ts * m * 2))) return rc;
    if ((rc = ensure(ctx, ctx->ins_partial, ts * (size_t)n * chunks))) return rc;
    if ((rc = ensure(ctx, ctx->ins_elems, sizeof(int32_t) * (size_t)n))) return rc; // coincidence flags
    if ((rc = ensure(ctx, ctx->ins_out, align256(ts * n) + (size_t)n))) return rc;
    char* in = (char*)ctx->ins_in.p;
    char* out = (char*)ctx->ins_out.p;
    WTP_HIP(ctx, hipMemcpyAsync(in, test_xy, ts * n * 2, hipMemcpyHostToDevice, ctx->stream));
    WTP_HIP(ctx, hipMemcpyAsync(in + o_p, poly_xy, ts * m * 2, hipMemcpyHostToDevice, ctx->stream));
    uint8_t* d_inside = (uint8_t*)(out + align256(ts * n));
    rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_isinside_winding<T>(ctx, (const T*)in, n, (const T*)(in + o_p), m, chunks, (T*)ctx->ins_partial.p,
                                          (int32_t*)ctx->ins_elems.p, (T*)out, d_inside);
    });
    if (rc) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(inside_out, d_inside, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (sum_out) WTP_HIP(ctx, hipMemcpyAsync(sum_out, out, ts * n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

// ---- sharded sessions ---------------------------------------------------------------------------------
WTP_API int wtp_set_stream(wtp_ctx* ctx, void* hip_stream, int external) {
    if (!ctx) return WTP_ERR_ARG;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    spans_collect(ctx); // events of open spans belong to the old stream
    WTP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = external ? (hipStream_t)hip_stream : ctx->own_stream;
    return WTP_OK;
}

// launches the two layer kernels on the current P; *d_tot_out = device address of the four counts
static int enqueue_layers(wtp_ctx* ctx, int axis, double lo_in, double hi_in, double lo_out, double hi_out, void* d_lo4,
                          void* d_hi4, int64_t cap, int32_t** d_tot_out, int slot = 0) {
    RelaxState& r = ctx->relax;
    if (axis < 0 || axis >= r.dim) return fail(ctx, WTP_ERR_ARG, "axis must be in [0, dim)");
    if (cap < 0 || (cap > 0 && (!d_lo4 || !d_hi4))) return fail(ctx, WTP_ERR_ARG, "layer buffers are NULL");
    if (int rcf = flush_pending(ctx)) return rcf;
    int rc;
    const int nblk = layer_blocks(r.n);
    // (three regions: wtp_relax_step_layers3 keeps the layers of all three axes in flight)
    const size_t region = (64 + sizeof(int2) * (size_t)nblk + 63) / 64 * 64;
    if ((rc = ensure(ctx, ctx->scratch, 3 * region))) return rc;
    int32_t* d_tot = (int32_t*)((char*)ctx->scratch.p + (size_t)slot * region);
    int2* d_blk = (int2*)((char*)d_tot + 64);
    // P is in the slot order of the last rebuild's grid (and nobody moved farther than one spacing,
    // src/repel.jl:286-289) whenever a sweep produced it: then only the boundary cell layers are scanned
    const bool slot_ordered = r.have_tree && r.have_point_data && axis == r.dim - 1 && r.bufP != r.bufS &&
                              !r.moved_by_hand;
    const double reach = 1.001 * r.spacing_max * (double)(r.sweeps_since_rebuild > 0 ? r.sweeps_since_rebuild : 1);
    rc = by_dtype(r.dtype, [&](auto t) {
        using T = decltype(t);
        return launch_layers<T>(ctx, pts_of<T>(ctx, r.bufP), r.n, r.n_fixed, axis, lo_in, hi_in, lo_out, hi_out, (Pt<T>*)d_lo4,
                                (Pt<T>*)d_hi4, cap, d_blk, d_tot, slot_ordered, reach);
    });
    *d_tot_out = d_tot;
    return rc;
}

WTP_API int wtp_relax_layers_dev(wtp_ctx* ctx, int axis, double lo_in, double hi_in, double lo_out, double hi_out,
                                 void* d_lo4, void* d_hi4, int64_t cap, int64_t counts[4]) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    if (!counts) return fail(ctx, WTP_ERR_ARG, "counts is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    int32_t* d_tot = nullptr;
    if ((rc = enqueue_layers(ctx, axis, lo_in, hi_in, lo_out, hi_out, d_lo4, d_hi4, cap, &d_tot))) return rc;
    if ((rc = ensure_pinned(ctx, 64))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, d_tot, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    for (int j = 0; j < 4; ++j) counts[j] = ((const int32_t*)ctx->host_pinned)[j];
    return WTP_OK;
}

// One sweep and, from the positions it produced, the boundary layers of the NEXT iteration, with a
// single read-back and a single synchronisation for both (a sharded iteration otherwise pays two).
WTP_API int wtp_relax_step_layers(wtp_ctx* ctx, int rebuild, wtp_step_stats* stats, int axis, double lo_in, double hi_in,
                                  double lo_out, double hi_out, void* d_lo4, void* d_hi4, int64_t cap,
                                  int64_t counts[4]) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    if (!stats || !counts) return fail(ctx, WTP_ERR_ARG, "stats/counts is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, ctx->stats, sizeof(wtp_step_stats)))) return rc;
    if ((rc = relax_step_any(ctx, rebuild, (wtp_step_stats*)ctx->stats.p))) return rc;
    int32_t* d_tot = nullptr;
    if ((rc = enqueue_layers(ctx, axis, lo_in, hi_in, lo_out, hi_out, d_lo4, d_hi4, cap, &d_tot))) return rc;
    return read_step(ctx, stats, 1, &d_tot, counts);
}

// Materialise a pending input view (wtp_relax_set_fixed_dev below): stale fixed points dropped, the
// appended ones moved to the head, ids renumbered.  Every entry point that reads P calls this first;
// the usual consumer, the next rebuild, never needs it.
static int flush_pending(wtp_ctx* ctx) {
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

// wtp_relax_step_layers for a block decomposition: the layers of up to three axes (bit a of axes_mask) come home
// with the statistics, one read-back and one synchronisation for everything.  counts[4*a .. 4*a+3] as in
// wtp_relax_layers_dev; d_lo4[a] / d_hi4[a] each hold `cap` rows.
WTP_API int wtp_relax_step_layers3(wtp_ctx* ctx, int rebuild, wtp_step_stats* stats, int axes_mask, const double lo_in[3],
                                   const double hi_in[3], const double lo_out[3], const double hi_out[3], void* const d_lo4[3],
                                   void* const d_hi4[3], int64_t cap, int64_t counts[12]) {
    int rc = need_session(ctx, __func__);
    if (rc) return rc;
    if (!stats || !counts || !lo_in || !hi_in || !lo_out || !hi_out || !d_lo4 || !d_hi4)
        return fail(ctx, WTP_ERR_ARG, "NULL argument");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure(ctx, ctx->stats, sizeof(wtp_step_stats)))) return rc;
    if ((rc = relax_step_any(ctx, rebuild, (wtp_step_stats*)ctx->stats.p))) return rc;
    int32_t* d_tot[3] = {nullptr, nullptr, nullptr};
    for (int ax = 0; ax < 3; ++ax)
        if (axes_mask & (1 << ax))
            if ((rc = enqueue_layers(ctx, ax, lo_in[ax], hi_in[ax], lo_out[ax], hi_out[ax], d_lo4[ax], d_hi4[ax], cap,
                                     &d_tot[ax], ax)))
                return rc;
    return read_step(ctx, stats, 3, d_tot, counts);
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

WTP_API int wtp_timers_get(wtp_ctx* ctx, double out[4]) {
    if (!ctx || !out) return WTP_ERR_ARG;
    hipSetDevice(ctx->device);
    spans_collect(ctx);
    out[0] = ctx->t_hash;
    out[1] = ctx->t_sweep;
    out[2] = ctx->t_other;
    out[3] = (double)ctx->n_sweep_launches;
    return WTP_OK;
}

WTP_API int wtp_timers_reset(wtp_ctx* ctx) {
    if (!ctx) return WTP_ERR_ARG;
    hipSetDevice(ctx->device);
    spans_collect(ctx);
    ctx->t_hash = ctx->t_sweep = ctx->t_other = 0;
    ctx->n_sweep_launches = 0;
    if (!ctx->timing_forced) ctx->timing = true; // the caller is going to read the timers
    return WTP_OK;
}

// Diagnostic builds (-DWTP_DIAG): per-phase wave-cycle sums of the brick kernel, accumulated
// over all launches since the last call; reading resets them.  Release builds leave zeros.
WTP_API int wtp_debug_diag(wtp_ctx* ctx, unsigned long long out[16]) {
    if (!ctx || !out) return WTP_ERR_ARG;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = ensure(ctx, ctx->diag, 128))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(out, ctx->diag.p, 128, hipMemcpyDeviceToHost, ctx->stream));
    WTP_HIP(ctx, hipMemsetAsync(ctx->diag.p, 0, 128, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    if (ctx->debug_kd) { // diagnostic builds: node visits of the spacing law's tree walk
        unsigned long long kd[2] = {0, 0};
        wtp::debug_kd_steps(kd);
        fprintf(stderr, "[wtp] kd walk: %llu node visits by %llu wave-walks (%.1f per walk)\n", kd[0], kd[1], kd[1] ? (double)kd[0] / (double)kd[1] : 0.0);
    }
    return WTP_OK;
}

// ---- device-side helpers for bench.py / the sharded driver (not part of the drop-in surface) -----
WTP_API int wtp_gen_uniform_dev(wtp_ctx* ctx, uint64_t seed, int64_t first, int64_t n, int dim, int dtype, void* d_out) {
    if (!ctx || !d_out || n < 0) return WTP_ERR_ARG;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    int rc = dtype == WTP_F32 ? launch_gen_uniform<float>(ctx, seed, first, n, dim, (float*)d_out)
                              : launch_gen_uniform<double>(ctx, seed, first, n, dim, (double*)d_out);
    if (rc) return rc;
    return sync(ctx);
}

