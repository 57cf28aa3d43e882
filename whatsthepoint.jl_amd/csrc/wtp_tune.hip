// wtp_tune.hip — measured grid tuning: the cell edge the points (not the box) ask for, the brick geometry of the
// k-selection and compact-support sweeps, the cached tuning of the topology calls, and who owns the context's grid.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "wtp_internal.hpp"

namespace wtp {

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
int build_hash_tuned(wtp_ctx* ctx, GridTune& t, HashBuild<T> b, Grid<T>* hg_out, double* rho_eff_out) {
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
double ksel_rho_for(int kq) {
    const double rho = kRhoKsel * (double)kq / 22.0;
    return rho > 1.26 ? 1.26 : rho;
}
// points the first filter ball is expected to hold: k + self plus the same number of standard deviations as
// kCapKsel leaves at 22
double ksel_cap_count(int kq) {
    return (double)kq + (kCapKsel - 22.0) / std::sqrt(22.0) * std::sqrt((double)kq);
}

// The k-selection layout of build b on the grid just measured (hg, with rho_eff the occupancy its points see): the occupancy
// whose grid fills the bricks' lanes best — one more measured build when the pick moves t.rho by more than 1 % — and the
// brick geometry of the final grid, into t.
template <typename T>
int ksel_tune(wtp_ctx* ctx, GridTune& t, HashBuild<T> b, Grid<T>& hg, double& rho_eff) {
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
template <typename T> int build_grid_cached(wtp_ctx* ctx, GridTune& t, HashBuild<T> b, bool ksel) {
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
void init_search(SearchArgs<T>& a, const wtp_ctx* ctx, const Pt<T>* snap, const Pt<T>* query, int64_t n, int k,
                        int include_self) {
    a.grid = (const Grid<T>*)ctx->grid.p;
    a.snap = snap;
    a.query = query;
    a.cell_start = (const int32_t*)ctx->cell_start.p;
    a.n = (int32_t)n;
    a.k = k;
    a.include_self = include_self;
}

// Brick geometry of the round-2 compact-support sweep (wtp_cs2.hip), from a census of the grid just built:
// the brick length BX is set so that 97 % of the non-empty bricks hold at most ~244 queries (one round of
// the 256-thread workgroup) and the LDS point area so that 99.9 % of the halos fit; the rest takes a second
// round / the exact path.  Two or three tiny launches and read-backs, once per session.
int cs2_tune(wtp_ctx* ctx, RelaxState& r, const Grid<float>& hg, double rho_eff) {
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

// The context's grid, cell table and point buffers get a new owner: every call that builds a hash on ctx->grid says so
// here.  What the previous owner left behind is void: the radius pair's count phase (wtp_radius_fill then refuses) and
// the session's tree (the next step rebuilds).  A radius count marks itself valid again once it has finished.
void grid_taken(wtp_ctx* ctx) {
    ctx->rad.valid = false;
    ctx->relax.have_tree = false;
}

// explicit instantiations
#define INST(T)                                                                                         \
    template int build_hash_tuned<T>(wtp_ctx*, GridTune&, HashBuild<T>, Grid<T>*, double*);             \
    template int ksel_tune<T>(wtp_ctx*, GridTune&, HashBuild<T>, Grid<T>&, double&);                    \
    template int build_grid_cached<T>(wtp_ctx*, GridTune&, HashBuild<T>, bool);                         \
    template void init_search<T>(SearchArgs<T>&, const wtp_ctx*, const Pt<T>*, const Pt<T>*, int64_t, int, int);
INST(float)
INST(double)
#undef INST

} // namespace wtp
