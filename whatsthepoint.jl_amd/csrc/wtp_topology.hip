// wtp_topology.hip — the topology calls of include/wtp.h: the call sequences that replace _build_knn_neighbors /
// _build_radius_neighbors (src/topology.jl:79-97) in fp32 and fp64, and the consumers of their rows.
#include <cmath>
#include <cstring>

#include "wtp_internal.hpp"

namespace wtp {

// ---- topology -----------------------------------------------------------------------------------
template <typename T>
static int knn_dev_t(wtp_ctx* ctx, const T* d_xyz, int64_t n, int dim, int k, int include_self,
                     int32_t* d_idx, T* d_dist) {
    int rc;
    if ((rc = ensure(ctx, ctx->pts[0], sizeof(Pt<T>) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->pts[1], sizeof(Pt<T>) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb_count, sizeof(StepCounters)))) return rc;
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
    StepCounters* counters = step_counters(ctx); // one block, cleared once
    a.fb_list = (int32_t*)ctx->fb_list.p;
    a.fb_count = &counters->brick_handbacks;
    a.fb2_list = (int32_t*)ctx->fb2_list.p;
    a.fb2_count = &counters->wave_handbacks;
    WTP_HIP(ctx, hipMemsetAsync(counters, 0, sizeof(StepCounters), ctx->stream));
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
    ctx->timers.n_sweep_launches += 1;
    grid_taken(ctx); // pts[] reused
    return rc;
}

// fp32 k-nearest candidates of a double4 cloud (knn_dev_f64, relax_f64_ksel_sweep; kernels in wtp_sweep64.hip): the cloud
// (w = its row) moved to its own origin (*org4_out) and rounded to float, hashed with the tuning cached in t, relabel(sorted32)
// run on the sorted float copy, then the kc nearest per query (self included) into cand_idx / cand_dist, on the x-slowest
// layout of wtp_ksel.hip where that applies (3-D, kc <= 24).  `b` comes with the caller's counter block; `sp`, the caller's
// hash span, is closed and the search span left open.
int f64_candidates(wtp_ctx* ctx, const double4* pts, int64_t n, int dim, int kc, GridTune& t, SearchArgs<float>& b,
                          int& sp, const double** org4_out, const std::function<int(float4*)>& relabel) {
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
    if ((rc = ensure(ctx, ctx->fb_count, sizeof(StepCounters)))) return rc;
    ctx->counters_clean = false; // (this call counts in the block; the next sweep clears it itself)
    if ((rc = ensure(ctx, ctx->fb2_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb2_count, 64))) return rc;
    double4* raw64 = (double4*)ctx->pts[0].p;
    int sp = span_begin(ctx, 0);
    if ((rc = load_points<double>(ctx, d_xyz, raw64, n, dim))) return rc;
    // k = 21 without self (kc = 24): search and re-ranking in slot order (see refine_f64_slots_kernel)
    const bool slots = kc == 24;
    double4* slot64 = (double4*)ctx->pts[1].p;
    StepCounters* counters = step_counters(ctx);
    SearchArgs<float> a{};
    a.fb_list = (int32_t*)ctx->fb_list.p;
    a.fb_count = &counters->brick_handbacks;
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
                                     (int32_t*)ctx->fb_list.p, &counters->brick_handbacks);
    else
        rc = launch_refine_f64(ctx, raw64, a.idx_out, a.dist_out, n, kc, k, include_self, org4, d_idx, d_dist,
                               (int32_t*)ctx->fb_list.p, &counters->brick_handbacks);
    span_end(ctx, sp);
    if (rc) return rc;
    ctx->timers.n_sweep_launches += 1;
    grid_taken(ctx);
    if ((rc = ensure_pinned(ctx, 64))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, &counters->brick_handbacks, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
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
        b.fb_count = &counters->brick_handbacks;
        b.fb2_list = (int32_t*)ctx->fb2_list.p;
        b.fb2_count = (int32_t*)ctx->fb2_count.p;
        if ((rc = launch_generic_topology<double>(ctx, b, false))) return rc;
    }
    *done = true;
    return WTP_OK;
}

} // namespace wtp

using namespace wtp;

#define WTP_API extern "C"

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

// ---- the metrics' reductions (wtp_stats.hip) ----------------------------------------------------
// has_spacing of a call's (h, h_const, coord_radius), or -1 with *why set
int wtp::knn_stats_spacing(const void* h, double h_const, double coord_radius, const char** why) {
    if (!h && (std::isnan(h_const) || (h_const > 0 && !std::isfinite(h_const)))) {
        *why = "h_const must be finite";
        return -1;
    }
    const int has = h || h_const > 0 ? 1 : 0;
    if (has && !(std::isfinite(coord_radius) && coord_radius >= 0)) {
        *why = "coord_radius must be finite and >= 0";
        return -1;
    }
    return has;
}

// n x k distance rows in device memory -> *out on the host; *bad_out: the first index whose spacing is not finite and > 0,
// or -1 (then *out is not meaningful: the caller reports it)
int wtp::knn_stats_rows(wtp_ctx* ctx, const void* d_dist, int64_t n, int k, int dtype, const double* d_h, double h_const,
                        int has_spacing, double coord_radius, const int64_t* d_gid, void* d_nn_out, double* d_mean_out,
                        KnnStats* out, int64_t* bad_out) {
    int rc;
    if ((rc = ensure(ctx, ctx->kstats, knn_stats_tmp_bytes(n)))) return rc;
    if ((rc = ensure_pinned(ctx, 256))) return rc;
    const KnnStats* d_res = nullptr;
    const unsigned long long* d_bad = nullptr;
    int sp = span_begin(ctx, 2);
    rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_knn_stats<T>(ctx, (const T*)d_dist, n, k, d_h, h_const, has_spacing, coord_radius, d_gid, (T*)d_nn_out,
                                   d_mean_out, ctx->kstats.p, &d_res, &d_bad);
    });
    span_end(ctx, sp);
    if (rc) return rc;
    // (the result and the index behind it are adjacent: one copy)
    WTP_HIP(ctx, hipMemcpyAsync(ctx->host_pinned, d_res, sizeof(KnnStats) + 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    memcpy(out, ctx->host_pinned, sizeof(KnnStats));
    unsigned long long bad;
    memcpy(&bad, (const char*)ctx->host_pinned + sizeof(KnnStats), 8);
    *bad_out = bad == ~0ull ? -1 : (int64_t)bad;
    return WTP_OK;
}

static int knn_stats_call(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, const double* h, double h_const,
                          double coord_radius, KnnStats* out, void* nn_out, double* mean_out, bool dev) {
    int rc = check_cloud(ctx, xyz, n, dim, dtype);
    if (rc) return rc;
    if (k < 2) return fail(ctx, WTP_ERR_ARG, "k must be >= 2 (k counts the point itself: a row needs one neighbour)");
    if ((rc = check_k(ctx, n, k, 1))) return rc;
    if ((rc = check_idle(ctx))) return rc;
    if (!out) return fail(ctx, WTP_ERR_ARG, "out is NULL");
    const char* why = nullptr;
    const int has = knn_stats_spacing(h, h_const, coord_radius, &why);
    if (has < 0) return fail(ctx, WTP_ERR_ARG, why);
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    if (dev) {
        if ((rc = ensure(ctx, ctx->idx_out, sizeof(int32_t) * (size_t)n * k))) return rc;
        if ((rc = ensure(ctx, ctx->dist_out, ts * (size_t)n * k))) return rc;
        rc = knn_on_device(ctx, xyz, n, dim, dtype, k, 1, (int32_t*)ctx->idx_out.p, ctx->dist_out.p);
    } else {
        rc = knn_rows_on_device(ctx, xyz, n, dim, dtype, k, 1, true);
    }
    if (rc) return rc;
    const double* d_h = h;
    void* d_nn = nn_out;
    double* d_mean = mean_out;
    if (!dev) { // staging of the host arrays: [h | mean | nn]
        const size_t o1 = sizeof(double) * (size_t)n;
        if ((rc = ensure(ctx, ctx->scratch, 2 * o1 + ts * (size_t)n))) return rc;
        char* b = (char*)ctx->scratch.p;
        if (h) WTP_HIP(ctx, hipMemcpyAsync(b, h, o1, hipMemcpyHostToDevice, ctx->stream));
        d_h = h ? (const double*)b : nullptr;
        d_mean = mean_out ? (double*)(b + o1) : nullptr;
        d_nn = nn_out ? b + 2 * o1 : nullptr;
    }
    int64_t bad = -1;
    if ((rc = knn_stats_rows(ctx, ctx->dist_out.p, n, k, dtype, d_h, h_const, has, coord_radius, nullptr, d_nn, d_mean, out, &bad)))
        return rc;
    if (bad >= 0) return fail(ctx, WTP_ERR_ARG, "h[" + std::to_string(bad) + "] is not finite and > 0");
    if (!dev && (nn_out || mean_out)) {
        if (nn_out) WTP_HIP(ctx, hipMemcpyAsync(nn_out, d_nn, ts * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        if (mean_out) WTP_HIP(ctx, hipMemcpyAsync(mean_out, d_mean, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        return sync(ctx);
    }
    return WTP_OK;
}

WTP_API int wtp_knn_stats(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, const double* h, double h_const,
                          double coord_radius, KnnStats* out, void* nn_out, double* mean_out) {
    return knn_stats_call(ctx, xyz, n, dim, dtype, k, h, h_const, coord_radius, out, nn_out, mean_out, false);
}

WTP_API int wtp_knn_stats_dev(wtp_ctx* ctx, const void* d_xyz, int64_t n, int dim, int dtype, int k, const double* d_h,
                              double h_const, double coord_radius, KnnStats* out, void* d_nn_out, double* d_mean_out) {
    return knn_stats_call(ctx, d_xyz, n, dim, dtype, k, d_h, h_const, coord_radius, out, d_nn_out, d_mean_out, true);
}

// ---- the graph part of orient_normals! / split_surface! (wtp_normal_graph.hip) ---------------------
// orient != 0: wtp_orient_normals (normals changed in place, mst_out or NULL); else wtp_normal_components (label_out)
static int normal_graph_call(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, void* normals, int32_t* mst_out,
                             double angle, int32_t* label_out, wtp_normal_graph_info* info, bool orient, bool dev) {
    int rc = check_cloud(ctx, xyz, n, dim, dtype);
    if (rc) return rc;
    if ((rc = check_k(ctx, n, k, 1))) return rc;
    if ((rc = check_idle(ctx))) return rc;
    if (!normals) return fail(ctx, WTP_ERR_ARG, "normals is NULL");
    if (!orient && !label_out) return fail(ctx, WTP_ERR_ARG, "label_out is NULL");
    if (!orient && std::isnan(angle)) return fail(ctx, WTP_ERR_ARG, "angle is NaN");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(dtype);
    if (dev) {
        if ((rc = ensure(ctx, ctx->idx_out, sizeof(int32_t) * (size_t)n * k))) return rc;
        rc = knn_on_device(ctx, xyz, n, dim, dtype, k, 1, (int32_t*)ctx->idx_out.p, nullptr);
    } else {
        rc = knn_rows_on_device(ctx, xyz, n, dim, dtype, k, 1, false);
    }
    if (rc) return rc;
    const int64_t syncs0 = ctx->n_syncs; // (the graph part's: the search's own are not counted)
    const void* d_xyz = dev ? xyz : ctx->raw_in.p;
    const int32_t* d_rows = (const int32_t*)ctx->idx_out.p;
    // staging of the host arrays: [normals | mst or labels]
    const size_t nb = (ts * (size_t)n * dim + 255) / 256 * 256;
    const size_t ob = orient ? sizeof(int32_t) * 2 * (size_t)(n - 1) : sizeof(int32_t) * (size_t)n;
    void* d_nrm = normals;
    int32_t* d_out = orient ? mst_out : label_out;
    if (!dev) {
        if ((rc = ensure(ctx, ctx->scratch, nb + ob))) return rc;
        d_nrm = ctx->scratch.p;
        d_out = (orient && !mst_out) ? nullptr : (int32_t*)((char*)ctx->scratch.p + nb);
        WTP_HIP(ctx, hipMemcpyAsync(d_nrm, normals, ts * (size_t)n * dim, hipMemcpyHostToDevice, ctx->stream));
    }
    // [control block | components x 2 | per-component minima x 2 | kept entries (split)]
    const size_t cb = normal_graph_ctl_bytes();
    const size_t vb = (sizeof(uint32_t) * (size_t)n + 255) / 256 * 256, mb = sizeof(unsigned long long) * (size_t)n;
    if ((rc = ensure(ctx, ctx->ngraph, cb + 2 * vb + 2 * mb + (orient ? 0 : (size_t)n * (k - 1))))) return rc;
    char* g = (char*)ctx->ngraph.p;
    unsigned long long* d_ctl = (unsigned long long*)g;
    uint32_t* bufs[2] = {(uint32_t*)(g + cb), (uint32_t*)(g + cb + vb)};
    unsigned long long* d_best_w = (unsigned long long*)(g + cb + 2 * vb);
    unsigned long long* d_best_e = d_best_w + n;
    uint8_t* d_keep = (uint8_t*)(d_best_e + n);
    if ((rc = ensure_pinned(ctx, cb))) return rc;
    unsigned long long* h = (unsigned long long*)ctx->host_pinned;
    int sp = span_begin(ctx, 2);
    rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_normal_graph_prep<T>(ctx, (const T*)d_xyz, (const T*)d_nrm, d_rows, n, dim, k, orient, angle, bufs[0], d_keep,
                                           d_ctl);
    });
    if (rc) return rc;
    int enq = 0; // rounds enqueued
    h[0] = k > 1 ? 0 : 1;
    while (!h[0]) { // batches: one read-back per 4 rounds
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return launch_normal_graph_rounds<T>(ctx, (const T*)d_nrm, d_rows, n, dim, k, orient, d_keep, bufs[0], bufs[1], d_best_w,
                                                 d_best_e, orient ? d_out : nullptr, enq, 4, d_ctl);
        });
        if (rc) return rc;
        enq += 4;
        WTP_HIP(ctx, hipMemcpyAsync(h, d_ctl, 128, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
        if (h[4] != ~0ull) break;
    }
    if (k == 1) { // no rounds: the control block is read here for the normals' check
        WTP_HIP(ctx, hipMemcpyAsync(h, d_ctl, 128, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
    }
    if (h[4] != ~0ull) { // (found before anything was written)
        span_end(ctx, sp);
        return fail(ctx, WTP_ERR_ARG, "normals[" + std::to_string((long long)h[4]) + "] has a non-finite component");
    }
    rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_normal_graph_apply<T>(ctx, (T*)d_nrm, n, dim, bufs[enq & 1], orient ? nullptr : d_out, d_ctl);
    });
    span_end(ctx, sp);
    if (rc) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(h, d_ctl, 128, hipMemcpyDeviceToHost, ctx->stream));
    if (!dev) {
        if (orient) {
            WTP_HIP(ctx, hipMemcpyAsync(normals, d_nrm, ts * (size_t)n * dim, hipMemcpyDeviceToHost, ctx->stream));
            if (mst_out && n > 1)
                WTP_HIP(ctx, hipMemcpyAsync(mst_out, d_out, sizeof(int32_t) * 2 * (size_t)(n - 1), hipMemcpyDeviceToHost, ctx->stream));
        } else {
            WTP_HIP(ctx, hipMemcpyAsync(label_out, d_out, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    if ((rc = sync(ctx))) return rc;
    if (info) {
        info->n_edges = (int64_t)h[11];
        info->n_components = (int64_t)h[8];
        info->n_reached = orient ? (int64_t)h[9] : 0;
        info->n_flipped = orient ? (int64_t)h[10] : 0;
        info->start = orient ? (int64_t)h[6] : -1;
        info->rounds = (int32_t)h[1];
        info->host_syncs = (int32_t)(ctx->n_syncs - syncs0);
    }
    return WTP_OK;
}

WTP_API int wtp_orient_normals(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype, int k, void* normals_inout,
                               int32_t* mst_out, wtp_normal_graph_info* info) {
    return normal_graph_call(ctx, xyz, n, dim, dtype, k, normals_inout, mst_out, 0.0, nullptr, info, true, false);
}

WTP_API int wtp_orient_normals_dev(wtp_ctx* ctx, const void* d_xyz, int64_t n, int dim, int dtype, int k, void* d_normals_inout,
                                   int32_t* d_mst_out, wtp_normal_graph_info* info) {
    return normal_graph_call(ctx, d_xyz, n, dim, dtype, k, d_normals_inout, d_mst_out, 0.0, nullptr, info, true, true);
}

WTP_API int wtp_normal_components(wtp_ctx* ctx, const void* xyz, const void* normals, int64_t n, int dim, int dtype, int k,
                                  double angle, int32_t* label_out, wtp_normal_graph_info* info) {
    return normal_graph_call(ctx, xyz, n, dim, dtype, k, (void*)normals, nullptr, angle, label_out, info, false, false);
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
    if ((rc = ensure(ctx, ctx->fb_count, sizeof(StepCounters)))) return rc;
    ctx->counters_clean = false; // (this call counts in the block; the next sweep clears it itself)
    a.fb_list = (int32_t*)ctx->fb_list.p; // queries the brick kernel hands back to the wave kernel
    a.fb_count = &step_counters(ctx)->brick_handbacks;
    // fp32: the brick kernel parks the rows it finds (32 ids per query) and marks the query, so that wtp_radius_fill copies
    // them instead of running the whole search a second time (128 B per point of scratch)
    if ((rc = ensure(ctx, ctx->rad.done, (size_t)n + 64))) return rc;
    WTP_HIP(ctx, hipMemsetAsync(ctx->rad.done.p, 0, (size_t)n, ctx->stream));
    a.rad_done = (uint8_t*)ctx->rad.done.p;
    if (sizeof(T) == 4 && !ctx->force_generic) { // the brick kernel's rows: 32 ids per query
        if ((rc = ensure(ctx, ctx->rad.tmp, sizeof(int32_t) * 32 * (size_t)n))) return rc;
        a.rad_tmp = (int32_t*)ctx->rad.tmp.p;
    }
    // the wave kernel's rows (any length up to its list), where it serves every query (fp64; fp32 grids whose rows are
    // expected to outgrow the brick kernel, Grid::rad_wave_only; WTP_FORCE_GENERIC=1): an arena of 48 ids per point,
    // shared out evenly among the waves; a row that does not fit any more is simply searched again by the fill phase.
    // (For the hand-backs of the fp32 brick kernel it buys nothing: measured 2.07 -> 2.14 ms per graded 1 M cloud —
    // ranking in the count phase costs what it saves in the fill phase; the kernel decides by the grid's flag.)
    const int64_t arena_cap = (int64_t)kRadArenaPerPoint * n;
    if ((rc = ensure(ctx, ctx->rad.arena, sizeof(int32_t) * (size_t)arena_cap))) return rc;
    if ((rc = ensure(ctx, ctx->rad.arena_off, sizeof(int64_t) * (size_t)(n + 2)))) return rc;
    a.rad_arena = (int32_t*)ctx->rad.arena.p;
    a.rad_arena_off = (int64_t*)ctx->rad.arena_off.p;
    if ((rc = ensure(ctx, ctx->rad.pos, 64))) return rc;
    RadCursor* cursor = (RadCursor*)ctx->rad.pos.p;
    WTP_HIP(ctx, hipMemsetAsync(cursor, 0, sizeof(RadCursor), ctx->stream));
    if ((rc = ensure(ctx, ctx->rad.bricks, sizeof(int32_t) * (size_t)(n + 64)))) return rc;
    a.rad_bricks = (int32_t*)ctx->rad.bricks.p;
    a.rad_arena_pos = &cursor->arena_next; // the dense kernel takes pieces of the arena (wtp_radb.hip)
    a.rad_arena_cap = arena_cap;
    sp = span_begin(ctx, 1);
    rc = launch_radius_count<T>(ctx, a, (T)r, d_counts);
    ctx->rad.dense_used = a.rad_dense > 0;
    span_end(ctx, sp);
    if (!rc && a.rad_dense > 0 && ctx->debug) {
        RadCursor h{};
        WTP_HIP(ctx, hipMemcpyAsync(&h, cursor, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        WTP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "[wtp] radius, dense kernel: %d bricks, %d of %lld queries, %lld ids parked\n", h.bricks_listed,
                h.dense_queries, (long long)n, (long long)h.arena_next);
    }
    return rc;
}

template <typename T> static int radius_fill_t(wtp_ctx* ctx, const int64_t* d_off, int32_t* d_idx) {
    SearchArgs<T> a{};
    init_search(a, ctx, (const Pt<T>*)ctx->pts[1].p, (const Pt<T>*)ctx->pts[1].p, ctx->rad.n, 0, 0);
    a.fb2_list = (int32_t*)ctx->fb2_list.p;
    a.fb2_count = (int32_t*)ctx->fb2_count.p;
    a.fb_list = (int32_t*)ctx->fb_list.p; // ensured by the count phase
    a.fb_count = &step_counters(ctx)->brick_handbacks;
    // the rows the count phase of this very cloud parked (rad.valid guards the pair of calls)
    a.rad_tmp = sizeof(T) == 4 && !ctx->force_generic ? (int32_t*)ctx->rad.tmp.p : nullptr;
    a.rad_done = (uint8_t*)ctx->rad.done.p;
    a.rad_arena = (int32_t*)ctx->rad.arena.p;
    a.rad_arena_off = (int64_t*)ctx->rad.arena_off.p;
    a.rad_arena_cap = (int64_t)kRadArenaPerPoint * ctx->rad.n;
    a.rad_dense = ctx->rad.dense_used ? 1 : 0; // (the hand-back list of the count phase is what is left to search)
    int sp = span_begin(ctx, 1);
    int rc = launch_radius_fill<T>(ctx, a, (T)ctx->rad.r, d_off, d_idx);
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
    grid_taken(ctx);
    ctx->rad.offsets_dev = false;
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
    ctx->rad.n = n;
    ctx->rad.dim = dim;
    ctx->rad.dtype = dtype;
    ctx->rad.r = r;
    ctx->rad.valid = true;
    ctx->rad.offsets_dev = offsets;
    if (offsets) ctx->rad.nnz = ((const int64_t*)out)[n];
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
    if (!ctx->rad.valid) return fail(ctx, WTP_ERR_STATE, "wtp_radius_fill needs a preceding wtp_radius_count");
    if (!offsets && !ctx->rad.offsets_dev)
        return fail(ctx, WTP_ERR_ARG, "offsets is NULL (only wtp_radius_offsets leaves them on the device)");
    const int64_t n = ctx->rad.n;
    if (offsets) {
        if (offsets[0] != 0) return fail(ctx, WTP_ERR_ARG, "offsets[0] must be 0");
        for (int64_t i = 0; i < n; ++i)
            if (offsets[i + 1] < offsets[i]) return fail(ctx, WTP_ERR_ARG, "offsets must be non-decreasing");
    }
    const int64_t nnz = offsets ? offsets[n] : ctx->rad.nnz;
    if (nnz > 0 && !idx_out) return fail(ctx, WTP_ERR_ARG, "idx_out is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = tsize(ctx->rad.dtype);
    int rc;
    if ((rc = ensure(ctx, ctx->idx_out, sizeof(int32_t) * (size_t)(nnz + 1)))) return rc;
    if ((rc = ensure(ctx, ctx->scratch, ts * (size_t)(nnz + 1)))) return rc;
    if ((rc = ensure(ctx, ctx->dist_out, sizeof(int64_t) * (size_t)(n + 1)))) return rc; // offsets staging
    if ((rc = ensure(ctx, ctx->fb2_list, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->fb2_count, 64))) return rc;
    if (offsets)
        WTP_HIP(ctx, hipMemcpyAsync(ctx->dist_out.p, offsets, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice,
                                    ctx->stream));
    rc = by_dtype(ctx->rad.dtype,
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
    if (!ctx->rad.valid) return fail(ctx, WTP_ERR_STATE, "wtp_radius_marks needs a preceding wtp_radius_count");
    if (!info_out) return fail(ctx, WTP_ERR_ARG, "info_out is NULL");
    const int64_t n = ctx->rad.n;
    if (marks_out && cap < n) return fail(ctx, WTP_ERR_ARG, "marks_out holds fewer than n marks (info_out[12] of a call with marks_out = NULL)");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if (marks_out && n > 0) WTP_HIP(ctx, hipMemcpyAsync(marks_out, ctx->rad.done.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return by_dtype(ctx->rad.dtype, [&](auto t) {
        using T = decltype(t);
        Grid<T> g;
        unsigned long long taken = 0;
        WTP_HIP(ctx, hipMemcpyAsync(&g, ctx->grid.p, sizeof(g), hipMemcpyDeviceToHost, ctx->stream));
        WTP_HIP(ctx, hipMemcpyAsync(&taken, &((const RadCursor*)ctx->rad.pos.p)->arena_next, sizeof(taken), hipMemcpyDeviceToHost, ctx->stream));
        int rc = sync(ctx);
        if (rc) return rc;
        info_out[0] = ctx->rad.dense_used ? 1 : 0;
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
    grid_taken(ctx); // (and wtp_radius_fill gets nothing to continue from: the rows go to the caller's buffers)
    ctx->rad.offsets_dev = false;
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
    ctx->rad.n = n;
    ctx->rad.dim = 3;
    ctx->rad.dtype = WTP_F32;
    ctx->rad.r = r;
    return radius_fill_t<float>(ctx, d_off, (int32_t*)d_idx.p);
}
