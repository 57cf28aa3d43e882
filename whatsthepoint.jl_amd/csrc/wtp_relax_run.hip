// wtp_relax_run.hip — the calls that drive a relax session's steps: one step, a batch, a batch under the reference's
// stop rules (src/repel.jl:305-334) on the device, and a step whose boundary layers come home with its statistics.
#include <cmath>
#include <cstring>

#include "wtp_internal.hpp"

using namespace wtp;

#define WTP_API extern "C"

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
    if ((rc = relax_step_enqueue(ctx, rebuild, (wtp_step_stats*)ctx->stats.p))) return rc;
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
        if ((rc = relax_step_enqueue(ctx, (i % rebuild_every) == 0, d + i))) return rc;
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
// After every sweep of a batch one thread applies the reference's rules (stop_rules_apply, wtp_internal.hpp) to that
// sweep's statistics.  Once a rule fires, every kernel of the later iterations of the batch that would touch the session's
// state returns at once (SearchArgs::stop / ctx->stop_dev), so the state is that of the stopping iteration.
__global__ void stop_rules_kernel(const wtp_step_stats* __restrict__ st, StopState* __restrict__ s, int iter1, double tol,
                                  int stall_after, double cv_target) {
    stop_rules_apply(*s, *st, iter1, tol, stall_after, cv_target);
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
            if ((rc = relax_step_enqueue(ctx, (i % rebuild_every) == 0, d + i))) {
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
    if ((rc = relax_step_enqueue(ctx, rebuild, (wtp_step_stats*)ctx->stats.p))) return rc;
    int32_t* d_tot = nullptr;
    if ((rc = enqueue_layers(ctx, axis, lo_in, hi_in, lo_out, hi_out, d_lo4, d_hi4, cap, &d_tot))) return rc;
    return read_step(ctx, stats, 1, &d_tot, counts);
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
    if ((rc = relax_step_enqueue(ctx, rebuild, (wtp_step_stats*)ctx->stats.p))) return rc;
    int32_t* d_tot[3] = {nullptr, nullptr, nullptr};
    for (int ax = 0; ax < 3; ++ax)
        if (axes_mask & (1 << ax))
            if ((rc = enqueue_layers(ctx, ax, lo_in[ax], hi_in[ax], lo_out[ax], hi_out[ax], d_lo4[ax], d_hi4[ax], cap,
                                     &d_tot[ax], ax)))
                return rc;
    return read_step(ctx, stats, 3, d_tot, counts);
}
