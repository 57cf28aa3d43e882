// wtp_context.hip — the context behind the C ABI of include/wtp.h: lifecycle, error plumbing, the buffer pool,
// timing spans and the argument checks every entry point shares.
// No CPU fallback exists: without a usable gfx950 device wtp_create fails.
#include <cstdlib>

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
    if (ctx->timers.ev_used == (int)ctx->timers.ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return -1;
        ctx->timers.ev_pool.push_back(e);
    }
    return ctx->timers.ev_used++;
}

// Spans of a step follow each other without a gap (hash | sweep | follow-ups | reduction | next hash ...), so the
// event that closes one opens the next: one record per span instead of two (an event record costs ~4 us of stream
// time; eight per step were a third of a 50 k-point step).  Work enqueued between two spans counts for the later one.
int span_begin(wtp_ctx* ctx, int kind) {
    if (!ctx->timers.timing) return -1;
    if (ctx->timers.spans.size() > 8192) spans_collect(ctx); // bounded pool; costs one sync
    int a = ctx->timers.ev_last_end;
    if (a < 0) {
        a = take_event(ctx);
        if (a < 0) return -1;
        hipEventRecord(ctx->timers.ev_pool[a], ctx->stream);
    }
    const int b = take_event(ctx);
    if (b < 0) return -1;
    ctx->timers.spans.push_back({a, b, kind});
    return (int)ctx->timers.spans.size() - 1;
}

void span_end(wtp_ctx* ctx, int span) {
    if (span < 0) return;
    hipEventRecord(ctx->timers.ev_pool[ctx->timers.spans[span].b], ctx->stream);
    ctx->timers.ev_last_end = ctx->timers.spans[span].b;
}

void spans_collect(wtp_ctx* ctx) {
    ctx->timers.ev_last_end = -1; // the pool is recycled below (and a caller that reads the timers has synchronised: a gap)
    if (ctx->timers.spans.empty()) return;
    hipStreamSynchronize(ctx->stream);
    for (auto& s : ctx->timers.spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->timers.ev_pool[s.a], ctx->timers.ev_pool[s.b]) == hipSuccess) {
            if (s.kind == 0) ctx->timers.t_hash += ms;
            else if (s.kind == 1) ctx->timers.t_sweep += ms;
            else ctx->timers.t_other += ms;
        }
    }
    ctx->timers.spans.clear();
    ctx->timers.ev_used = 0;
}

int sync(wtp_ctx* ctx) {
    ctx->timers.ev_last_end = -1; // the host waits here: whatever it does next is not part of a span
    ctx->n_syncs += 1;
    WTP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WTP_OK;
}

size_t tsize(int dtype) { return dtype == WTP_F64 ? 8 : 4; }
size_t pt_size(int dtype) { return by_dtype(dtype, [](auto t) { return sizeof(Pt<decltype(t)>); }); }

int need_session(wtp_ctx* ctx, const char* entry) {
    if (!ctx) return WTP_ERR_ARG;
    if (!ctx->relax.active) return fail(ctx, WTP_ERR_STATE, std::string(entry) + " before wtp_relax_init");
    return WTP_OK;
}

int check_cloud(wtp_ctx* ctx, const void* xyz, int64_t n, int dim, int dtype) {
    if (!ctx) return WTP_ERR_ARG;
    if (!xyz) return fail(ctx, WTP_ERR_ARG, "xyz is NULL");
    if (n < 1) return fail(ctx, WTP_ERR_ARG, "n must be >= 1");
    if (n > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "n exceeds the int32 index space");
    if (dim != 2 && dim != 3) return fail(ctx, WTP_ERR_ARG, "dim must be 2 or 3");
    if (dtype != WTP_F32 && dtype != WTP_F64) return fail(ctx, WTP_ERR_ARG, "dtype must be WTP_F32 or WTP_F64");
    return WTP_OK;
}

int check_idle(wtp_ctx* ctx) {
    if (ctx->relax.active)
        return fail(ctx, WTP_ERR_STATE,
                    "context holds a relax session (its buffers are live): call wtp_relax_end or use another context");
    return WTP_OK;
}

int check_k(wtp_ctx* ctx, int64_t n, int k, int include_self) {
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
        ctx->timers.timing = atoi(e) != 0;
        ctx->timers.timing_forced = true;
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
    for (auto e : ctx->timers.ev_pool) hipEventDestroy(e);
    if (ctx->ev_comm_a) hipEventDestroy(ctx->ev_comm_a);
    if (ctx->ev_comm_b) hipEventDestroy(ctx->ev_comm_b);
    if (ctx->comm_stream) hipStreamDestroy(ctx->comm_stream);
    hipStreamDestroy(ctx->own_stream);
    delete ctx; // (frees the device buffers)
    return WTP_OK;
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

WTP_API int wtp_timers_get(wtp_ctx* ctx, double out[4]) {
    if (!ctx || !out) return WTP_ERR_ARG;
    hipSetDevice(ctx->device);
    spans_collect(ctx);
    out[0] = ctx->timers.t_hash;
    out[1] = ctx->timers.t_sweep;
    out[2] = ctx->timers.t_other;
    out[3] = (double)ctx->timers.n_sweep_launches;
    return WTP_OK;
}

WTP_API int wtp_timers_reset(wtp_ctx* ctx) {
    if (!ctx) return WTP_ERR_ARG;
    hipSetDevice(ctx->device);
    spans_collect(ctx);
    ctx->timers.t_hash = ctx->timers.t_sweep = ctx->timers.t_other = 0;
    ctx->timers.n_sweep_launches = 0;
    if (!ctx->timers.timing_forced) ctx->timers.timing = true; // the caller is going to read the timers
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
