// wtp_comm.hip — the context owns an RCCL communicator (multi-GPU behind the boundary).
//
// One process per GPU, one context per process.  The block decomposition of DESIGN.md §7b needs three things from
// the transport: a point-to-point round with the two neighbours along an axis (variable row counts), a reduction
// of the step's statistics, and somebody to carry the communicator id to the other ranks.  The first two live here,
// on the context's stream, so a caller without torch (the Julia side: INTEGRATION.md) drives the whole exchange
// through the C ABI; the id (128 bytes) travels by whatever the caller has (MPI.bcast, a file, an environment
// variable).  The Python host mirror keeps torch.distributed as its default transport and can be switched to this one
// (WTP_COMM=abi), which is how the entry points are exercised.
//
// librccl is opened at the first wtp_comm_* call (dlopen), not linked: a single-GPU user of libwtp never loads it.
//
// The block driver (wtp_block.hip) and the sharded topology (wtp_block_topo.hip) reach the other ranks
// through the context's Transport (wtp_internal.hpp), at the end of this file: the caller's host callbacks
// (wtp_block_set_transport) or this communicator, behind one readiness check, one all-gather and one grouped exchange.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <cstring>

#include "wtp_internal.hpp"

namespace wtp {

struct Rccl {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

static Rccl g_rccl;

static int rccl_load(wtp_ctx* ctx) {
    if (g_rccl.lib) return WTP_OK;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(ctx, WTP_ERR_STATE, "wtp_comm: librccl.so not found (dlopen)");
    Rccl r;
    r.lib = h;
#define WTP_SYM(name)                                                               \
    r.name = (decltype(r.name))dlsym(h, "nccl" #name);                              \
    if (!r.name) return fail(ctx, WTP_ERR_STATE, "wtp_comm: librccl lacks nccl" #name);
    WTP_SYM(GetUniqueId)
    WTP_SYM(CommInitRank)
    WTP_SYM(CommDestroy)
    WTP_SYM(GroupStart)
    WTP_SYM(GroupEnd)
    WTP_SYM(Send)
    WTP_SYM(Recv)
    WTP_SYM(AllReduce)
    WTP_SYM(AllGather)
    WTP_SYM(GetErrorString)
#undef WTP_SYM
    g_rccl = r;
    return WTP_OK;
}

#define WTP_NCCL(ctx, call)                                                     \
    do {                                                                        \
        ncclResult_t e_ = (call);                                               \
        if (e_ != ncclSuccess) return fail(ctx, WTP_ERR_HIP, g_rccl.GetErrorString(e_)); \
    } while (0)

static_assert(sizeof(ncclUniqueId) == WTP_COMM_ID_BYTES, "wtp.h promises 128 bytes");

} // namespace wtp

using namespace wtp;
#define WTP_API extern "C"

WTP_API int wtp_comm_unique_id(wtp_ctx* ctx, void* id_out) {
    if (!ctx || !id_out) return WTP_ERR_ARG;
    int rc;
    if ((rc = rccl_load(ctx))) return rc;
    ncclUniqueId id;
    WTP_NCCL(ctx, g_rccl.GetUniqueId(&id));
    memcpy(id_out, &id, sizeof(id));
    return WTP_OK;
}

WTP_API int wtp_comm_init(wtp_ctx* ctx, const void* id_in, int rank, int nranks) {
    if (!ctx || !id_in) return WTP_ERR_ARG;
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, WTP_ERR_ARG, "wtp_comm_init: 0 <= rank < nranks");
    if (ctx->comm) return fail(ctx, WTP_ERR_STATE, "wtp_comm_init: the context has a communicator already");
    int rc;
    if ((rc = rccl_load(ctx))) return rc;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    ncclUniqueId id;
    memcpy(&id, id_in, sizeof(id));
    ncclComm_t comm = nullptr;
    WTP_NCCL(ctx, g_rccl.CommInitRank(&comm, nranks, id, rank));
    ctx->comm = comm;
    ctx->comm_rank = rank;
    ctx->comm_size = nranks;
    if ((rc = ensure(ctx, ctx->comm_scratch, 256))) return rc; // counts out [0..1], counts in [2..3], statistics [8..]
    return WTP_OK;
}

WTP_API int wtp_comm_finalize(wtp_ctx* ctx) {
    if (!ctx) return WTP_ERR_ARG;
    if (!ctx->comm) return WTP_OK;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    g_rccl.CommDestroy((ncclComm_t)ctx->comm);
    ctx->comm = nullptr;
    ctx->comm_size = 0;
    return WTP_OK;
}

// One round with the low and the high neighbour along an axis.  What this rank sends to its high neighbour is what
// that rank receives from its low one, so both sides post (send lo, recv lo, send hi, recv hi) in the same order and
// the pairs match; a rank that is its own neighbour (one rank, or a periodic axis of extent 1) gets its own rows back.
WTP_API int wtp_comm_exchange_rows(wtp_ctx* ctx, int peer_lo, int peer_hi, const void* d_send_lo, int64_t n_send_lo,
                                   const void* d_send_hi, int64_t n_send_hi, void* d_recv_lo, void* d_recv_hi, int64_t cap,
                                   int64_t* n_recv_lo, int64_t* n_recv_hi) {
    if (!ctx || !n_recv_lo || !n_recv_hi) return WTP_ERR_ARG;
    if (!ctx->comm) return fail(ctx, WTP_ERR_STATE, "wtp_comm_exchange_rows before wtp_comm_init");
    if (n_send_lo < 0 || n_send_hi < 0 || cap < 0) return fail(ctx, WTP_ERR_ARG, "wtp_comm_exchange_rows: negative count");
    if (peer_lo >= ctx->comm_size || peer_hi >= ctx->comm_size) return fail(ctx, WTP_ERR_ARG, "wtp_comm_exchange_rows: peer out of range");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    ncclComm_t comm = (ncclComm_t)ctx->comm;
    int rc;
    if ((rc = ensure_pinned(ctx, 64))) return rc;
    int64_t* h = (int64_t*)ctx->host_pinned;
    int64_t* d = (int64_t*)ctx->comm_scratch.p;
    // 1. the counts
    h[0] = peer_lo >= 0 ? n_send_lo : 0;
    h[1] = peer_hi >= 0 ? n_send_hi : 0;
    h[2] = h[3] = 0;
    WTP_HIP(ctx, hipMemcpyAsync(d, h, 4 * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    WTP_NCCL(ctx, g_rccl.GroupStart());
    if (peer_lo >= 0) {
        WTP_NCCL(ctx, g_rccl.Send(d + 0, 1, ncclInt64, peer_lo, comm, ctx->stream));
        WTP_NCCL(ctx, g_rccl.Recv(d + 2, 1, ncclInt64, peer_lo, comm, ctx->stream));
    }
    if (peer_hi >= 0) {
        WTP_NCCL(ctx, g_rccl.Send(d + 1, 1, ncclInt64, peer_hi, comm, ctx->stream));
        WTP_NCCL(ctx, g_rccl.Recv(d + 3, 1, ncclInt64, peer_hi, comm, ctx->stream));
    }
    WTP_NCCL(ctx, g_rccl.GroupEnd());
    WTP_HIP(ctx, hipMemcpyAsync(h + 4, d + 2, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    WTP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t in_lo = peer_lo >= 0 ? h[4] : 0, in_hi = peer_hi >= 0 ? h[5] : 0;
    *n_recv_lo = in_lo;
    *n_recv_hi = in_hi;
    if ((h[0] > 0 && !d_send_lo) || (h[1] > 0 && !d_send_hi))
        return fail(ctx, WTP_ERR_ARG, "wtp_comm_exchange_rows: NULL send buffer with a non-zero count");
    // a receive buffer that is too small (or missing) must not leave the peer hanging in its send: the rows are
    // drained into scratch memory and the call reports the error afterwards
    const bool over_lo = in_lo > 0 && (in_lo > cap || !d_recv_lo), over_hi = in_hi > 0 && (in_hi > cap || !d_recv_hi);
    if (over_lo || over_hi) {
        if ((rc = ensure(ctx, ctx->scratch, (size_t)(in_lo + in_hi) * 16))) return rc;
        if (over_lo) d_recv_lo = ctx->scratch.p;
        if (over_hi) d_recv_hi = (char*)ctx->scratch.p + (size_t)in_lo * 16;
    }
    // 2. the rows (16 bytes each), stream-ordered: the caller's next launch on this context sees them
    WTP_NCCL(ctx, g_rccl.GroupStart());
    if (peer_lo >= 0) {
        if (h[0] > 0) WTP_NCCL(ctx, g_rccl.Send(d_send_lo, (size_t)h[0] * 16, ncclUint8, peer_lo, comm, ctx->stream));
        if (in_lo > 0) WTP_NCCL(ctx, g_rccl.Recv(d_recv_lo, (size_t)in_lo * 16, ncclUint8, peer_lo, comm, ctx->stream));
    }
    if (peer_hi >= 0) {
        if (h[1] > 0) WTP_NCCL(ctx, g_rccl.Send(d_send_hi, (size_t)h[1] * 16, ncclUint8, peer_hi, comm, ctx->stream));
        if (in_hi > 0) WTP_NCCL(ctx, g_rccl.Recv(d_recv_hi, (size_t)in_hi * 16, ncclUint8, peer_hi, comm, ctx->stream));
    }
    WTP_NCCL(ctx, g_rccl.GroupEnd());
    if (over_lo || over_hi)
        return fail(ctx, WTP_ERR_ARG, "wtp_comm_exchange_rows: a peer sent more rows than the receive buffer holds (counts returned; rows dropped)");
    return WTP_OK;
}

// The global view of a sweep (what `_relax!`'s stop rules read, src/repel.jl:293,305-334): maximum of max_force; sums
// of sum_u, sum_u2, n_move, n_fallback, n_uncovered, n_escaped.  The closest pair is the one of the rank that holds
// the smallest argmin_r; its indices stay that rank's local ones and are set to -1 on the others.
WTP_API int wtp_comm_allreduce_stats(wtp_ctx* ctx, wtp_step_stats* st) {
    if (!ctx || !st) return WTP_ERR_ARG;
    if (!ctx->comm) return fail(ctx, WTP_ERR_STATE, "wtp_comm_allreduce_stats before wtp_comm_init");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    ncclComm_t comm = (ncclComm_t)ctx->comm;
    int rc;
    if ((rc = ensure_pinned(ctx, 256))) return rc;
    double* h = (double*)ctx->host_pinned;
    double* d = (double*)ctx->comm_scratch.p + 8;
    h[0] = st->max_force;
    h[1] = -st->argmin_r; // minimum through the same max reduction
    h[2] = st->sum_u;
    h[3] = st->sum_u2;
    h[4] = (double)st->n_move;
    h[5] = (double)st->n_fallback;
    h[6] = (double)st->n_uncovered;
    h[7] = (double)st->n_escaped;
    WTP_HIP(ctx, hipMemcpyAsync(d, h, 8 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    WTP_NCCL(ctx, g_rccl.GroupStart());
    WTP_NCCL(ctx, g_rccl.AllReduce(d, d, 2, ncclFloat64, ncclMax, comm, ctx->stream));
    WTP_NCCL(ctx, g_rccl.AllReduce(d + 2, d + 2, 6, ncclFloat64, ncclSum, comm, ctx->stream));
    WTP_NCCL(ctx, g_rccl.GroupEnd());
    WTP_HIP(ctx, hipMemcpyAsync(h + 8, d, 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    WTP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double* g = h + 8;
    const bool mine = st->argmin_r == -g[1];
    st->max_force = g[0];
    st->argmin_r = -g[1];
    if (!mine) st->argmin_i = st->argmin_j = -1;
    st->sum_u = g[2];
    st->sum_u2 = g[3];
    st->n_move = (int64_t)g[4];
    st->n_fallback = (int64_t)g[5];
    st->n_uncovered = (int64_t)g[6];
    st->n_escaped = (int64_t)g[7];
    return WTP_OK;
}

// ---- primitives of the block iteration (also exported) -------------------------------------------------------------
// One grouped round: every message is a send to and a receive from peers[j].  Both sides walk their peer lists in
// ascending rank order and post (send, recv) per peer inside ONE group, so the pairs match without any ordering between
// different peers; the counts were agreed on beforehand (they ride with the previous iteration's all-gather).
// (on a stream of the caller's choosing: transport_exchange posts it on the context's second stream when it overlaps)
static int exchange_peers_on(wtp_ctx* ctx, hipStream_t stream, int n_msgs, const int* peers, const void* const* d_send,
                             const int64_t* n_send, void* const* d_recv, const int64_t* n_recv) {
    if (!ctx->comm) return fail(ctx, WTP_ERR_STATE, "wtp_comm_exchange_peers before wtp_comm_init");
    if (n_msgs < 0 || (n_msgs > 0 && (!peers || !d_send || !n_send || !d_recv || !n_recv)))
        return fail(ctx, WTP_ERR_ARG, "wtp_comm_exchange_peers: NULL argument");
    for (int j = 0; j < n_msgs; ++j) {
        if (peers[j] < 0 || peers[j] >= ctx->comm_size) return fail(ctx, WTP_ERR_ARG, "wtp_comm_exchange_peers: peer out of range");
        if (n_send[j] < 0 || n_recv[j] < 0) return fail(ctx, WTP_ERR_ARG, "wtp_comm_exchange_peers: negative count");
        if ((n_send[j] > 0 && !d_send[j]) || (n_recv[j] > 0 && !d_recv[j]))
            return fail(ctx, WTP_ERR_ARG, "wtp_comm_exchange_peers: NULL buffer with a non-zero count");
    }
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    ncclComm_t comm = (ncclComm_t)ctx->comm;
    bool any = false;
    for (int j = 0; j < n_msgs; ++j) any = any || n_send[j] > 0 || n_recv[j] > 0;
    if (!any) return WTP_OK;
    WTP_NCCL(ctx, g_rccl.GroupStart());
    for (int j = 0; j < n_msgs; ++j) {
        if (n_send[j] > 0) WTP_NCCL(ctx, g_rccl.Send(d_send[j], (size_t)n_send[j] * 16, ncclUint8, peers[j], comm, stream));
        if (n_recv[j] > 0) WTP_NCCL(ctx, g_rccl.Recv(d_recv[j], (size_t)n_recv[j] * 16, ncclUint8, peers[j], comm, stream));
    }
    WTP_NCCL(ctx, g_rccl.GroupEnd());
    return WTP_OK;
}

WTP_API int wtp_comm_exchange_peers(wtp_ctx* ctx, int n_msgs, const int* peers, const void* const* d_send,
                                    const int64_t* n_send, void* const* d_recv, const int64_t* n_recv) {
    if (!ctx) return WTP_ERR_ARG;
    return exchange_peers_on(ctx, ctx->stream, n_msgs, peers, d_send, n_send, d_recv, n_recv);
}

WTP_API int wtp_comm_allgather_dev(wtp_ctx* ctx, const void* d_send, void* d_recv, int64_t bytes) {
    if (!ctx || !d_send || !d_recv) return WTP_ERR_ARG;
    if (!ctx->comm) return fail(ctx, WTP_ERR_STATE, "wtp_comm_allgather_dev before wtp_comm_init");
    if (bytes <= 0 || (bytes & 7)) return fail(ctx, WTP_ERR_ARG, "wtp_comm_allgather_dev: bytes must be a positive multiple of 8");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    WTP_NCCL(ctx, g_rccl.AllGather(d_send, d_recv, (size_t)bytes / 8, ncclUint64, (ncclComm_t)ctx->comm, ctx->stream));
    return WTP_OK;
}

// ---- the transport of the block driver and the sharded topology (Transport, wtp_internal.hpp) ------------------------
WTP_API int wtp_block_set_transport(wtp_ctx* ctx, const wtp_transport* t) {
    if (!ctx) return WTP_ERR_ARG;
    if (block_session_open(ctx)) return fail(ctx, WTP_ERR_STATE, "wtp_block_set_transport while a block session is open");
    if (t) {
        if (!t->allgather || !t->exchange) return fail(ctx, WTP_ERR_ARG, "wtp_block_set_transport: both callbacks are needed");
        ctx->transport.tr = *t;
    }
    ctx->transport.host = t != nullptr;
    return WTP_OK;
}

int wtp::transport_ready(wtp_ctx* ctx, int rank, int nranks, const std::string& who) {
    if (ctx->transport.host || nranks <= 1 || (ctx->comm && ctx->comm_size == nranks && ctx->comm_rank == rank)) return WTP_OK;
    return fail(ctx, WTP_ERR_STATE, who + "wtp_comm_init (same rank / nranks) or wtp_block_set_transport first");
}

int wtp::transport_allgather(wtp_ctx* ctx, int nranks, const void* mine, bool on_device, int64_t* all, int64_t nwords,
                             const char* who) {
    Transport& t = ctx->transport;
    const size_t bytes = 8 * (size_t)nwords;
    int rc;
    if (nranks == 1 && !on_device) { // nothing to gather and nothing to fetch: no transport is asked
        memcpy(all, mine, bytes);
        return WTP_OK;
    }
    if (t.host) {
        if (on_device) {
            t.hbuf_a.resize(bytes);
            WTP_HIP(ctx, hipMemcpyAsync(t.hbuf_a.data(), mine, bytes, hipMemcpyDeviceToHost, ctx->stream));
            if ((rc = sync(ctx))) return rc;
            mine = t.hbuf_a.data();
        }
        if (t.tr.allgather(t.tr.user, mine, all, (int64_t)bytes) != 0)
            return fail(ctx, WTP_ERR_STATE, std::string(who) + ": the caller's allgather callback failed");
        return WTP_OK;
    }
    if (nranks == 1) { // no communicator needed: the words themselves
        WTP_HIP(ctx, hipMemcpyAsync(all, mine, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return sync(ctx);
    }
    if ((rc = ensure(ctx, t.gbuf, bytes * (size_t)(nranks + 1)))) return rc;
    char* d = (char*)t.gbuf.p;
    if (!on_device) {
        WTP_HIP(ctx, hipMemcpyAsync(d, mine, bytes, hipMemcpyHostToDevice, ctx->stream));
        mine = d;
    }
    if ((rc = wtp_comm_allgather_dev(ctx, mine, d + bytes, (int64_t)bytes))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(all, d + bytes, bytes * (size_t)nranks, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

int wtp::transport_exchange(wtp_ctx* ctx, int n_msgs, const int* peers, const void* const* d_send, const int64_t* n_send,
                            void* const* d_recv, const int64_t* n_recv, int n_regions, const RowRegion* send, const RowRegion* recv,
                            int (*meanwhile)(wtp_ctx*, void*), void* arg, const char* who) {
    Transport& t = ctx->transport;
    int rc;
    if (meanwhile) { // the second stream and the two events that tie it to the first (created on first use)
        if (!ctx->comm_stream) WTP_HIP(ctx, hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
        if (!ctx->ev_comm_a) WTP_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_comm_a, hipEventDisableTiming));
        if (!ctx->ev_comm_b) WTP_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_comm_b, hipEventDisableTiming));
    }
    if (!t.host) {
        if (!meanwhile) return wtp_comm_exchange_peers(ctx, n_msgs, peers, d_send, n_send, d_recv, n_recv);
        // Exchange and compute overlap: the grouped round runs on the context's second stream, every peer on
        // its own link; the first stream does the caller's work meanwhile and waits for the rows only behind it.
        WTP_HIP(ctx, hipEventRecord(ctx->ev_comm_a, ctx->stream)); // (the send rows and the receive regions' last readers are in stream order before it)
        WTP_HIP(ctx, hipStreamWaitEvent(ctx->comm_stream, ctx->ev_comm_a, 0));
        if ((rc = exchange_peers_on(ctx, ctx->comm_stream, n_msgs, peers, d_send, n_send, d_recv, n_recv))) return rc;
        WTP_HIP(ctx, hipEventRecord(ctx->ev_comm_b, ctx->comm_stream));
        rc = meanwhile(ctx, arg);
        WTP_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_comm_b, 0)); // (also when the work failed: the streams join again)
        return rc;
    }
    // host transport: regions out, callback, regions in; the host layout is the regions one behind the other
    std::vector<size_t> so(n_regions + 1, 0), ro(n_regions + 1, 0); // byte offset of every region in hbuf_a / hbuf_b
    for (int r = 0; r < n_regions; ++r) {
        so[r + 1] = so[r] + 16 * (size_t)send[r].rows;
        ro[r + 1] = ro[r] + 16 * (size_t)recv[r].rows;
    }
    const size_t out_bytes = so[n_regions], in_bytes = ro[n_regions];
    t.hbuf_a.resize(out_bytes + 16);
    t.hbuf_b.resize(in_bytes + 16);
    for (int r = 0; r < n_regions; ++r)
        if (send[r].rows)
            WTP_HIP(ctx, hipMemcpyAsync(t.hbuf_a.data() + so[r], send[r].d, so[r + 1] - so[r], hipMemcpyDeviceToHost, ctx->stream));
    if (meanwhile) {
        // the host waits for the rows only; the stream goes on with the caller's work under the callback
        WTP_HIP(ctx, hipEventRecord(ctx->ev_comm_a, ctx->stream));
        if ((rc = meanwhile(ctx, arg))) return rc;
        ctx->timers.ev_last_end = -1;
        WTP_HIP(ctx, hipEventSynchronize(ctx->ev_comm_a));
        ctx->n_syncs += 1;
    } else if (out_bytes && (rc = sync(ctx))) {
        return rc;
    }
    // a message's host address: where its region was staged plus its offset in the region; NULL if the message does
    // not lie inside one region (an empty message may lie anywhere: it gets the buffer's start)
    auto staged = [&](const RowRegion* reg, const std::vector<size_t>& at, unsigned char* h, const void* p, size_t bytes) {
        for (int r = 0; r < n_regions; ++r) {
            const uintptr_t a = (uintptr_t)p, base = (uintptr_t)reg[r].d;
            if (a >= base && a - base + bytes <= at[r + 1] - at[r]) return h + at[r] + (a - base);
        }
        return bytes ? nullptr : h;
    };
    std::vector<const void*> hs(n_msgs);
    std::vector<void*> hr(n_msgs);
    std::vector<int64_t> sb(n_msgs), rb(n_msgs);
    for (int j = 0; j < n_msgs; ++j) {
        sb[j] = 16 * n_send[j];
        rb[j] = 16 * n_recv[j];
        hs[j] = staged(send, so, t.hbuf_a.data(), d_send[j], (size_t)sb[j]);
        hr[j] = staged(recv, ro, t.hbuf_b.data(), d_recv[j], (size_t)rb[j]);
        if (!hs[j] || !hr[j]) return fail(ctx, WTP_ERR_ARG, std::string(who) + ": a message of the exchange lies outside its regions");
    }
    if (t.tr.exchange(t.tr.user, n_msgs, peers, hs.data(), sb.data(), hr.data(), rb.data()) != 0)
        return fail(ctx, WTP_ERR_STATE, std::string(who) + ": the caller's exchange callback failed");
    if (!in_bytes) return WTP_OK;
    for (int r = 0; r < n_regions; ++r)
        if (recv[r].rows)
            WTP_HIP(ctx, hipMemcpyAsync(recv[r].d, t.hbuf_b.data() + ro[r], ro[r + 1] - ro[r], hipMemcpyHostToDevice, ctx->stream));
    return sync(ctx); // (the host buffers are reused)
}
