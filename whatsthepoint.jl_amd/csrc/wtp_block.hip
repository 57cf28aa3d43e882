// wtp_block.hip — one rank's share of a block-decomposed repel, the whole iteration behind the C ABI
// (include/wtp.h: wtp_block_*).
//
// The reference has one address space and one kd-tree (src/repel.jl:243-334); this is the build's own decomposition
// of the same Jacobi sweep.  The cloud is cut into the cells of an orthtree partition (axis-aligned boxes, one per
// rank, any shape: equidistant octants for the uniform benchmark cloud, count medians for a graded one).  Per
// iteration and rank:
//
//   1. exchange: ONE grouped ncclSend/ncclRecv round with every rank whose box lies within w + margin of this one
//      (faces, edges and corners directly — xGMI is point-to-point, every peer has its own link).  The row counts
//      are already known on both sides: they rode with the previous iteration's all-gather.
//   2. migration: arrivals are appended to the owned set, departures leave it (ordered compaction; 64-bit global ids
//      follow); only when somebody actually crossed a box face by more than `margin`.
//   3. [selected wall points ; ghosts] -> fixed head of the snapshot (wtp_relax_set_fixed_dev: appended, no pass over
//      the cloud).  The wall (wtp_block_set_wall) is replicated: every rank holds all of it and keeps the points inside
//      its coverage box; nobody sends one.
//   4. hash + sweep of [ghosts ; owned] (relax_step_enqueue).
//   5. from the new positions: classify every owned point against the peers' boxes (which ranks need it as a ghost,
//      does it change owner), count per peer, fill the send rows of the NEXT exchange — three launches.
//   6. one all-gather of {step statistics, row counts per destination rank}, read back with the iteration's only host
//      synchronisation; every rank reduces the statistics in rank order (fixed order: reproducible sums).
//   7. if any rank counted a query whose support reaches past its covered box: undo, widen, repeat.
//
// How the rows and the gathered words travel (the context's RCCL communicator or the caller's host callbacks, and the
// overlap of step 1 with the first half of step 4) is the context's Transport: wtp_comm.hip.
//
// Order of the rows a peer receives = slot order of the sender's sorted state = a pure function of the sender's
// points, so the ghost ids on the receiving side (and with them every sum) do not depend on scheduling.
//
// Global numbering of the closest pair: the snapshot index of the assembled cloud [wall ; volume] — wall point k is k,
// the volume point with global id g is n_wall + g.  A ghost row carries the low 32 bits of its gid in the w word
// (the fixed-head install overwrites w without reading it), so the pack kernel can translate either end of the pair.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "wtp_device.hpp"

namespace wtp {

constexpr int kBlkMaxPeers = 26;
constexpr int kBlkPasses = 16;                 // a wave owns 64 * 16 consecutive slots ("span")
constexpr int kBlkSpan = 64 * kBlkPasses;
constexpr int kBlkWaves = 4;                   // waves per workgroup
constexpr uint32_t kBlkMigrate = 0x80000000u;  // flag bit 31: the point changes owner; bits 26..30: peer index of the new owner
constexpr int kBlkStatWords = 10;              // wtp_step_stats as 8-byte words
constexpr uint32_t kBlkNoGid = 0xFFFFFFFFu;    // w word of a ghost row whose gid does not fit in 32 bits

struct BlkGeom {
    int np;
    float in_lo[kBlkMaxPeers][3], in_hi[kBlkMaxPeers][3]; // peer box widened by w + margin: who needs a point as a ghost
    float bx_lo[kBlkMaxPeers][3], bx_hi[kBlkMaxPeers][3]; // peer box itself: who owns a point
    float out_lo[3], out_hi[3];                           // own box widened by margin: beyond it a point changes owner
    float deep_lo[3], deep_hi[3];                         // own box shrunk by w + margin: a point in there is nobody's ghost
};

// columns of the per-span count table: [0, np) ghost rows per peer, [np, 2 np) migrants per peer, 2 np points that stay
__host__ __device__ inline int blk_cols(int np) { return 2 * np + 1; }

struct BlockState {
    bool active = false;
    int rank = 0, nranks = 1;
    std::vector<double> boxes; // nranks x 6
    double w = 0, margin = 0;
    std::vector<int> peers;    // ascending ranks
    BlkGeom geom{};
    int widened = 0;
    // device
    DevBuf flags, span_counts, totals, send, send_mig, gid[2], pool, recv_mig, gsend, lost;
    int gid_cur = 0;
    int64_t n_owned = 0, n_ghost = 0;
    int64_t send_cap = 0, mig_cap = 0;
    // the plan of the next exchange (host): rows to / from each peer
    bool plan_ready = false;
    std::vector<int64_t> send_cnt, mig_cnt, recv_cnt, rmig_cnt;
    // the boundary wall (wtp_block_set_wall): all of it on the host, the part inside the coverage box as 16-byte rows
    // {x, y, z, bits(wall index)} in ascending wall index on both sides; the rows lead the fixed head
    std::vector<float> wall;             // n_wall x 3
    std::vector<float> wall_sel;         // n_sel x 4
    int64_t n_wall = 0, n_sel = 0;
    DevBuf wall_rows, snap;              // selected rows (device); [selection ; owned] xyz while a session opens
    bool wall_dirty = false;             // the selection changed since the session's head was installed
    bool pool_wall_ok = false;           // the pool's prefix holds the current selection (false after any regrowth)
    // last info
    wtp_block_info info{};
};

static BlockState* bs_of(wtp_ctx* ctx) { return (BlockState*)ctx->block; }

void block_destroy(wtp_ctx* ctx) {
    BlockState* b = bs_of(ctx);
    if (!b) return;
    hipSetDevice(ctx->device);
    delete b; // (frees the device buffers)
    ctx->block = nullptr;
}

// ---- kernels --------------------------------------------------------------------------------------------------------

__device__ inline bool blk_inside(const float4& p, const float (&lo)[3], const float (&hi)[3]) {
    return p.x >= lo[0] && p.x < hi[0] && p.y >= lo[1] && p.y < hi[1] && p.z >= lo[2] && p.z < hi[2];
}

// Pass 1: flag of every slot (which peers need the point as a ghost, does it change owner and to whom) and the span's
// counts per column.  97 % of the waves see no flagged point and only pay the load.
__global__ __launch_bounds__(64 * kBlkWaves) void blk_classify_kernel(const float4* __restrict__ P, int64_t n, int32_t n_fixed,
                                                                     BlkGeom g, uint32_t* __restrict__ flags,
                                                                     int32_t* __restrict__ span_counts, int32_t* __restrict__ lost) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t span = (int64_t)blockIdx.x * kBlkWaves + wave;
    const int64_t first = span * kBlkSpan;
    if (first >= n) return;
    const int np = g.np, ncol = blk_cols(np);
    int cnt = 0; // lane c holds the span's count of column c
    int n_lost = 0;
    // the span's sixteen loads in flight together (in a loop with the ballots between them they were sixteen round trips)
    float4 pp[kBlkPasses];
#pragma unroll
    for (int pass = 0; pass < kBlkPasses; ++pass) {
        const int64_t i = first + (int64_t)pass * 64 + lane;
        pp[pass] = P[i < n ? i : n - 1];
    }
#pragma unroll
    for (int pass = 0; pass < kBlkPasses; ++pass) {
        const int64_t i = first + (int64_t)pass * 64 + lane;
        uint32_t flag = 0;
        bool movable = false;
        if (i < n) {
            const float4 p = pp[pass];
            movable = w_to_id(p.w) >= n_fixed;
            // (most points lie deeper inside the box than any peer's layer reaches: six compares settle them)
            if (movable && !blk_inside(p, g.deep_lo, g.deep_hi)) {
                const bool leaves = !blk_inside(p, g.out_lo, g.out_hi);
                int owner = -1;
                for (int q = 0; q < np; ++q) {
                    if (blk_inside(p, g.in_lo[q], g.in_hi[q])) flag |= 1u << q;
                    if (leaves && owner < 0 && blk_inside(p, g.bx_lo[q], g.bx_hi[q])) owner = q;
                }
                if (leaves) {
                    if (owner >= 0) flag = (flag & ~(1u << owner)) | kBlkMigrate | ((uint32_t)owner << 26);
                    else n_lost += 1; // outside every neighbouring box: stays (reported)
                }
            }
            flags[i] = flag;
        }
        const unsigned long long stay = __ballot(movable && !(flag & kBlkMigrate));
        if (lane == 2 * np) cnt += __popcll(stay);
        if (__ballot(flag != 0) == 0ull) continue;
        for (int q = 0; q < np; ++q) {
            const unsigned long long m = __ballot((flag >> q) & 1u);
            if (lane == q) cnt += __popcll(m);
            const unsigned long long mm = __ballot((flag & kBlkMigrate) && (int)((flag >> 26) & 31u) == q);
            if (lane == np + q) cnt += __popcll(mm);
        }
    }
    if (lane < ncol) span_counts[span * ncol + lane] = cnt;
    if (n_lost) atomicAdd(lost, n_lost);
}

// Pass 2: exclusive scan of every column over the spans (one workgroup per column), the column totals behind them.
__global__ __launch_bounds__(256) void blk_scan_kernel(int32_t* __restrict__ span_counts, int64_t nspans, int ncol,
                                                      int32_t* __restrict__ totals) {
    __shared__ int part[256];
    const int col = blockIdx.x, t = threadIdx.x;
    const int64_t per = (nspans + 255) / 256, a = t * per, b = a + per < nspans ? a + per : nspans;
    int s = 0;
    for (int64_t i = a; i < b; ++i) s += span_counts[i * ncol + col];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int j = 0; j < 256; ++j) {
            const int v = part[j];
            part[j] = run;
            run += v;
        }
        totals[col] = run;
    }
    __syncthreads();
    int run = part[t];
    for (int64_t i = a; i < b; ++i) {
        const int v = span_counts[i * ncol + col];
        span_counts[i * ncol + col] = run;
        run += v;
    }
}

// Where a local snapshot index of the pair lies in the global numbering (see the top of the file); -1 if unknown.
struct BlkIds {
    const int64_t* gid;      // owned points, by movable index
    const float4* wall_rows; // [0, n_sel) of the head
    const float4* ghosts;    // [n_sel, n_fixed) of the head
    int64_t n_fixed, n_sel, n_wall;
};

__device__ inline int64_t blk_global_id(const BlkIds& t, int64_t l) {
    if (l < 0) return -1;
    if (l >= t.n_fixed) return t.n_wall + t.gid[l - t.n_fixed];
    if (l < t.n_sel) return (int64_t)__builtin_bit_cast(uint32_t, t.wall_rows[l].w);
    const uint32_t g = __builtin_bit_cast(uint32_t, t.ghosts[l - t.n_sel].w);
    return g == kBlkNoGid ? -1 : t.n_wall + (int64_t)g;
}

// The all-gather payload: [0, 10) the step's statistics, the closest pair in global numbering, then per DESTINATION
// rank the ghost rows and the migrants this rank will send, then {points lost, owned points}.  One thread: a few
// dozen words.
__global__ void blk_pack_kernel(const wtp_step_stats* __restrict__ st, BlkIds ids, const int32_t* __restrict__ totals, int np,
                                const int* __restrict__ peer_rank, int nranks, const int32_t* __restrict__ lost,
                                int64_t n_owned, int64_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    wtp_step_stats s{};
    if (st) {
        s = *st;
        if (s.argmin_i >= 0) {
            s.argmin_i = blk_global_id(ids, s.argmin_i);
            s.argmin_j = blk_global_id(ids, s.argmin_j);
        }
    }
    const int64_t* sw = (const int64_t*)&s;
    for (int j = 0; j < kBlkStatWords; ++j) out[j] = sw[j];
    for (int r = 0; r < 2 * nranks; ++r) out[kBlkStatWords + r] = 0;
    for (int q = 0; q < np; ++q) {
        out[kBlkStatWords + peer_rank[q]] = totals[q];
        out[kBlkStatWords + nranks + peer_rank[q]] = totals[np + q];
    }
    out[kBlkStatWords + 2 * nranks] = lost ? *lost : 0;
    out[kBlkStatWords + 2 * nranks + 1] = n_owned;
}

// Pass 3: the send rows.  Ghost rows {x, y, z, bits(gid low)} (kBlkNoGid for gid >= 2^32 - 1) of peer q start at row
// sum_{j<q} totals[j]; a migrant is two rows {x, y, z, bits(gid low)}, {bits(gid high), 0, 0, 0}, peer q's start at
// 2 * sum_{j<q} totals[np + j].  Order inside a peer's rows: slot order.
__global__ __launch_bounds__(64 * kBlkWaves) void blk_fill_kernel(const float4* __restrict__ P, int64_t n, int32_t n_fixed, int np,
                                                                 const uint32_t* __restrict__ flags,
                                                                 const int32_t* __restrict__ span_off,
                                                                 const int32_t* __restrict__ totals, const int64_t* __restrict__ gid,
                                                                 float4* __restrict__ send, int64_t send_cap,
                                                                 float4* __restrict__ send_mig, int64_t mig_cap) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t span = (int64_t)blockIdx.x * kBlkWaves + wave;
    const int64_t first = span * kBlkSpan;
    if (first >= n) return;
    const int ncol = blk_cols(np);
    // lane c: where column c's next row of this span goes
    int run = 0;
    if (lane < 2 * np) {
        const int c0 = lane < np ? 0 : np;
        int base = 0;
        for (int j = c0; j < lane; ++j) base += totals[j];
        run = base + span_off[span * ncol + lane];
    }
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    uint32_t ff[kBlkPasses]; // the span's flags, all loads in flight together
#pragma unroll
    for (int pass = 0; pass < kBlkPasses; ++pass) {
        const int64_t i = first + (int64_t)pass * 64 + lane;
        ff[pass] = i < n ? flags[i] : 0u;
    }
#pragma unroll
    for (int pass = 0; pass < kBlkPasses; ++pass) {
        const int64_t i = first + (int64_t)pass * 64 + lane;
        const uint32_t flag = ff[pass];
        if (__ballot(flag != 0) == 0ull) continue;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        int64_t gd = 0;
        if (flag) {
            p = P[i];
            gd = gid[w_to_id(p.w) - n_fixed];
        }
        const float gw = __builtin_bit_cast(float, (uint64_t)gd < kBlkNoGid ? (uint32_t)gd : kBlkNoGid);
        for (int q = 0; q < np; ++q) {
            const bool g = (flag >> q) & 1u;
            const unsigned long long m = __ballot(g);
            if (m) {
                const int off = __builtin_amdgcn_readlane(run, q);
                if (g) {
                    const int64_t o = (int64_t)off + __popcll(m & below);
                    if (o < send_cap) send[o] = make_float4(p.x, p.y, p.z, gw);
                }
                if (lane == q) run += __popcll(m);
            }
            const bool mg = (flag & kBlkMigrate) && (int)((flag >> 26) & 31u) == q;
            const unsigned long long mm = __ballot(mg);
            if (mm) {
                const int off = __builtin_amdgcn_readlane(run, np + q);
                if (mg) {
                    const int64_t o = (int64_t)off + __popcll(mm & below);
                    if (o < mig_cap) {
                        send_mig[2 * o] = make_float4(p.x, p.y, p.z, __builtin_bit_cast(float, (uint32_t)(gd & 0xFFFFFFFFll)));
                        send_mig[2 * o + 1] = make_float4(__builtin_bit_cast(float, (uint32_t)((uint64_t)gd >> 32)), 0.f, 0.f, 0.f);
                    }
                }
                if (lane == np + q) run += __popcll(mm);
            }
        }
    }
}

// Migration: the points that stay, in slot order, renumbered 0 .. n_stay; their global ids follow.
__global__ __launch_bounds__(64 * kBlkWaves) void blk_compact_kernel(const float4* __restrict__ P, int64_t n, int32_t n_fixed, int np,
                                                                    const uint32_t* __restrict__ flags,
                                                                    const int32_t* __restrict__ span_off,
                                                                    const int64_t* __restrict__ gid_old, float4* __restrict__ Pn,
                                                                    int64_t* __restrict__ gid_new) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t span = (int64_t)blockIdx.x * kBlkWaves + wave;
    const int64_t first = span * kBlkSpan;
    if (first >= n) return;
    const int ncol = blk_cols(np);
    int64_t pos = span_off[span * ncol + 2 * np];
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int pass = 0; pass < kBlkPasses; ++pass) {
        const int64_t i = first + (int64_t)pass * 64 + lane;
        bool keep = false;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n) {
            p = P[i];
            keep = w_to_id(p.w) >= n_fixed && !(flags[i] & kBlkMigrate);
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int64_t o = pos + __popcll(m & below);
            gid_new[o] = gid_old[w_to_id(p.w) - n_fixed];
            p.w = id_to_w(0.f, (int32_t)o);
            Pn[o] = p;
        }
        pos += __popcll(m);
    }
}

// arrivals behind the points that stayed
__global__ void blk_arrivals_kernel(const float4* __restrict__ rows, int64_t n_arr, int64_t n_stay, float4* __restrict__ Pn,
                                    int64_t* __restrict__ gid_new) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_arr; k += (int64_t)gridDim.x * blockDim.x) {
        const float4 a = rows[2 * k], b = rows[2 * k + 1];
        const uint64_t lo = __builtin_bit_cast(uint32_t, a.w), hi = __builtin_bit_cast(uint32_t, b.x);
        gid_new[n_stay + k] = (int64_t)(lo | (hi << 32));
        Pn[n_stay + k] = make_float4(a.x, a.y, a.z, id_to_w(0.f, (int32_t)(n_stay + k)));
    }
}

// this rank's own emigrants stay around as ghosts for the iteration (their new owner cut its layers before they arrived)
__global__ void blk_emigrant_ghosts_kernel(const float4* __restrict__ mig_rows, int64_t n_mig, float4* __restrict__ pool_tail) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_mig; k += (int64_t)gridDim.x * blockDim.x) {
        const float4 a = mig_rows[2 * k], b = mig_rows[2 * k + 1];
        const uint32_t lo = __builtin_bit_cast(uint32_t, a.w), hi = __builtin_bit_cast(uint32_t, b.x);
        pool_tail[k] = make_float4(a.x, a.y, a.z, hi == 0 && lo != kBlkNoGid ? a.w : __builtin_bit_cast(float, kBlkNoGid));
    }
}

__global__ void blk_iota_gid_kernel(int64_t* gid, int64_t n) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) gid[k] = k;
}

__global__ void blk_gather_gid_kernel(const float4* __restrict__ P, int64_t n, int32_t n_fixed, const int64_t* __restrict__ gid,
                                      int64_t* __restrict__ out) {
    // (movable order is the order wtp_relax_get_dev writes: by movable index — gid is stored that way already)
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n - n_fixed; k += (int64_t)gridDim.x * blockDim.x)
        out[k] = gid[k];
    (void)P;
}

// ---- host side --------------------------------------------------------------------------------------------------------

static bool boxes_near(const double* a, const double* c, double reach) {
    for (int ax = 0; ax < 3; ++ax)
        if (a[ax] - reach >= c[3 + ax] || c[ax] - reach >= a[3 + ax]) return false;
    return true;
}

// what the snapshot is complete for: the box plus the layers the peers send, rounded to fp32
static void blk_coverage(const BlockState* b, double lo[3], double hi[3]) {
    const double w_eff = b->w + b->margin;
    const double* mine = &b->boxes[(size_t)b->rank * 6];
    for (int ax = 0; ax < 3; ++ax) {
        lo[ax] = (double)(float)(mine[ax] - w_eff);
        hi[ax] = (double)(float)(mine[3 + ax] + w_eff);
    }
}

// The wall points inside the coverage box (inclusive, fp32 compares on the coverage thresholds), ascending wall index.
// Host work on the replicated copy, at open and on a widening only.  A changed selection goes to the device and marks
// the session's head and the pool's prefix stale.
static int blk_select_wall(wtp_ctx* ctx, BlockState* b, const double lo[3], const double hi[3]) {
    std::vector<float> sel;
    float flo[3], fhi[3];
    for (int ax = 0; ax < 3; ++ax) {
        flo[ax] = (float)lo[ax];
        fhi[ax] = (float)hi[ax];
    }
    for (int64_t k = 0; k < b->n_wall; ++k) {
        const float* q = &b->wall[(size_t)k * 3];
        bool in = true;
        for (int ax = 0; ax < 3; ++ax) in = in && q[ax] >= flo[ax] && q[ax] <= fhi[ax];
        if (!in) continue;
        uint32_t kb = (uint32_t)k;
        float kw;
        memcpy(&kw, &kb, 4);
        sel.insert(sel.end(), {q[0], q[1], q[2], kw});
    }
    if (sel.size() == b->wall_sel.size() && (sel.empty() || !memcmp(sel.data(), b->wall_sel.data(), 4 * sel.size())))
        return WTP_OK;
    // (the previous rows may still be the source of a copy in flight: the stream drains before they are replaced)
    int rc;
    if ((rc = sync(ctx))) return rc;
    b->wall_sel.swap(sel);
    b->n_sel = (int64_t)(b->wall_sel.size() / 4);
    b->wall_dirty = true;
    b->pool_wall_ok = false;
    if ((rc = ensure(ctx, b->wall_rows, 16 * (size_t)b->n_sel))) return rc;
    if (b->n_sel)
        WTP_HIP(ctx, hipMemcpyAsync(b->wall_rows.p, b->wall_sel.data(), 16 * (size_t)b->n_sel, hipMemcpyHostToDevice, ctx->stream));
    return WTP_OK;
}

// peers and the kernel's geometry block for the current ghost width
static int blk_geometry(wtp_ctx* ctx, BlockState* b) {
    const double w_eff = b->w + b->margin;
    const double* mine = &b->boxes[(size_t)b->rank * 6];
    for (int ax = 0; ax < 3; ++ax)
        if (mine[3 + ax] - mine[ax] < b->w + 2.0 * b->margin)
            return fail(ctx, WTP_ERR_ARG, "wtp_block: this rank's box is thinner than a ghost layer (w + 2 margin): use fewer ranks");
    b->peers.clear();
    for (int r = 0; r < b->nranks; ++r) {
        if (r == b->rank) continue;
        // anybody whose box my points can come within w_eff of (my points stray at most ~margin beyond my box)
        if (boxes_near(mine, &b->boxes[(size_t)r * 6], w_eff + b->margin + 1e-12)) b->peers.push_back(r);
    }
    if ((int)b->peers.size() > kBlkMaxPeers)
        return fail(ctx, WTP_ERR_ARG, "wtp_block: more than 26 neighbouring boxes (boxes too thin for this ghost width)");
    BlkGeom& g = b->geom;
    g.np = (int)b->peers.size();
    for (int q = 0; q < g.np; ++q) {
        const double* bx = &b->boxes[(size_t)b->peers[q] * 6];
        for (int ax = 0; ax < 3; ++ax) {
            g.bx_lo[q][ax] = (float)bx[ax];
            g.bx_hi[q][ax] = (float)bx[3 + ax];
            g.in_lo[q][ax] = (float)(bx[ax] - w_eff);
            g.in_hi[q][ax] = (float)(bx[3 + ax] + w_eff);
        }
    }
    for (int ax = 0; ax < 3; ++ax) {
        g.out_lo[ax] = (float)(mine[ax] - b->margin);
        g.out_hi[ax] = (float)(mine[3 + ax] + b->margin);
        // every peer's box lies outside mine, so its layer reaches at most w_eff into my box (one float ulp of slack)
        g.deep_lo[ax] = std::nextafter((float)(mine[ax] + w_eff), std::numeric_limits<float>::infinity());
        g.deep_hi[ax] = std::nextafter((float)(mine[3 + ax] - w_eff), -std::numeric_limits<float>::infinity());
    }
    const size_t np = b->peers.size();
    b->send_cnt.assign(np, 0);
    b->mig_cnt.assign(np, 0);
    b->recv_cnt.assign(np, 0);
    b->rmig_cnt.assign(np, 0);
    // the coverage box certifies the wall and the ghosts together
    double lo[3], hi[3];
    blk_coverage(b, lo, hi);
    int rc;
    if ((rc = blk_select_wall(ctx, b, lo, hi))) return rc;
    return wtp_relax_set_coverage_box(ctx, lo, hi);
}

static int64_t blk_nspans(int64_t n) { return (n + kBlkSpan - 1) / kBlkSpan; }

// launches the fill pass with the current send buffers (again after they grew)
static int blk_fill(wtp_ctx* ctx, BlockState* b) {
    RelaxState& r = ctx->relax;
    const int np = b->geom.np;
    if (np == 0) return WTP_OK;
    int rc;
    if ((rc = ensure(ctx, b->send, 16 * (size_t)b->send_cap))) return rc;
    if ((rc = ensure(ctx, b->send_mig, 32 * (size_t)b->mig_cap))) return rc;
    const int64_t n = r.n, nsp = blk_nspans(n);
    const int grid = (int)((nsp + kBlkWaves - 1) / kBlkWaves);
    hipLaunchKernelGGL(blk_fill_kernel, dim3(grid), dim3(64 * kBlkWaves), 0, ctx->stream, (const float4*)ctx->pts[r.bufP].p, n,
                       (int32_t)r.n_fixed, np, (const uint32_t*)b->flags.p, (const int32_t*)b->span_counts.p,
                       (const int32_t*)b->totals.p, (const int64_t*)b->gid[b->gid_cur].p, (float4*)b->send.p, b->send_cap,
                       (float4*)b->send_mig.p, b->mig_cap);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

// classify + count + fill from the session's current P, then the all-gather payload (d_stats may be NULL)
static int blk_classify(wtp_ctx* ctx, BlockState* b, const wtp_step_stats* d_stats) {
    RelaxState& r = ctx->relax;
    if (r.pending.active) return fail(ctx, WTP_ERR_STATE, "wtp_block: classification with a pending fixed head");
    const int np = b->geom.np, ncol = blk_cols(np);
    const int64_t n = r.n, nsp = blk_nspans(n);
    int rc;
    if ((rc = ensure(ctx, b->flags, sizeof(uint32_t) * (size_t)(n + n / 8)))) return rc;
    if ((rc = ensure(ctx, b->span_counts, sizeof(int32_t) * (size_t)(nsp + nsp / 8 + 1) * ncol))) return rc;
    if ((rc = ensure(ctx, b->totals, sizeof(int32_t) * (size_t)(ncol + kBlkMaxPeers + 8)))) return rc;
    if ((rc = ensure(ctx, b->lost, 64))) return rc;
    if (b->send_cap == 0) {
        b->send_cap = 65536 + b->n_owned / 3;
        b->mig_cap = 16384 + b->n_owned / 16;
    }
    const size_t gwords = (size_t)kBlkStatWords + 2 * (size_t)b->nranks + 2;
    if ((rc = ensure(ctx, b->gsend, 8 * gwords))) return rc;
    const float4* P = (const float4*)ctx->pts[r.bufP].p;
    int32_t* totals = (int32_t*)b->totals.p;
    int* d_peer_rank = (int*)(totals + ncol + 4);
    WTP_HIP(ctx, hipMemsetAsync(b->lost.p, 0, 4, ctx->stream));
    if (np > 0) {
        WTP_HIP(ctx, hipMemcpyAsync(d_peer_rank, b->peers.data(), sizeof(int) * (size_t)np, hipMemcpyHostToDevice, ctx->stream));
        const int grid = (int)((nsp + kBlkWaves - 1) / kBlkWaves);
        hipLaunchKernelGGL(blk_classify_kernel, dim3(grid), dim3(64 * kBlkWaves), 0, ctx->stream, P, n, (int32_t)r.n_fixed,
                           b->geom, (uint32_t*)b->flags.p, (int32_t*)b->span_counts.p, (int32_t*)b->lost.p);
        hipLaunchKernelGGL(blk_scan_kernel, dim3(ncol), dim3(256), 0, ctx->stream, (int32_t*)b->span_counts.p, nsp, ncol, totals);
        if ((rc = blk_fill(ctx, b))) return rc;
    } else {
        WTP_HIP(ctx, hipMemsetAsync(totals, 0, sizeof(int32_t) * (size_t)ncol, ctx->stream));
    }
    BlkIds ids{(const int64_t*)b->gid[b->gid_cur].p, (const float4*)b->wall_rows.p, (const float4*)b->pool.p + b->n_sel,
               r.n_fixed, b->n_sel, b->n_wall};
    hipLaunchKernelGGL(blk_pack_kernel, dim3(1), dim3(64), 0, ctx->stream, d_stats, ids, (const int32_t*)totals, np,
                       (const int*)d_peer_rank, b->nranks, (const int32_t*)b->lost.p, b->n_owned, (int64_t*)b->gsend.p);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

// all-gather of the payload + read-back: the iteration's host synchronisation.  Fills the plan; returns the global
// statistics in *g (if d_stats was given to blk_classify) and whether a send buffer overflowed anywhere.
static int blk_gather(wtp_ctx* ctx, BlockState* b, wtp_step_stats* g, bool* overflow, int64_t* lost_total) {
    const size_t gwords = (size_t)kBlkStatWords + 2 * (size_t)b->nranks + 2;
    int rc;
    if ((rc = ensure_pinned(ctx, 8 * gwords * (size_t)b->nranks + 64))) return rc;
    int64_t* h = (int64_t*)ctx->host_pinned;
    if ((rc = transport_allgather(ctx, b->nranks, b->gsend.p, true, h, (int64_t)gwords, "wtp_block"))) return rc;
    // the plan: what I send (my own row) and what every peer sends me
    const int np = b->geom.np;
    const int64_t* mine = h + (size_t)b->rank * gwords;
    int64_t tot_s = 0, tot_m = 0;
    for (int q = 0; q < np; ++q) {
        b->send_cnt[q] = mine[kBlkStatWords + b->peers[q]];
        b->mig_cnt[q] = mine[kBlkStatWords + b->nranks + b->peers[q]];
        const int64_t* theirs = h + (size_t)b->peers[q] * gwords;
        b->recv_cnt[q] = theirs[kBlkStatWords + b->rank];
        b->rmig_cnt[q] = theirs[kBlkStatWords + b->nranks + b->rank];
        tot_s += b->send_cnt[q];
        tot_m += b->mig_cnt[q];
    }
    // a rank that names me although I do not list it as a peer would be left hanging: boxes must be identical everywhere
    for (int rnk = 0; rnk < b->nranks; ++rnk) {
        if (rnk == b->rank) continue;
        const int64_t* theirs = h + (size_t)rnk * gwords;
        if (theirs[kBlkStatWords + b->rank] || theirs[kBlkStatWords + b->nranks + b->rank]) {
            bool listed = false;
            for (int q = 0; q < np; ++q) listed = listed || b->peers[q] == rnk;
            if (!listed) return fail(ctx, WTP_ERR_STATE, "wtp_block: a rank that is not a neighbour announces rows (boxes differ between ranks?)");
        }
    }
    int64_t lost = 0;
    for (int rnk = 0; rnk < b->nranks; ++rnk) lost += (h + (size_t)rnk * gwords)[kBlkStatWords + 2 * b->nranks];
    // the announced counts are the true ones (the count pass does not look at capacities); rows beyond the capacity
    // of MY send buffers were not written: a local matter, fixed by filling again into larger buffers
    *overflow = tot_s > b->send_cap || tot_m > b->mig_cap;
    *lost_total = lost;
    if (g) {
        // global statistics, reduced in rank order (a fixed order: the sums are reproducible)
        wtp_step_stats out{};
        out.argmin_r = std::numeric_limits<double>::infinity();
        out.argmin_i = out.argmin_j = -1;
        for (int rnk = 0; rnk < b->nranks; ++rnk) {
            wtp_step_stats s;
            memcpy(&s, h + (size_t)rnk * gwords, sizeof(s));
            out.max_force = s.max_force > out.max_force ? s.max_force : out.max_force;
            out.sum_u += s.sum_u;
            out.sum_u2 += s.sum_u2;
            out.n_move += s.n_move;
            out.n_fallback += s.n_fallback;
            out.n_uncovered += s.n_uncovered;
            out.n_escaped += s.n_escaped;
            // the closest pair in global numbering: smallest distance, on a tie the smallest argmin_i (cs2_kernel's rule)
            if (s.n_move > 0 && s.argmin_i >= 0 &&
                (out.argmin_i < 0 || s.argmin_r < out.argmin_r || (s.argmin_r == out.argmin_r && s.argmin_i < out.argmin_i))) {
                out.argmin_r = s.argmin_r;
                out.argmin_i = s.argmin_i;
                out.argmin_j = s.argmin_j;
            }
        }
        *g = out;
    }
    return WTP_OK;
}

// The plan for the next exchange from the session's current positions: rows filled, counts known on every rank.
static int blk_plan(wtp_ctx* ctx, BlockState* b, const wtp_step_stats* d_stats, wtp_step_stats* g) {
    int rc;
    if ((rc = blk_classify(ctx, b, d_stats))) return rc;
    bool over = false;
    int64_t lost = 0;
    if ((rc = blk_gather(ctx, b, g, &over, &lost))) return rc;
    if (lost > 0)
        return fail(ctx, WTP_ERR_STATE, "wtp_block: " + std::to_string(lost) + " points left their box for a region no neighbouring rank owns");
    if (over) { // my send buffers were too small: the counts stand, the rows are written again into larger ones
        int64_t tot_s = 0, tot_m = 0;
        for (size_t q = 0; q < b->send_cnt.size(); ++q) {
            tot_s += b->send_cnt[q];
            tot_m += b->mig_cnt[q];
        }
        if (tot_s > b->send_cap) b->send_cap = tot_s + tot_s / 2 + 65536;
        if (tot_m > b->mig_cap) b->mig_cap = tot_m + tot_m / 2 + 16384;
        if ((rc = blk_fill(ctx, b))) return rc;
    }
    b->plan_ready = true;
    return WTP_OK;
}

// ---- what the sharded topology (wtp_block_topo.hip) takes from the driver -------------------------------------------
bool block_session_open(wtp_ctx* ctx) { return bs_of(ctx) && bs_of(ctx)->active; }

int launch_blk_scan(wtp_ctx* ctx, int32_t* span_counts, int64_t nspans, int ncol, int32_t* totals) {
    hipLaunchKernelGGL(blk_scan_kernel, dim3(ncol), dim3(256), 0, ctx->stream, span_counts, nspans, ncol, totals);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

} // namespace wtp

using namespace wtp;
#define WTP_API extern "C"

WTP_API int wtp_block_grid(int nranks, int p_out[3]) {
    if (nranks < 1 || !p_out) return WTP_ERR_ARG;
    long best = -1;
    for (int px = 1; px <= nranks; ++px) {
        if (nranks % px) continue;
        for (int py = px; py <= nranks / px; ++py) {
            if ((nranks / px) % py) continue;
            const int pz = nranks / (px * py);
            if (pz < py) continue;
            const long score = pz - px;
            if (best < 0 || score < best) {
                best = score;
                p_out[0] = px;
                p_out[1] = py;
                p_out[2] = pz;
            }
        }
    }
    return WTP_OK;
}

WTP_API int wtp_block_morton_rank(int ix, int iy, int iz, const int p[3]) {
    if (!p) return -1;
    bool pow2 = true;
    for (int a = 0; a < 3; ++a) pow2 = pow2 && p[a] >= 1 && (p[a] & (p[a] - 1)) == 0;
    if (!pow2) return (iz * p[1] + iy) * p[0] + ix;
    int idx[3] = {ix, iy, iz}, sizes[3] = {p[0], p[1], p[2]};
    int out = 0, bit = 0;
    while (sizes[0] > 1 || sizes[1] > 1 || sizes[2] > 1) {
        for (int a = 0; a < 3; ++a) {
            if (sizes[a] > 1) {
                out |= (idx[a] & 1) << bit;
                idx[a] >>= 1;
                sizes[a] >>= 1;
                ++bit;
            }
        }
    }
    return out;
}

WTP_API int wtp_block_set_wall(wtp_ctx* ctx, const void* d_wall_xyz, int64_t n_wall) {
    if (!ctx) return WTP_ERR_ARG;
    if (n_wall < 0 || (n_wall > 0 && !d_wall_xyz)) return fail(ctx, WTP_ERR_ARG, "wtp_block_set_wall: n_wall >= 0, and an array when n_wall > 0");
    if (n_wall > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "wtp_block_set_wall: n_wall exceeds the int32 index space");
    if (!ctx->block) ctx->block = new BlockState();
    BlockState* b = bs_of(ctx);
    if (b->active) return fail(ctx, WTP_ERR_STATE, "wtp_block_set_wall while a block session is open");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<float> h((size_t)n_wall * 3);
    if (n_wall) WTP_HIP(ctx, hipMemcpyAsync(h.data(), d_wall_xyz, 12 * (size_t)n_wall, hipMemcpyDeviceToHost, ctx->stream));
    WTP_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the caller's array is free again, no copy reads the old selection
    b->wall.swap(h);
    b->n_wall = n_wall;
    b->wall_sel.clear();
    b->n_sel = 0;
    b->pool_wall_ok = false;
    return WTP_OK;
}

WTP_API int wtp_block_close(wtp_ctx* ctx) {
    if (!ctx) return WTP_ERR_ARG;
    BlockState* b = bs_of(ctx);
    if (!b || !b->active) return WTP_OK;
    b->active = false;
    b->plan_ready = false;
    return wtp_relax_end(ctx);
}

WTP_API int wtp_block_open(wtp_ctx* ctx, const wtp_block_desc* desc, const void* d_owned_xyz, const int64_t* d_gid,
                           int64_t n_owned, const wtp_spacing_desc* spacing, const wtp_force_desc* force, int k,
                           double alpha_lo, double alpha_max) {
    if (!ctx) return WTP_ERR_ARG;
    if (!desc || !desc->boxes) return fail(ctx, WTP_ERR_ARG, "wtp_block_open: descriptor / boxes is NULL");
    if (desc->nranks < 1 || desc->rank < 0 || desc->rank >= desc->nranks) return fail(ctx, WTP_ERR_ARG, "wtp_block_open: 0 <= rank < nranks");
    if (!(desc->ghost_width > 0)) return fail(ctx, WTP_ERR_ARG, "wtp_block_open: ghost_width must be > 0");
    if (n_owned < 1 || !d_owned_xyz) return fail(ctx, WTP_ERR_ARG, "wtp_block_open: every rank needs at least one owned point");
    if (spacing && spacing->kind == WTP_SPACING_PER_POINT)
        return fail(ctx, WTP_ERR_ARG, "wtp_block_open: constant spacing or a device-evaluated law (not a PER_POINT array)");
    if (!ctx->block) ctx->block = new BlockState();
    BlockState* b = bs_of(ctx);
    if (b->active) return fail(ctx, WTP_ERR_STATE, "wtp_block_open: a block session is open already");
    if (int rc = transport_ready(ctx, desc->rank, desc->nranks, "wtp_block_open: ")) return rc;
    for (int r = 0; r < desc->nranks; ++r)
        for (int ax = 0; ax < 3; ++ax)
            if (!(desc->boxes[(size_t)r * 6 + ax] < desc->boxes[(size_t)r * 6 + 3 + ax]))
                return fail(ctx, WTP_ERR_ARG, "wtp_block_open: every box needs lo < hi on every axis");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    b->rank = desc->rank;
    b->nranks = desc->nranks;
    b->boxes.assign(desc->boxes, desc->boxes + (size_t)desc->nranks * 6);
    b->w = desc->ghost_width;
    b->margin = desc->margin < 0 ? 0.25 * desc->ghost_width : desc->margin;
    int rc;
    // the session starts on [selected wall ; owned] with the wall as its fixed head: one rank is the plain session
    double lo[3], hi[3];
    blk_coverage(b, lo, hi);
    if ((rc = blk_select_wall(ctx, b, lo, hi))) return rc;
    const void* snap = d_owned_xyz;
    if (b->n_sel) {
        if (b->n_sel + n_owned > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "wtp_block_open: wall + owned points exceed the int32 index space");
        if ((rc = ensure(ctx, b->snap, 12 * (size_t)(b->n_sel + n_owned)))) return rc;
        WTP_HIP(ctx, hipMemcpy2DAsync(b->snap.p, 12, b->wall_rows.p, 16, 12, (size_t)b->n_sel, hipMemcpyDeviceToDevice, ctx->stream));
        WTP_HIP(ctx, hipMemcpyAsync((char*)b->snap.p + 12 * (size_t)b->n_sel, d_owned_xyz, 12 * (size_t)n_owned,
                                    hipMemcpyDeviceToDevice, ctx->stream));
        snap = b->snap.p;
    }
    if ((rc = wtp_relax_init_dev(ctx, snap, b->n_sel + n_owned, b->n_sel, 3, WTP_F32, spacing, force, k, alpha_lo, alpha_max)))
        return rc;
    b->wall_dirty = false;
    b->pool_wall_ok = false;
    ctx->relax.shard_grid_reuse = true;
    b->widened = 0;
    b->n_owned = n_owned;
    b->n_ghost = 0;
    b->send_cap = b->mig_cap = 0;
    b->plan_ready = false;
    b->gid_cur = 0;
    b->info = wtp_block_info{};
    if ((rc = ensure(ctx, b->gid[0], sizeof(int64_t) * (size_t)n_owned))) return rc;
    if (d_gid) {
        WTP_HIP(ctx, hipMemcpyAsync(b->gid[0].p, d_gid, sizeof(int64_t) * (size_t)n_owned, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        hipLaunchKernelGGL(blk_iota_gid_kernel, dim3(1024), dim3(256), 0, ctx->stream, (int64_t*)b->gid[0].p, n_owned);
    }
    WTP_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the caller's arrays are free again
    b->snap = DevBuf();                               // (the session holds its own copy of [wall ; owned])
    if ((rc = blk_geometry(ctx, b))) {
        wtp_relax_end(ctx);
        return rc;
    }
    b->active = true;
    return WTP_OK;
}

// the exchange the plan describes: ghost rows into the pool, migrants into recv_mig; then the owned set and the ghosts
static int blk_exchange_and_apply(wtp_ctx* ctx, BlockState* b) {
    RelaxState& r = ctx->relax;
    const int np = b->geom.np;
    int64_t n_recv = 0, n_rmig = 0, n_send = 0, n_mig = 0;
    for (int q = 0; q < np; ++q) {
        n_recv += b->recv_cnt[q];
        n_rmig += b->rmig_cnt[q];
        n_send += b->send_cnt[q];
        n_mig += b->mig_cnt[q];
    }
    int rc;
    const int64_t n_pool = n_recv + n_mig; // peers' rows + my own emigrants
    // pool = [selected wall (a resident prefix) ; peers' rows ; my emigrants]: the whole fixed head in one array
    const int64_t n_sel = b->n_sel;
    // (ensure frees and allocates anew when it grows the buffer, possibly at the same address: the capacity tells)
    const size_t pool_cap0 = b->pool.cap;
    if ((rc = ensure(ctx, b->pool, 16 * (size_t)(n_sel + n_pool + 16)))) return rc;
    if (b->pool.cap != pool_cap0) b->pool_wall_ok = false;
    if (n_sel && !b->pool_wall_ok) {
        WTP_HIP(ctx, hipMemcpyAsync(b->pool.p, b->wall_rows.p, 16 * (size_t)n_sel, hipMemcpyDeviceToDevice, ctx->stream));
        b->pool_wall_ok = true;
    }
    char* const ghost_base = (char*)b->pool.p + 16 * (size_t)n_sel;
    if ((rc = ensure(ctx, b->recv_mig, 32 * (size_t)(n_rmig + 16)))) return rc;
    // nobody crosses in this iteration (the usual case): the owned set stays, so its part of the rebuild can start early
    const bool early = ctx->block_overlap && np > 0 && n_mig == 0 && n_rmig == 0;
    // messages: per peer (ascending rank) ghosts, then migrants
    std::vector<int> peers;
    std::vector<const void*> sp;
    std::vector<void*> rp;
    std::vector<int64_t> sn, rn;
    int64_t so = 0, mo = 0, ro = 0, rmo = 0;
    for (int q = 0; q < np; ++q) {
        peers.push_back(b->peers[q]);
        sp.push_back((const char*)b->send.p + 16 * (size_t)so);
        sn.push_back(b->send_cnt[q]);
        rp.push_back(ghost_base + 16 * (size_t)ro);
        rn.push_back(b->recv_cnt[q]);
        peers.push_back(b->peers[q]);
        sp.push_back((const char*)b->send_mig.p + 32 * (size_t)mo);
        sn.push_back(2 * b->mig_cnt[q]);
        rp.push_back((char*)b->recv_mig.p + 32 * (size_t)rmo);
        rn.push_back(2 * b->rmig_cnt[q]);
        so += b->send_cnt[q];
        mo += b->mig_cnt[q];
        ro += b->recv_cnt[q];
        rmo += b->rmig_cnt[q];
    }
    if (np > 0) { // (a rank without neighbours posts no round)
        const RowRegion out[2] = {{b->send.p, n_send}, {b->send_mig.p, 2 * n_mig}};
        const RowRegion in[2] = {{ghost_base, n_recv}, {b->recv_mig.p, 2 * n_rmig}};
        // while the rows travel, the stream ranks the owned points into the cells (the first pass of the rebuild, which
        // does not need the ghosts)
        int64_t n_head = n_sel + n_pool;
        auto prerank = [](wtp_ctx* c, void* n_fixed_new) { return relax_prerank(c, *(const int64_t*)n_fixed_new); };
        if ((rc = transport_exchange(ctx, (int)peers.size(), peers.data(), sp.data(), sn.data(), rp.data(), rn.data(), 2, out, in,
                                     early ? +prerank : nullptr, &n_head, "wtp_block")))
            return rc;
    }
    // my emigrants: ghosts for this iteration
    if (n_mig)
        hipLaunchKernelGGL(blk_emigrant_ghosts_kernel, dim3(64), dim3(256), 0, ctx->stream, (const float4*)b->send_mig.p, n_mig,
                           (float4*)ghost_base + n_recv);
    // the owned set changes only when somebody crossed
    if (n_mig || n_rmig) {
        const int64_t n_stay = b->n_owned - n_mig, n_new = n_stay + n_rmig;
        if (n_new < 1) return fail(ctx, WTP_ERR_STATE, "wtp_block: every owned point of this rank migrated away");
        const int nxt = 1 - b->gid_cur;
        if ((rc = ensure(ctx, b->gid[nxt], sizeof(int64_t) * (size_t)(n_new + n_new / 8)))) return rc;
        const float4* P = (const float4*)ctx->pts[r.bufP].p;
        const int64_t n = r.n;
        const int32_t n_fixed = (int32_t)r.n_fixed;
        void* buf = nullptr;
        if ((rc = relax_swap_begin(ctx, n_new, &buf))) return rc;
        const int64_t nsp = blk_nspans(n);
        const int grid = (int)((nsp + kBlkWaves - 1) / kBlkWaves);
        hipLaunchKernelGGL(blk_compact_kernel, dim3(grid), dim3(64 * kBlkWaves), 0, ctx->stream, P, n, n_fixed, np,
                           (const uint32_t*)b->flags.p, (const int32_t*)b->span_counts.p, (const int64_t*)b->gid[b->gid_cur].p,
                           (float4*)buf, (int64_t*)b->gid[nxt].p);
        if (n_rmig)
            hipLaunchKernelGGL(blk_arrivals_kernel, dim3(64), dim3(256), 0, ctx->stream, (const float4*)b->recv_mig.p, n_rmig, n_stay,
                               (float4*)buf, (int64_t*)b->gid[nxt].p);
        WTP_HIP(ctx, hipGetLastError());
        if ((rc = relax_swap_commit(ctx, n_new))) return rc;
        b->gid_cur = nxt;
        b->n_owned = n_new;
    }
    b->info.n_emigrated = n_mig;
    b->info.n_immigrated = n_rmig;
    b->info.n_sent_rows = n_send;
    b->info.n_recv_rows = n_recv;
    b->n_ghost = n_pool;
    WTP_HIP(ctx, hipGetLastError());
    // no ghosts before, none now, the same wall: the session is untouched (one rank: it IS the plain session)
    if (n_pool == 0 && r.n_fixed == n_sel && !b->wall_dirty) return WTP_OK;
    b->wall_dirty = false;
    const int64_t n_head = n_sel + n_pool;
    return relax_set_fixed_dev_impl(ctx, n_head ? b->pool.p : nullptr, n_head, true); // (the pool is ours: no wait for the copy)
}

WTP_API int wtp_block_step(wtp_ctx* ctx, wtp_step_stats* stats, wtp_block_info* info) {
    if (!ctx) return WTP_ERR_ARG;
    BlockState* b = bs_of(ctx);
    if (!b || !b->active) return fail(ctx, WTP_ERR_STATE, "wtp_block_step before wtp_block_open");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    const int64_t syncs0 = ctx->n_syncs, pre0 = ctx->preranked_builds;
    b->info.redone = 0;
    if ((rc = ensure(ctx, ctx->stats, sizeof(wtp_step_stats)))) return rc;
    wtp_step_stats g{};
    for (int attempt = 0;; ++attempt) {
        if (!b->plan_ready)
            if ((rc = blk_plan(ctx, b, nullptr, nullptr))) return rc; // first iteration / after a widening: one extra gather
        b->plan_ready = false;
        if ((rc = blk_exchange_and_apply(ctx, b))) return rc;
        if ((rc = relax_step_enqueue(ctx, 1, (wtp_step_stats*)ctx->stats.p))) return rc;
        // the next exchange's rows and counts, from the positions this sweep produced; they ride with its statistics
        if ((rc = blk_plan(ctx, b, (const wtp_step_stats*)ctx->stats.p, &g))) return rc;
        if (g.n_uncovered == 0) break;
        // some query's support reaches past the covered box somewhere: everybody undoes the step, widens and repeats it
        if (attempt >= 4) return fail(ctx, WTP_ERR_STATE, "wtp_block: queries still reach past the ghost layer after 4 widenings");
        if ((rc = wtp_relax_revert(ctx))) return rc;
        b->w *= 1.5;
        b->widened += 1;
        b->info.redone = 1;
        b->plan_ready = false;
        if ((rc = blk_geometry(ctx, b))) return rc;
    }
    b->info.host_syncs = (int32_t)(ctx->n_syncs - syncs0);
    b->info.overlapped = (int32_t)(ctx->preranked_builds - pre0);
    b->info.reserved = 0;
    b->info.n_owned = b->n_owned;
    b->info.n_ghost = b->n_ghost;
    b->info.n_peers = b->geom.np;
    b->info.widened = b->widened;
    b->info.ghost_width = b->w;
    if (stats) *stats = g;
    if (info) *info = b->info;
    return WTP_OK;
}

WTP_API int wtp_block_run(wtp_ctx* ctx, int n_iters, double* conv_out, wtp_step_stats* last, wtp_block_info* info) {
    if (!ctx) return WTP_ERR_ARG;
    if (n_iters < 0) return fail(ctx, WTP_ERR_ARG, "n_iters must be >= 0");
    wtp_step_stats st{};
    wtp_block_info inf{};
    int syncs = 0;
    for (int i = 0; i < n_iters; ++i) {
        int rc = wtp_block_step(ctx, &st, &inf);
        if (rc) return rc;
        syncs += inf.host_syncs;
        if (conv_out) conv_out[i] = st.max_force;
    }
    inf.host_syncs = syncs;
    if (last) *last = st;
    if (info) *info = inf;
    return WTP_OK;
}

// The stop rules of `_relax!` (src/repel.jl:305-334; stop_rules_apply, wtp_internal.hpp) on the global statistics, with
// the positions reverted on cv_target.  Every rank evaluates the same numbers.
WTP_API int wtp_block_run_until(wtp_ctx* ctx, int max_iters, double tol, int stall_after, double cv_target, double* conv_out,
                                int* n_done, int* reason, wtp_step_stats* last) {
    if (!ctx) return WTP_ERR_ARG;
    if (max_iters < 0) return fail(ctx, WTP_ERR_ARG, "max_iters must be >= 0");
    BlockState* b = bs_of(ctx);
    if (!b || !b->active) return fail(ctx, WTP_ERR_STATE, "wtp_block_run_until before wtp_block_open");
    wtp_step_stats st{};
    StopState ss{};
    ss.best_cv = std::numeric_limits<double>::infinity();
    for (int i = 1; i <= max_iters && !ss.stopped; ++i) {
        int rc = wtp_block_step(ctx, &st, nullptr);
        if (rc) return rc;
        if (conv_out) conv_out[i - 1] = st.max_force;
        stop_rules_apply(ss, st, i, tol, stall_after, cv_target);
        if (ss.reason == 2) {
            // p .= p_old (src/repel.jl:314): the sweep is undone; the plan made from its positions is void
            if ((rc = wtp_relax_revert(ctx))) return rc;
            b->plan_ready = false;
        }
    }
    if (n_done) *n_done = ss.n_done;
    if (reason) *reason = ss.reason;
    if (last) *last = st;
    return WTP_OK;
}

WTP_API int wtp_block_get(wtp_ctx* ctx, void* d_xyz_out, int64_t* d_gid_out, int64_t cap, int64_t* n_owned) {
    if (!ctx) return WTP_ERR_ARG;
    BlockState* b = bs_of(ctx);
    if (!b || !b->active) return fail(ctx, WTP_ERR_STATE, "wtp_block_get before wtp_block_open");
    if (n_owned) *n_owned = b->n_owned;
    if (!d_xyz_out && !d_gid_out) return WTP_OK;
    if (cap < b->n_owned) return fail(ctx, WTP_ERR_ARG, "wtp_block_get: buffers too small");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if (d_gid_out)
        WTP_HIP(ctx, hipMemcpyAsync(d_gid_out, b->gid[b->gid_cur].p, sizeof(int64_t) * (size_t)b->n_owned, hipMemcpyDeviceToDevice, ctx->stream));
    if (d_xyz_out) {
        if ((rc = wtp_relax_get_dev(ctx, d_xyz_out))) return rc; // (synchronises)
    } else {
        WTP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return WTP_OK;
}
