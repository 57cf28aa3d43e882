// wtp_block_topo.hip — sharded set_topology: KNN and radius rows of a cloud that stays split across ranks
// (include/wtp.h: wtp_block_knn, wtp_block_radius_*).
//
// Same decomposition as the block driver (wtp_block.hip) and the same Transport (wtp_comm.hip), no iteration.  Per call
// and rank:
//
//   1. one all-gather of a header {status, owned count, bounding box of the owned points, gid range and fingerprint,
//      arguments}; every check that needs global knowledge runs on the gathered words, so every rank returns the same
//      status and none waits alone in a later collective.
//   2. ghosts: rank r sends rank q every owned point inside q's box grown by q's own width (inclusive; thresholds rounded
//      outward) — per-span counts, the driver's column scan, fill in slot order; one all-gather of the row counts per
//      destination, then one grouped exchange with exact sizes.
//   3. gid order: the local set [owned ; ghosts] is laid out by ascending gid (a bitmap of N_total bits, marked with
//      atomic ORs — a bit found set is a gid seen twice — then a popcount scan gives every gid its local index).  The
//      single-context kernels rank by (d², local index), which is then (d², gid): every tie resolves as on one GPU.
//   4. the k-NN / radius kernels of wtp_knn_dev / wtp_radius_* search the whole local set.
//   5. certificate + translation (one kernel): owned row i is complete if its k-th d² (radius: r²) lies strictly below
//      the squared distance to the nearest face of the grown box, with a margin for fp32 rounding; faces beyond the
//      global bounding box are infinitely far.  The same kernel writes the row in global ids, in the caller's order.
//      One all-gather of {status, incomplete rows}: ranks with incomplete rows widen by 1.5x and all redo 2-5.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "wtp_device.hpp"

namespace wtp {

constexpr int kTpMaxDest = 64;   // destinations of one rank's ghost rows: lane c of a wave holds column c's count
constexpr int kTpPasses = 16;    // a wave owns 64 * 16 consecutive points ("span"), as in the block driver
constexpr int kTpSpan = 64 * kTpPasses;
constexpr int kTpWaves = 4;
constexpr int kTpHdr = 16;       // words of the header all-gather
constexpr int kTpMaxRounds = 40; // widenings by 1.5x: from any estimate past the global box long before this
// relative slack of the certificate: a computed fp32 d² is within a few ulps (~4e-7) of the exact one, and the stored
// distance is sqrt(d²) rounded to fp32
constexpr double kTpSlack = 1.0e-5;
constexpr double kTpGrow = 1.5;

struct TpGeom {
    int nd;
    float lo[kTpMaxDest][3], hi[kTpMaxDest][3]; // destination's box grown by its width, rounded outward (inclusive)
};

struct TpBox {
    double lo[3], hi[3]; // this rank's box grown by its width; +-inf where that face lies beyond the global box
};

struct TpStats {
    uint32_t key_lo[3], key_hi[3]; // bounding box of the owned points as ordered keys (tp_key)
    unsigned long long gmax;       // largest gid as uint64: a negative gid shows as >= 2^31
    unsigned long long fp;         // sum of tp_mix(gid) mod 2^64
    unsigned long long dup;        // gids found twice in the local set
    unsigned long long n_uncert;   // owned rows without a certificate
};

__host__ __device__ inline uint32_t tp_key(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float tp_unkey(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__host__ __device__ inline unsigned long long tp_mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct TopoState {
    DevBuf own4, recv, send, span_counts, totals, stats, bm, pc, off, scan_tmp;
    DevBuf lxyz, lgid, opos, lidx, ldist, lcnt, loff, ridx, cnt_own, own_off;
    DevBuf sdist;           // wtp_block_knn_stats: the owned rows' distances
    bool rad_ready = false; // a wtp_block_radius_offsets call left its rows here for wtp_block_radius_fill
    int64_t rad_n_owned = 0, rad_nnz = 0;
};

static TopoState* ts_of(wtp_ctx* ctx) {
    if (!ctx->block_topo) ctx->block_topo = new TopoState();
    return (TopoState*)ctx->block_topo;
}

void block_topo_destroy(wtp_ctx* ctx) {
    if (!ctx->block_topo) return;
    hipSetDevice(ctx->device);
    delete (TopoState*)ctx->block_topo; // (frees the device buffers)
    ctx->block_topo = nullptr;
}

// ---- kernels --------------------------------------------------------------------------------------------------------

// owned points -> rows {x, y, z, bits(gid)}; bounding box, largest gid and gid fingerprint (wave sums, one atomic each)
__global__ __launch_bounds__(256) void tp_pack_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ gid, int64_t n,
                                                      float4* __restrict__ own4, TpStats* __restrict__ st) {
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    unsigned long long gmax = 0, fp = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        const int64_t g = gid[i];
        own4[i] = make_float4(x, y, z, __builtin_bit_cast(float, (uint32_t)g));
        const uint32_t k[3] = {tp_key(x), tp_key(y), tp_key(z)};
        for (int a = 0; a < 3; ++a) {
            lo[a] = k[a] < lo[a] ? k[a] : lo[a];
            hi[a] = k[a] > hi[a] ? k[a] : hi[a];
        }
        gmax = (unsigned long long)g > gmax ? (unsigned long long)g : gmax;
        fp += tp_mix((unsigned long long)g);
    }
    for (int m = 32; m > 0; m >>= 1) {
        for (int a = 0; a < 3; ++a) {
            const uint32_t l = __shfl_xor(lo[a], m), h = __shfl_xor(hi[a], m);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
        const unsigned long long g = __shfl_xor(gmax, m);
        gmax = g > gmax ? g : gmax;
        fp += __shfl_xor(fp, m);
    }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) {
            atomicMin(&st->key_lo[a], lo[a]);
            atomicMax(&st->key_hi[a], hi[a]);
        }
        atomicMax(&st->gmax, gmax);
        atomicAdd(&st->fp, fp);
    }
}

// sum of tp_mix(g) over g = 0 .. n-1: the fingerprint of a gid set that is exactly a permutation
__global__ __launch_bounds__(256) void tp_fingerprint_kernel(int64_t n, unsigned long long* __restrict__ out) {
    unsigned long long s = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        s += tp_mix((unsigned long long)i);
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, s);
}

__device__ inline bool tp_inside(const float4& p, const TpGeom& g, int d) {
    return p.x >= g.lo[d][0] && p.x <= g.hi[d][0] && p.y >= g.lo[d][1] && p.y <= g.hi[d][1] && p.z >= g.lo[d][2] &&
           p.z <= g.hi[d][2];
}

// per span and destination: rows this span sends (layout of blk_scan_kernel: span_counts[span * nd + d])
__global__ __launch_bounds__(64 * kTpWaves) void tp_count_kernel(const float4* __restrict__ P, int64_t n, TpGeom g,
                                                                 int32_t* __restrict__ span_counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t span = (int64_t)blockIdx.x * kTpWaves + wave;
    const int64_t first = span * kTpSpan;
    if (first >= n) return;
    float4 pp[kTpPasses];
#pragma unroll
    for (int pass = 0; pass < kTpPasses; ++pass) {
        const int64_t i = first + (int64_t)pass * 64 + lane;
        pp[pass] = P[i < n ? i : n - 1];
    }
    int cnt = 0;
#pragma unroll
    for (int pass = 0; pass < kTpPasses; ++pass) {
        const bool live = first + (int64_t)pass * 64 + lane < n;
        for (int d = 0; d < g.nd; ++d) {
            const unsigned long long m = __ballot(live && tp_inside(pp[pass], g, d));
            if (lane == d) cnt += __popcll(m);
        }
    }
    if (lane < g.nd) span_counts[span * g.nd + lane] = cnt;
}

// the send rows: destination d's rows start at sum_{j<d} totals[j], in slot order inside (same predicate as the count)
__global__ __launch_bounds__(64 * kTpWaves) void tp_fill_kernel(const float4* __restrict__ P, int64_t n, TpGeom g,
                                                                const int32_t* __restrict__ span_off,
                                                                const int32_t* __restrict__ totals, float4* __restrict__ send) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t span = (int64_t)blockIdx.x * kTpWaves + wave;
    const int64_t first = span * kTpSpan;
    if (first >= n) return;
    int run = 0; // lane d: where destination d's next row of this span goes
    if (lane < g.nd) {
        int base = 0;
        for (int j = 0; j < lane; ++j) base += totals[j];
        run = base + span_off[span * g.nd + lane];
    }
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int pass = 0; pass < kTpPasses; ++pass) {
        const int64_t i = first + (int64_t)pass * 64 + lane;
        const bool live = i < n;
        const float4 p = P[live ? i : n - 1];
        for (int d = 0; d < g.nd; ++d) {
            const bool in = live && tp_inside(p, g, d);
            const unsigned long long m = __ballot(in);
            if (m) {
                const int o = __builtin_amdgcn_readlane(run, d);
                if (in) send[(int64_t)o + __popcll(m & below)] = p;
                if (lane == d) run += __popcll(m);
            }
        }
    }
}

__device__ inline float4 tp_elem(const float4* own4, int64_t n_own, const float4* recv, int64_t e) {
    return e < n_own ? own4[e] : recv[e - n_own];
}

// one bit per gid of the local set; a bit that was set already is a gid seen twice
__global__ __launch_bounds__(256) void tp_mark_kernel(const float4* __restrict__ own4, int64_t n_own, const float4* __restrict__ recv,
                                                      int64_t n_all, uint32_t* __restrict__ bm, TpStats* __restrict__ st) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_all; e += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t g = __builtin_bit_cast(uint32_t, tp_elem(own4, n_own, recv, e).w);
        const uint32_t bit = 1u << (g & 31u);
        if (atomicOr(&bm[g >> 5], bit) & bit) atomicAdd(&st->dup, 1ull);
    }
}

__global__ __launch_bounds__(256) void tp_popc_kernel(const uint32_t* __restrict__ bm, int64_t nwords, int32_t* __restrict__ cnt) {
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (int64_t)gridDim.x * blockDim.x)
        cnt[w] = __popc(bm[w]);
}

// local index of gid g = set bits below g; the local set by ascending gid: xyz, gid, and where each owned point went
__global__ __launch_bounds__(256) void tp_scatter_kernel(const float4* __restrict__ own4, int64_t n_own, const float4* __restrict__ recv,
                                                         int64_t n_all, const uint32_t* __restrict__ bm, const int64_t* __restrict__ off,
                                                         float* __restrict__ lxyz, int32_t* __restrict__ lgid,
                                                         int32_t* __restrict__ opos) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_all; e += (int64_t)gridDim.x * blockDim.x) {
        const float4 p = tp_elem(own4, n_own, recv, e);
        const uint32_t g = __builtin_bit_cast(uint32_t, p.w);
        const uint32_t w = g >> 5;
        const int64_t pos = off[w] + __popc(bm[w] & ((1u << (g & 31u)) - 1u));
        lxyz[3 * pos] = p.x;
        lxyz[3 * pos + 1] = p.y;
        lxyz[3 * pos + 2] = p.z;
        lgid[pos] = (int32_t)g;
        if (e < n_own) opos[e] = (int32_t)pos;
    }
}

// squared distance from p to the nearest face of the certificate box (+inf if every face lies beyond the cloud)
__device__ inline double tp_gap2(const float4& p, const TpBox& b) {
    const double c[3] = {(double)p.x, (double)p.y, (double)p.z};
    double gap = __builtin_inf();
    for (int a = 0; a < 3; ++a) {
        const double l = c[a] - b.lo[a], h = b.hi[a] - c[a];
        gap = l < gap ? l : gap;
        gap = h < gap ? h : gap;
    }
    return gap * gap;
}

// k-NN: owned row i (caller order) in global ids, distances; the thread of the row's last entry checks its certificate
__global__ __launch_bounds__(256) void tp_knn_rows_kernel(const float4* __restrict__ own4, int64_t n_own, const int32_t* __restrict__ opos,
                                                          const int32_t* __restrict__ lidx, const float* __restrict__ ldist,
                                                          const int32_t* __restrict__ lgid, int k, TpBox box,
                                                          int64_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                          TpStats* __restrict__ st) {
    const int64_t total = n_own * k;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / k;
        const int j = (int)(e - i * k);
        const int64_t src = (int64_t)opos[i] * k + j;
        if (out_idx) out_idx[e] = lgid[lidx[src]];
        const float d = ldist[src];
        if (out_dist) out_dist[e] = d;
        if (j == k - 1) {
            const double d2 = (double)d * (double)d;
            if (!(d2 * (1.0 + kTpSlack) < tp_gap2(own4[i], box))) atomicAdd(&st->n_uncert, 1ull);
        }
    }
}

// radius: owned row lengths in caller order, and the certificate (r² below the gap: the row cannot miss a point)
__global__ __launch_bounds__(256) void tp_radius_rows_kernel(const float4* __restrict__ own4, int64_t n_own,
                                                             const int32_t* __restrict__ opos, const int32_t* __restrict__ lcnt,
                                                             double r2s, TpBox box, int32_t* __restrict__ cnt_own,
                                                             TpStats* __restrict__ st) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_own; i += (int64_t)gridDim.x * blockDim.x) {
        cnt_own[i] = lcnt[opos[i]];
        if (!(r2s < tp_gap2(own4[i], box))) atomicAdd(&st->n_uncert, 1ull);
    }
}

// radius fill: owned row i copied out of the local CSR, local indices -> gids
__global__ __launch_bounds__(256) void tp_radius_fill_kernel(int64_t n_own, const int32_t* __restrict__ opos,
                                                             const int64_t* __restrict__ loff, const int32_t* __restrict__ ridx,
                                                             const int32_t* __restrict__ lgid, const int64_t* __restrict__ own_off,
                                                             int64_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_own; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = loff[opos[i]], o = own_off[i], len = own_off[i + 1] - o;
        for (int64_t j = 0; j < len; ++j) out[o + j] = lgid[ridx[a + j]];
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------

struct TpCall {
    int rank, nranks;
    const float* xyz;
    const int64_t* gid;
    int64_t n;
    int k, include_self; // k == 0: radius
    double r, width;
    int64_t* idx_out;
    float* dist_out;
    int64_t* off_out;
    bool stats = false;   // wtp_block_knn_stats: k >= 2, the rows' ids are not wanted
    int local_reason = 0; // a check the entry point made on its own arguments failed (tp_reason)
};

static double hdr_d(int64_t w) { return __builtin_bit_cast(double, w); }
static int64_t hdr_w(double v) { return __builtin_bit_cast(int64_t, v); }

// local reasons a rank reports in its header (all ranks fail with the reporting rank's status)
static const char* tp_reason(int64_t code) {
    switch (code) {
    case 1: return "a relax or block session is open on the context";
    case 2: return "a NULL input or output array with n_owned > 0";
    case 3: return "n_owned < 0";
    case 4: return "k must be >= 1";
    case 5: return "radius must be finite and > 0";
    case 6: return "width must not be NaN";
    case 7: return "k must be >= 2 (k counts the point itself)";
    case 8: return "out is NULL";
    case 9: return "h_const must be finite, coord_radius finite and >= 0";
    default: return "failed its checks";
    }
}

static float tp_down(double v) {
    float f = (float)v;
    if ((double)f > v) f = std::nextafter(f, -std::numeric_limits<float>::infinity());
    return f;
}
static float tp_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
}

static int tp_run(wtp_ctx* ctx, const TpCall& c, wtp_block_topo_info* info) {
    const bool knn = c.k != 0;
    const char* who = c.stats ? "wtp_block_knn_stats: " : knn ? "wtp_block_knn: " : "wtp_block_radius_offsets: ";
    if (c.nranks < 1 || c.rank < 0 || c.rank >= c.nranks) return fail(ctx, WTP_ERR_ARG, std::string(who) + "0 <= rank < nranks");
    if (int rcr = transport_ready(ctx, c.rank, c.nranks, who)) return rcr;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    TopoState* s = ts_of(ctx);
    s->rad_ready = false;
    // every rank's words into all[nranks * nwords], rank-major
    auto allgather = [&](const int64_t* mine, int64_t* all, int nwords) {
        return transport_allgather(ctx, c.nranks, mine, false, all, nwords, "wtp_block topology");
    };
    const int64_t syncs0 = ctx->n_syncs;
    const int R = c.nranks, me = c.rank;
    const int64_t n = c.n;
    int rc;

    // ---- 1. the header ----
    int64_t status = 0, reason = 0;
    if (ctx->relax.active || block_session_open(ctx)) status = WTP_ERR_STATE, reason = 1;
    else if (n < 0) status = WTP_ERR_ARG, reason = 3;
    else if (c.local_reason) status = WTP_ERR_ARG, reason = c.local_reason;
    else if (knn && c.k < (c.stats ? 2 : 1)) status = WTP_ERR_ARG, reason = c.stats ? 7 : 4;
    else if (!knn && !(c.r > 0 && std::isfinite(c.r))) status = WTP_ERR_ARG, reason = 5;
    else if (std::isnan(c.width)) status = WTP_ERR_ARG, reason = 6;
    else if (n > 0 && (!c.xyz || !c.gid || !(c.stats ? (const void*)c.dist_out : knn ? (const void*)c.idx_out : (const void*)c.off_out))) status = WTP_ERR_ARG, reason = 2;
    TpStats hs{};
    if ((rc = ensure(ctx, s->stats, sizeof(TpStats) + 64))) return rc; // (the fingerprint sum sits behind the statistics)
    if (!status && n > 0) {
        if ((rc = ensure(ctx, s->own4, 16 * (size_t)n))) return rc;
        for (int a = 0; a < 3; ++a) hs.key_lo[a] = 0xFFFFFFFFu;
        WTP_HIP(ctx, hipMemcpyAsync(s->stats.p, &hs, sizeof(TpStats), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(tp_pack_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, ctx->stream, c.xyz, c.gid, n,
                           (float4*)s->own4.p, (TpStats*)s->stats.p);
        WTP_HIP(ctx, hipGetLastError());
        WTP_HIP(ctx, hipMemcpyAsync(&hs, s->stats.p, sizeof(TpStats), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
    }
    int64_t hdr[kTpHdr] = {status, reason, status ? 0 : n, (int64_t)hs.gmax, (int64_t)hs.fp, c.k, c.include_self ? 1 : 0,
                           hdr_w(c.r), hdr_w(c.width)};
    for (int a = 0; a < 3; ++a) {
        hdr[9 + a] = hdr_w((double)tp_unkey(hs.key_lo[a]));
        hdr[12 + a] = hdr_w((double)tp_unkey(hs.key_hi[a]));
    }
    std::vector<int64_t> all((size_t)R * kTpHdr);
    if ((rc = allgather(hdr, all.data(), kTpHdr))) return rc;
    auto H = [&](int q, int w) { return all[(size_t)q * kTpHdr + w]; };

    // ---- global checks on the gathered words: the same verdict on every rank ----
    for (int q = 0; q < R; ++q)
        if (H(q, 0))
            return fail(ctx, (int)H(q, 0), std::string(who) + "rank " + std::to_string(q) + ": " + tp_reason(H(q, 1)));
    int64_t N = 0;
    unsigned long long gmax = 0, fp = 0;
    bool any = false;
    for (int q = 0; q < R; ++q) {
        if (H(q, 5) != H(0, 5) || H(q, 6) != H(0, 6) || H(q, 7) != H(0, 7))
            return fail(ctx, WTP_ERR_ARG, std::string(who) + "ranks disagree on k / include_self / r");
        const int64_t nq = H(q, 2);
        if (nq == 0) continue;
        if ((unsigned long long)H(q, 3) >= (1ull << 31))
            return fail(ctx, WTP_ERR_ARG, std::string(who) + "rank " + std::to_string(q) + " holds a gid outside [0, 2^31)");
        N += nq;
        gmax = !any || (unsigned long long)H(q, 3) > gmax ? (unsigned long long)H(q, 3) : gmax;
        fp += (unsigned long long)H(q, 4);
        any = true;
    }
    if (N >= (1ll << 31)) return fail(ctx, WTP_ERR_ARG, std::string(who) + "more than 2^31 - 1 points in all");
    if (knn) {
        if (c.k > kGenericKMax) return fail(ctx, WTP_ERR_ARG, std::string(who) + "k > 128 is not supported");
        if ((int64_t)c.k > N - (c.include_self ? 0 : 1))
            return fail(ctx, WTP_ERR_ARG, std::string(who) + "k exceeds the number of available neighbours (k+1 > N_total)");
    }
    if (N > 0 && gmax >= (unsigned long long)N)
        return fail(ctx, WTP_ERR_ARG, std::string(who) + "the gids of all ranks must be exactly 0 .. N_total - 1 (a gid >= N_total)");
    if (N > 0) { // with the count and the largest gid right, a fingerprint off the permutation's means a gid owned twice
        unsigned long long* d_fp = (unsigned long long*)((char*)s->stats.p + sizeof(TpStats));
        WTP_HIP(ctx, hipMemsetAsync(d_fp, 0, 8, ctx->stream));
        hipLaunchKernelGGL(tp_fingerprint_kernel, dim3(grid_for(N, 256, 2048)), dim3(256), 0, ctx->stream, N, d_fp);
        WTP_HIP(ctx, hipGetLastError());
        unsigned long long want = 0;
        WTP_HIP(ctx, hipMemcpyAsync(&want, d_fp, 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
        if (want != fp)
            return fail(ctx, WTP_ERR_ARG, std::string(who) + "a gid is owned by more than one rank (the gids must be 0 .. N_total - 1, each once)");
    }
    if (N == 0) {
        if (!knn && c.off_out) WTP_HIP(ctx, hipMemsetAsync(c.off_out, 0, 8, ctx->stream));
        if (info) *info = wtp_block_topo_info{};
        return sync(ctx);
    }

    // ---- boxes and widths (identical on every rank) ----
    std::vector<double> box((size_t)R * 6, 0.0), w(R, 0.0);
    double glo[3], ghi[3];
    for (int a = 0; a < 3; ++a) glo[a] = std::numeric_limits<double>::infinity(), ghi[a] = -glo[a];
    for (int q = 0; q < R; ++q) {
        if (!H(q, 2)) continue;
        for (int a = 0; a < 3; ++a) {
            box[(size_t)q * 6 + a] = hdr_d(H(q, 9 + a));
            box[(size_t)q * 6 + 3 + a] = hdr_d(H(q, 12 + a));
            glo[a] = std::min(glo[a], box[(size_t)q * 6 + a]);
            ghi[a] = std::max(ghi[a], box[(size_t)q * 6 + 3 + a]);
        }
    }
    double gext = 0;
    for (int a = 0; a < 3; ++a) gext = std::max(gext, ghi[a] - glo[a]);
    if (!(gext > 0)) gext = 1.0; // (every point in one place: any width covers the cloud)
    for (int q = 0; q < R; ++q) {
        if (!H(q, 2)) continue;
        if (!knn) {
            w[q] = c.r * (1.0 + 2.0 * kTpSlack); // r rounded outward: every row certifies in the first round
        } else if (hdr_d(H(q, 8)) > 0) {
            w[q] = hdr_d(H(q, 8));
        } else {
            // a few times the expected k-th neighbour distance at this rank's own density
            double vol = 1.0;
            for (int a = 0; a < 3; ++a) vol *= std::max(box[(size_t)q * 6 + 3 + a] - box[(size_t)q * 6 + a], 1e-3 * gext);
            const double h = std::cbrt(vol / (double)H(q, 2));
            w[q] = 1.55 * h * std::cbrt((double)c.k + 1.0);
        }
    }
    auto touches = [&](int r, int q) { // rank r's points may lie in rank q's grown box
        for (int a = 0; a < 3; ++a)
            if (box[(size_t)r * 6 + 3 + a] < box[(size_t)q * 6 + a] - w[q] || box[(size_t)r * 6 + a] > box[(size_t)q * 6 + 3 + a] + w[q])
                return false;
        return true;
    };

    // ---- rounds ----
    const float4* own4 = (const float4*)s->own4.p;
    const int64_t nwords = (N + 31) / 32;
    int64_t n_all = n, n_recv = 0;
    int n_from = 0, round = 0;
    std::vector<int64_t> send_to(R), cnt_all((size_t)R * R), w2(2), g2((size_t)2 * R);
    for (;; ++round) {
        // my destinations and their grown boxes; every rank checks everybody's destination count
        std::vector<int> dest;
        for (int r = 0; r < R; ++r) {
            int nd = 0;
            for (int q = 0; q < R; ++q)
                if (q != r && H(q, 2) && H(r, 2) && touches(r, q)) {
                    ++nd;
                    if (r == me) dest.push_back(q);
                }
            if (nd > kTpMaxDest)
                return fail(ctx, WTP_ERR_ARG, std::string(who) + "a rank's points reach more than 64 other ranks' ghost layers");
        }
        TpGeom geo{};
        geo.nd = (int)dest.size();
        for (int d = 0; d < geo.nd; ++d)
            for (int a = 0; a < 3; ++a) {
                geo.lo[d][a] = tp_down(box[(size_t)dest[d] * 6 + a] - w[dest[d]]);
                geo.hi[d][a] = tp_up(box[(size_t)dest[d] * 6 + 3 + a] + w[dest[d]]);
            }
        // counts per destination, then the rows
        std::fill(send_to.begin(), send_to.end(), 0);
        int64_t n_send = 0;
        const int64_t nsp = (n + kTpSpan - 1) / kTpSpan;
        const int sgrid = (int)((nsp + kTpWaves - 1) / kTpWaves);
        int sp = span_begin(ctx, 2);
        if (geo.nd > 0) {
            if ((rc = ensure(ctx, s->span_counts, sizeof(int32_t) * (size_t)nsp * geo.nd))) return rc;
            if ((rc = ensure(ctx, s->totals, sizeof(int32_t) * kTpMaxDest))) return rc;
            hipLaunchKernelGGL(tp_count_kernel, dim3(sgrid), dim3(64 * kTpWaves), 0, ctx->stream, own4, n, geo,
                               (int32_t*)s->span_counts.p);
            WTP_HIP(ctx, hipGetLastError());
            if ((rc = launch_blk_scan(ctx, (int32_t*)s->span_counts.p, nsp, geo.nd, (int32_t*)s->totals.p))) return rc;
            int32_t tot[kTpMaxDest];
            WTP_HIP(ctx, hipMemcpyAsync(tot, s->totals.p, sizeof(int32_t) * geo.nd, hipMemcpyDeviceToHost, ctx->stream));
            if ((rc = sync(ctx))) return rc;
            for (int d = 0; d < geo.nd; ++d) {
                send_to[dest[d]] = tot[d];
                n_send += tot[d];
            }
            if ((rc = ensure(ctx, s->send, 16 * (size_t)n_send))) return rc;
            if (n_send > 0) {
                hipLaunchKernelGGL(tp_fill_kernel, dim3(sgrid), dim3(64 * kTpWaves), 0, ctx->stream, own4, n, geo,
                                   (const int32_t*)s->span_counts.p, (const int32_t*)s->totals.p, (float4*)s->send.p);
                WTP_HIP(ctx, hipGetLastError());
            }
        }
        span_end(ctx, sp);
        // row counts of every rank to every rank, then one grouped exchange with exact sizes
        if ((rc = allgather(send_to.data(), cnt_all.data(), R))) return rc;
        std::vector<int> peers;
        std::vector<int64_t> sn, rn;
        n_recv = 0;
        n_from = 0;
        for (int q = 0; q < R; ++q) {
            if (q == me) continue;
            const int64_t in = cnt_all[(size_t)q * R + me], out = send_to[q];
            if (in || out) {
                peers.push_back(q);
                sn.push_back(out);
                rn.push_back(in);
            }
            n_recv += in;
            n_from += in > 0;
        }
        if ((rc = ensure(ctx, s->recv, 16 * (size_t)n_recv))) return rc;
        // one grouped round: rows to / from every peer (ascending rank), counts agreed on beforehand
        // (a caller's transport is a collective of all ranks: it is called by every rank of a round, with or without peers)
        if (R > 1 && (!peers.empty() || ctx->transport.host)) {
            std::vector<const void*> sp(peers.size());
            std::vector<void*> rp(peers.size());
            int64_t so = 0, ro = 0;
            for (size_t j = 0; j < peers.size(); ++j) {
                sp[j] = (const float4*)s->send.p + so;
                rp[j] = (float4*)s->recv.p + ro;
                so += sn[j];
                ro += rn[j];
            }
            const RowRegion out{s->send.p, so}, in{s->recv.p, ro};
            if ((rc = transport_exchange(ctx, (int)peers.size(), peers.data(), sp.data(), sn.data(), rp.data(), rn.data(), 1, &out, &in,
                                         nullptr, nullptr, "wtp_block topology")))
                return rc;
        }
        n_all = n + n_recv;

        // the local set in gid order
        int64_t my_status = 0, uncert = 0;
        if (n > 0) {
            sp = span_begin(ctx, 2);
            if ((rc = ensure(ctx, s->bm, 4 * (size_t)nwords))) return rc;
            if ((rc = ensure(ctx, s->pc, 4 * (size_t)nwords))) return rc;
            if ((rc = ensure(ctx, s->off, 8 * (size_t)(nwords + 1)))) return rc;
            if ((rc = ensure(ctx, s->scan_tmp, offsets_scan_tmp_bytes(nwords)))) return rc;
            if ((rc = ensure(ctx, s->lxyz, 12 * (size_t)n_all))) return rc;
            if ((rc = ensure(ctx, s->lgid, 4 * (size_t)n_all))) return rc;
            if ((rc = ensure(ctx, s->opos, 4 * (size_t)n))) return rc;
            TpStats* dst = (TpStats*)s->stats.p;
            WTP_HIP(ctx, hipMemsetAsync(s->stats.p, 0, sizeof(TpStats), ctx->stream));
            WTP_HIP(ctx, hipMemsetAsync(s->bm.p, 0, 4 * (size_t)nwords, ctx->stream));
            const int eg = grid_for(n_all, 256, 4096);
            hipLaunchKernelGGL(tp_mark_kernel, dim3(eg), dim3(256), 0, ctx->stream, own4, n, (const float4*)s->recv.p, n_all,
                               (uint32_t*)s->bm.p, dst);
            hipLaunchKernelGGL(tp_popc_kernel, dim3(grid_for(nwords, 256, 4096)), dim3(256), 0, ctx->stream,
                               (const uint32_t*)s->bm.p, nwords, (int32_t*)s->pc.p);
            WTP_HIP(ctx, hipGetLastError());
            if ((rc = launch_offsets_scan(ctx, (const int32_t*)s->pc.p, nwords, (int64_t*)s->scan_tmp.p, (int64_t*)s->off.p))) return rc;
            hipLaunchKernelGGL(tp_scatter_kernel, dim3(eg), dim3(256), 0, ctx->stream, own4, n, (const float4*)s->recv.p, n_all,
                               (const uint32_t*)s->bm.p, (const int64_t*)s->off.p, (float*)s->lxyz.p, (int32_t*)s->lgid.p,
                               (int32_t*)s->opos.p);
            WTP_HIP(ctx, hipGetLastError());
            span_end(ctx, sp);
            unsigned long long dup = 0;
            WTP_HIP(ctx, hipMemcpyAsync(&dup, &dst->dup, 8, hipMemcpyDeviceToHost, ctx->stream));
            if ((rc = sync(ctx))) return rc;
            // (a gid seen twice leaves holes in the local set: it is not searched)
            if (dup) my_status = WTP_ERR_ARG;
            TpBox cb;
            for (int a = 0; a < 3; ++a) {
                const double lo = box[(size_t)me * 6 + a] - w[me], hi = box[(size_t)me * 6 + 3 + a] + w[me];
                cb.lo[a] = lo <= glo[a] ? -std::numeric_limits<double>::infinity() : lo;
                cb.hi[a] = hi >= ghi[a] ? std::numeric_limits<double>::infinity() : hi;
            }
            const int64_t need = knn ? (int64_t)c.k + (c.include_self ? 0 : 1) : 1;
            if (!my_status && n_all < need) {
                uncert = n; // too few points to search: widen
            } else if (!my_status) {
                if (knn) {
                    if ((rc = ensure(ctx, s->lidx, 4 * (size_t)n_all * c.k))) return rc;
                    if ((rc = ensure(ctx, s->ldist, 4 * (size_t)n_all * c.k))) return rc;
                    if ((rc = topo_knn_local(ctx, (const float*)s->lxyz.p, n_all, c.k, c.include_self, (int32_t*)s->lidx.p,
                                             (float*)s->ldist.p)))
                        return rc;
                    sp = span_begin(ctx, 2);
                    hipLaunchKernelGGL(tp_knn_rows_kernel, dim3(grid_for(n * c.k, 256, 8192)), dim3(256), 0, ctx->stream, own4, n,
                                       (const int32_t*)s->opos.p, (const int32_t*)s->lidx.p, (const float*)s->ldist.p,
                                       (const int32_t*)s->lgid.p, c.k, cb, c.idx_out, c.dist_out, dst);
                } else {
                    if ((rc = ensure(ctx, s->lcnt, 4 * (size_t)n_all))) return rc;
                    if ((rc = ensure(ctx, s->loff, 8 * (size_t)(n_all + 1)))) return rc;
                    if ((rc = ensure(ctx, s->cnt_own, 4 * (size_t)n))) return rc;
                    int64_t nnz_local = 0;
                    if ((rc = topo_radius_local(ctx, (const float*)s->lxyz.p, n_all, c.r, (int32_t*)s->lcnt.p, (int64_t*)s->loff.p,
                                                s->ridx, &nnz_local)))
                        return rc;
                    sp = span_begin(ctx, 2);
                    hipLaunchKernelGGL(tp_radius_rows_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, ctx->stream, own4, n,
                                       (const int32_t*)s->opos.p, (const int32_t*)s->lcnt.p, c.r * c.r * (1.0 + kTpSlack), cb,
                                       (int32_t*)s->cnt_own.p, dst);
                }
                WTP_HIP(ctx, hipGetLastError());
                span_end(ctx, sp);
                unsigned long long nu = 0;
                WTP_HIP(ctx, hipMemcpyAsync(&nu, &dst->n_uncert, 8, hipMemcpyDeviceToHost, ctx->stream));
                if ((rc = sync(ctx))) return rc;
                uncert = (int64_t)nu;
            }
        }
        // {status, incomplete rows} of every rank
        w2[0] = my_status;
        w2[1] = uncert;
        if ((rc = allgather(w2.data(), g2.data(), 2))) return rc;
        int64_t total = 0;
        for (int q = 0; q < R; ++q)
            if (g2[2 * q])
                return fail(ctx, (int)g2[2 * q], std::string(who) + "rank " + std::to_string(q) + " found a gid twice in its local set");
        for (int q = 0; q < R; ++q) total += g2[2 * q + 1];
        if (total == 0) break;
        if (!knn) return fail(ctx, WTP_ERR_STATE, std::string(who) + "radius rows without a certificate at width r");
        if (round + 1 >= kTpMaxRounds)
            return fail(ctx, WTP_ERR_STATE, std::string(who) + "rows still without a certificate after " + std::to_string(round) + " widenings");
        for (int q = 0; q < R; ++q)
            if (g2[2 * q + 1] > 0) w[q] *= kTpGrow;
    }

    if (!knn) { // offsets of the owned rows in caller order
        if ((rc = ensure(ctx, s->own_off, 8 * (size_t)(n + 1)))) return rc;
        if (n > 0) {
            if ((rc = ensure(ctx, s->scan_tmp, offsets_scan_tmp_bytes(std::max(n, nwords))))) return rc;
            if ((rc = launch_offsets_scan(ctx, (const int32_t*)s->cnt_own.p, n, (int64_t*)s->scan_tmp.p, (int64_t*)s->own_off.p)))
                return rc;
        } else {
            WTP_HIP(ctx, hipMemsetAsync(s->own_off.p, 0, 8, ctx->stream));
        }
        if (c.off_out)
            WTP_HIP(ctx, hipMemcpyAsync(c.off_out, s->own_off.p, 8 * (size_t)(n + 1), hipMemcpyDeviceToDevice, ctx->stream));
        int64_t nnz = 0;
        WTP_HIP(ctx, hipMemcpyAsync(&nnz, (int64_t*)s->own_off.p + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
        s->rad_ready = true;
        s->rad_n_owned = n;
        s->rad_nnz = nnz;
    } else if ((rc = sync(ctx))) {
        return rc;
    }
    if (info) {
        info->width = w[me];
        info->n_ghost = n > 0 ? n_all - n : 0;
        info->n_recv_rows = n_recv;
        info->n_peers = n_from;
        info->widened = round;
        info->host_syncs = (int32_t)(ctx->n_syncs - syncs0);
        info->reserved = 0;
    }
    return WTP_OK;
}

} // namespace wtp

using namespace wtp;
#define WTP_API extern "C"

WTP_API int wtp_block_knn(wtp_ctx* ctx, int rank, int nranks, const void* d_xyz, const int64_t* d_gid, int64_t n_owned, int k,
                          int include_self, double width, int64_t* d_idx_out, float* d_dist_out, wtp_block_topo_info* info) {
    if (!ctx) return WTP_ERR_ARG;
    TpCall c{rank, nranks, (const float*)d_xyz, d_gid, n_owned, k < 1 ? -1 : k, include_self, 0.0, width, d_idx_out, d_dist_out, nullptr};
    return tp_run(ctx, c, info);
}

// The sharded metrics: rows as wtp_block_knn's (self included) into an internal buffer, the reductions of wtp_stats.hip on
// the owned rows, one all-gather of {status, first bad spacing index, partial struct}, merged in rank order on every rank.
WTP_API int wtp_block_knn_stats(wtp_ctx* ctx, int rank, int nranks, const void* d_xyz, const int64_t* d_gid, int64_t n_owned, int k,
                                const double* d_h, double h_const, double coord_radius, double width, KnnStats* out,
                                float* d_nn_out, wtp_block_topo_info* info) {
    if (!ctx) return WTP_ERR_ARG;
    const char* who = "wtp_block_knn_stats: ";
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, WTP_ERR_ARG, std::string(who) + "0 <= rank < nranks");
    const char* why = nullptr;
    const int has = knn_stats_spacing(d_h, h_const, coord_radius, &why);
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    TopoState* s = ts_of(ctx);
    const int kk = k < 2 ? -1 : k;
    int rc;
    if (n_owned > 0 && kk > 0 && (rc = ensure(ctx, s->sdist, sizeof(float) * (size_t)n_owned * kk))) return rc;
    TpCall c{rank, nranks, (const float*)d_xyz, d_gid, n_owned, kk, 1, 0.0, width, nullptr, (float*)s->sdist.p, nullptr};
    c.stats = true;
    c.local_reason = !out ? 8 : has < 0 ? 9 : 0;
    if ((rc = tp_run(ctx, c, info))) return rc; // (the same status on every rank)
    constexpr int kWords = 2 + (int)(sizeof(KnnStats) / 8);
    static_assert(sizeof(KnnStats) % 8 == 0, "gathered as 8-byte words");
    int64_t mine[kWords] = {0, -1};
    KnnStats part = knn_stats_neutral();
    if (n_owned > 0) {
        int64_t bad = -1;
        const int lrc = knn_stats_rows(ctx, s->sdist.p, n_owned, k, WTP_F32, d_h, h_const, has, coord_radius, d_gid, d_nn_out, nullptr,
                                       &part, &bad);
        mine[0] = lrc ? lrc : bad >= 0 ? WTP_ERR_ARG : 0;
        mine[1] = bad;
    }
    memcpy(mine + 2, &part, sizeof(part));
    std::vector<int64_t> all((size_t)nranks * kWords);
    if ((rc = transport_allgather(ctx, nranks, mine, false, all.data(), kWords, "wtp_block_knn_stats"))) return rc;
    if (info) info->host_syncs += n_owned > 0 ? 1 : 0;
    KnnStats g = knn_stats_neutral();
    int spacing_seen = -1;
    for (int q = 0; q < nranks; ++q) {
        const int64_t* w = all.data() + (size_t)q * kWords;
        if (w[0]) {
            if (q == rank && w[1] < 0) return (int)w[0]; // (this rank's own failure: its message stands)
            return fail(ctx, (int)w[0], std::string(who) + "rank " + std::to_string(q) +
                                           (w[1] >= 0 ? ": h[" + std::to_string(w[1]) + "] is not finite and > 0" : " failed in its reduction"));
        }
        KnnStats pq;
        memcpy(&pq, w + 2, sizeof(pq));
        if (pq.n > 0) {
            if (spacing_seen >= 0 && spacing_seen != pq.has_spacing)
                return fail(ctx, WTP_ERR_ARG, std::string(who) + "ranks disagree on whether there is a spacing");
            spacing_seen = pq.has_spacing;
        }
        knn_stats_merge(g, pq);
    }
    *out = g;
    return WTP_OK;
}

WTP_API int wtp_block_radius_offsets(wtp_ctx* ctx, int rank, int nranks, const void* d_xyz, const int64_t* d_gid, int64_t n_owned,
                                     double r, int64_t* d_offsets_out, wtp_block_topo_info* info) {
    if (!ctx) return WTP_ERR_ARG;
    TpCall c{rank, nranks, (const float*)d_xyz, d_gid, n_owned, 0, 0, r, 0.0, nullptr, nullptr, d_offsets_out};
    return tp_run(ctx, c, info);
}

WTP_API int wtp_block_radius_fill(wtp_ctx* ctx, int64_t* d_idx_out) {
    if (!ctx) return WTP_ERR_ARG;
    TopoState* s = (TopoState*)ctx->block_topo;
    if (!s || !s->rad_ready) return fail(ctx, WTP_ERR_STATE, "wtp_block_radius_fill needs a preceding wtp_block_radius_offsets");
    if (s->rad_nnz > 0 && !d_idx_out) return fail(ctx, WTP_ERR_ARG, "wtp_block_radius_fill: idx_out is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = s->rad_n_owned;
    if (n > 0 && s->rad_nnz > 0) {
        hipLaunchKernelGGL(tp_radius_fill_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, ctx->stream, n,
                           (const int32_t*)s->opos.p, (const int64_t*)s->loff.p, (const int32_t*)s->ridx.p,
                           (const int32_t*)s->lgid.p, (const int64_t*)s->own_off.p, d_idx_out);
        WTP_HIP(ctx, hipGetLastError());
    }
    return sync(ctx);
}
