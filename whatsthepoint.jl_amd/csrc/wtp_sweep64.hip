// The Float64 candidate stage: exact fp64 answers from an fp32 search.  The cloud is moved to its own origin and rounded to
// float (origin_kernel, to_local_f32_kernel), the fp32 k-selection kernels (wtp_ksel.hip) find the kc nearest CANDIDATES per
// query on that copy, and one lane per query re-ranks them exactly in fp64 and certifies the first k: the fp32 search
// excluded nothing nearer than its last candidate minus the rounding bound (f64_certified).  Queries the certificate turns
// down take the exact path.  Two users (through f64_candidates, wtp_topology.hip):
//  - Float64 KNNTopology (knn_dev_f64): refine_f64_kernel for any kc, refine_f64_slots_kernel for k = 21 without self;
//  - Float64 sweeps of the laws that need the explicit k nearest neighbours (relax_f64_ksel_sweep; src/repel.jl:256-292
//    with InverseDistance, Spacing, LennardJones forces: everything but ClippedSpacingForce, which has its compact-support
//    kernels): refine_sweep_f64_kernel does with its k rows what the wave kernel does — the forces of the k neighbours in
//    ascending (d2, index), added in that order, the step, the statistics.  Same expressions, same order: the same bits
//    as the exact path.
// The slot kernels run in SLOT order: the fp32 search ran on points relabelled with their slot in the sorted copy
// (relabel_slots_kernel), so its rows are in slot order and name slots; a query's candidates sit next to it in the fp64
// points gathered into the same order instead of anywhere in the input — the gathers hit the cache lines the neighbouring
// queries just used — and the candidate list lives in registers (KC at compile time; the rows arrive in fp32 order, so
// exchange passes until nothing moves replace the insertion sort whose dynamically indexed arrays lived in scratch).
#include "wtp_device.hpp"
#include "wtp_internal.hpp"

namespace wtp {

// bbox partials -> {min x, min y, min z, largest extent}
__global__ void origin_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out4) {
    double mn[3], mx[3];
    for (int a = 0; a < 3; ++a) {
        double lo = Lim<double>::inf(), hi = -Lim<double>::inf();
        for (int b = threadIdx.x; b < nparts; b += 64) {
            lo = part[b * 6 + a] < lo ? part[b * 6 + a] : lo;
            hi = part[b * 6 + 3 + a] > hi ? part[b * 6 + 3 + a] : hi;
        }
        for (int d = 32; d >= 1; d >>= 1) {
            double o = __shfl_down(lo, d, 64);
            lo = o < lo ? o : lo;
            o = __shfl_down(hi, d, 64);
            hi = o > hi ? o : hi;
        }
        mn[a] = lo;
        mx[a] = hi;
    }
    if (threadIdx.x == 0) {
        double ext = 0;
        for (int a = 0; a < 3; ++a) {
            const double e = mx[a] - mn[a];
            out4[a] = mn[a] == mn[a] && mn[a] > -Lim<double>::inf() && mn[a] < Lim<double>::inf() ? mn[a] : 0.0;
            if (e == e && e > ext && e < Lim<double>::inf()) ext = e;
        }
        out4[3] = ext;
    }
}

// points (w = their index: load_points_kernel's ids, or the session's slots) -> float copy in the frame of org4, w = the row
__global__ void to_local_f32_kernel(const double4* __restrict__ in, int64_t n, const double* __restrict__ org4,
                                    float4* __restrict__ out) {
    const double ox = org4[0], oy = org4[1], oz = org4[2];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double4 p = in[i];
        float4 o;
        o.x = (float)(p.x - ox);
        o.y = (float)(p.y - oy);
        o.z = (float)(p.z - oz);
        o.w = id_to_w(0.f, (int32_t)i);
        out[i] = o;
    }
}

// the float copy sorted by its own grid: entry i came from row w of raw.  Afterwards w = i (the search names slots of THIS
// order), sorted64[i] = that fp64 point (its w, the point's index, is the tie-break of the canonical order), and, when
// sslot is given, sslot[i] = the row
__global__ void relabel_slots_kernel(const double4* __restrict__ raw, float4* __restrict__ sorted32, double4* __restrict__ sorted64,
                                     int32_t* __restrict__ sslot, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float4 p = sorted32[i];
        const int32_t s = w_to_id(p.w);
        if (sslot) sslot[i] = s;
        sorted64[i] = raw[s];
        p.w = id_to_w(0.f, (int32_t)i);
        sorted32[i] = p;
    }
}

// Certificate: every point the fp32 search excluded is at least as far, in fp32-local arithmetic, as its last candidate
// (distance dmax32); rounding the coordinates to float and evaluating in float moves a distance by less than
// eps = extent 2^-21 + dmax32 2^-20, so an excluded point's exact distance exceeds dmax32 - eps.  If the exact kq-th
// candidate distance (squared: d2kq) is strictly below that, the first kq candidates in exact order are the answer.
__device__ inline bool f64_certified(double d2kq, double dmax32, double extent) {
    const double eps = extent * 0x1p-21 + dmax32 * 0x1p-20;
    return wsqrt(d2kq) < dmax32 - eps;
}

static constexpr int kRefineMax = 32;

// KNNTopology, any kc: one thread per query, exact d2 to its kc candidates (self among them), canonical order by insertion,
// the first k; uncertified queries are listed for the exact fp64 path.
__global__ void refine_f64_kernel(const double4* __restrict__ raw, const int32_t* __restrict__ cand,
                                  const float* __restrict__ cdist, int64_t n, int kc, int k, int include_self,
                                  const double* __restrict__ org4, int32_t* __restrict__ idx_out,
                                  double* __restrict__ dist_out, int32_t* __restrict__ fail_list,
                                  int32_t* __restrict__ fail_count) {
    const double extent = org4[3];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double4 q = raw[i];
        double kd[kRefineMax];
        int32_t ki[kRefineMax];
        int m = 0;
        for (int j = 0; j < kc; ++j) {
            const int32_t c = cand[i * kc + j];
            const double4 p = raw[c];
            const double d = dist2<double>(q.x, q.y, q.z, p.x, p.y, p.z);
            int pos = m++;
            while (pos > 0 && lex_lt(d, c, kd[pos - 1], ki[pos - 1])) {
                kd[pos] = kd[pos - 1];
                ki[pos] = ki[pos - 1];
                --pos;
            }
            kd[pos] = d;
            ki[pos] = c;
        }
        const int kq = include_self ? k : k + 1;
        const double dmax32 = (double)cdist[i * kc + kc - 1];
        const bool certified = (int64_t)kc >= n || f64_certified(kd[kq - 1], dmax32, extent);
        int out = 0;
        for (int j = 0; j < kc && out < k; ++j) {
            if (!include_self && ki[j] == (int32_t)i) continue; // self removed by index (src/topology.jl:82)
            idx_out[i * k + out] = ki[j];
            if (dist_out) dist_out[i * k + out] = wsqrt(kd[j]);
            ++out;
        }
        if (!certified || out < k) {
            const int pos = atomicAdd(fail_count, 1);
            fail_list[pos] = (int32_t)i;
        }
    }
}

// KNNTopology in slot order: canonical order and the row's place are by ORIGINAL id (kept in sorted[].w); failed queries
// are listed by original id.  refine_sweep_f64_kernel repeats the gather and the exchange passes with the candidate's row
// carried along: one inline function for both costs each kernel registers (184 -> 186, 286 -> 288 VGPRs at best).
template <int KC>
__global__ __launch_bounds__(128) void refine_f64_slots_kernel(const double4* __restrict__ sorted, const int32_t* __restrict__ cand,
                                                               const float* __restrict__ cdist, int64_t n, int k, int include_self,
                                                               const double* __restrict__ org4, int32_t* __restrict__ idx_out,
                                                               double* __restrict__ dist_out, int32_t* __restrict__ fail_list,
                                                               int32_t* __restrict__ fail_count) {
    const double extent = org4[3];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double4 q = sorted[i];
        const int32_t qid = w_to_id(q.w);
        double kd[KC];
        int32_t ki[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const double4 p = sorted[cand[i * KC + j]];
            kd[j] = dist2<double>(q.x, q.y, q.z, p.x, p.y, p.z);
            ki[j] = w_to_id(p.w);
        }
        bool again = true;
        while (again) { // (lane-local: the lists arrive almost sorted, one or two passes)
            again = false;
#pragma unroll
            for (int j = 0; j + 1 < KC; ++j) {
                const bool sw = lex_lt(kd[j + 1], ki[j + 1], kd[j], ki[j]);
                const double td = kd[j];
                const int32_t ti = ki[j];
                kd[j] = sw ? kd[j + 1] : td;
                ki[j] = sw ? ki[j + 1] : ti;
                kd[j + 1] = sw ? td : kd[j + 1];
                ki[j + 1] = sw ? ti : ki[j + 1];
                again = again || sw;
            }
        }
        const int kq = include_self ? k : k + 1;
        const double dmax32 = (double)cdist[i * KC + KC - 1];
        double dkq = kd[KC - 1];
#pragma unroll
        for (int j = 0; j < KC; ++j) dkq = (j == kq - 1) ? kd[j] : dkq;
        const bool certified = (int64_t)KC >= n || f64_certified(dkq, dmax32, extent);
        int out = 0;
        int32_t* orow = idx_out + (int64_t)qid * k;
        double* drow = dist_out ? dist_out + (int64_t)qid * k : nullptr;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const bool take = out < k && (include_self || ki[j] != qid); // self removed by index (src/topology.jl:82)
            if (take) {
                orow[out] = ki[j];
                if (drow) drow[out] = wsqrt(kd[j]);
                ++out;
            }
        }
        if (!certified || out < k) {
            const int pos = atomicAdd(fail_count, 1);
            fail_list[pos] = qid;
        }
    }
}

constexpr int kS64Threads = 128;

// Sweep of a k-nearest law in slot order: s64 = the snapshot in the float copy's order, sslot = the session slot of each
// entry (the answer's place; uncertified queries are listed by session slot).
template <int KC>
__global__ __launch_bounds__(kS64Threads) void refine_sweep_f64_kernel(SearchArgs<double> a, const double4* __restrict__ s64,
                                                                       const int32_t* __restrict__ sslot,
                                                                       const int32_t* __restrict__ cand,
                                                                       const float* __restrict__ cdist,
                                                                       const double* __restrict__ org4, int part_base) {
    __shared__ Acc sm_acc[kS64Threads / 64];
    if (a.stop && *a.stop) return; // wtp_relax_run_until: a stop rule fired earlier in this batch
    Acc acc = acc_empty();
    const double extent = org4[3];
    const int Kq = a.k; // the k nearest, self among them (src/repel.jl:262: knn(tree, xi, k); :271 skips j == i)
    const int dim = a.grid->dim;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const double4 q = s64[i];
        const int32_t id = w_to_id(q.w);
        const int32_t slot = sslot[i];
        if (id < a.n_fixed) { // the wall: never moves (src/repel.jl:80,256)
            a.out[slot] = q;
            a.forces[slot] = 0.0;
            a.nn_dist[slot] = Lim<double>::inf();
            a.nn_id[slot] = -1;
            continue;
        }
        double kd[KC];
        int32_t ki[KC], kc[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            kc[j] = cand[i * KC + j];
            const double4 p = s64[kc[j]];
            kd[j] = dist2<double>(q.x, q.y, q.z, p.x, p.y, p.z);
            ki[j] = w_to_id(p.w);
        }
        bool again = true;
        while (again) { // (lane-local: the lists arrive almost sorted, one or two passes)
            again = false;
#pragma unroll
            for (int j = 0; j + 1 < KC; ++j) {
                const bool sw = lex_lt(kd[j + 1], ki[j + 1], kd[j], ki[j]);
                const double td = kd[j];
                const int32_t ti = ki[j], tc = kc[j];
                kd[j] = sw ? kd[j + 1] : td;
                ki[j] = sw ? ki[j + 1] : ti;
                kc[j] = sw ? kc[j + 1] : tc;
                kd[j + 1] = sw ? td : kd[j + 1];
                ki[j + 1] = sw ? ti : ki[j + 1];
                kc[j + 1] = sw ? tc : kc[j + 1];
                again = again || sw;
            }
        }
        const double dmax32 = (double)cdist[i * KC + KC - 1];
        double dkq = kd[KC - 1];
#pragma unroll
        for (int j = 0; j < KC; ++j) dkq = (j == Kq - 1) ? kd[j] : dkq;
        if (!f64_certified(dkq, dmax32, extent)) { // not certified: the exact path (its list holds session slots)
            a.fb_list[atomicAdd(a.fb_count, 1)] = slot;
            continue;
        }
        const double s = a.spacing_pp ? a.spacing_pp[id] : a.spacing_const;
        double Fx = 0, Fy = 0, Fz = 0, nd = Lim<double>::inf();
        int32_t nid = -1;
#pragma unroll
        for (int j = 0; j < KC; ++j) { // ascending (d2, id), self skipped by index (:271)
            if (j < Kq && ki[j] != id) {
                const double4 c = s64[kc[j]];
                double fx = 0, fy = 0, fz = 0;
                add_force<double>(a, dim, s, q.x, q.y, q.z, id, c.x, c.y, c.z, ki[j], kd[j], fx, fy, fz);
                if (nid < 0) {
                    nid = ki[j];
                    nd = wsqrt(kd[j]);
                }
                Fx = Fx + fx;
                Fy = Fy + fy;
                Fz = Fz + fz;
            }
        }
        double4 o;
        const double f = step_point<double>(a, s, q.x, q.y, q.z, Fx, Fy, Fz, o.x, o.y, o.z);
        o.w = q.w;
        a.out[slot] = o;
        a.forces[slot] = f;
        a.nn_dist[slot] = nd;
        a.nn_id[slot] = nid;
        acc_point<double>(acc, f, nd, s, id, nid);
        // sharded sessions: what the answer rests on is the k-th neighbour
        if (reaches_past_cover<double>(a, q.x, q.y, q.z, dkq)) atomicAdd(a.uncovered, 1);
    }
    __syncthreads();
    acc_block_reduce(acc, sm_acc);
    if (threadIdx.x == 0) acc_store(&a.partials[part_base + blockIdx.x], acc);
}

int launch_origin(wtp_ctx* ctx, const double4* pts, int64_t n, double* d_org4) {
    int nbb, rc;
    if ((rc = launch_bbox64(ctx, pts, n, &nbb))) return rc;
    hipLaunchKernelGGL(origin_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double*)ctx->bbox_part.p, nbb, d_org4);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

int launch_to_local_f32(wtp_ctx* ctx, const double4* in, int64_t n, const double* d_org4, float4* out) {
    hipLaunchKernelGGL(to_local_f32_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, ctx->stream, in, n, d_org4, out);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

int launch_relabel_slots(wtp_ctx* ctx, const double4* raw, float4* sorted32, double4* sorted64, int32_t* sslot, int64_t n) {
    hipLaunchKernelGGL(relabel_slots_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, ctx->stream, raw, sorted32, sorted64,
                       sslot, n);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

int launch_refine_f64(wtp_ctx* ctx, const double4* raw, const int32_t* cand, const float* cdist, int64_t n, int kc, int k,
                      int include_self, const double* d_org4, int32_t* idx_out, double* dist_out, int32_t* fail_list,
                      int32_t* fail_count) {
    WTP_HIP(ctx, hipMemsetAsync(fail_count, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(refine_f64_kernel, dim3(grid_for(n, 128, 16384)), dim3(128), 0, ctx->stream, raw, cand, cdist, n, kc,
                       k, include_self, d_org4, idx_out, dist_out, fail_list, fail_count);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

// kc must be 24 (k = 21 without self, the reference's default) — the caller checks
int launch_refine_f64_slots(wtp_ctx* ctx, const double4* sorted, const int32_t* cand, const float* cdist, int64_t n, int kc, int k,
                            int include_self, const double* d_org4, int32_t* idx_out, double* dist_out, int32_t* fail_list,
                            int32_t* fail_count) {
    if (kc != 24) return fail(ctx, WTP_ERR_ARG, "launch_refine_f64_slots: kc must be 24");
    WTP_HIP(ctx, hipMemsetAsync(fail_count, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(refine_f64_slots_kernel<24>, dim3(grid_for(n, 128, 16384)), dim3(128), 0, ctx->stream, sorted, cand, cdist, n,
                       k, include_self, d_org4, idx_out, dist_out, fail_list, fail_count);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

// candidates: 24 per query (the caller searched with k = 24).  Partials go to the brick range [0, used_brick).
int launch_refine_sweep_f64(wtp_ctx* ctx, SearchArgs<double>& a, const double4* s64, const int32_t* sslot, const int32_t* cand,
                            const float* cdist, const double* d_org4) {
    const int blocks = grid_for(a.n, kS64Threads, 1024);
    a.used_brick = blocks;
    hipLaunchKernelGGL(refine_sweep_f64_kernel<24>, dim3(blocks), dim3(kS64Threads), 0, ctx->stream, a, s64, sslot, cand, cdist,
                       d_org4, 0);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

} // namespace wtp
