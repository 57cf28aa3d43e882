// wtp_normal_graph.hip — the graph part of orient_normals! (src/normals.jl:75-161) and split_surface!
// (src/surface_operations.jl:58-94) on the k-NN rows where the search left them.
//
//   orient   the unique minimum spanning forest of the row graph under the total edge order (w, a, b), by Borůvka rounds
//            that carry one parity bit per vertex: par(v) = the number (mod 2) of tree edges e on v's path to its
//            component's representative with sigma(e) = [n_u . n_v < 0], taken on the input normals.  The reference's
//            walk flips v iff par(v) ^ par(start) ^ [start flipped]: no rooted tree, no walk.
//   split    connected components of the rows' edges whose normals differ by less than an angle: every component hooks
//            onto its smallest neighbouring representative, so a representative is the smallest id of its component.
//
// One 32-bit word per vertex holds (representative << 1 | parity); a single aligned word is read and written whole, so
// pointer jumping runs in place: whatever a racing read returns is a valid (ancestor, parity to it) pair.  A round:
//   clear   best[c] = none, nxt = cur
//   offer   thread per row entry: both endpoints' components differ -> integer atomicMin of the weight's ordered key into
//           both components (stage 1), then of (a << 32 | b) among the edges that attain it (stage 2).  An edge is
//           offered to both sides because the row graph is directed.  No floating-point atomics; minima do not depend on
//           arrival order.
//   hook    thread per representative: onto the component at the other end of its best edge; two components that chose
//           the same edge keep the smaller representative.  The hooking side records the edge.
//   jump    nxt[v] <- nxt[nxt[v]] with parities added, ceil(log2(components that can still hook)) + 1 launches: a round
//           at least halves those, so the launch count is known on the host; launches after the forest is flat return
//           at once (a flag per launch).
// A round without a hook sets `done`, and the kernels of later rounds in the same batch return at once: the host reads
// the control block once per batch (wtp_gradient_limit's scheme).
#include "wtp_device.hpp"

namespace wtp {

static constexpr int kNgThreads = 256;
static constexpr unsigned long long kNgNone = ~0ull;

// control block, 64-bit words
enum {
    NG_DONE = 0, NG_ROUNDS, NG_HOOKS, NG_MST, NG_BAD, NG_ZMAX, NG_START, NG_SFLIP, NG_NCOMP, NG_REACHED, NG_FLIPPED, NG_NEDGES,
    NG_JFLAG = 16, // one word per jump launch of the round in flight
    NG_WORDS = 64
};
size_t normal_graph_ctl_bytes() { return sizeof(unsigned long long) * NG_WORDS; }

// IEEE order as unsigned order; -0 counts as +0 (they compare equal), NaN behind everything (a stable sort leaves it last)
__device__ inline unsigned long long ord_key(float w) {
    if (w != w) return kNgNone - 1;
    if (w == 0.0f) w = 0.0f;
    const uint32_t u = f2u(w);
    return (u & 0x80000000u) ? (uint32_t)~u : (u | 0x80000000u);
}
__device__ inline unsigned long long ord_key(double w) {
    if (w != w) return kNgNone - 1;
    if (w == 0.0) w = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(w);
    const unsigned long long key = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return key > kNgNone - 2 ? kNgNone - 2 : key; // (never: the largest finite-or-inf key is far below)
}

// ((x x' + y y') + z z'), term by term
template <typename T> __device__ inline T ng_dot(const T* __restrict__ nrm, int dim, int64_t a, int64_t b) {
    T d = nrm[a * dim] * nrm[b * dim] + nrm[a * dim + 1] * nrm[b * dim + 1];
    if (dim == 3) d = d + nrm[a * dim + 2] * nrm[b * dim + 2];
    return d;
}
template <typename T> __device__ inline T ng_eps100();
template <> __device__ inline float ng_eps100<float>() { return 1.1920928955078125e-07f * 1.0e2f; }
template <> __device__ inline double ng_eps100<double>() { return 2.220446049250313e-16 * 1.0e2; }

// build_normal_weighted_graph (src/normals.jl:150-161): (1 - |dot|) + 100 eps
template <typename T> __device__ inline T ng_weight(const T* __restrict__ nrm, int dim, int64_t a, int64_t b) {
    const T d = ng_dot<T>(nrm, dim, a, b);
    const T one_minus = (T)1 - (d < 0 ? -d : d);
    return one_minus + ng_eps100<T>();
}

__device__ inline void min_u64(unsigned long long* p, unsigned long long v) {
    // the word only ever decreases: a stale read can only make the atomic run needlessly, never skip a smaller value
    if (v < __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMin(p, v);
}

__device__ inline unsigned long long wave_max_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)shfl_down_i64((int64_t)v, o);
        v = other > v ? other : v;
    }
    return v;
}
__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)shfl_down_i64((int64_t)v, o);
        v = other < v ? other : v;
    }
    return v;
}
__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)shfl_down_i64((int64_t)v, o);
    return v;
}

// ---- before the rounds ------------------------------------------------------------------------------------------
__global__ void ng_ctl_init_kernel(unsigned long long* __restrict__ ctl) {
    const int t = threadIdx.x;
    if (t < NG_WORDS) ctl[t] = (t == NG_BAD || t == NG_START) ? kNgNone : 0ull;
}

// every vertex its own component; the first vertex with a non-finite normal; the largest last coordinate
template <typename T>
__global__ void __launch_bounds__(kNgThreads)
ng_prep_kernel(const T* __restrict__ xyz, const T* __restrict__ nrm, int64_t n, int dim, int want_start,
               uint32_t* __restrict__ cur, unsigned long long* __restrict__ ctl) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bad = kNgNone, zkey = 0;
    if (v < n) {
        cur[v] = (uint32_t)v << 1;
        bool ok = true;
        for (int c = 0; c < dim; ++c) {
            const T x = nrm[v * dim + c];
            ok = ok && (x - x == (T)0); // false for NaN and +-inf
        }
        if (!ok) bad = (unsigned long long)v;
        if (want_start) zkey = ord_key(xyz[v * dim + dim - 1]);
    }
    bad = wave_min_u64(bad);
    zkey = wave_max_u64(zkey);
    if ((threadIdx.x & 63) == 0) {
        if (bad != kNgNone) atomicMin(&ctl[NG_BAD], bad);
        if (want_start && zkey > __atomic_load_n(&ctl[NG_ZMAX], __ATOMIC_RELAXED)) atomicMax(&ctl[NG_ZMAX], zkey);
    }
}

// the first index that attains the largest last coordinate
template <typename T>
__global__ void __launch_bounds__(kNgThreads)
ng_start_kernel(const T* __restrict__ xyz, int64_t n, int dim, unsigned long long* __restrict__ ctl) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cand = kNgNone;
    if (v < n && ord_key(xyz[v * dim + dim - 1]) == ctl[NG_ZMAX]) cand = (unsigned long long)v;
    cand = wave_min_u64(cand);
    if ((threadIdx.x & 63) == 0 && cand != kNgNone) min_u64(&ctl[NG_START], cand);
}

// the start faces up: flipped if its last component is < 0 (read before any normal is changed)
template <typename T>
__global__ void ng_start_flip_kernel(const T* __restrict__ nrm, int dim, unsigned long long* __restrict__ ctl) {
    const int64_t s = (int64_t)ctl[NG_START];
    ctl[NG_SFLIP] = nrm[s * dim + dim - 1] < (T)0 ? 1ull : 0ull;
}

// distinct undirected edges of the row graph.  A row whose slot 0 is another point belongs to a coincident twin and
// repeats that point's own row (same coordinates, same canonical order), so only own rows count; of an edge that both
// ends name, the smaller end's entry counts.
__global__ void __launch_bounds__(kNgThreads)
ng_count_edges_kernel(const int32_t* __restrict__ rows, int64_t n, int k, unsigned long long* __restrict__ ctl) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int km = k - 1;
    unsigned long long c = 0;
    if (e < n * km) {
        const int64_t i = e / km;
        const int j = (int)(e - i * km) + 1;
        const int64_t u = rows[i * k], v = rows[i * k + j];
        if (u == i && u != v) {
            c = 1;
            if (v < u && rows[v * k] == v) {
                for (int t = 1; t < k; ++t)
                    if (rows[v * k + t] == u) c = 0;
            }
        }
    }
    c = wave_sum_u64(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ctl[NG_NEDGES], c);
}

// split: which row entries are kept, |_angle(n_src, n_dst)| < angle (src/utils.jl:18-23), in double
template <typename T>
__global__ void __launch_bounds__(kNgThreads)
ng_keep_kernel(const int32_t* __restrict__ rows, const T* __restrict__ nrm, int64_t n, int dim, int k, double angle,
               uint8_t* __restrict__ keep) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int km = k - 1;
    if (e >= n * km) return;
    const int64_t i = e / km;
    const int j = (int)(e - i * km) + 1;
    const int64_t u = rows[i * k], v = rows[i * k + j];
    const double ux = (double)nrm[u * dim], uy = (double)nrm[u * dim + 1], vx = (double)nrm[v * dim], vy = (double)nrm[v * dim + 1];
    double th;
    if (dim == 2) {
        th = atan2(ux * vy - uy * vx, ux * vx + uy * vy);
    } else {
        const double uz = (double)nrm[u * dim + 2], vz = (double)nrm[v * dim + 2];
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        th = atan2(__builtin_sqrt((cx * cx + cy * cy) + cz * cz), (ux * vx + uy * vy) + uz * vz);
    }
    keep[e] = (th < 0 ? -th : th) < angle ? 1 : 0;
}

// ---- one round ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kNgThreads)
ng_clear_kernel(const uint32_t* __restrict__ cur, uint32_t* __restrict__ nxt, unsigned long long* __restrict__ best_w,
                unsigned long long* __restrict__ best_e, int64_t n, unsigned long long* __restrict__ ctl) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < NG_WORDS - NG_JFLAG) ctl[NG_JFLAG + v] = 0;
    if (v >= n) return;
    nxt[v] = cur[v]; // (also after `done`: the buffers swap every round)
    best_w[v] = kNgNone;
    best_e[v] = kNgNone;
}

// stage 1 (best_e == NULL): the smallest weight leaving each component; stage 2: the smallest (a, b) among those edges
template <typename T>
__global__ void __launch_bounds__(kNgThreads)
ng_offer_kernel(const int32_t* __restrict__ rows, const T* __restrict__ nrm, int64_t n, int dim, int k,
                const uint32_t* __restrict__ cur, unsigned long long* __restrict__ best_w,
                unsigned long long* __restrict__ best_e, const unsigned long long* __restrict__ ctl) {
    if (ctl[NG_DONE]) return;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int km = k - 1;
    if (e >= n * km) return;
    const int64_t i = e / km;
    const int j = (int)(e - i * km) + 1;
    const int64_t u = rows[i * k], v = rows[i * k + j];
    const uint32_t cu = cur[u] >> 1, cv = cur[v] >> 1;
    if (cu == cv) return;
    const unsigned long long key = ord_key(ng_weight<T>(nrm, dim, u, v));
    if (!best_e) {
        min_u64(&best_w[cu], key);
        min_u64(&best_w[cv], key);
    } else {
        const unsigned long long ab = u < v ? ((unsigned long long)u << 32 | (unsigned long long)v)
                                            : ((unsigned long long)v << 32 | (unsigned long long)u);
        if (key == best_w[cu]) min_u64(&best_e[cu], ab);
        if (key == best_w[cv]) min_u64(&best_e[cv], ab);
    }
}

template <typename T>
__global__ void __launch_bounds__(kNgThreads)
ng_hook_kernel(const T* __restrict__ nrm, int64_t n, int dim, const uint32_t* __restrict__ cur, uint32_t* __restrict__ nxt,
               const unsigned long long* __restrict__ best_e, int32_t* __restrict__ mst_out,
               unsigned long long* __restrict__ ctl) {
    if (ctl[NG_DONE]) return;
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n || cur[c] != ((uint32_t)c << 1)) return; // representatives only
    const unsigned long long ab = best_e[c];
    if (ab == kNgNone) return;
    const int64_t a = (int64_t)(ab >> 32), b = (int64_t)(ab & 0xffffffffull);
    const uint32_t sa = cur[a], sb = cur[b];
    const uint32_t p = (sa >> 1) == (uint32_t)c ? (sb >> 1) : (sa >> 1);
    if (best_e[p] == ab && (uint32_t)c < p) return; // both chose this edge: the smaller representative stays
    const uint32_t sigma = ng_dot<T>(nrm, dim, a, b) < (T)0 ? 1u : 0u;
    nxt[c] = (p << 1) | ((sa ^ sb ^ sigma) & 1u);
    const unsigned long long slot = atomicAdd(&ctl[NG_MST], 1ull);
    if (mst_out && slot < (unsigned long long)(n - 1)) {
        mst_out[2 * slot] = (int32_t)a;
        mst_out[2 * slot + 1] = (int32_t)b;
    }
    atomicAdd(&ctl[NG_HOOKS], 1ull);
}

// split, stage 1 only: the smallest representative among the neighbouring components
__global__ void __launch_bounds__(kNgThreads)
ng_offer_label_kernel(const int32_t* __restrict__ rows, const uint8_t* __restrict__ keep, int64_t n, int k,
                      const uint32_t* __restrict__ cur, unsigned long long* __restrict__ best_w,
                      const unsigned long long* __restrict__ ctl) {
    if (ctl[NG_DONE]) return;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int km = k - 1;
    if (e >= n * km || !keep[e]) return;
    const int64_t i = e / km;
    const int j = (int)(e - i * km) + 1;
    const uint32_t cu = cur[rows[i * k]] >> 1, cv = cur[rows[i * k + j]] >> 1;
    if (cu == cv) return;
    if (cv < cu) min_u64(&best_w[cu], cv);
    else min_u64(&best_w[cv], cu);
}

__global__ void __launch_bounds__(kNgThreads)
ng_hook_label_kernel(int64_t n, const uint32_t* __restrict__ cur, uint32_t* __restrict__ nxt,
                     const unsigned long long* __restrict__ best_w, unsigned long long* __restrict__ ctl) {
    if (ctl[NG_DONE]) return;
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n || cur[c] != ((uint32_t)c << 1)) return;
    const unsigned long long m = best_w[c];
    if (m == kNgNone) return; // (only smaller representatives are ever offered)
    nxt[c] = (uint32_t)m << 1;
    atomicAdd(&ctl[NG_HOOKS], 1ull);
}

// launch t of a round: returns at once when launch t - 1 moved nothing
__global__ void __launch_bounds__(kNgThreads)
ng_jump_kernel(uint32_t* __restrict__ nxt, int64_t n, int t, unsigned long long* __restrict__ ctl) {
    if (ctl[NG_DONE] || (t > 0 && !ctl[NG_JFLAG + t - 1])) return;
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t s = __atomic_load_n(&nxt[v], __ATOMIC_RELAXED);
    const uint32_t p = s >> 1;
    if (p == (uint32_t)v) return;
    const uint32_t q = __atomic_load_n(&nxt[p], __ATOMIC_RELAXED);
    if ((q >> 1) == p) return; // p is a representative
    __atomic_store_n(&nxt[v], (q & ~1u) | ((s ^ q) & 1u), __ATOMIC_RELAXED);
    if (!__atomic_load_n(&ctl[NG_JFLAG + t], __ATOMIC_RELAXED)) __atomic_store_n(&ctl[NG_JFLAG + t], 1ull, __ATOMIC_RELAXED);
}

__global__ void ng_finish_kernel(unsigned long long* __restrict__ ctl) {
    if (ctl[NG_DONE]) return;
    if (ctl[NG_HOOKS] == 0) ctl[NG_DONE] = 1;
    else ctl[NG_ROUNDS] += 1;
    ctl[NG_HOOKS] = 0;
}

// ---- after the rounds -------------------------------------------------------------------------------------------------
// orient: flips the vertices of the start's component whose parity says so; counts.  split: labels; counts.
template <typename T>
__global__ void __launch_bounds__(kNgThreads)
ng_apply_kernel(T* __restrict__ nrm, int64_t n, int dim, const uint32_t* __restrict__ cur, int32_t* __restrict__ label_out,
                unsigned long long* __restrict__ ctl) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long roots = 0, reached = 0, flipped = 0;
    if (v < n) {
        const uint32_t s = cur[v];
        roots = (s >> 1) == (uint32_t)v;
        if (label_out) {
            label_out[v] = (int32_t)(s >> 1);
        } else {
            const uint32_t s0 = cur[ctl[NG_START]];
            if ((s >> 1) == (s0 >> 1)) {
                reached = 1;
                if (((s ^ s0) & 1u) ^ (uint32_t)ctl[NG_SFLIP]) {
                    flipped = 1;
                    for (int c = 0; c < dim; ++c) nrm[v * dim + c] = -nrm[v * dim + c];
                }
            }
        }
    }
    roots = wave_sum_u64(roots);
    reached = wave_sum_u64(reached);
    flipped = wave_sum_u64(flipped);
    if ((threadIdx.x & 63) == 0) {
        if (roots) atomicAdd(&ctl[NG_NCOMP], roots);
        if (reached) atomicAdd(&ctl[NG_REACHED], reached);
        if (flipped) atomicAdd(&ctl[NG_FLIPPED], flipped);
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------
static inline unsigned ng_blocks(int64_t work) { return (unsigned)((work + kNgThreads - 1) / kNgThreads); }

// control block, components, the bad-normal index, the start and its flip, the edge count, split's kept entries
template <typename T>
int launch_normal_graph_prep(wtp_ctx* ctx, const T* d_xyz, const T* d_nrm, const int32_t* d_rows, int64_t n, int dim, int k,
                             int orient, double angle, uint32_t* d_cur, uint8_t* d_keep, unsigned long long* d_ctl) {
    hipLaunchKernelGGL(ng_ctl_init_kernel, dim3(1), dim3(NG_WORDS), 0, ctx->stream, d_ctl);
    hipLaunchKernelGGL(ng_prep_kernel<T>, dim3(ng_blocks(n)), dim3(kNgThreads), 0, ctx->stream, d_xyz, d_nrm, n, dim, orient,
                       d_cur, d_ctl);
    if (orient) {
        hipLaunchKernelGGL(ng_start_kernel<T>, dim3(ng_blocks(n)), dim3(kNgThreads), 0, ctx->stream, d_xyz, n, dim, d_ctl);
        hipLaunchKernelGGL(ng_start_flip_kernel<T>, dim3(1), dim3(1), 0, ctx->stream, d_nrm, dim, d_ctl);
    }
    if (k > 1) {
        const int64_t ne = n * (k - 1);
        hipLaunchKernelGGL(ng_count_edges_kernel, dim3(ng_blocks(ne)), dim3(kNgThreads), 0, ctx->stream, d_rows, n, k, d_ctl);
        if (!orient)
            hipLaunchKernelGGL(ng_keep_kernel<T>, dim3(ng_blocks(ne)), dim3(kNgThreads), 0, ctx->stream, d_rows, d_nrm, n, dim, k,
                               angle, d_keep);
    }
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

// rounds first .. first + rounds - 1; the components are in bufs[r & 1] before round r
template <typename T>
int launch_normal_graph_rounds(wtp_ctx* ctx, const T* d_nrm, const int32_t* d_rows, int64_t n, int dim, int k, int orient,
                               const uint8_t* d_keep, uint32_t* d_buf0, uint32_t* d_buf1, unsigned long long* d_best_w,
                               unsigned long long* d_best_e, int32_t* d_mst_out, int first, int rounds,
                               unsigned long long* d_ctl) {
    const unsigned nb = ng_blocks(n), eb = ng_blocks(n * (k - 1));
    for (int r = first; r < first + rounds; ++r) {
        uint32_t* cur = (r & 1) ? d_buf1 : d_buf0;
        uint32_t* nxt = (r & 1) ? d_buf0 : d_buf1;
        hipLaunchKernelGGL(ng_clear_kernel, dim3(nb), dim3(kNgThreads), 0, ctx->stream, (const uint32_t*)cur, nxt, d_best_w, d_best_e,
                           n, d_ctl);
        if (orient) {
            hipLaunchKernelGGL(ng_offer_kernel<T>, dim3(eb), dim3(kNgThreads), 0, ctx->stream, d_rows, d_nrm, n, dim, k,
                               (const uint32_t*)cur, d_best_w, (unsigned long long*)nullptr, (const unsigned long long*)d_ctl);
            hipLaunchKernelGGL(ng_offer_kernel<T>, dim3(eb), dim3(kNgThreads), 0, ctx->stream, d_rows, d_nrm, n, dim, k,
                               (const uint32_t*)cur, d_best_w, d_best_e, (const unsigned long long*)d_ctl);
            hipLaunchKernelGGL(ng_hook_kernel<T>, dim3(nb), dim3(kNgThreads), 0, ctx->stream, d_nrm, n, dim, (const uint32_t*)cur, nxt,
                               (const unsigned long long*)d_best_e, d_mst_out, d_ctl);
        } else {
            hipLaunchKernelGGL(ng_offer_label_kernel, dim3(eb), dim3(kNgThreads), 0, ctx->stream, d_rows, d_keep, n, k,
                               (const uint32_t*)cur, d_best_w, (const unsigned long long*)d_ctl);
            hipLaunchKernelGGL(ng_hook_label_kernel, dim3(nb), dim3(kNgThreads), 0, ctx->stream, n, (const uint32_t*)cur, nxt,
                               (const unsigned long long*)d_best_w, d_ctl);
        }
        // at most n >> r components can still hook in round r, so no vertex is deeper than that below its new representative
        const int64_t active = r < 62 ? (n >> r) : 0;
        int jumps = 1;
        while (jumps < NG_WORDS - NG_JFLAG - 1 && ((int64_t)1 << (jumps - 1)) < active) ++jumps;
        for (int t = 0; t < jumps; ++t)
            hipLaunchKernelGGL(ng_jump_kernel, dim3(nb), dim3(kNgThreads), 0, ctx->stream, nxt, n, t, d_ctl);
        hipLaunchKernelGGL(ng_finish_kernel, dim3(1), dim3(1), 0, ctx->stream, d_ctl);
    }
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

template <typename T>
int launch_normal_graph_apply(wtp_ctx* ctx, T* d_nrm, int64_t n, int dim, const uint32_t* d_cur, int32_t* d_label_out,
                              unsigned long long* d_ctl) {
    hipLaunchKernelGGL(ng_apply_kernel<T>, dim3(ng_blocks(n)), dim3(kNgThreads), 0, ctx->stream, d_nrm, n, dim, d_cur, d_label_out,
                       d_ctl);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

#define INST(T)                                                                                                        \
    template int launch_normal_graph_prep<T>(wtp_ctx*, const T*, const T*, const int32_t*, int64_t, int, int, int, double,      \
                                             uint32_t*, uint8_t*, unsigned long long*);                               \
    template int launch_normal_graph_rounds<T>(wtp_ctx*, const T*, const int32_t*, int64_t, int, int, int, const uint8_t*,      \
                                               uint32_t*, uint32_t*, unsigned long long*, unsigned long long*, int32_t*, int, \
                                               int, unsigned long long*);                                              \
    template int launch_normal_graph_apply<T>(wtp_ctx*, T*, int64_t, int, const uint32_t*, int32_t*, unsigned long long*);
INST(float)
INST(double)
#undef INST

} // namespace wtp
