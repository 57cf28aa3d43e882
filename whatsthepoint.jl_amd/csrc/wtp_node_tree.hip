// wtp_node_tree.hip — the spacing-driven node octree of the Orthtree algorithm, built, balanced, classified and read on
// the device (include/wtp.h states the contract term by term; DESIGN.md §8f.9 the design).
//
//   build_node_octree / _subdivide_node_octree! / _box_may_contain_interior   src/octree/spacing_criterion.jl:88-198
//   balance_octree! / needs_balancing / find_leaf / _classify_leaf_conservative   src/octree/spatial_octree.jl
//   _estimate_volume_points / _bridson_h_min / _leaf_spacing_field   src/discretization/algorithms/octree.jl:590-662
//
// The tree is ONE array: the leaves' 64-bit keys in Morton order.  A key is the box's Morton code at its own depth, a
// one behind it, then zeros up to depth 20, so depth and cell come back out of the key and disjoint boxes compare as
// their lower corners do.  A split writes the 8 children where the parent stood (the scan of "1 or 8" gives every leaf
// its new place), so the array stays sorted through every level of the build and every round of the balance and no
// sort is needed.  Internal boxes are not stored: a box is internal iff the first leaf at or behind its lower corner lies
// inside it and is deeper, one binary search.  The build is level-synchronous (the boxes of depth d are decided
// together; the host reads one count per level), the balance runs in rounds that read the tree the round began with and
// write the next one (one count per round).  No kernel waits on another thread's store, every loop is bounded by a
// count known at launch, and the only atomics are integer ones.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "wtp_device.hpp"

namespace wtp {

static constexpr int kNtThreads = 256;
static constexpr int kNtMaxDepth = 20;
static constexpr int64_t kNtChunk = int64_t(1) << 18; // boxes whose probe points are in flight at once
static constexpr int64_t kNtMaxLeaves = int64_t(1) << 28;
static constexpr int kNtParts = 1024;                 // block partials of the integral

template <typename T> struct NtEps;
template <> struct NtEps<float> { static constexpr float v = 1.1920928955078125e-07f; };
template <> struct NtEps<double> { static constexpr double v = 2.220446049250313e-16; };

template <typename T> struct NodeRoot {
    T org[3];
    T size, absmin, alpha, hconst, sqrt_eps;
};

struct NtRed {
    unsigned long long n_int, n_bnd, n_ext, hmin_bits; // hmin: bits of the smallest h (as double) of a non-exterior leaf
    int32_t depth_max, bad, pad_[2];
    double part[kNtParts];
};

// ---- keys ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t nt_spread(uint32_t v) { // 21 bits, two zeros between neighbours
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
__host__ __device__ inline uint32_t nt_compact(uint64_t x) {
    x &= 0x1249249249249249ull;
    x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
    x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
    x = (x ^ (x >> 8)) & 0x1f0000ff0000ffull;
    x = (x ^ (x >> 16)) & 0x1f00000000ffffull;
    x = (x ^ (x >> 32)) & 0x1fffffull;
    return (uint32_t)x;
}
__host__ __device__ inline uint64_t nt_morton(const int32_t c[3]) {
    return nt_spread((uint32_t)c[0]) | nt_spread((uint32_t)c[1]) << 1 | nt_spread((uint32_t)c[2]) << 2;
}
__host__ __device__ inline uint64_t nt_key(int d, const int32_t c[3]) { return ((nt_morton(c) << 1) | 1ull) << (3 * (kNtMaxDepth - d)); }
__host__ __device__ inline int nt_depth(uint64_t key) { return kNtMaxDepth - __builtin_ctzll(key) / 3; }
__host__ __device__ inline void nt_decode(uint64_t key, int* d, int32_t c[3]) {
    const int s = __builtin_ctzll(key);
    *d = kNtMaxDepth - s / 3;
    const uint64_t m = key >> (s + 1);
    c[0] = (int32_t)nt_compact(m), c[1] = (int32_t)nt_compact(m >> 1), c[2] = (int32_t)nt_compact(m >> 2);
}
// Morton code of the box's lower corner at depth 20: strictly increasing along the leaf array
__host__ __device__ inline uint64_t nt_start(uint64_t key) {
    const int s = __builtin_ctzll(key);
    return (key >> (s + 1)) << s;
}
// first leaf whose lower corner is at or behind `target`
__device__ inline int64_t nt_lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t target) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (nt_start(keys[mid]) < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// is the box (d, c), d < 20, an internal box of the tree?
__device__ inline bool nt_internal(const uint64_t* __restrict__ keys, int64_t n, int d, const int32_t c[3]) {
    const int s = 3 * (kNtMaxDepth - d);
    const uint64_t a = nt_morton(c) << s;
    const int64_t p = nt_lower_bound(keys, n, a);
    if (p >= n) return false;
    const uint64_t k = keys[p];
    return nt_start(k) < a + (1ull << s) && nt_depth(k) > d;
}

// ---- box geometry (spatial_octree.jl:107-128) -----------------------------------------------------------------------
template <typename T> __device__ inline T nt_hbox(const NodeRoot<T>& r, int d) { return r.size / (T)(1 << d); }
template <typename T> __device__ inline void nt_bounds(const NodeRoot<T>& r, int d, const int32_t c[3], T lo[3], T hi[3]) {
    const T h = nt_hbox(r, d);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = r.org[a] + (T)c[a] * h;
        hi[a] = lo[a] + h;
    }
}
template <typename T> __device__ inline void nt_centre(const NodeRoot<T>& r, int d, const int32_t c[3], T out[3]) {
    const T h = nt_hbox(r, d);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = r.org[a] + ((T)(2 * c[a] + 1) * h) / (T)2;
}

// per box of a pass (position front[f] of the leaf array, or f itself): centre, {lo, hi} and the probe tolerance
template <typename T>
__global__ void __launch_bounds__(kNtThreads)
nt_boxes_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ front, int64_t nf, NodeRoot<T> root,
                T* __restrict__ ctr, T* __restrict__ lohi, T* __restrict__ tol) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += stride) {
        int d;
        int32_t c[3];
        nt_decode(keys[front ? front[f] : f], &d, c);
        T lo[3], hi[3], m[3];
        nt_bounds(root, d, c, lo, hi);
        nt_centre(root, d, c, m);
        const T t = nt_hbox(root, d) * (T)1.0e-6;
#pragma unroll
        for (int a = 0; a < 3; ++a) ctr[3 * f + a] = m[a], lohi[6 * f + a] = lo[a], lohi[6 * f + 3 + a] = hi[a];
        tol[f] = (T)1.0e-8 > t ? (T)1.0e-8 : t;
    }
}

// should_subdivide (spacing_criterion.jl:43-52) and the depth cap; a value that is not finite is an error of the call
template <typename T>
__global__ void __launch_bounds__(kNtThreads)
nt_criterion_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ front, int64_t nf, NodeRoot<T> root,
                    const T* __restrict__ h, uint8_t* __restrict__ flag, int32_t* __restrict__ bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += stride) {
        const int d = nt_depth(keys[front[f]]);
        const T hb = nt_hbox(root, d), hl = h ? h[f] : root.hconst;
        if (!(hl == hl) || hl == Lim<T>::inf() || hl == -Lim<T>::inf()) atomicOr(bad, 1);
        flag[f] = (d < kNtMaxDepth && hb > root.absmin && hl > NtEps<T>::v && hb > root.alpha * hl) ? 1 : 0;
    }
}

// _box_probe_points (spacing_criterion.jl:137-187): per axis 0 = lo, 1 = hi, 2 = mid, two bits each
__device__ const uint8_t kNtProbe[27] = {42, 0, 1, 4, 5, 16, 17, 20, 21, 40, 41, 34, 38, 10, 26,
                                        2, 6, 18, 22, 8, 9, 24, 25, 32, 33, 36, 37};

// probe points of boxes f0 .. f0 + nb - 1 of a pass, `per` each (27: the refinement's; 9: the leaf vote's, whose first
// point is the box's centre as box_center computes it, not the mean of its corners)
template <typename T>
__global__ void __launch_bounds__(kNtThreads)
nt_probes_kernel(const T* __restrict__ ctr, const T* __restrict__ lohi, int64_t f0, int64_t nb, int per, T* __restrict__ pts) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, total = nb * per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t f = f0 + i / per;
        const int p = (int)(i % per);
        const int sel = kNtProbe[p];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const T lo = lohi[6 * f + a], hi = lohi[6 * f + 3 + a];
            const int s = (sel >> (2 * a)) & 3;
            pts[3 * i + a] = s == 0 ? lo : (s == 1 ? hi : (per == 9 ? ctr[3 * f + a] : (lo + hi) / (T)2));
        }
    }
}

// refinement: a box that passed the size tests splits if a probe is not exterior; if all are, the touch walk decides
__global__ void __launch_bounds__(kNtThreads)
nt_probe_any_kernel(const uint8_t* __restrict__ pcls, int64_t f0, int64_t nb, uint8_t* __restrict__ flag, uint8_t* __restrict__ need) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride) {
        const int64_t f = f0 + b;
        if (!flag[f]) {
            need[f] = 0;
            continue;
        }
        bool any = false;
        for (int p = 0; p < 27; ++p) any = any || pcls[27 * b + p] != 0;
        need[f] = any ? 0 : 1; // flag stays 1: "passed the size tests"; the touch answer settles it below
    }
}

// leaf vote (_classify_leaf_conservative): 1 if any probe is boundary or they disagree, else the common class
__global__ void __launch_bounds__(kNtThreads)
nt_vote_kernel(const uint8_t* __restrict__ pcls, int64_t f0, int64_t nb, uint8_t* __restrict__ cls, uint8_t* __restrict__ need) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride) {
        const uint8_t first = pcls[9 * b];
        bool same = true, bnd = false;
        for (int p = 0; p < 9; ++p) {
            const uint8_t c = pcls[9 * b + p];
            same = same && c == first;
            bnd = bnd || c == 1;
        }
        const uint8_t v = (bnd || !same) ? 1 : first;
        cls[f0 + b] = v;
        need[f0 + b] = v != 1;
    }
}

__global__ void __launch_bounds__(kNtThreads) nt_ones_kernel(int32_t* __restrict__ cnt, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) cnt[i] = 1;
}

// the level's verdicts into the leaf array's counts
__global__ void __launch_bounds__(kNtThreads)
nt_level_counts_kernel(const int32_t* __restrict__ front, int64_t nf, const uint8_t* __restrict__ flag,
                       const uint8_t* __restrict__ need, const uint8_t* __restrict__ touch, int32_t* __restrict__ cnt) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += stride)
        if (flag[f] && (!need[f] || touch[f])) cnt[front[f]] = 8;
}

// needs_balancing && can_subdivide (spatial_octree.jl:452-464, 488) of every leaf, on the tree as the round found it
template <typename T>
__global__ void __launch_bounds__(kNtThreads)
nt_balance_kernel(const uint64_t* __restrict__ keys, int64_t n, NodeRoot<T> root, int32_t* __restrict__ cnt) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        int d;
        int32_t c[3];
        nt_decode(keys[i], &d, c);
        bool split = false;
        if (d < kNtMaxDepth - 1 && nt_hbox(root, d) > root.absmin) { // a grandchild of a neighbour has depth d + 2 <= 20
            for (int dir = 0; dir < 6 && !split; ++dir) {
                int32_t nc[3] = {c[0], c[1], c[2]};
                nc[dir >> 1] += (dir & 1) ? 1 : -1;
                if (nc[dir >> 1] < 0 || nc[dir >> 1] >= (1 << d)) continue;
                if (!nt_internal(keys, n, d, nc)) continue;
                for (int m = 0; m < 8 && !split; ++m) {
                    const int32_t cc[3] = {2 * nc[0] + (m & 1), 2 * nc[1] + ((m >> 1) & 1), 2 * nc[2] + ((m >> 2) & 1)};
                    split = nt_internal(keys, n, d + 1, cc);
                }
            }
        }
        cnt[i] = split ? 8 : 1;
    }
}

// every leaf to its new place; a split leaf's children in child order, which is Morton order.  off[i] - i is 7 times the
// splits before i, which numbers the children of the level for the next level's list.
__global__ void __launch_bounds__(kNtThreads)
nt_expand_kernel(const uint64_t* __restrict__ keys, int64_t n, const int32_t* __restrict__ cnt, const int64_t* __restrict__ off,
                 uint64_t* __restrict__ out, int32_t* __restrict__ front_out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t o = off[i];
        if (cnt[i] == 1) {
            out[o] = keys[i];
            continue;
        }
        int d;
        int32_t c[3];
        nt_decode(keys[i], &d, c);
        const int64_t r = (o - i) / 7 * 8;
        for (int m = 0; m < 8; ++m) {
            const int32_t cc[3] = {2 * c[0] + (m & 1), 2 * c[1] + ((m >> 1) & 1), 2 * c[2] + ((m >> 2) & 1)};
            out[o + m] = nt_key(d + 1, cc);
            if (front_out) front_out[r + m] = (int32_t)(o + m);
        }
    }
}

// the final class, h = max(h(centre), sqrt(eps)) and the info's reductions.  The integral's terms are summed per thread
// in stride order and per block in a fixed tree: the partials do not depend on arrival order.
template <typename T>
__global__ void __launch_bounds__(kNtThreads)
nt_finish_kernel(const uint64_t* __restrict__ keys, int64_t n, NodeRoot<T> root, const T* __restrict__ h, uint8_t* __restrict__ cls,
                 const uint8_t* __restrict__ need, const uint8_t* __restrict__ touch, T* __restrict__ hout, NtRed* __restrict__ red) {
    __shared__ double sm[kNtThreads];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double acc = 0;
    unsigned long long n_int = 0, n_bnd = 0, n_ext = 0, hmin = ~0ull;
    int dmax = 0;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int d = nt_depth(keys[i]);
        const T hl = h ? h[i] : root.hconst;
        bad = bad || !(hl == hl) || hl == Lim<T>::inf() || hl == -Lim<T>::inf();
        const T hv = hl > root.sqrt_eps ? hl : root.sqrt_eps;
        hout[i] = hv;
        uint8_t c = cls[i];
        if (need[i] && touch[i]) c = 1;
        cls[i] = c;
        dmax = d > dmax ? d : dmax;
        if (c == 0) {
            ++n_ext;
            continue;
        }
        n_int += c == 2, n_bnd += c == 1;
        const T hb = nt_hbox(root, d);
        acc += (double)(((hb * hb) * hb) / ((hv * hv) * hv));
        const unsigned long long hb64 = (unsigned long long)__double_as_longlong((double)hv); // positive: bits order as values
        hmin = hb64 < hmin ? hb64 : hmin;
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kNtThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) red->part[blockIdx.x] = sm[0];
    if (n_int) atomicAdd(&red->n_int, n_int);
    if (n_bnd) atomicAdd(&red->n_bnd, n_bnd);
    if (n_ext) atomicAdd(&red->n_ext, n_ext);
    if (hmin != ~0ull) atomicMin(&red->hmin_bits, hmin);
    if (dmax) atomicMax(&red->depth_max, dmax);
    if (bad) atomicOr(&red->bad, 1);
}

// find_leaf (spatial_octree.jl:223-234).  The path of a point does not depend on where the tree stops, so it is walked
// to depth 20 and the leaf that holds that cell is found by one search.
template <typename TM, typename TP>
__global__ void __launch_bounds__(kNtThreads)
nt_locate_kernel(const uint64_t* __restrict__ keys, int64_t n, NodeRoot<TM> root, const TP* __restrict__ xyz, int64_t np,
                 int64_t* __restrict__ leaf) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += stride) {
        const TM p[3] = {(TM)xyz[3 * i], (TM)xyz[3 * i + 1], (TM)xyz[3 * i + 2]};
        bool in = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) in = in && p[a] >= root.org[a] && p[a] <= root.org[a] + root.size;
        if (!in) {
            leaf[i] = -1;
            continue;
        }
        int32_t c[3] = {0, 0, 0};
        for (int d = 0; d < kNtMaxDepth; ++d) {
            TM m[3];
            nt_centre(root, d, c, m);
#pragma unroll
            for (int a = 0; a < 3; ++a) c[a] = 2 * c[a] + (p[a] >= m[a] ? 1 : 0);
        }
        const uint64_t q = nt_morton(c);
        // the last leaf whose lower corner is at or before q: leaves tile the root, so it holds q
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (nt_start(keys[mid]) <= q) lo = mid + 1;
            else hi = mid;
        }
        leaf[i] = lo - 1;
    }
}

static int nt_grid(int64_t n) { return grid_for(n, kNtThreads, 4096); }

template <typename T> static NodeRoot<T> nt_root_of(const wtp_ctx* ctx, double alpha, double ratio, double hconst) {
    NodeRoot<T> r;
    T top[3];
    for (int a = 0; a < 3; ++a) {
        const T lo = (T)ctx->mesh.bbox[a], hi = (T)ctx->mesh.bbox[3 + a];
        const T centre = (lo + hi) * (T)0.5, half = ((hi - lo) * (T)0.5) * (T)1.02;
        r.org[a] = centre - half;
        top[a] = centre + half;
    }
    r.size = std::max(top[0] - r.org[0], std::max(top[1] - r.org[1], top[2] - r.org[2]));
    T e[3];
    for (int a = 0; a < 3; ++a) e[a] = (r.org[a] + r.size) - r.org[a];
    const T diag = std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    r.absmin = diag * (T)ratio;
    r.alpha = (T)alpha;
    r.hconst = (T)hconst;
    r.sqrt_eps = std::sqrt(NtEps<T>::v);
    return r;
}

template <typename T> static NodeRoot<T> nt_root_held(const NodeTreeState& S) { // the root of the resident tree
    NodeRoot<T> r{};
    for (int a = 0; a < 3; ++a) r.org[a] = (T)S.info.origin[a];
    r.size = (T)S.info.root_size;
    r.absmin = (T)S.info.absolute_min;
    return r;
}

// probes of the boxes of a pass, chunk by chunk: classes of `per` points per box, then `reduce` over the chunk
template <typename T, typename Reduce>
static int nt_probe_pass(wtp_ctx* ctx, int64_t nb, int per, const uint8_t* d_need, Reduce&& reduce) {
    NodeTreeState& S = ctx->ntree;
    int rc;
    const int64_t chunk = std::min(nb, kNtChunk);
    if ((rc = ensure(ctx, S.pts, sizeof(T) * 3 * (size_t)(chunk * per)))) return rc;
    if ((rc = ensure(ctx, S.pcls, (size_t)(chunk * per)))) return rc;
    for (int64_t f0 = 0; f0 < nb; f0 += chunk) {
        const int64_t m = std::min(chunk, nb - f0);
        hipLaunchKernelGGL(nt_probes_kernel<T>, dim3(nt_grid(m * per)), dim3(kNtThreads), 0, ctx->stream, (const T*)S.ctr.p,
                           (const T*)S.lohi.p, f0, m, per, (T*)S.pts.p);
        // exterior by default: a box that is not wanted leaves its probes unwritten
        WTP_HIP(ctx, hipMemsetAsync(S.pcls.p, 0, (size_t)(m * per), ctx->stream));
        if ((rc = launch_mesh_point_class<T>(ctx, (const T*)S.pts.p, m * per, (const T*)S.tol.p + f0, per,
                                             d_need ? d_need + f0 : nullptr, (uint8_t*)S.pcls.p)))
            return rc;
        reduce(f0, m);
        WTP_HIP(ctx, hipGetLastError());
    }
    return WTP_OK;
}

// room for the per-box arrays of a pass over nb boxes
template <typename T> static int nt_ensure_pass(wtp_ctx* ctx, int64_t nb) {
    NodeTreeState& S = ctx->ntree;
    int rc;
    if ((rc = ensure(ctx, S.ctr, sizeof(T) * 3 * (size_t)nb))) return rc;
    if ((rc = ensure(ctx, S.lohi, sizeof(T) * 6 * (size_t)nb))) return rc;
    if ((rc = ensure(ctx, S.tol, sizeof(T) * (size_t)nb))) return rc;
    if ((rc = ensure(ctx, S.h, sizeof(T) * (size_t)nb))) return rc;
    if ((rc = ensure(ctx, S.flag, (size_t)nb))) return rc;
    if ((rc = ensure(ctx, S.need, (size_t)nb))) return rc;
    if ((rc = ensure(ctx, S.touch, (size_t)nb))) return rc;
    return WTP_OK;
}

// counts -> offsets -> the next leaf array; *n_new from the host's one read of the pass.  *bad: the spacing flag
template <typename T> static int nt_apply_counts(wtp_ctx* ctx, int64_t n, bool want_front, int64_t* n_new, int32_t* bad) {
    NodeTreeState& S = ctx->ntree;
    int rc;
    if ((rc = ensure(ctx, S.off, sizeof(int64_t) * (size_t)(n + 1)))) return rc;
    if ((rc = ensure(ctx, S.scan_tmp, offsets_scan_tmp_bytes(n)))) return rc;
    if ((rc = launch_offsets_scan(ctx, (const int32_t*)S.cnt.p, n, (int64_t*)S.scan_tmp.p, (int64_t*)S.off.p))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(n_new, (const int64_t*)S.off.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    WTP_HIP(ctx, hipMemcpyAsync(bad, &((NtRed*)S.red.p)->bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    if (*bad) return fail(ctx, WTP_ERR_ARG, "the spacing at a box centre of the node tree is not finite");
    if (*n_new == n) return WTP_OK;
    if (*n_new > kNtMaxLeaves) return fail(ctx, WTP_ERR_ARG, "the node tree exceeds 2^28 leaves: raise alpha or node_min_ratio");
    const int nxt = 1 - S.cur;
    if ((rc = ensure(ctx, S.keys[nxt], sizeof(uint64_t) * (size_t)*n_new))) return rc;
    if (want_front && (rc = ensure(ctx, S.front[nxt], sizeof(int32_t) * (size_t)(*n_new - n) / 7 * 8))) return rc;
    hipLaunchKernelGGL(nt_expand_kernel, dim3(nt_grid(n)), dim3(kNtThreads), 0, ctx->stream, (const uint64_t*)S.keys[S.cur].p, n,
                       (const int32_t*)S.cnt.p, (const int64_t*)S.off.p, (uint64_t*)S.keys[nxt].p,
                       want_front ? (int32_t*)S.front[nxt].p : (int32_t*)nullptr);
    WTP_HIP(ctx, hipGetLastError());
    S.cur = nxt;
    return WTP_OK;
}

template <typename T>
static int node_tree_build_t(wtp_ctx* ctx, const wtp_spacing_desc* sp, double alpha, double ratio, wtp_node_tree_info* out) {
    NodeTreeState& S = ctx->ntree;
    const int64_t syncs0 = ctx->n_syncs;
    const bool law = spacing_on_device(sp->kind);
    int rc;
    if (law && (rc = ensure_kd(ctx, sp, 3, ctx->mesh.dtype))) return rc;
    const NodeRoot<T> root = nt_root_of<T>(ctx, alpha, ratio, sp->constant);
    const auto eval_h = [&](int64_t nb) { // h at the centres of the pass
        return law ? launch_spacing_eval<T>(ctx, (const T*)S.ctr.p, nb, 3, ctx->kd.nodes.p, ctx->kd.m, sp->kind, sp->p0, sp->p1,
                                            sp->p2, (T*)S.h.p)
                   : (int)WTP_OK;
    };
    if ((rc = ensure(ctx, S.red, sizeof(NtRed)))) return rc;
    NtRed* red = (NtRed*)S.red.p;
    WTP_HIP(ctx, hipMemsetAsync(red, 0, sizeof(NtRed), ctx->stream));
    WTP_HIP(ctx, hipMemsetAsync(&red->hmin_bits, 0xff, sizeof(unsigned long long), ctx->stream));
    // the root is the only leaf, and the first level's only box
    S.cur = 0;
    if ((rc = ensure(ctx, S.keys[0], sizeof(uint64_t)))) return rc;
    if ((rc = ensure(ctx, S.front[0], sizeof(int32_t)))) return rc;
    const uint64_t root_key = 1ull << (3 * kNtMaxDepth);
    const int32_t zero = 0;
    WTP_HIP(ctx, hipMemcpyAsync(S.keys[0].p, &root_key, sizeof root_key, hipMemcpyHostToDevice, ctx->stream));
    WTP_HIP(ctx, hipMemcpyAsync(S.front[0].p, &zero, sizeof zero, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = sync(ctx))) return rc; // the two host words go out of use
    int64_t n = 1, nf = 1;
    int32_t bad = 0;
    // ---- refinement, one level per pass (_subdivide_node_octree!) ----
    for (int level = 0; level <= kNtMaxDepth && nf > 0; ++level) {
        if ((rc = nt_ensure_pass<T>(ctx, nf))) return rc;
        if ((rc = ensure(ctx, S.cnt, sizeof(int32_t) * (size_t)n))) return rc;
        const uint64_t* keys = (const uint64_t*)S.keys[S.cur].p;
        const int32_t* front = (const int32_t*)S.front[S.cur].p;
        hipLaunchKernelGGL(nt_boxes_kernel<T>, dim3(nt_grid(nf)), dim3(kNtThreads), 0, ctx->stream, keys, front, nf, root,
                           (T*)S.ctr.p, (T*)S.lohi.p, (T*)S.tol.p);
        if ((rc = eval_h(nf))) return rc;
        hipLaunchKernelGGL(nt_criterion_kernel<T>, dim3(nt_grid(nf)), dim3(kNtThreads), 0, ctx->stream, keys, front, nf, root,
                           law ? (const T*)S.h.p : (const T*)nullptr, (uint8_t*)S.flag.p, &red->bad);
        WTP_HIP(ctx, hipGetLastError());
        // 27 probes of every box that passed the size tests, one lane per probe; all exterior: touch
        if ((rc = nt_probe_pass<T>(ctx, nf, 27, (const uint8_t*)S.flag.p, [&](int64_t f0, int64_t m) {
                hipLaunchKernelGGL(nt_probe_any_kernel, dim3(nt_grid(m)), dim3(kNtThreads), 0, ctx->stream,
                                   (const uint8_t*)S.pcls.p, f0, m, (uint8_t*)S.flag.p, (uint8_t*)S.need.p);
            })))
            return rc;
        WTP_HIP(ctx, hipMemsetAsync(S.touch.p, 0, (size_t)nf, ctx->stream));
        if ((rc = launch_mesh_box_touch<T>(ctx, (const T*)S.lohi.p, nf, (const uint8_t*)S.need.p, (uint8_t*)S.touch.p))) return rc;
        hipLaunchKernelGGL(nt_ones_kernel, dim3(nt_grid(n)), dim3(kNtThreads), 0, ctx->stream, (int32_t*)S.cnt.p, n);
        hipLaunchKernelGGL(nt_level_counts_kernel, dim3(nt_grid(nf)), dim3(kNtThreads), 0, ctx->stream, front, nf,
                           (const uint8_t*)S.flag.p, (const uint8_t*)S.need.p, (const uint8_t*)S.touch.p, (int32_t*)S.cnt.p);
        WTP_HIP(ctx, hipGetLastError());
        int64_t n_new = n;
        if ((rc = nt_apply_counts<T>(ctx, n, true, &n_new, &bad))) return rc;
        nf = (n_new - n) / 7 * 8;
        n = n_new;
    }
    // ---- 2:1 balance (balance_octree!) ----
    int rounds = 0;
    for (;;) {
        if (rounds == 100) return fail(ctx, WTP_ERR_INTERNAL, "the node tree's balance did not settle within 100 rounds");
        ++rounds;
        if ((rc = ensure(ctx, S.cnt, sizeof(int32_t) * (size_t)n))) return rc;
        hipLaunchKernelGGL(nt_balance_kernel<T>, dim3(nt_grid(n)), dim3(kNtThreads), 0, ctx->stream,
                           (const uint64_t*)S.keys[S.cur].p, n, root, (int32_t*)S.cnt.p);
        WTP_HIP(ctx, hipGetLastError());
        int64_t n_new = n;
        if ((rc = nt_apply_counts<T>(ctx, n, false, &n_new, &bad))) return rc;
        if (n_new == n) break;
        n = n_new;
    }
    // ---- classes, h and the info ----
    if ((rc = nt_ensure_pass<T>(ctx, n))) return rc;
    if ((rc = ensure(ctx, S.cls, (size_t)n))) return rc;
    if ((rc = ensure(ctx, S.hout, sizeof(T) * (size_t)n))) return rc;
    const uint64_t* keys = (const uint64_t*)S.keys[S.cur].p;
    hipLaunchKernelGGL(nt_boxes_kernel<T>, dim3(nt_grid(n)), dim3(kNtThreads), 0, ctx->stream, keys, (const int32_t*)nullptr, n,
                       root, (T*)S.ctr.p, (T*)S.lohi.p, (T*)S.tol.p);
    if ((rc = eval_h(n))) return rc;
    if ((rc = nt_probe_pass<T>(ctx, n, 9, nullptr, [&](int64_t f0, int64_t m) {
            hipLaunchKernelGGL(nt_vote_kernel, dim3(nt_grid(m)), dim3(kNtThreads), 0, ctx->stream, (const uint8_t*)S.pcls.p, f0, m,
                               (uint8_t*)S.cls.p, (uint8_t*)S.need.p);
        })))
        return rc;
    WTP_HIP(ctx, hipMemsetAsync(S.touch.p, 0, (size_t)n, ctx->stream));
    if ((rc = launch_mesh_box_touch<T>(ctx, (const T*)S.lohi.p, n, (const uint8_t*)S.need.p, (uint8_t*)S.touch.p))) return rc;
    const int blocks = grid_for(n, kNtThreads, kNtParts);
    hipLaunchKernelGGL(nt_finish_kernel<T>, dim3(blocks), dim3(kNtThreads), 0, ctx->stream, keys, n, root,
                       law ? (const T*)S.h.p : (const T*)nullptr, (uint8_t*)S.cls.p, (const uint8_t*)S.need.p,
                       (const uint8_t*)S.touch.p, (T*)S.hout.p, red);
    WTP_HIP(ctx, hipGetLastError());
    std::vector<char> hostred(sizeof(NtRed));
    WTP_HIP(ctx, hipMemcpyAsync(hostred.data(), red, sizeof(NtRed), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    const NtRed& R = *(const NtRed*)hostred.data();
    if (R.bad) return fail(ctx, WTP_ERR_ARG, "the spacing at a leaf centre of the node tree is not finite");
    wtp_node_tree_info& I = S.info;
    I = wtp_node_tree_info{};
    I.n_leaves = n;
    I.n_interior = (int64_t)R.n_int, I.n_boundary = (int64_t)R.n_bnd, I.n_exterior = (int64_t)R.n_ext;
    I.n_boxes = n + (n - 1) / 7;
    I.depth_max = R.depth_max, I.n_levels = R.depth_max + 1, I.balance_rounds = rounds;
    double integral = 0;
    for (int b = 0; b < blocks; ++b) integral += R.part[b];
    I.integral = integral;
    const double auto_cap = std::ceil(1.5 * integral); // h clamped to sqrt(eps) in a coarse box: up to 1e24 in Float64
    I.max_points_auto = auto_cap >= 9223372036854775808.0 ? INT64_MAX : (int64_t)auto_cap;
    I.h_min = 0;
    if (R.hmin_bits != ~0ull) memcpy(&I.h_min, &R.hmin_bits, sizeof(double));
    for (int a = 0; a < 3; ++a) I.origin[a] = (double)root.org[a];
    I.root_size = (double)root.size, I.absolute_min = (double)root.absmin;
    I.host_syncs = (int32_t)(ctx->n_syncs - syncs0);
    S.n = n;
    S.dtype = ctx->mesh.dtype;
    S.valid = true;
    if (out) *out = I;
    return WTP_OK;
}

// ---- per-leaf placements (include/wtp.h: wtp_node_place) ------------------------------------------------------------------
// Every step is one thread per leaf, per draw or per point; "which leaf" is always the same search, the first leaf whose
// inclusive running sum exceeds a number, over sums that cover ALL leaves with zeros outside the group, so that a group
// needs no list of its own and a leaf's index is its place in leaf order.
__device__ inline uint64_t np_splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ inline uint64_t np_draw(uint64_t seed, int stage, uint64_t j, int a) {
    return np_splitmix64((seed << 40) + 3ull * (((uint64_t)stage << 36) + j) + (uint64_t)a);
}
template <typename T> __device__ inline T np_uniform(uint64_t seed, int stage, uint64_t j, int a) {
    return (T)((float)(np_draw(seed, stage, j, a) >> 40) * (1.0f / 16777216.0f));
}
// first i with cum[i] > x; the caller guarantees x < cum[n - 1]
__device__ inline int64_t np_first_above(const uint64_t* __restrict__ cum, int64_t n, uint64_t x) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cum[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// w[i] (interior leaves) and w[n + i] (boundary leaves), zero elsewhere, and their block partials in fixed order
template <typename T>
__global__ void __launch_bounds__(kNtThreads)
np_weights_kernel(const uint64_t* __restrict__ keys, int64_t n, NodeRoot<T> root, const T* __restrict__ hout,
                  const uint8_t* __restrict__ cls, double* __restrict__ w, double* __restrict__ part) {
    __shared__ double sm[2][kNtThreads];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double a_int = 0, a_ns = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const T hb = nt_hbox(root, nt_depth(keys[i])), hv = hout[i];
        const double t = (double)(((hb * hb) * hb) / ((hv * hv) * hv));
        const uint8_t c = cls[i];
        w[i] = c == 2 ? t : 0.0;
        w[n + i] = c == 1 ? t : 0.0;
        a_int += c == 2 ? t : 0.0;
        a_ns += c == 1 ? t : 0.0;
    }
    sm[0][threadIdx.x] = a_int, sm[1][threadIdx.x] = a_ns;
    __syncthreads();
    for (int s = kNtThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[0][threadIdx.x] += sm[0][threadIdx.x + s], sm[1][threadIdx.x] += sm[1][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sm[0][0], part[kNtParts + blockIdx.x] = sm[1][0];
}

// inclusive running sums of 64-bit integers: a thread sums its tile of 256, one thread scans the tiles, a thread rescans
static constexpr int kNpTile = 256;
__global__ void __launch_bounds__(kNtThreads) np_tile_sum_kernel(const uint64_t* __restrict__ v, int64_t n, uint64_t* __restrict__ tile) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t * kNpTile < n; t += stride) {
        uint64_t s = 0;
        for (int64_t i = t * kNpTile; i < (t + 1) * kNpTile && i < n; ++i) s += v[i];
        tile[t] = s;
    }
}
__global__ void np_tile_scan_kernel(uint64_t* __restrict__ tile, int64_t ntiles) {
    uint64_t run = 0;
    for (int64_t i = 0; i < ntiles; ++i) {
        const uint64_t t = tile[i];
        tile[i] = run;
        run += t;
    }
}
__global__ void __launch_bounds__(kNtThreads)
np_tile_apply_kernel(const uint64_t* __restrict__ v, int64_t n, const uint64_t* __restrict__ tile, uint64_t* __restrict__ cum) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t * kNpTile < n; t += stride) {
        uint64_t run = tile[t];
        for (int64_t i = t * kNpTile; i < (t + 1) * kNpTile && i < n; ++i) cum[i] = (run += v[i]);
    }
}

// mode 0: base counts and the fractions' F of a group for `count` points; 1: the deficit's F = floor(w / W 2^32); 2: the
// uniform rule, F = 1 on the group's leaves (class `group`)
__global__ void __launch_bounds__(kNtThreads)
np_shares_kernel(const double* __restrict__ w, int64_t n, double W, int64_t count, int mode, const uint8_t* __restrict__ cls,
                 uint8_t group, uint64_t* __restrict__ cnt, uint64_t* __restrict__ F) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (mode == 2) {
            F[i] = cls[i] == group ? 1 : 0;
        } else if (mode == 1) {
            F[i] = (uint64_t)floor((w[i] / W) * 4294967296.0);
        } else {
            const double e = (double)count * (w[i] / W), b = floor(e);
            cnt[i] = (uint64_t)b;
            F[i] = (uint64_t)floor((e - b) * 4294967296.0);
        }
    }
}

// the leftover of a group's counts: draw t adds one to the leaf it picks (integer atomics: the sums do not depend on order)
__global__ void __launch_bounds__(kNtThreads)
np_leftover_kernel(const uint64_t* __restrict__ fcum, int64_t n, uint64_t ftotal, uint64_t seed, int stage, int64_t leftover,
                   unsigned long long* __restrict__ cnt) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < leftover; t += stride)
        atomicAdd(&cnt[np_first_above(fcum, n, __umul64hi(np_draw(seed, stage, (uint64_t)t, 0), ftotal))], 1ull);
}

// point j of a stage: its leaf from the counts' running sums, its rank in the leaf, then the placement's formula
template <typename T>
__global__ void __launch_bounds__(kNtThreads)
np_points_kernel(const uint64_t* __restrict__ keys, int64_t n, NodeRoot<T> root, const uint64_t* __restrict__ cnt,
                 const uint64_t* __restrict__ cum, int64_t total, int placement, uint64_t seed, int stage, T* __restrict__ xyz,
                 int64_t* __restrict__ leaf) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) {
        const int64_t i = np_first_above(cum, n, (uint64_t)j);
        const uint64_t nn = cnt[i], k = (uint64_t)j - (cum[i] - nn);
        int d;
        int32_t c[3];
        nt_decode(keys[i], &d, c);
        T lo[3], hi[3];
        nt_bounds(root, d, c, lo, hi);
        uint64_t g = 1;
        while (g * g * g < nn) ++g;
        const uint64_t cell[3] = {k % g, (k / g) % g, k / (g * g)};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const T e = hi[a] - lo[a];
            T p;
            if (placement == 0) {
                p = lo[a] + np_uniform<T>(seed, stage, (uint64_t)j, a) * e;
            } else {
                const T cs = e / (T)g, cmin = lo[a] + (T)cell[a] * cs;
                p = placement == 2 ? cmin + cs / (T)2 : cmin + np_uniform<T>(seed, stage, (uint64_t)j, a) * cs;
            }
            xyz[3 * j + a] = p;
        }
        leaf[j] = i;
    }
}

// deficit point t: a leaf by pick (stage 5), a uniform point in it (stage 2)
template <typename T>
__global__ void __launch_bounds__(kNtThreads)
np_deficit_kernel(const uint64_t* __restrict__ keys, int64_t n, NodeRoot<T> root, const uint64_t* __restrict__ fcum,
                  uint64_t ftotal, uint64_t seed, int64_t count, T* __restrict__ xyz, int64_t* __restrict__ leaf) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += stride) {
        const int64_t i = np_first_above(fcum, n, __umul64hi(np_draw(seed, 5, (uint64_t)t, 0), ftotal));
        int d;
        int32_t c[3];
        nt_decode(keys[i], &d, c);
        T lo[3], hi[3];
        nt_bounds(root, d, c, lo, hi);
#pragma unroll
        for (int a = 0; a < 3; ++a) xyz[3 * t + a] = lo[a] + np_uniform<T>(seed, 2, (uint64_t)t, a) * (hi[a] - lo[a]);
        leaf[t] = i;
    }
}

__global__ void __launch_bounds__(kNtThreads) np_flags_kernel(const uint8_t* __restrict__ in, int64_t m, uint64_t* __restrict__ f) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) f[i] = in[i] ? 1 : 0;
}

// the inside candidates, in candidate order, as far as there is room
template <typename T>
__global__ void __launch_bounds__(kNtThreads)
np_compact_kernel(const T* __restrict__ cand, const int64_t* __restrict__ cleaf, const uint8_t* __restrict__ in,
                  const uint64_t* __restrict__ cum, int64_t m, int64_t room, T* __restrict__ xyz, int64_t* __restrict__ leaf) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        if (!in[i]) continue;
        const int64_t o = (int64_t)cum[i] - 1;
        if (o >= room) continue;
        xyz[3 * o] = cand[3 * i], xyz[3 * o + 1] = cand[3 * i + 1], xyz[3 * o + 2] = cand[3 * i + 2];
        leaf[o] = cleaf[i];
    }
}

// cum = inclusive running sums of v[0 .. m); *total (host) = cum[m - 1] after the caller's sync
static int np_scan(wtp_ctx* ctx, const uint64_t* v, int64_t m, uint64_t* cum, uint64_t* total) {
    NodeTreeState& S = ctx->ntree;
    const int64_t ntiles = (m + kNpTile - 1) / kNpTile;
    int rc;
    if ((rc = ensure(ctx, S.p_tile, sizeof(uint64_t) * (size_t)ntiles))) return rc;
    uint64_t* tile = (uint64_t*)S.p_tile.p;
    hipLaunchKernelGGL(np_tile_sum_kernel, dim3(nt_grid(ntiles)), dim3(kNtThreads), 0, ctx->stream, v, m, tile);
    hipLaunchKernelGGL(np_tile_scan_kernel, dim3(1), dim3(1), 0, ctx->stream, tile, ntiles);
    hipLaunchKernelGGL(np_tile_apply_kernel, dim3(nt_grid(ntiles)), dim3(kNtThreads), 0, ctx->stream, v, m, (const uint64_t*)tile, cum);
    WTP_HIP(ctx, hipGetLastError());
    if (total) WTP_HIP(ctx, hipMemcpyAsync(total, cum + (m - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    return WTP_OK;
}

// F (as np_shares_kernel's mode makes it) and its running sums; the uniform rule if they come to nothing.  *ftotal on return
static int np_pick_table(wtp_ctx* ctx, const double* w, double W, int64_t count, int mode, uint8_t group, uint64_t* ftotal,
                         uint64_t* base_total) {
    NodeTreeState& S = ctx->ntree;
    const int64_t n = S.n;
    uint64_t *cnt = (uint64_t*)S.p_cnt.p, *F = (uint64_t*)S.p_f.p, *fcum = (uint64_t*)S.p_fcum.p, *cum = (uint64_t*)S.p_cum.p;
    int rc;
    hipLaunchKernelGGL(np_shares_kernel, dim3(nt_grid(n)), dim3(kNtThreads), 0, ctx->stream, w, n, W, count, mode,
                       (const uint8_t*)S.cls.p, group, cnt, F);
    if ((rc = np_scan(ctx, F, n, fcum, ftotal))) return rc;
    if (base_total && (rc = np_scan(ctx, cnt, n, cum, base_total))) return rc;
    if ((rc = sync(ctx))) return rc;
    if (*ftotal == 0) {
        hipLaunchKernelGGL(np_shares_kernel, dim3(nt_grid(n)), dim3(kNtThreads), 0, ctx->stream, w, n, W, count, 2,
                           (const uint8_t*)S.cls.p, group, cnt, F);
        if ((rc = np_scan(ctx, F, n, fcum, ftotal))) return rc;
        if ((rc = sync(ctx))) return rc;
    }
    return WTP_OK;
}

// `count` points of a group (weights w, sum W, class `group`) into xyz / leaf: counts, their running sums, the points
template <typename T>
static int np_group_points(wtp_ctx* ctx, const NodeRoot<T>& root, const double* w, double W, uint8_t group, int64_t count,
                           int placement, uint64_t seed, int pick_stage, int point_stage, T* xyz, int64_t* leaf) {
    if (count < 1) return WTP_OK;
    NodeTreeState& S = ctx->ntree;
    const int64_t n = S.n;
    uint64_t ftotal = 0, base_total = 0;
    int rc;
    if ((rc = np_pick_table(ctx, w, W, count, 0, group, &ftotal, &base_total))) return rc;
    const int64_t leftover = (int64_t)base_total < count ? count - (int64_t)base_total : 0;
    if (leftover > 0 && ftotal == 0) return fail(ctx, WTP_ERR_INTERNAL, "wtp_node_place: a group with points to place has no leaf");
    if (leftover > 0)
        hipLaunchKernelGGL(np_leftover_kernel, dim3(nt_grid(leftover)), dim3(kNtThreads), 0, ctx->stream, (const uint64_t*)S.p_fcum.p,
                           n, ftotal, seed, pick_stage, leftover, (unsigned long long*)S.p_cnt.p);
    if ((rc = np_scan(ctx, (const uint64_t*)S.p_cnt.p, n, (uint64_t*)S.p_cum.p, nullptr))) return rc;
    const int64_t total = (int64_t)base_total + leftover; // = count unless the bases alone exceed it
    if (total != count) return fail(ctx, WTP_ERR_INTERNAL, "wtp_node_place: the base counts exceed the points to place");
    hipLaunchKernelGGL(np_points_kernel<T>, dim3(nt_grid(total)), dim3(kNtThreads), 0, ctx->stream, (const uint64_t*)S.keys[S.cur].p,
                       n, root, (const uint64_t*)S.p_cnt.p, (const uint64_t*)S.p_cum.p, total, placement, seed, point_stage, xyz, leaf);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

template <typename T>
static int node_place_t(wtp_ctx* ctx, int placement, int64_t max_points, double oversampling, uint64_t seed,
                        wtp_node_place_info* out) {
    NodeTreeState& S = ctx->ntree;
    const int64_t syncs0 = ctx->n_syncs, n = S.n;
    const NodeRoot<T> root = nt_root_held<T>(S);
    int rc;
    if ((rc = ensure(ctx, S.p_w, sizeof(double) * 2 * (size_t)n))) return rc;
    for (DevBuf* b : {&S.p_cnt, &S.p_cum, &S.p_f, &S.p_fcum})
        if ((rc = ensure(ctx, *b, sizeof(uint64_t) * (size_t)n))) return rc;
    double* w = (double*)S.p_w.p;
    if ((rc = ensure(ctx, S.p_tile, sizeof(double) * 2 * kNtParts))) return rc;
    double* parts = (double*)S.p_tile.p; // both groups' block partials; the scans' tiles take the buffer over afterwards
    const int blocks = grid_for(n, kNtThreads, kNtParts);
    hipLaunchKernelGGL(np_weights_kernel<T>, dim3(blocks), dim3(kNtThreads), 0, ctx->stream, (const uint64_t*)S.keys[S.cur].p, n, root,
                       (const T*)S.hout.p, (const uint8_t*)S.cls.p, w, parts);
    WTP_HIP(ctx, hipGetLastError());
    std::vector<double> hp(2 * kNtParts);
    WTP_HIP(ctx, hipMemcpyAsync(hp.data(), parts, sizeof(double) * 2 * kNtParts, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    double W_int = 0, W_ns = 0;
    for (int b = 0; b < blocks; ++b) W_int += hp[b], W_ns += hp[kNtParts + b];
    wtp_node_place_info I{};
    I.placement = placement, I.W_int = W_int, I.W_ns = W_ns;
    if (W_int + W_ns > 0) {
        const int64_t n_int = (int64_t)std::nearbyint((double)max_points * (W_int / (W_int + W_ns)));
        const int64_t n_ns = max_points - n_int;
        const double cand = std::nearbyint((double)n_ns * oversampling);
        if (!(cand <= 2147483648.0)) return fail(ctx, WTP_ERR_ARG, "boundary_oversampling asks for more than 2^31 candidates");
        const int64_t n_cand = (int64_t)cand;
        if ((rc = ensure(ctx, S.p_xyz, sizeof(T) * 3 * (size_t)max_points))) return rc;
        if ((rc = ensure(ctx, S.p_leaf, sizeof(int64_t) * (size_t)max_points))) return rc;
        T* xyz = (T*)S.p_xyz.p;
        int64_t* leaf = (int64_t*)S.p_leaf.p;
        if ((rc = np_group_points<T>(ctx, root, w, W_int, 2, n_int, placement, seed, 3, 0, xyz, leaf))) return rc;
        int64_t so_far = n_int, n_acc = 0;
        if (n_cand > 0) {
            if ((rc = ensure(ctx, S.p_cand, sizeof(T) * 3 * (size_t)n_cand))) return rc;
            if ((rc = ensure(ctx, S.p_cleaf, sizeof(int64_t) * (size_t)n_cand))) return rc;
            if ((rc = ensure(ctx, S.p_in, (size_t)n_cand))) return rc;
            if ((rc = np_group_points<T>(ctx, root, w + n, W_ns, 1, n_cand, placement, seed, 4, 1, (T*)S.p_cand.p, (int64_t*)S.p_cleaf.p)))
                return rc;
            if ((rc = launch_mesh_inside<T>(ctx, (const T*)S.p_cand.p, n_cand, (uint8_t*)S.p_in.p))) return rc;
            // the flags' running sums (the per-leaf arrays are free again, but too short for the candidates: two of their own)
            DevBuf fl, flc;
            if ((rc = ensure(ctx, fl, sizeof(uint64_t) * (size_t)n_cand))) return rc;
            if ((rc = ensure(ctx, flc, sizeof(uint64_t) * (size_t)n_cand))) return rc;
            hipLaunchKernelGGL(np_flags_kernel, dim3(nt_grid(n_cand)), dim3(kNtThreads), 0, ctx->stream, (const uint8_t*)S.p_in.p, n_cand,
                               (uint64_t*)fl.p);
            uint64_t n_in = 0;
            if ((rc = np_scan(ctx, (const uint64_t*)fl.p, n_cand, (uint64_t*)flc.p, &n_in))) return rc;
            const int64_t room = max_points - so_far;
            hipLaunchKernelGGL(np_compact_kernel<T>, dim3(nt_grid(n_cand)), dim3(kNtThreads), 0, ctx->stream, (const T*)S.p_cand.p,
                               (const int64_t*)S.p_cleaf.p, (const uint8_t*)S.p_in.p, (const uint64_t*)flc.p, n_cand, room,
                               xyz + 3 * so_far, leaf + so_far);
            WTP_HIP(ctx, hipGetLastError());
            if ((rc = sync(ctx))) return rc; // n_in is read, and fl / flc may go
            n_acc = std::min<int64_t>((int64_t)n_in, room);
            so_far += n_acc;
        }
        int64_t n_def = 0;
        if (so_far < max_points && W_int > 0) {
            n_def = max_points - so_far;
            uint64_t ftotal = 0;
            if ((rc = np_pick_table(ctx, w, W_int, 0, 1, 2, &ftotal, nullptr))) return rc;
            if (ftotal == 0) return fail(ctx, WTP_ERR_INTERNAL, "wtp_node_place: no interior leaf to fill the deficit from");
            hipLaunchKernelGGL(np_deficit_kernel<T>, dim3(nt_grid(n_def)), dim3(kNtThreads), 0, ctx->stream,
                               (const uint64_t*)S.keys[S.cur].p, n, root, (const uint64_t*)S.p_fcum.p, ftotal, seed, n_def,
                               xyz + 3 * so_far, leaf + so_far);
            WTP_HIP(ctx, hipGetLastError());
            so_far += n_def;
        }
        if ((rc = sync(ctx))) return rc;
        I.n_points = so_far, I.n_interior = n_int, I.n_candidates = n_cand, I.n_accepted = n_acc, I.n_deficit = n_def;
    }
    I.host_syncs = (int32_t)(ctx->n_syncs - syncs0);
    S.pinfo = I;
    S.placed = true;
    if (out) *out = I;
    return WTP_OK;
}

void node_tree_invalidate(wtp_ctx* ctx) {
    ctx->ntree.valid = false;
    ctx->ntree.placed = false;
    ctx->ntree.n = 0;
}

static int need_tree(wtp_ctx* ctx, const char* entry) {
    if (!ctx) return WTP_ERR_ARG;
    if (ctx->mesh.nt < 1) return fail(ctx, WTP_ERR_STATE, "no mesh: call wtp_mesh_set first");
    if (!ctx->ntree.valid) return fail(ctx, WTP_ERR_STATE, std::string(entry) + " before a successful wtp_node_tree_build");
    return WTP_OK;
}

} // namespace wtp

using namespace wtp;
#define WTP_API extern "C"

WTP_API int wtp_node_tree_build(wtp_ctx* ctx, const wtp_spacing_desc* sp, double alpha, double node_min_ratio,
                                wtp_node_tree_info* info_out) {
    if (!ctx) return WTP_ERR_ARG;
    if (ctx->mesh.nt < 1) return fail(ctx, WTP_ERR_STATE, "no mesh: call wtp_mesh_set first");
    if (!sp) return fail(ctx, WTP_ERR_ARG, "NULL spacing");
    if (sp->kind == WTP_SPACING_PER_POINT)
        return fail(ctx, WTP_ERR_ARG, "wtp_node_tree_build needs a spacing law it can evaluate at box centres: CONSTANT, LOGLIKE or BOUNDARY_LAYER");
    if (sp->kind != WTP_SPACING_CONSTANT && !spacing_on_device(sp->kind)) return fail(ctx, WTP_ERR_ARG, "unknown spacing kind");
    if (!std::isfinite(alpha) || !(alpha > 0)) return fail(ctx, WTP_ERR_ARG, "alpha must be positive");
    if (!(node_min_ratio > 0) || !(node_min_ratio <= 1)) return fail(ctx, WTP_ERR_ARG, "node_min_ratio must be in (0, 1]");
    if (sp->kind == WTP_SPACING_CONSTANT && !std::isfinite(sp->constant))
        return fail(ctx, WTP_ERR_ARG, "the spacing at a box centre of the node tree is not finite");
    int rc;
    if (spacing_on_device(sp->kind) && (rc = check_spacing_law(ctx, sp))) return rc;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    node_tree_invalidate(ctx);
    return by_dtype(ctx->mesh.dtype, [&](auto t) { return node_tree_build_t<decltype(t)>(ctx, sp, alpha, node_min_ratio, info_out); });
}

WTP_API int wtp_node_tree_get(wtp_ctx* ctx, int32_t* cell_out, int32_t* depth_out, int8_t* class_out, void* h_out) {
    int rc = need_tree(ctx, __func__);
    if (rc) return rc;
    NodeTreeState& S = ctx->ntree;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)S.n;
    std::vector<uint64_t> keys(cell_out || depth_out ? n : 0);
    if (!keys.empty())
        WTP_HIP(ctx, hipMemcpyAsync(keys.data(), S.keys[S.cur].p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (class_out) WTP_HIP(ctx, hipMemcpyAsync(class_out, S.cls.p, n, hipMemcpyDeviceToHost, ctx->stream));
    if (h_out) WTP_HIP(ctx, hipMemcpyAsync(h_out, S.hout.p, tsize(S.dtype) * n, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    for (size_t i = 0; i < keys.size(); ++i) { // depth and cell are the key's own bits
        int d;
        int32_t c[3];
        nt_decode(keys[i], &d, c);
        if (depth_out) depth_out[i] = d;
        if (cell_out) cell_out[3 * i] = c[0], cell_out[3 * i + 1] = c[1], cell_out[3 * i + 2] = c[2];
    }
    return WTP_OK;
}

WTP_API int wtp_node_tree_locate(wtp_ctx* ctx, const void* xyz, int64_t n, int dtype, int64_t* leaf_out) {
    int rc = need_tree(ctx, __func__);
    if (rc) return rc;
    if (dtype != WTP_F32 && dtype != WTP_F64) return fail(ctx, WTP_ERR_ARG, "dtype must be WTP_F32 or WTP_F64");
    if (n < 0 || n > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "bad n");
    if (n == 0) return WTP_OK;
    if (!xyz || !leaf_out) return fail(ctx, WTP_ERR_ARG, "NULL array");
    NodeTreeState& S = ctx->ntree;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_bytes = (tsize(dtype) * 3 * (size_t)n + 255) / 256 * 256;
    if ((rc = ensure(ctx, S.io, in_bytes + sizeof(int64_t) * (size_t)n))) return rc;
    char* b = (char*)S.io.p;
    WTP_HIP(ctx, hipMemcpyAsync(b, xyz, tsize(dtype) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    rc = by_dtype(dtype, [&](auto tp) {
        using TP = decltype(tp);
        return by_dtype(S.dtype, [&](auto tm) {
            using TM = decltype(tm);
            hipLaunchKernelGGL((nt_locate_kernel<TM, TP>), dim3(nt_grid(n)), dim3(kNtThreads), 0, ctx->stream,
                               (const uint64_t*)S.keys[S.cur].p, S.n, nt_root_held<TM>(S), (const TP*)b, n, (int64_t*)(b + in_bytes));
            WTP_HIP(ctx, hipGetLastError());
            return (int)WTP_OK;
        });
    });
    if (rc) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(leaf_out, b + in_bytes, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_node_tree_clear(wtp_ctx* ctx) { // and the placement with it
    if (!ctx) return WTP_ERR_ARG;
    node_tree_invalidate(ctx);
    return WTP_OK;
}

WTP_API int wtp_node_place(wtp_ctx* ctx, int placement, int64_t max_points, double boundary_oversampling, uint64_t seed,
                           wtp_node_place_info* info_out) {
    int rc = need_tree(ctx, __func__);
    if (rc) return rc;
    if (placement < 0 || placement > 2) return fail(ctx, WTP_ERR_ARG, "placement must be 0 (random), 1 (jittered) or 2 (lattice)");
    if (max_points < 1 || max_points > (int64_t(1) << 31)) return fail(ctx, WTP_ERR_ARG, "max_points must be in [1, 2^31]");
    if (!std::isfinite(boundary_oversampling) || !(boundary_oversampling > 0))
        return fail(ctx, WTP_ERR_ARG, "boundary_oversampling must be positive");
    if (seed >= (1ull << 24)) return fail(ctx, WTP_ERR_ARG, "seed must be below 2^24");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    ctx->ntree.placed = false;
    return by_dtype(ctx->ntree.dtype, [&](auto t) {
        return node_place_t<decltype(t)>(ctx, placement, max_points, boundary_oversampling, seed, info_out);
    });
}

static int node_place_read(wtp_ctx* ctx, void* xyz_out, int64_t* leaf_out, hipMemcpyKind kind, const char* entry) {
    int rc = need_tree(ctx, entry);
    if (rc) return rc;
    NodeTreeState& S = ctx->ntree;
    if (!S.placed) return fail(ctx, WTP_ERR_STATE, std::string(entry) + " before a successful wtp_node_place");
    const size_t m = (size_t)S.pinfo.n_points;
    if (m == 0) return WTP_OK;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if (xyz_out) WTP_HIP(ctx, hipMemcpyAsync(xyz_out, S.p_xyz.p, tsize(S.dtype) * 3 * m, kind, ctx->stream));
    if (leaf_out) WTP_HIP(ctx, hipMemcpyAsync(leaf_out, S.p_leaf.p, sizeof(int64_t) * m, kind, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_node_place_get(wtp_ctx* ctx, void* xyz_out, int64_t* leaf_out) {
    return node_place_read(ctx, xyz_out, leaf_out, hipMemcpyDeviceToHost, __func__);
}

WTP_API int wtp_node_place_get_dev(wtp_ctx* ctx, void* d_xyz_out, int64_t* d_leaf_out) {
    return node_place_read(ctx, d_xyz_out, d_leaf_out, hipMemcpyDeviceToDevice, __func__);
}
