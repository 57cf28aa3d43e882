// wtp_loops.hip — the 2-D geometry index: closed boundary loops (outer boundaries and holes) of a planar domain.
//
//   SegmentQuadtree(boundary) / SegmentIndex        src/octree/segment_quadtree.jl:115-238
//   _dedup_loop, _loop_signed_area, _point_in_loop  :93-139
//   _compute_bbox_raw_2d                            :240-251
//   closest_point_on_segment_feature, signed distance from the closest feature's (pseudo)normal
//
// The 2-D twin of wtp_mesh.hip.  The reference walks a quadtree of segment lists per query; here the loops are static
// between wtp_loops_set calls, so they get the mesh's left-balanced bounding-volume tree, restated for segments: heap
// order (children of node i are 2i+1, 2i+2), one segment per node (the median of its subtree along the wider axis of
// the midpoints) and the box of everything below it.  A node carries what a query needs of its segment — the two end
// points, the unit normal and the two vertex pseudonormals — so the sign costs no second fetch: 64 bytes (fp32) or
// 128 bytes (fp64) per node.
//
// The walk is the mesh's (mesh_nearest_guess): every lane walks alone, stackless (pre-order with arithmetic skips in
// the heap-ordered tree), from a first guess found by a greedy descent.  The fill's darts are uniform over the box, so
// the 64 queries of a wave share little of their paths and a packet walk would visit their union.
//
// Exactness: every lane keeps the minimum of (d2, segment index) over the segments it evaluated, d2 computed as
// include/wtp.h states it (no contraction).  A subtree is skipped only when its box is farther than the lane's best by
// more than the rounding slack of a computed closest point (64 eps x the coordinate scale), so the result is the
// brute-force minimum.  Every loop is bounded by the node count; nothing here uses floating-point atomics.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "wtp_device.hpp"

namespace wtp {

static constexpr int kLoopThreads = 256;

template <typename T> struct LoopNode {
    T a[2], b[2];     // the node's segment a -> b
    T lo[2], hi[2];   // box of the whole subtree (own segment included)
    T nf[2];          // unit normal of the segment (out of the domain)
    T na[2], nb[2];   // pseudonormals of its end points (sum of the two adjacent segments' normals)
    int32_t seg;      // segment index
    int32_t pad_[sizeof(T) == 4 ? 1 : 3];
};
static_assert(sizeof(LoopNode<float>) == 64, "one cache line per node");
static_assert(sizeof(LoopNode<double>) == 128, "two cache lines per node");

template <typename T> struct LoopEps;
template <> struct LoopEps<float> {
    static constexpr float eps = 1.1920928955078125e-07f;
    static constexpr float tiny = FLT_MIN;
};
template <> struct LoopEps<double> {
    static constexpr double eps = 2.220446049250313e-16;
    static constexpr double tiny = DBL_MIN;
};

// ---- host build: SegmentIndex, in T, term by term ------------------------------------------------------------------
template <typename T> struct V2 { T x, y; };

template <typename T> static T norm2(T dx, T dy) { return std::sqrt(dx * dx + dy * dy); }

template <typename T> static void loop_box(const std::vector<V2<T>>& v, T lo[2], T hi[2]) {
    lo[0] = hi[0] = v[0].x, lo[1] = hi[1] = v[0].y;
    for (const V2<T>& p : v) {
        lo[0] = std::min(lo[0], p.x), hi[0] = std::max(hi[0], p.x);
        lo[1] = std::min(lo[1], p.y), hi[1] = std::max(hi[1], p.y);
    }
}

// _point_in_loop (:129-139)
template <typename T> static bool point_in_loop(const V2<T>& p, const std::vector<V2<T>>& loop) {
    bool c = false;
    const size_t n = loop.size();
    for (size_t i = 0; i < n; ++i) {
        const V2<T>&a = loop[i], &b = loop[(i + 1) % n];
        if ((a.y > p.y) == (b.y > p.y)) continue;
        const T x = a.x + (p.y - a.y) / (b.y - a.y) * (b.x - a.x);
        if (x > p.x) c = !c;
    }
    return c;
}

static int64_t loop_left_size(int64_t n) { // nodes in the left subtree of a left-balanced tree of n
    if (n <= 1) return 0;
    int h = 0;
    while ((int64_t(1) << (h + 1)) <= n) ++h;
    const int64_t full = (int64_t(1) << h) - 1, last = n - full, half = int64_t(1) << (h - 1);
    return (full - 1) / 2 + (last < half ? last : half);
}

template <typename T> struct SegItem {
    T c[2];          // midpoint (ordering only)
    T lo[2], hi[2];  // extents
    int32_t seg;
};

template <typename T>
static void loop_tree_rec(std::vector<SegItem<T>>& it, int64_t lo, int64_t hi, int64_t node, const LoopNode<T>* segs,
                          LoopNode<T>* out) {
    while (hi > lo) {
        T mn[2], mx[2], cmn[2], cmx[2];
        for (int a = 0; a < 2; ++a) {
            mn[a] = it[lo].lo[a], mx[a] = it[lo].hi[a];
            cmn[a] = cmx[a] = it[lo].c[a];
        }
        for (int64_t i = lo + 1; i < hi; ++i)
            for (int a = 0; a < 2; ++a) {
                mn[a] = std::min(mn[a], it[i].lo[a]);
                mx[a] = std::max(mx[a], it[i].hi[a]);
                cmn[a] = std::min(cmn[a], it[i].c[a]);
                cmx[a] = std::max(cmx[a], it[i].c[a]);
            }
        const int sd = cmx[1] - cmn[1] > cmx[0] - cmn[0] ? 1 : 0;
        const int64_t L = loop_left_size(hi - lo);
        std::nth_element(it.begin() + lo, it.begin() + lo + L, it.begin() + hi, [sd](const SegItem<T>& a, const SegItem<T>& b) {
            return a.c[sd] < b.c[sd] || (a.c[sd] == b.c[sd] && a.seg < b.seg);
        });
        LoopNode<T> nd = segs[it[lo + L].seg];
        for (int a = 0; a < 2; ++a) nd.lo[a] = mn[a], nd.hi[a] = mx[a];
        out[node] = nd;
        loop_tree_rec<T>(it, lo, lo + L, 2 * node + 1, segs, out);
        lo = lo + L + 1;
        node = 2 * node + 2;
    }
}

// The cleaned, oriented loops as one node per segment (segment order; boxes not yet set), the box and the error text.
template <typename T>
static int loops_build_host(const T* xy, const int64_t* start, int64_t n_loops, std::vector<LoopNode<T>>& segs, double bbox[4],
                            std::string& why) {
    const T eps = LoopEps<T>::eps;
    std::vector<std::vector<V2<T>>> cleaned((size_t)n_loops);
    for (int64_t l = 0; l < n_loops; ++l) {
        const int64_t k = start[l + 1] - start[l];
        if (k < 3) {
            why = "boundary loop " + std::to_string(l) + " has " + std::to_string(k) + " vertices; a closed loop needs at least 3";
            return WTP_ERR_ARG;
        }
        std::vector<V2<T>> raw((size_t)k);
        for (int64_t i = 0; i < k; ++i) raw[i] = V2<T>{xy[2 * (start[l] + i)], xy[2 * (start[l] + i) + 1]};
        T lo[2], hi[2];
        loop_box<T>(raw, lo, hi);
        const T diag = norm2<T>(hi[0] - lo[0], hi[1] - lo[1]);
        const T tol = std::max((T)8 * eps * diag, LoopEps<T>::tiny);
        std::vector<V2<T>>& out = cleaned[l];
        for (const V2<T>& v : raw)
            if (out.empty() || norm2<T>(v.x - out.back().x, v.y - out.back().y) > tol) out.push_back(v);
        while (out.size() > 1 && norm2<T>(out.back().x - out[0].x, out.back().y - out[0].y) <= tol) out.pop_back();
        if (out.size() < 3) {
            why = "boundary loop " + std::to_string(l) + " has " + std::to_string(out.size()) +
                  " distinct vertices after dropping duplicates; a closed loop needs at least 3";
            return WTP_ERR_ARG;
        }
    }
    segs.clear();
    for (int64_t l = 0; l < n_loops; ++l) {
        std::vector<V2<T>> loop = cleaned[l];
        const size_t n = loop.size();
        T sa = 0;
        const V2<T> o = loop[0];
        for (size_t i = 0; i < n; ++i) {
            const V2<T>&p = loop[i], &q = loop[(i + 1) % n];
            const T ax = p.x - o.x, ay = p.y - o.y, bx = q.x - o.x, by = q.y - o.y;
            sa = sa + (ax * by - bx * ay);
        }
        sa = sa / (T)2;
        T lo[2], hi[2];
        loop_box<T>(loop, lo, hi);
        const T ex = hi[0] - lo[0], ey = hi[1] - lo[1];
        const T bbox_area = ex * ey;
        const T noise = ((T)(int64_t)n * eps) * (ex * ex + ey * ey);
        if (std::fabs(sa) < std::max((T)1.0e-10 * bbox_area, (T)4 * noise)) {
            why = "boundary loop " + std::to_string(l) +
                  " has (near-)zero signed area: its vertices are collinear or not ordered sequentially around the loop";
            return WTP_ERR_ARG;
        }
        int64_t depth = 0;
        for (int64_t j = 0; j < n_loops; ++j)
            if (j != l && point_in_loop<T>(loop[0], cleaned[j])) ++depth;
        const bool want_ccw = depth % 2 == 0;
        if ((sa > 0) != want_ccw) std::reverse(loop.begin(), loop.end());
        const size_t base = segs.size();
        segs.resize(base + n);
        for (size_t i = 0; i < n; ++i) {
            LoopNode<T>& s = segs[base + i];
            memset(&s, 0, sizeof(s));
            const V2<T>&p = loop[i], &q = loop[(i + 1) % n];
            s.a[0] = p.x, s.a[1] = p.y, s.b[0] = q.x, s.b[1] = q.y;
            const T dx = q.x - p.x, dy = q.y - p.y;
            const T mag = std::sqrt(dx * dx + dy * dy);
            s.nf[0] = dy / mag, s.nf[1] = -dx / mag;
            s.seg = (int32_t)(base + i);
        }
        for (size_t i = 0; i < n; ++i) { // vertex i ends segment i - 1 and starts segment i: the sum of their normals
            LoopNode<T>&prev = segs[base + (i + n - 1) % n], &s = segs[base + i];
            for (int a = 0; a < 2; ++a) prev.nb[a] = s.na[a] = prev.nf[a] + s.nf[a];
        }
    }
    // _compute_bbox_raw_2d (:240-251): over all vertices, flat axes widened
    T mn[2] = {segs[0].a[0], segs[0].a[1]}, mx[2] = {segs[0].a[0], segs[0].a[1]};
    for (const LoopNode<T>& s : segs)
        for (int a = 0; a < 2; ++a) mn[a] = std::min(mn[a], s.a[a]), mx[a] = std::max(mx[a], s.a[a]);
    const T e = std::max(eps * 100, (T)1.0e-10);
    for (int a = 0; a < 2; ++a) {
        if (mn[a] == mx[a]) mn[a] -= e, mx[a] += e;
        bbox[a] = (double)mn[a], bbox[2 + a] = (double)mx[a];
    }
    return WTP_OK;
}

// ---- device ------------------------------------------------------------------------------------------------------------
// closest point of segment a -> b to p and its feature: 0 interior, 1 vertex a, 2 vertex b (include/wtp.h)
template <typename T> __device__ inline int seg_closest(const T* p, const T* a, const T* b, T* cp) {
    const T abx = b[0] - a[0], aby = b[1] - a[1];
    const T den = abx * abx + aby * aby;
    const T t = ((p[0] - a[0]) * abx + (p[1] - a[1]) * aby) / den;
    if (t <= (T)0) {
        cp[0] = a[0], cp[1] = a[1];
        return 1;
    }
    if (t >= (T)1) {
        cp[0] = b[0], cp[1] = b[1];
        return 2;
    }
    cp[0] = a[0] + t * abx, cp[1] = a[1] + t * aby;
    return 0;
}

template <typename T> struct SegNearest {
    T d2;
    T cp[2];
    T nrm[2]; // the closest feature's normal
    int32_t seg;
};

template <typename T> __device__ inline T box2_d2(const T* lo, const T* hi, const T* q) {
    T t[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const T below = lo[a] - q[a], above = q[a] - hi[a];
        const T mm = below > above ? below : above;
        t[a] = mm > (T)0 ? mm : (T)0;
    }
    return t[0] * t[0] + t[1] * t[1];
}

// (sqrt(best) + 2 delta)^2: a box farther than this cannot hold a segment whose COMPUTED d2 ties or beats best
template <typename T> __device__ inline T loop_prune_limit(T best, T delta) {
    return best + ((T)4 * delta) * (wsqrt(best) + delta);
}

// next node in pre-order after skipping the subtree of i (1-based heap index, m nodes); 1 = walk finished.  At most
// 32 steps: i loses a bit each time
__device__ inline uint32_t loop_heap_escape(uint32_t i, uint32_t m) {
    for (int it = 0; it < 32; ++it) {
        const uint32_t j = i + 1;
        i = j >> __builtin_ctz(j);
        if (i <= m) break;
    }
    return i;
}

// the node's own segment against the lane's best
template <typename T> __device__ inline bool seg_offer(const LoopNode<T>& nd, const T* q, SegNearest<T>& r) {
    T cp[2];
    const T a[2] = {nd.a[0], nd.a[1]}, b[2] = {nd.b[0], nd.b[1]};
    const int f = seg_closest<T>(q, a, b, cp);
    const T dx = q[0] - cp[0], dy = q[1] - cp[1];
    const T d2 = dx * dx + dy * dy;
    if (!(d2 < r.d2 || (d2 == r.d2 && nd.seg < r.seg))) return false; // (a NaN never wins)
    r.d2 = d2, r.seg = nd.seg;
    r.cp[0] = cp[0], r.cp[1] = cp[1];
    const T* nrm = f == 0 ? nd.nf : (f == 1 ? nd.na : nd.nb);
    r.nrm[0] = nrm[0], r.nrm[1] = nrm[1];
    return true;
}

// The brute-force minimum of (d2, segment index) for one lane.  First guess: down from the root into the child whose
// box is nearer (ties: left), at most 32 levels; then the pre-order walk, every node at most once.
template <typename T>
__device__ inline SegNearest<T> loops_nearest(const LoopNode<T>* __restrict__ nodes, int32_t m, const T* q, T scale) {
    SegNearest<T> r;
    r.d2 = Lim<T>::inf();
    r.cp[0] = q[0], r.cp[1] = q[1];
    r.nrm[0] = r.nrm[1] = (T)0;
    r.seg = INT32_MAX;
    const T ax = q[0] < 0 ? -q[0] : q[0], ay = q[1] < 0 ? -q[1] : q[1];
    T aq = ax > ay ? ax : ay;
    aq = aq > scale ? aq : scale;
    const T delta = (T)64 * LoopEps<T>::eps * aq;
    uint32_t g = 1;
    for (int lvl = 0; lvl < 32; ++lvl) {
        const uint32_t l = 2 * g, rr = 2 * g + 1;
        if (l > (uint32_t)m) break;
        if (rr > (uint32_t)m) {
            g = l;
            break;
        }
        const T dl = box2_d2<T>(nodes[l - 1].lo, nodes[l - 1].hi, q), dr = box2_d2<T>(nodes[rr - 1].lo, nodes[rr - 1].hi, q);
        g = dr < dl ? rr : l;
    }
    seg_offer<T>(nodes[g - 1], q, r);
    T limit = loop_prune_limit<T>(r.d2, delta);
    uint32_t i = 1;
    for (int32_t step = 0; step < m; ++step) {
        const LoopNode<T>& nd = nodes[i - 1];
        if (box2_d2<T>(nd.lo, nd.hi, q) <= limit) {
            if (i != g && seg_offer<T>(nd, q, r)) limit = loop_prune_limit<T>(r.d2, delta);
            i = 2 * i <= (uint32_t)m ? 2 * i : loop_heap_escape(i, (uint32_t)m);
        } else {
            i = loop_heap_escape(i, (uint32_t)m);
        }
        if (i == 1) break;
    }
    return r;
}

template <typename T> struct LoopsView {
    const LoopNode<T>* nodes;
    int32_t m;
    T lo[2], hi[2]; // the index's box
    T scale;        // largest |coordinate| of the box
};

template <typename T> __device__ inline bool in_box2(const LoopsView<T>& v, const T* q) {
    return !((q[0] < v.lo[0]) || (q[0] > v.hi[0]) || (q[1] < v.lo[1]) || (q[1] > v.hi[1]));
}

// n x 2 points -> any of {signed distance, segment, closest point, inside flag}
template <typename TM, typename TP>
__global__ void __launch_bounds__(kLoopThreads)
loops_query_kernel(const TP* __restrict__ xy, int64_t n, LoopsView<TM> v, TP* __restrict__ sd_out, int32_t* __restrict__ seg_out,
                   TP* __restrict__ cp_out, uint8_t* __restrict__ inside_out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const TM q[2] = {(TM)xy[2 * i], (TM)xy[2 * i + 1]}; // seam: convert once at entry
        const SegNearest<TM> r = loops_nearest<TM>(v.nodes, v.m, q, v.scale);
        const TM s = (q[0] - r.cp[0]) * r.nrm[0] + (q[1] - r.cp[1]) * r.nrm[1];
        const TM dist = wsqrt(r.d2);
        const TM sd = s > (TM)0 ? dist : (s < (TM)0 ? -dist : (TM)0);
        if (sd_out) sd_out[i] = (TP)sd;
        if (seg_out) seg_out[i] = r.seg;
        if (cp_out) cp_out[2 * i] = (TP)r.cp[0], cp_out[2 * i + 1] = (TP)r.cp[1];
        if (inside_out) inside_out[i] = (in_box2<TM>(v, q) && sd < (TM)0) ? 1 : 0;
    }
}

// loops_query_kernel's inside flag alone, for rows of 3 columns of the index's own type (the darts of wtp_loops_fill; z
// is ignored).  A point outside the box is outside without a search.
template <typename T>
__global__ void __launch_bounds__(kLoopThreads)
loops_inside_kernel(const T* __restrict__ xyz, int64_t n, LoopsView<T> v, uint8_t* __restrict__ inside_out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const T q[2] = {xyz[3 * i], xyz[3 * i + 1]};
        uint8_t in = 0;
        if (in_box2<T>(v, q)) {
            const SegNearest<T> r = loops_nearest<T>(v.nodes, v.m, q, v.scale);
            const T s = (q[0] - r.cp[0]) * r.nrm[0] + (q[1] - r.cp[1]) * r.nrm[1];
            in = (s < (T)0 && r.d2 > (T)0) ? 1 : 0; // sd = -sqrt(d2) < 0
        }
        inside_out[i] = in;
    }
}

static int loops_grid(int64_t n) { return grid_for(n, kLoopThreads, 16384); }

template <typename T> static LoopsView<T> loops_view(const wtp_ctx* ctx) {
    LoopsView<T> v;
    v.nodes = (const LoopNode<T>*)ctx->loops.nodes.p;
    v.m = (int32_t)ctx->loops.ns;
    for (int a = 0; a < 2; ++a) v.lo[a] = (T)ctx->loops.bbox[a], v.hi[a] = (T)ctx->loops.bbox[2 + a];
    v.scale = (T)ctx->loops.scale;
    return v;
}

template <typename T> int launch_loops_inside(wtp_ctx* ctx, const T* d_xyz, int64_t n, uint8_t* d_inside) {
    hipLaunchKernelGGL((loops_inside_kernel<T>), dim3(loops_grid(n)), dim3(kLoopThreads), 0, ctx->stream, d_xyz, n,
                       loops_view<T>(ctx), d_inside);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}
template int launch_loops_inside<float>(wtp_ctx*, const float*, int64_t, uint8_t*);
template int launch_loops_inside<double>(wtp_ctx*, const double*, int64_t, uint8_t*);

template <typename T> static int loops_set_t(wtp_ctx* ctx, const T* xy, const int64_t* start, int64_t n_loops) {
    std::vector<LoopNode<T>> segs;
    std::string why;
    int rc = loops_build_host<T>(xy, start, n_loops, segs, ctx->loops.bbox, why);
    if (rc) return fail(ctx, rc, why);
    const int64_t ns = (int64_t)segs.size();
    if (ns >= (int64_t(1) << 30)) return fail(ctx, WTP_ERR_ARG, "more than 2^30 segments");
    std::vector<SegItem<T>> it((size_t)ns);
    for (int64_t s = 0; s < ns; ++s) {
        SegItem<T>& x = it[s];
        x.seg = (int32_t)s;
        for (int a = 0; a < 2; ++a) {
            x.lo[a] = std::min(segs[s].a[a], segs[s].b[a]);
            x.hi[a] = std::max(segs[s].a[a], segs[s].b[a]);
            x.c[a] = (segs[s].a[a] + segs[s].b[a]) / (T)2;
        }
    }
    std::vector<LoopNode<T>> nodes((size_t)ns);
    loop_tree_rec<T>(it, 0, ns, 0, segs.data(), nodes.data());
    double sc = 0;
    for (int a = 0; a < 4; ++a) sc = std::max(sc, std::fabs(ctx->loops.bbox[a]));
    ctx->loops.scale = sc;
    if ((rc = ensure(ctx, ctx->loops.nodes, sizeof(LoopNode<T>) * (size_t)ns))) return rc;
    WTP_HIP(ctx, hipMemcpyAsync(ctx->loops.nodes.p, nodes.data(), sizeof(LoopNode<T>) * (size_t)ns, hipMemcpyHostToDevice,
                                ctx->stream));
    if ((rc = sync(ctx))) return rc; // the host vectors go out of scope
    ctx->loops.ns = ns;
    return WTP_OK;
}

static size_t al256(size_t b) { return (b + 255) / 256 * 256; }

} // namespace wtp

using namespace wtp;
#define WTP_API extern "C"

WTP_API int wtp_loops_set(wtp_ctx* ctx, const void* xy, int64_t nv, const int64_t* loop_start, int64_t n_loops, int dtype) {
    if (!ctx) return WTP_ERR_ARG;
    if (dtype != WTP_F32 && dtype != WTP_F64) return fail(ctx, WTP_ERR_ARG, "dtype must be WTP_F32 or WTP_F64");
    if (!xy || !loop_start) return fail(ctx, WTP_ERR_ARG, "NULL array");
    if (n_loops < 1) return fail(ctx, WTP_ERR_ARG, "at least one boundary loop is needed");
    if (nv < 0 || nv >= (int64_t(1) << 30)) return fail(ctx, WTP_ERR_ARG, "bad vertex count");
    if (loop_start[0] != 0 || loop_start[n_loops] != nv)
        return fail(ctx, WTP_ERR_ARG, "loop_start must run from 0 to the vertex count");
    for (int64_t l = 0; l < n_loops; ++l)
        if (loop_start[l + 1] < loop_start[l]) return fail(ctx, WTP_ERR_ARG, "loop_start must increase");
    for (int64_t i = 0; i < 2 * nv; ++i)
        if (!std::isfinite(dtype == WTP_F32 ? (double)((const float*)xy)[i] : ((const double*)xy)[i]))
            return fail(ctx, WTP_ERR_ARG, "vertex " + std::to_string(i / 2) + " has a coordinate that is not finite");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    ctx->loops.ns = 0;
    sample_invalidate(ctx);
    const int rc = dtype == WTP_F32 ? loops_set_t<float>(ctx, (const float*)xy, loop_start, n_loops)
                                    : loops_set_t<double>(ctx, (const double*)xy, loop_start, n_loops);
    if (rc) {
        ctx->loops.ns = 0;
        return rc;
    }
    ctx->loops.dtype = dtype;
    return WTP_OK;
}

WTP_API int wtp_loops_clear(wtp_ctx* ctx) {
    if (!ctx) return WTP_ERR_ARG;
    ctx->loops.ns = 0;
    sample_invalidate(ctx);
    return WTP_OK;
}

WTP_API int wtp_loops_bounds(wtp_ctx* ctx, double bbox_out[4], int64_t* n_segments_out) {
    if (!ctx) return WTP_ERR_ARG;
    if (ctx->loops.ns < 1) return fail(ctx, WTP_ERR_STATE, "no loops: call wtp_loops_set first");
    if (bbox_out) memcpy(bbox_out, ctx->loops.bbox, sizeof(double) * 4);
    if (n_segments_out) *n_segments_out = ctx->loops.ns;
    return WTP_OK;
}

WTP_API int wtp_loops_query(wtp_ctx* ctx, const void* xy, int64_t n, int dtype, void* sd_out, int32_t* seg_out,
                            void* closest_out, uint8_t* inside_out) {
    if (!ctx) return WTP_ERR_ARG;
    if (dtype != WTP_F32 && dtype != WTP_F64) return fail(ctx, WTP_ERR_ARG, "dtype must be WTP_F32 or WTP_F64");
    if (ctx->loops.ns < 1) return fail(ctx, WTP_ERR_STATE, "no loops: call wtp_loops_set first");
    if (n < 0 || n > 2000000000LL) return fail(ctx, WTP_ERR_ARG, "bad n");
    if (n == 0) return WTP_OK;
    if (!xy) return fail(ctx, WTP_ERR_ARG, "NULL array");
    for (int64_t i = 0; i < 2 * n; ++i)
        if (!std::isfinite(dtype == WTP_F32 ? (double)((const float*)xy)[i] : ((const double*)xy)[i]))
            return fail(ctx, WTP_ERR_ARG, "query point " + std::to_string(i / 2) + " has a coordinate that is not finite");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ts = dtype == WTP_F64 ? 8 : 4;
    // loops.io: [xy n*2 | sd n | cp n*2 | seg n (int32) | inside n (u8)]
    const size_t o_sd = al256(ts * n * 2), o_cp = o_sd + al256(ts * n), o_sg = o_cp + al256(ts * n * 2),
                 o_in = o_sg + al256(4 * (size_t)n);
    int rc;
    if ((rc = ensure(ctx, ctx->loops.io, o_in + (size_t)n))) return rc;
    char* b = (char*)ctx->loops.io.p;
    WTP_HIP(ctx, hipMemcpyAsync(b, xy, ts * n * 2, hipMemcpyHostToDevice, ctx->stream));
    int32_t* seg = seg_out ? (int32_t*)(b + o_sg) : nullptr;
    uint8_t* inside = inside_out ? (uint8_t*)(b + o_in) : nullptr;
    const int sp = span_begin(ctx, 2);
    by_dtype(dtype, [&](auto tp) { // the points' dtype, then the index's
        using TP = decltype(tp);
        TP *sd = sd_out ? (TP*)(b + o_sd) : nullptr, *cp = closest_out ? (TP*)(b + o_cp) : nullptr;
        by_dtype(ctx->loops.dtype, [&](auto tm) {
            using TM = decltype(tm);
            hipLaunchKernelGGL((loops_query_kernel<TM, TP>), dim3(loops_grid(n)), dim3(kLoopThreads), 0, ctx->stream,
                               (const TP*)b, n, loops_view<TM>(ctx), sd, seg, cp, inside);
            return 0;
        });
        return 0;
    });
    span_end(ctx, sp);
    WTP_HIP(ctx, hipGetLastError());
    if (sd_out) WTP_HIP(ctx, hipMemcpyAsync(sd_out, b + o_sd, ts * n, hipMemcpyDeviceToHost, ctx->stream));
    if (closest_out) WTP_HIP(ctx, hipMemcpyAsync(closest_out, b + o_cp, ts * n * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (seg_out) WTP_HIP(ctx, hipMemcpyAsync(seg_out, b + o_sg, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (inside_out) WTP_HIP(ctx, hipMemcpyAsync(inside_out, b + o_in, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}
