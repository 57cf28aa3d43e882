// wtp_sample.hip — graded Poisson-disk sampling of the mesh surface.
//
//   sample_surface(mesh, spacing; factor, max_points, stall_limit)     src/surface_sampling.jl:34-104
//   PointBoundary(mesh, spacing)                                       :113-118
//
// The reference throws one dart at a time: area-weighted triangle, uniform point in it, accepted iff it keeps
// min(r_i, r_j) from every accepted sample, r = factor h(x).  include/wtp.h pins the darts to a counter-based stream, so
// the serial loop over that stream is the definition of the result; this file computes it in batches of B consecutive
// darts.  Dart throwing in a fixed order is the greedy maximal independent set under fixed priorities, and that set is
// reached by rounds of "decide every dart whose lower-numbered conflicting darts are all decided":
//   1. generate      one thread per dart: triangle by binary search of the area sums (double), position and r in T
//                    (wtp_sample_streams.hip, as are the darts and candidates of the other two streams below);
//   2. cull          a dart in conflict with an accepted sample is dead; the live ones enter the batch's cell table;
//   3. rounds        an undecided dart is rejected if a lower-numbered conflicting dart was accepted in an EARLIER round,
//                    accepted if all of them were rejected earlier (Jacobi: a word per dart holds the round of its
//                    decision, so the round count is as unique as the result); the lowest undecided dart is decided
//                    every round, so B rounds bound a batch; in practice about ten do;
//   4. stop + append a scan over the accept flags in dart order carries the miss run and the sample count in, finds the
//                    first dart at which the run ends, and appends the accepted darts before it by prefix sum.
// Rounds are launched in groups of kGroup; a per-round device counter of undecided darts turns the rest of a group into
// no-ops, and the scan, the append and the insertion into the accepted table follow in the same group, guarded by the
// same counter: the host reads one control block per group.  No kernel waits for another thread's store; every loop is
// bounded by a count known at launch.
//
// Cells.  Both the accepted samples and a batch's live darts are kept in an open-addressing table of 64-bit cell keys
// (three 20-bit cell coordinates over the mesh's bounding box), each slot heading a chain of the points in that cell: a
// dense array over the box would hold O((L / r)^3) cells of which the surface fills O((L / r)^2).  A sample in conflict
// with dart p lies within r_p of it, so p scans the cells its ball touches; the cell map is monotone and the ball is
// widened by the rounding of its own bounds, so nothing rests on one point per cell or on an r_min known in advance.  A
// ball that touches more cells than there are points scans the points instead.  The chain order depends on arrival;
// nothing read from a chain does (a conflict exists or not).  The cell edge is sqrt(r_min r_max) of the first batch.
//
// The volume fill (wtp_mesh_fill) is the same run over another stream: darts uniform in the mesh's
// bounding box, of which only those inside the mesh (wtp_mesh_query's flag, wtp_mesh.hip) may be taken, and seed points
// that occupy space from the start.  The seeds sit at the front of the accepted array and in its table; the counts the
// stop rule carries are of accepted darts alone.  Everything from the cull to the insertion is the sampler's.
//
// The advancing front (wtp_mesh_front) is the run once more, over candidates that depend on what was
// accepted: the accepted array, seeds first, is the queue, and candidate j = q n + s is thrown from queue entry q at its
// spacing h_q.  A batch is the n candidates each of a range of parents that were all in the queue when it began, so its
// candidates are known at launch and ordered as the serial loop takes them.  The conflict rule is one-sided (r_j alone)
// and exempts the parent; the cull and the rounds are instantiated for it (kFront), the stop scan runs with a stall limit
// it cannot reach, and the appended rows get their own h before the next batch can read them as parents.
//
// This file is the core: the cell table, cull, rounds, stop scan, append and insert, decide_batch over them, and the
// driver.  A run is run_begin, then per batch batch_prepare, the stream's points (wtp_sample_streams.hip) and
// decide_batch, then run_finish; sample_run and front_run hold what differs between the streams: how a batch is sized,
// the rows it needs room for, who wants the class grid, the front's own-h pass and its stop reasons.
#include <climits>
#include <cmath>

#include "wtp_device.hpp"

namespace wtp {

static constexpr int kGroup = kSampleGroup;            // rounds per host read-back
static constexpr int kScanItems = 8;                   // darts per thread of the stop scan
static constexpr int kTile = kSmThreads * kScanItems;  // darts per block of the stop scan
static constexpr int64_t kBatchFirst = 4096, kBatchMax = 1 << 20; // batch = 0: doubled from / up to
static constexpr unsigned long long kEmpty = ~0ull;

// dart states: 0 undecided, else ((round of the decision + 1) << 1) | accepted; culled darts count as round 0
static constexpr int32_t kCulled = 2;

template <typename T> struct CellMap {
    T org[3];
    T inv_c;
    int32_t nc[3];
};

template <typename T> struct SmEps;
template <> struct SmEps<float> { static constexpr float v = 1.1920928955078125e-07f; };
template <> struct SmEps<double> { static constexpr double v = 2.220446049250313e-16; };

struct Table {
    unsigned long long* keys;
    int32_t* heads;
    uint32_t mask;
    int32_t shift;
};

template <typename T> __device__ inline int cell_of(const CellMap<T>& m, T v, int a) {
    const T s = (v - m.org[a]) * m.inv_c; // monotone in v; anything outside the box piles into the edge cells
    if (!(s > (T)0)) return 0;
    if (s >= (T)(m.nc[a] - 1)) return m.nc[a] - 1;
    return (int)s;
}

__device__ inline unsigned long long cell_key(int cx, int cy, int cz) {
    return ((unsigned long long)cz << 40) | ((unsigned long long)cy << 20) | (unsigned long long)cx;
}

template <typename T> __device__ inline unsigned long long key_of(const CellMap<T>& m, const Pt<T>& p) {
    return cell_key(cell_of(m, p.x, 0), cell_of(m, p.y, 1), cell_of(m, p.z, 2));
}

__device__ inline uint32_t slot_of(const Table& t, unsigned long long key) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> t.shift) & t.mask;
}

// the table holds at most half as many keys as slots, so a probe ends within mask + 1 steps
__device__ inline void table_insert(const Table& t, int32_t* next, unsigned long long key, int32_t i) {
    uint32_t s = slot_of(t, key);
    for (uint32_t it = 0; it <= t.mask; ++it) {
        const unsigned long long prev = atomicCAS(&t.keys[s], kEmpty, key);
        if (prev == kEmpty || prev == key) {
            next[i] = atomicExch(&t.heads[s], i);
            return;
        }
        s = (s + 1) & t.mask;
    }
}

__device__ inline int32_t table_find(const Table& t, unsigned long long key) {
    uint32_t s = slot_of(t, key);
    for (uint32_t it = 0; it <= t.mask; ++it) {
        const unsigned long long k = t.keys[s];
        if (k == key) return t.heads[s];
        if (k == kEmpty) return -1;
        s = (s + 1) & t.mask;
    }
    return -1;
}

template <typename T> __device__ inline bool conflict(const Pt<T>& p, const Pt<T>& q) {
    const T dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    const T m = p.w < q.w ? p.w : q.w;
    return ((dx * dx + dy * dy) + dz * dz) < m * m;
}

// the front's rule: p's radius alone; q's own spacing plays no part
template <typename T> __device__ inline bool conflict_one_sided(const Pt<T>& p, const Pt<T>& q) {
    const T dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return ((dx * dx + dy * dy) + dz * dz) < p.w * p.w;
}

// Calls f(j, pts[j]) for every point j < count of the table that can be in conflict with p (and maybe others), until f
// returns true.  A conflict has |fl(p.x - q.x)| < r_p on every axis, so q lies in a cell between those of the ball's
// bounds, widened by the rounding of the bounds themselves.
template <typename T, typename F>
__device__ inline void for_near(const CellMap<T>& m, const Table& t, const int32_t* __restrict__ next,
                                const Pt<T>* __restrict__ pts, int64_t count, const Pt<T>& p, F f) {
    int lo[3], hi[3];
    const T c[3] = {p.x, p.y, p.z};
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        const T marg = (T)8 * SmEps<T>::v * ((c[a] < 0 ? -c[a] : c[a]) + p.w);
        lo[a] = cell_of(m, (c[a] - p.w) - marg, a);
        hi[a] = cell_of(m, (c[a] + p.w) + marg, a);
        cells *= (int64_t)(hi[a] - lo[a] + 1);
    }
    if (cells > count) { // fewer points than cells: look at the points
        for (int64_t j = 0; j < count; ++j)
            if (f((int32_t)j, pts[j])) return;
        return;
    }
    for (int cz = lo[2]; cz <= hi[2]; ++cz)
        for (int cy = lo[1]; cy <= hi[1]; ++cy)
            for (int cx = lo[0]; cx <= hi[0]; ++cx) {
                int32_t j = table_find(t, cell_key(cx, cy, cz));
                for (int64_t steps = 0; j >= 0 && steps < count; ++steps) { // a chain is no longer than the table's points
                    if (f(j, pts[j])) return;
                    j = next[j];
                }
            }
}

// smallest and largest good r of pts[0, n) into ctl (integer atomics on the bits of positive doubles)
template <typename T>
__global__ void sample_range_kernel(const Pt<T>* __restrict__ pts, int64_t n, SampleCtl* __restrict__ ctl) {
    __shared__ unsigned long long s_lo[kSmThreads], s_hi[kSmThreads];
    unsigned long long lo = kEmpty, hi = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const T r = pts[i].w;
        if (!good_value(r)) continue;
        const unsigned long long b = __builtin_bit_cast(unsigned long long, (double)r);
        lo = b < lo ? b : lo;
        hi = b > hi ? b : hi;
    }
    s_lo[threadIdx.x] = lo, s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int d = kSmThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            if (s_lo[threadIdx.x + d] < s_lo[threadIdx.x]) s_lo[threadIdx.x] = s_lo[threadIdx.x + d];
            if (s_hi[threadIdx.x + d] > s_hi[threadIdx.x]) s_hi[threadIdx.x] = s_hi[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s_lo[0] != kEmpty) atomicMin(&ctl->rmin, s_lo[0]);
        if (s_hi[0] != 0) atomicMax(&ctl->rmax, s_hi[0]);
    }
}

__global__ void sample_begin_kernel(SampleCtl* __restrict__ ctl) {
    ctl->end = INT_MAX;
    ctl->n_new = 0;
}

// ---- step 2: cull against the accepted samples; the live darts enter the batch's table ----------------------------------
// kFront: the one-sided rule, never against the candidate's own parent (par0 + i / per), in the cell path and in the
// linear scan alike
template <typename T, bool kFront>
__global__ void sample_cull_kernel(CellMap<T> m, const Pt<T>* __restrict__ b_pts, int32_t B, int32_t* __restrict__ st,
                                   Table acc, const int32_t* __restrict__ s_next, const Pt<T>* __restrict__ s_pts,
                                   int64_t n_acc, Table bt, int32_t* __restrict__ b_next,
                                   const uint8_t* __restrict__ inside, int64_t first, int32_t par0, int32_t per,
                                   SampleCtl* __restrict__ ctl) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const Pt<T> p = b_pts[i];
    bool dead = !good_value(p.w); // a bad spacing value: never sampled with (the stop scan decides whether it is an error)
    if (inside) { // the volume fill: a dart outside the mesh is a miss whatever its spacing value; one inside reports a bad one
        if (!inside[i]) dead = true;
        else if (dead) atomicMin(&ctl->bad, (unsigned long long)(first + i));
    }
    if constexpr (kFront) {
        const int32_t parent = par0 + i / per;
        if (!dead)
            for_near<T>(m, acc, s_next, s_pts, n_acc, p, [&](int32_t j, const Pt<T>& q) {
                return dead = (j != parent && conflict_one_sided<T>(p, q));
            });
    } else {
        if (!dead)
            for_near<T>(m, acc, s_next, s_pts, n_acc, p, [&](int32_t, const Pt<T>& q) { return dead = conflict<T>(p, q); });
    }
    st[i] = dead ? kCulled : 0;
    if (!dead) table_insert(bt, b_next, key_of(m, p), i);
}

// ---- step 3: one round.  g: position in the group; round: 1-based round of the batch -----------------------------------
template <typename T, bool kFront>
__global__ void sample_round_kernel(CellMap<T> m, const Pt<T>* __restrict__ b_pts, int32_t B, int32_t* __restrict__ st,
                                    Table bt, const int32_t* __restrict__ b_next, int g, int32_t round,
                                    SampleCtl* __restrict__ ctl) {
    if (g > 0 && ctl->und[g - 1] == 0) return; // nothing was left undecided: the rest of the group does nothing
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B || st[i] != 0) return;
    const Pt<T> p = b_pts[i];
    bool rejected = false, pending = false;
    // the points of the table are the live darts; of a linear scan (count = i) the lower-numbered darts, culled ones too
    for_near<T>(m, bt, b_next, b_pts, (int64_t)B, p, [&](int32_t j, const Pt<T>& q) {
        if (j >= i || !(kFront ? conflict_one_sided<T>(p, q) : conflict<T>(p, q))) return false;
        const int32_t s = __atomic_load_n(&st[j], __ATOMIC_RELAXED);
        if (s == 0 || (s >> 1) > round) pending = true; // undecided before this round
        else if (s & 1) rejected = true;
        return rejected;
    });
    if (rejected) __atomic_store_n(&st[i], (round + 1) << 1, __ATOMIC_RELAXED);
    else if (!pending) __atomic_store_n(&st[i], ((round + 1) << 1) | 1, __ATOMIC_RELAXED);
    else atomicAdd(&ctl->und[g], 1);
}

// ---- step 4: the stop rule as a scan in dart order ---------------------------------------------------------------------
__device__ inline bool is_accepted(const int32_t* __restrict__ st, int32_t B, int64_t i) { return i < B && (st[i] & 1); }

// per tile: accepted darts, index of the last one (-1: none)
__global__ void sample_scan_a_kernel(const int32_t* __restrict__ st, int32_t B, int2* __restrict__ blk,
                                     const SampleCtl* __restrict__ ctl) {
    if (ctl->und[kGroup - 1] != 0) return;
    __shared__ int32_t s_cnt[kSmThreads], s_last[kSmThreads];
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kScanItems;
    int32_t cnt = 0, last = -1;
    for (int e = 0; e < kScanItems; ++e)
        if (is_accepted(st, B, base + e)) ++cnt, last = (int32_t)(base + e);
    s_cnt[threadIdx.x] = cnt, s_last[threadIdx.x] = last;
    __syncthreads();
    for (int d = kSmThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + d];
            if (s_last[threadIdx.x + d] > s_last[threadIdx.x]) s_last[threadIdx.x] = s_last[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) blk[blockIdx.x] = make_int2(s_cnt[0], s_last[0]);
}

// Exclusive (sum, max) scan of s_cnt / s_last over the block's threads, in place; returns the block's totals.
__device__ inline int2 block_scan_excl(int32_t* s_cnt, int32_t* s_last, int32_t cnt, int32_t last) {
    const int t = threadIdx.x;
    s_cnt[t] = cnt, s_last[t] = last;
    __syncthreads();
    for (int d = 1; d < kSmThreads; d <<= 1) {
        const int32_t c = t >= d ? s_cnt[t - d] : 0, l = t >= d ? s_last[t - d] : -1;
        __syncthreads();
        s_cnt[t] += c;
        if (l > s_last[t]) s_last[t] = l;
        __syncthreads();
    }
    const int2 total = make_int2(s_cnt[kSmThreads - 1], s_last[kSmThreads - 1]);
    const int32_t ec = t > 0 ? s_cnt[t - 1] : 0, el = t > 0 ? s_last[t - 1] : -1;
    __syncthreads();
    s_cnt[t] = ec, s_last[t] = el;
    __syncthreads();
    return total;
}

// one block: what precedes each tile (accepted darts, index of the last one)
__global__ void sample_scan_b_kernel(const int2* __restrict__ blk, int32_t nblk, int2* __restrict__ blk_ex,
                                     const SampleCtl* __restrict__ ctl) {
    if (ctl->und[kGroup - 1] != 0) return;
    __shared__ int32_t s_cnt[kSmThreads], s_last[kSmThreads];
    int32_t carry_c = 0, carry_l = -1;
    for (int32_t base = 0; base < nblk; base += kSmThreads) {
        const int32_t b = base + threadIdx.x;
        const int2 v = b < nblk ? blk[b] : make_int2(0, -1);
        const int2 tot = block_scan_excl(s_cnt, s_last, v.x, v.y);
        if (b < nblk) blk_ex[b] = make_int2(carry_c + s_cnt[threadIdx.x], s_last[threadIdx.x] > carry_l ? s_last[threadIdx.x] : carry_l);
        carry_c += tot.x;
        carry_l = tot.y > carry_l ? tot.y : carry_l;
        __syncthreads();
    }
}

// per dart i of [0, B] (B: the position behind the batch): accepted darts before it, index of the last one; the first i
// at which the run ends goes to ctl->end
__global__ void sample_scan_c_kernel(const int32_t* __restrict__ st, int32_t B, const int2* __restrict__ blk_ex,
                                     int32_t* __restrict__ pos, int32_t* __restrict__ lastb, int64_t max_points,
                                     int64_t stall_limit, SampleCtl* __restrict__ ctl) {
    if (ctl->und[kGroup - 1] != 0) return;
    __shared__ int32_t s_cnt[kSmThreads], s_last[kSmThreads];
    __shared__ int32_t s_end;
    if (threadIdx.x == 0) s_end = INT_MAX;
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kScanItems;
    int32_t cnt = 0, last = -1;
    for (int e = 0; e < kScanItems; ++e)
        if (is_accepted(st, B, base + e)) ++cnt, last = (int32_t)(base + e);
    block_scan_excl(s_cnt, s_last, cnt, last);
    const int2 pre = blk_ex[blockIdx.x];
    int32_t c = pre.x + s_cnt[threadIdx.x];
    int32_t l = s_last[threadIdx.x] > pre.y ? s_last[threadIdx.x] : pre.y;
    const long long n0 = ctl->n, miss0 = ctl->miss;
    int32_t end = INT_MAX;
    for (int e = 0; e < kScanItems; ++e) {
        const int64_t i = base + e;
        if (i > B) break;
        pos[i] = c, lastb[i] = l;
        const long long miss = l >= 0 ? i - l - 1 : miss0 + i;
        if (end == INT_MAX && (n0 + c >= max_points || miss >= stall_limit)) end = (int32_t)i;
        if (is_accepted(st, B, i)) ++c, l = (int32_t)i;
    }
    if (end != INT_MAX) atomicMin(&s_end, end);
    __syncthreads();
    if (threadIdx.x == 0 && s_end != INT_MAX) atomicMin(&ctl->end, s_end);
}

template <typename T>
__global__ void sample_append_kernel(const Pt<T>* __restrict__ b_pts, const int32_t* __restrict__ b_tri,
                                     const int32_t* __restrict__ st, int32_t B, const int32_t* __restrict__ pos, int64_t first,
                                     int64_t off, Pt<T>* __restrict__ s_pts, int32_t* __restrict__ s_tri,
                                     int64_t* __restrict__ s_dart, const SampleCtl* __restrict__ ctl) {
    if (ctl->und[kGroup - 1] != 0) return;
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B || i >= ctl->end || !(st[i] & 1)) return;
    const int64_t j = off + ctl->n + pos[i]; // dart order, behind the fill's `off` seeds
    s_pts[j] = b_pts[i];
    if (b_tri) s_tri[j] = b_tri[i];
    s_dart[j] = first + i;
}

// wtp_mesh_fill: the darts before the batch's end that were inside the mesh (integer count, one atomic per block)
__global__ void fill_count_kernel(const uint8_t* __restrict__ inside, int32_t B, SampleCtl* __restrict__ ctl) {
    if (ctl->und[kGroup - 1] != 0) return;
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t e = ctl->end < B ? ctl->end : B;
    const int cnt = __syncthreads_count(i < e && inside[i < e ? i : 0] != 0);
    if (threadIdx.x == 0 && cnt > 0) atomicAdd(&ctl->n_inside, (unsigned long long)cnt);
}

__global__ void sample_finish_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ lastb, int32_t B,
                                     int64_t first, int64_t max_points, SampleCtl* __restrict__ ctl) {
    if (ctl->und[kGroup - 1] != 0) return;
    const bool ended = ctl->end != INT_MAX;
    const int32_t e = ended ? ctl->end : B;
    const int32_t l = lastb[e];
    ctl->n_new = pos[e];
    ctl->n += pos[e];
    ctl->miss = l >= 0 ? e - l - 1 : ctl->miss + e;
    ctl->n_darts = first + e;
    if (ended) {
        ctl->stopped = 1;
        ctl->reason = ctl->n >= max_points ? 2 : 1;
    }
    if (ctl->bad < (unsigned long long)(first + e)) ctl->stopped = 3; // a dart the run took
}

// the batch's new samples into the accepted table
template <typename T>
__global__ void sample_insert_kernel(CellMap<T> m, const Pt<T>* __restrict__ s_pts, Table acc, int32_t* __restrict__ s_next,
                                     int32_t B, int64_t off, const SampleCtl* __restrict__ ctl) {
    if (ctl->und[kGroup - 1] != 0) return;
    const int32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B || k >= ctl->n_new) return;
    const int64_t j = off + ctl->n - ctl->n_new + k;
    table_insert(acc, s_next, key_of(m, s_pts[j]), (int32_t)j);
}

// every sample again, into a table that was just enlarged
template <typename T>
__global__ void sample_rehash_kernel(CellMap<T> m, const Pt<T>* __restrict__ s_pts, Table acc, int32_t* __restrict__ s_next,
                                     int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
        table_insert(acc, s_next, key_of(m, s_pts[j]), (int32_t)j);
}

template <typename T>
__global__ void sample_unpack_kernel(const Pt<T>* __restrict__ pts, int64_t n, T* __restrict__ xyz, T* __restrict__ r) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const Pt<T> p = pts[i];
        if (xyz) xyz[3 * i] = p.x, xyz[3 * i + 1] = p.y, xyz[3 * i + 2] = p.z;
        if (r) r[i] = p.w;
    }
}

// the first two of every `stride` values: the area fill's read-back
template <typename T>
__global__ void sample_unpack_xy_kernel(const T* __restrict__ src, int stride, int64_t n, T* __restrict__ xy) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        xy[2 * i] = src[stride * i], xy[2 * i + 1] = src[stride * i + 1];
}

// ---- host side -----------------------------------------------------------------------------------------------------------
void sample_invalidate(wtp_ctx* ctx) {
    ctx->sample.kind = SampleKind::none;
    ctx->sample.n = 0;
    ctx->sample.n_seeds = 0;
}

static int64_t pow2_at_least(int64_t v) {
    int64_t p = 2;
    while (p < v) p <<= 1;
    return p;
}

static Table table_view(const DevBuf& b, int64_t tsz) {
    Table t;
    t.keys = (unsigned long long*)b.p;
    t.heads = (int32_t*)((char*)b.p + 8 * (size_t)tsz);
    t.mask = (uint32_t)(tsz - 1);
    int lg = 0;
    while ((int64_t(1) << lg) < tsz) ++lg;
    t.shift = 64 - lg;
    return t;
}

static int32_t scan_tiles(int64_t B) { return (int32_t)((B + 1 + kTile - 1) / kTile); }

// the batch buffers, for B darts
template <typename T> int ensure_batch(wtp_ctx* ctx, int64_t B) {
    SampleState& S = ctx->sample;
    int rc;
    if ((rc = ensure(ctx, S.ctl, sizeof(SampleCtl)))) return rc;
    if (S.bcap >= B && S.dtype == (sizeof(T) == 4 ? WTP_F32 : WTP_F64)) return WTP_OK;
    const size_t b = (size_t)B;
    S.b_tsz = pow2_at_least(2 * B);
    if ((rc = ensure(ctx, S.b_xyz, sizeof(T) * 3 * b))) return rc;
    if ((rc = ensure(ctx, S.b_h, sizeof(T) * b))) return rc;
    if ((rc = ensure(ctx, S.b_pts, sizeof(Pt<T>) * b))) return rc;
    if ((rc = ensure(ctx, S.b_tri, 4 * b))) return rc;
    if ((rc = ensure(ctx, S.b_st, 4 * b))) return rc;
    if ((rc = ensure(ctx, S.b_next, 4 * b))) return rc;
    if ((rc = ensure(ctx, S.b_pos, 4 * (b + 1)))) return rc;
    if ((rc = ensure(ctx, S.b_last, 4 * (b + 1)))) return rc;
    if ((rc = ensure(ctx, S.b_blk, sizeof(int2) * 2 * (size_t)scan_tiles(B)))) return rc;
    if ((rc = ensure(ctx, S.b_table, 12 * (size_t)S.b_tsz))) return rc;
    if ((rc = ensure(ctx, S.b_in, b))) return rc;
    S.bcap = B;
    return WTP_OK;
}

// a larger buffer that keeps the first `keep` bytes
static int grow_keep(wtp_ctx* ctx, DevBuf& b, size_t keep, size_t bytes) {
    if (b.cap >= bytes) return WTP_OK;
    DevBuf nb;
    int rc;
    if ((rc = ensure(ctx, nb, bytes))) return rc;
    if (keep) WTP_HIP(ctx, hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream));
    WTP_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the old block is freed when nb leaves this scope
    b = std::move(nb);
    return WTP_OK;
}

static int sm_grid(int64_t n) { return grid_for(n, kSmThreads, 1 << 20); }

// loops: a run over the boundary loops of wtp_loops_set instead of the mesh
static int check_sample_args(wtp_ctx* ctx, const wtp_spacing_desc* sp, double factor, uint64_t seed, bool loops = false) {
    if (loops && ctx->loops.ns < 1) return fail(ctx, WTP_ERR_STATE, "no loops: call wtp_loops_set first");
    if (!loops && ctx->mesh.nt < 1) return fail(ctx, WTP_ERR_STATE, "no mesh: call wtp_mesh_set first");
    if (!sp) return fail(ctx, WTP_ERR_ARG, "spacing is NULL");
    if (!(factor > 0) || !std::isfinite(factor)) return fail(ctx, WTP_ERR_ARG, "factor must be positive");
    if (seed >= (1ull << 24)) return fail(ctx, WTP_ERR_ARG, "seed must be below 2^24 (the stream's key layout)");
    if (sp->kind == WTP_SPACING_PER_POINT)
        return fail(ctx, WTP_ERR_ARG, "a per-point spacing array cannot be evaluated at a new position: pass a constant or a device law");
    if (sp->kind != WTP_SPACING_CONSTANT && !spacing_on_device(sp->kind)) return fail(ctx, WTP_ERR_ARG, "unknown spacing kind");
    if (spacing_on_device(sp->kind)) {
        const int rc = check_spacing_law(ctx, sp);
        if (rc) return rc;
    }
    if (!loops && (!(ctx->mesh.total_area > 0) || !std::isfinite(ctx->mesh.total_area)))
        return fail(ctx, WTP_ERR_ARG, "mesh has zero surface area");
    return WTP_OK;
}

static std::string bad_spacing_text(unsigned long long dart) {
    return "the spacing at dart " + std::to_string(dart) + " is not finite and > 0";
}

// room for `rows` accepted rows of which the first `keep` hold data, and a table of at least twice as many slots;
// *rehash: the table was replaced
template <typename T> static int ensure_rows(wtp_ctx* ctx, int64_t keep, int64_t rows, bool* rehash) {
    SampleState& S = ctx->sample;
    if (rows <= S.cap) return WTP_OK;
    int rc;
    const int64_t cap = std::max(rows, 2 * S.cap);
    if ((rc = grow_keep(ctx, S.pts, sizeof(Pt<T>) * (size_t)keep, sizeof(Pt<T>) * (size_t)cap))) return rc;
    if ((rc = grow_keep(ctx, S.tri, 4 * (size_t)keep, 4 * (size_t)cap))) return rc;
    if ((rc = grow_keep(ctx, S.dart, 8 * (size_t)keep, 8 * (size_t)cap))) return rc;
    if ((rc = ensure(ctx, S.next, 4 * (size_t)cap))) return rc; // rebuilt with the table
    S.tsz = pow2_at_least(2 * cap);
    if ((rc = ensure(ctx, S.table, 12 * (size_t)S.tsz))) return rc;
    S.cap = cap;
    *rehash = true;
    return WTP_OK;
}

// The cell map, once a first batch of B points is in b_pts: cell edge sqrt(r_min r_max) of that batch (it changes time
// only), cells over the mesh's box; the n_acc rows the accepted array already holds (seeds) enter its table now that
// cells exist.  One host read.
template <typename T>
static int first_batch_map(wtp_ctx* ctx, const SampleDomain& dom, int64_t B, int64_t n_acc, CellMap<T>* map_out, double* cell_edge) {
    SampleState& S = ctx->sample;
    SampleCtl* d_ctl = (SampleCtl*)S.ctl.p;
    SampleCtl* pin = (SampleCtl*)ctx->host_pinned;
    int rc;
    hipLaunchKernelGGL(sample_range_kernel<T>, dim3(sm_stride_grid(B)), dim3(kSmThreads), 0, ctx->stream,
                       (const Pt<T>*)S.b_pts.p, B, d_ctl);
    WTP_HIP(ctx, hipMemcpyAsync(pin, d_ctl, sizeof(SampleCtl), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    double ext = 0;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, dom.hi[a] - dom.lo[a]);
    double c = ext;
    if (pin->rmin != kEmpty)
        c = std::sqrt(__builtin_bit_cast(double, pin->rmin) * __builtin_bit_cast(double, pin->rmax));
    c = std::min(std::max(c, ext / 1.0e6), ext > 0 ? ext : c); // at most 2^20 cells per axis, at least one
    if (!(c > 0) || !std::isfinite(c)) c = 1;
    CellMap<T> map{};
    for (int a = 0; a < 3; ++a) {
        map.org[a] = (T)dom.lo[a];
        map.nc[a] = (int32_t)std::min(1048575.0, std::floor((dom.hi[a] - dom.lo[a]) / c) + 1);
    }
    map.inv_c = (T)(1.0 / c);
    *map_out = map;
    *cell_edge = c;
    if (n_acc > 0) {
        hipLaunchKernelGGL(sample_rehash_kernel<T>, dim3(sm_stride_grid(n_acc)), dim3(kSmThreads), 0, ctx->stream, map,
                           (const Pt<T>*)S.pts.p, table_view(S.table, S.tsz), (int32_t*)S.next.p, n_acc);
        WTP_HIP(ctx, hipGetLastError());
    }
    return WTP_OK;
}

// the two domains a run can have: the mesh of wtp_mesh_set, the boundary loops of wtp_loops_set
static SampleDomain mesh_domain(const wtp_ctx* ctx) {
    SampleDomain d{};
    for (int a = 0; a < 3; ++a) d.lo[a] = ctx->mesh.bbox[a], d.hi[a] = ctx->mesh.bbox[3 + a];
    d.dtype = ctx->mesh.dtype, d.dim = 3, d.loops = false;
    return d;
}

static SampleDomain loops_domain(const wtp_ctx* ctx) {
    SampleDomain d{};
    for (int a = 0; a < 2; ++a) d.lo[a] = ctx->loops.bbox[a], d.hi[a] = ctx->loops.bbox[2 + a];
    d.lo[2] = d.hi[2] = 0; // every row keeps z = 0: one layer of cells, and dz * dz adds an exact zero to every distance
    d.dtype = ctx->loops.dtype, d.dim = 2, d.loops = true;
    return d;
}

// what a run carries from batch to batch
template <typename T> struct Run {
    SampleDomain dom{};        // the run's domain, as its entry point described it
    CellMap<T> map{};          // made by the first batch (first_batch_map)
    bool have_map = false, classes = false;
    double cell_edge = 0;
    int64_t n = 0, ns = 0;     // rows of the accepted array, the ns seeds at its front included
    int32_t n_batches = 0, rounds_max = 0;
    int64_t syncs0 = 0;
};

// what decide_batch needs to know of a batch whose points are in b_pts
struct BatchArgs {
    int64_t B, n_acc;          // points in the batch; rows of the accepted array (seeds included)
    int64_t first, off;        // stream index of the batch's first point; seed rows at the front of the accepted array
    int64_t max_points, stall_limit;
    const uint8_t* inside;     // the domain test's flags (NULL: the surface sampler), counted into n_inside
    const int32_t* tri;        // parent triangles to append (NULL: none)
    int32_t par0, per;         // kFront: the batch's first parent and the candidates per parent
};

// Steps 2 to 4 for one batch: cull, rounds in groups of kGroup, and behind each group the stop scan, append, count,
// finish and insert, all guarded by the group's last undecided count; one control-block read per group, left in the
// pinned block for the caller.  The run's first batch makes the cell map first; a decided batch counts into the run.
// kFront: the front's one-sided rule with the parent exempt.
template <typename T, bool kFront> static int decide_batch(wtp_ctx* ctx, Run<T>& run, const BatchArgs& a) {
    SampleState& S = ctx->sample;
    SampleCtl* d_ctl = (SampleCtl*)S.ctl.p;
    SampleCtl* pin = (SampleCtl*)ctx->host_pinned;
    int rc;
    if (!run.have_map) {
        if ((rc = first_batch_map<T>(ctx, run.dom, a.B, run.n, &run.map, &run.cell_edge))) return rc;
        run.have_map = true;
    }
    const CellMap<T>& map = run.map;
    const Table acc = table_view(S.table, S.tsz), bt = table_view(S.b_table, S.b_tsz);
    const int64_t B = a.B;
    const int32_t Bi = (int32_t)B;
    WTP_HIP(ctx, hipMemsetAsync(S.b_table.p, 0xFF, 12 * (size_t)S.b_tsz, ctx->stream));
    hipLaunchKernelGGL((sample_cull_kernel<T, kFront>), dim3(sm_grid(B)), dim3(kSmThreads), 0, ctx->stream, map,
                       (const Pt<T>*)S.b_pts.p, Bi, (int32_t*)S.b_st.p, acc, (const int32_t*)S.next.p,
                       (const Pt<T>*)S.pts.p, a.n_acc, bt, (int32_t*)S.b_next.p, a.inside, a.first, a.par0, a.per, d_ctl);
    WTP_HIP(ctx, hipGetLastError());
    int32_t round0 = 0;
    for (;;) {
        WTP_HIP(ctx, hipMemsetAsync(d_ctl->und, 0, sizeof(SampleCtl::und), ctx->stream));
        for (int g = 0; g < kGroup; ++g)
            hipLaunchKernelGGL((sample_round_kernel<T, kFront>), dim3(sm_grid(B)), dim3(kSmThreads), 0, ctx->stream, map,
                               (const Pt<T>*)S.b_pts.p, Bi, (int32_t*)S.b_st.p, bt, (const int32_t*)S.b_next.p, g,
                               round0 + g + 1, d_ctl);
        int2* blk = (int2*)S.b_blk.p;
        const int32_t nblk = scan_tiles(B);
        hipLaunchKernelGGL(sample_scan_a_kernel, dim3(nblk), dim3(kSmThreads), 0, ctx->stream, (const int32_t*)S.b_st.p, Bi,
                           blk, d_ctl);
        hipLaunchKernelGGL(sample_scan_b_kernel, dim3(1), dim3(kSmThreads), 0, ctx->stream, blk, nblk, blk + nblk, d_ctl);
        hipLaunchKernelGGL(sample_scan_c_kernel, dim3(nblk), dim3(kSmThreads), 0, ctx->stream, (const int32_t*)S.b_st.p, Bi,
                           blk + nblk, (int32_t*)S.b_pos.p, (int32_t*)S.b_last.p, a.max_points, a.stall_limit, d_ctl);
        hipLaunchKernelGGL(sample_append_kernel<T>, dim3(sm_grid(B)), dim3(kSmThreads), 0, ctx->stream,
                           (const Pt<T>*)S.b_pts.p, a.tri, (const int32_t*)S.b_st.p, Bi, (const int32_t*)S.b_pos.p, a.first,
                           a.off, (Pt<T>*)S.pts.p, (int32_t*)S.tri.p, (int64_t*)S.dart.p, d_ctl);
        if (a.inside)
            hipLaunchKernelGGL(fill_count_kernel, dim3(sm_grid(B)), dim3(kSmThreads), 0, ctx->stream, a.inside, Bi, d_ctl);
        hipLaunchKernelGGL(sample_finish_kernel, dim3(1), dim3(1), 0, ctx->stream, (const int32_t*)S.b_pos.p,
                           (const int32_t*)S.b_last.p, Bi, a.first, a.max_points, d_ctl);
        hipLaunchKernelGGL(sample_insert_kernel<T>, dim3(sm_grid(B)), dim3(kSmThreads), 0, ctx->stream, map,
                           (const Pt<T>*)S.pts.p, acc, (int32_t*)S.next.p, Bi, a.off, d_ctl);
        WTP_HIP(ctx, hipGetLastError());
        WTP_HIP(ctx, hipMemcpyAsync(pin, d_ctl, sizeof(SampleCtl), hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = sync(ctx))) return rc;
        if (pin->und[kGroup - 1] == 0) {
            int g = 0;
            while (pin->und[g] != 0) ++g;
            ++run.n_batches;
            run.rounds_max = std::max(run.rounds_max, round0 + g + 1);
            return WTP_OK;
        }
        round0 += kGroup;
        if (round0 >= B) return fail(ctx, WTP_ERR_INTERNAL, "a batch was not decided within as many rounds as it has points");
    }
}

// what a run reports: the fields the three public info structs share (n_darts: the front's candidates)
struct RunInfo {
    int64_t n_points, n_darts, n_inside, batch;
    int32_t stop_reason, n_batches, rounds_max, host_syncs;
    double r_min, r_max;
};

// Run begin, up to the control block's upload: nothing is resident any more, the law's tree, batch buffers for B darts
// of the domain's type, and the ns seeds (r = T(factor) h, every one checked) in front of an accepted array with room for
// `room` more rows.
template <typename T>
static int run_begin(wtp_ctx* ctx, const SampleDomain& dom, const wtp_spacing_desc* sp, double factor, const T* seeds, int64_t ns,
                     int64_t B, int64_t room, Run<T>* run) {
    SampleState& S = ctx->sample;
    const int dtype = sizeof(T) == 4 ? WTP_F32 : WTP_F64;
    int rc;
    run->dom = dom;
    run->syncs0 = ctx->n_syncs;
    run->n = run->ns = ns;
    sample_invalidate(ctx);
    if (spacing_on_device(sp->kind) && (rc = ensure_kd(ctx, sp, dom.dim, dtype))) return rc;
    if ((rc = ensure_pinned(ctx, sizeof(SampleCtl)))) return rc;
    if (S.dtype != dtype) S.cap = 0, S.bcap = 0; // the rows have another size
    if ((rc = ensure_batch<T>(ctx, B))) return rc;
    S.dtype = dtype;
    if (ns > 0) {
        bool replaced = false;
        if (ns + room >= (int64_t(1) << 31) - 1) return fail(ctx, WTP_ERR_ARG, "seeds + batch exceed the int32 index space");
        if ((rc = ensure_rows<T>(ctx, 0, ns + room, &replaced))) return rc;
        if ((rc = fill_seeds<T>(ctx, sp, factor, seeds, ns, dom.dim))) return rc;
    }
    SampleCtl* pin = (SampleCtl*)ctx->host_pinned;
    *pin = SampleCtl{};
    pin->bad = kEmpty, pin->rmin = kEmpty, pin->rmax = 0, pin->end = INT_MAX;
    WTP_HIP(ctx, hipMemcpyAsync(S.ctl.p, pin, sizeof(SampleCtl), hipMemcpyHostToDevice, ctx->stream));
    return WTP_OK;
}

// Before a batch's points are generated (`first`: the stream index of its first point): the class grid if the run wants
// one (want_classes) and has by now walked the mesh's tree for more points than a grid of its cell size has cells (an
// exact test per cell; from here on the points of cells wholly inside or outside skip the walk); room for `room` more
// rows; the accepted table emptied and refilled where it is stale or was replaced; the control block's batch fields.
template <typename T> static int batch_prepare(wtp_ctx* ctx, Run<T>& run, int64_t first, int64_t room, bool want_classes) {
    SampleState& S = ctx->sample;
    int rc;
    if (want_classes && run.have_map && !run.classes) {
        const int64_t cells = mesh_class_cells(ctx, run.cell_edge);
        if (cells <= first && cells <= (int64_t(1) << 26)) {
            if ((rc = mesh_ensure_classes(ctx, run.cell_edge))) return rc;
            run.classes = true;
        }
    }
    bool rehash = false;
    if ((rc = ensure_rows<T>(ctx, run.n, run.n + room, &rehash))) return rc;
    if (run.n_batches == 0) {
        S.tsz = pow2_at_least(2 * S.cap); // buffers of an earlier call, or the seeds' own: the table is stale
        rehash = true;
    }
    if (rehash) WTP_HIP(ctx, hipMemsetAsync(S.table.p, 0xFF, 12 * (size_t)S.tsz, ctx->stream));
    if (rehash && run.n > 0 && run.have_map) {
        hipLaunchKernelGGL(sample_rehash_kernel<T>, dim3(sm_stride_grid(run.n)), dim3(kSmThreads), 0, ctx->stream, run.map,
                           (const Pt<T>*)S.pts.p, table_view(S.table, S.tsz), (int32_t*)S.next.p, run.n);
        WTP_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(sample_begin_kernel, dim3(1), dim3(1), 0, ctx->stream, (SampleCtl*)S.ctl.p);
    return WTP_OK;
}

// Run finish, from the last group's control block in the pinned block: r over the rows behind the seeds (one pass, one
// read), the result resident as `kind`, and the info fields every run reports (stop_reason as the stop scan left it).
template <typename T> static int run_finish(wtp_ctx* ctx, const Run<T>& run, SampleKind kind, RunInfo* info) {
    SampleState& S = ctx->sample;
    SampleCtl* d_ctl = (SampleCtl*)S.ctl.p;
    SampleCtl* pin = (SampleCtl*)ctx->host_pinned;
    const SampleCtl h = *pin;
    const int64_t n_new = run.n - run.ns;
    int rc;
    pin->rmin = kEmpty, pin->rmax = 0;
    WTP_HIP(ctx, hipMemcpyAsync(d_ctl, pin, sizeof(SampleCtl), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(sample_range_kernel<T>, dim3(sm_stride_grid(n_new)), dim3(kSmThreads), 0, ctx->stream,
                       (const Pt<T>*)S.pts.p + run.ns, n_new, d_ctl);
    WTP_HIP(ctx, hipGetLastError());
    WTP_HIP(ctx, hipMemcpyAsync(pin, d_ctl, sizeof(SampleCtl), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    S.n = n_new;
    S.n_seeds = run.ns;
    S.kind = kind;
    info->n_points = n_new;
    info->n_darts = h.n_darts;
    info->n_inside = (int64_t)h.n_inside;
    info->stop_reason = h.reason;
    info->n_batches = run.n_batches;
    info->rounds_max = run.rounds_max;
    info->host_syncs = (int32_t)(ctx->n_syncs - run.syncs0);
    info->r_min = pin->rmin != kEmpty ? __builtin_bit_cast(double, pin->rmin) : 0.0;
    info->r_max = __builtin_bit_cast(double, pin->rmax);
    return WTP_OK;
}

// The run of wtp_mesh_sample (kind sample), wtp_mesh_fill (fill) or wtp_loops_fill (area); the last two over the darts of
// the domain's box, with ns seeds in the domain's type: batches of consecutive darts, doubled from kBatchFirst to
// kBatchMax unless `batch` fixes their size.
template <typename T>
static int sample_run(wtp_ctx* ctx, const SampleDomain& dom, const wtp_spacing_desc* sp, double factor, int64_t max_points,
                      int64_t stall_limit, uint64_t seed, int64_t batch, SampleKind kind, const T* seeds, int64_t ns, RunInfo* info) {
    SampleState& S = ctx->sample;
    const bool fill = kind != SampleKind::sample;
    Run<T> run;
    int64_t B = batch > 0 ? batch : kBatchFirst, first = 0;
    int rc;
    if ((rc = run_begin<T>(ctx, dom, sp, factor, seeds, ns, B, B, &run))) return rc;
    const SampleCtl* pin = (const SampleCtl*)ctx->host_pinned; // decide_batch leaves the last group's control block there
    for (;;) {
        if (run.n + B >= (int64_t(1) << 31) - 1) return fail(ctx, WTP_ERR_ARG, "samples + batch exceed the int32 index space");
        if ((rc = ensure_batch<T>(ctx, B))) return rc;
        if ((rc = batch_prepare<T>(ctx, run, first, B, fill && !dom.loops))) return rc; // only the fill tests darts against the mesh
        if ((rc = enqueue_darts<T>(ctx, dom, sp, factor, seed, first, B, fill))) return rc;
        const BatchArgs args{B, run.n, first, ns, max_points, stall_limit, fill ? (const uint8_t*)S.b_in.p : (const uint8_t*)nullptr,
                             fill ? (const int32_t*)nullptr : (const int32_t*)S.b_tri.p, 0, 1};
        if ((rc = decide_batch<T, false>(ctx, run, args))) return rc;
        if (pin->stopped == 3) return fail(ctx, WTP_ERR_ARG, bad_spacing_text(pin->bad));
        run.n = ns + pin->n;
        if (pin->stopped) break;
        first += B;
        if (batch == 0) B = std::min(2 * B, kBatchMax);
    }
    info->batch = B;
    return run_finish<T>(ctx, run, kind, info);
}

// The run of wtp_mesh_front: parents in queue order, batches of whole parents that were in the queue when the batch began.
template <typename T>
static int front_run(wtp_ctx* ctx, const wtp_spacing_desc* sp, int per, const T* seeds, int64_t ns, int64_t max_points,
                     uint64_t seed, int64_t batch, RunInfo* info) {
    SampleState& S = ctx->sample;
    const int dtype = sizeof(T) == 4 ? WTP_F32 : WTP_F64;
    const bool law = spacing_on_device(sp->kind);
    const auto bad_h = [&](unsigned long long cand) {
        return fail(ctx, WTP_ERR_ARG, "the spacing at the point accepted from candidate " + std::to_string(cand) + " is not finite and > 0");
    };
    int rc;
    *info = RunInfo{};
    info->stop_reason = 1;
    if (ns == 0) { // nothing to expand: the front has died out before it began
        sample_invalidate(ctx);
        S.dtype = S.dtype < 0 ? dtype : S.dtype;
        S.kind = SampleKind::front, S.front_per = per;
        return WTP_OK;
    }
    // parents per batch: at most kBatchMax candidates, whatever `batch` asks for (the kernels run one thread per candidate
    // of a grid of at most 2^20 blocks, and the batch changes time only)
    const int64_t par_cap = std::max<int64_t>(kBatchMax / per, 1);
    const int64_t par_max = batch > 0 ? std::min(batch, par_cap) : par_cap;
    int64_t B = std::min(ns, par_max) * per;
    Run<T> run;
    if ((rc = run_begin<T>(ctx, mesh_domain(ctx), sp, 1.0, seeds, ns, pow2_at_least(std::max(B, kBatchFirst)), std::min(B, max_points), &run)))
        return rc; // (factor 1: a seed's w = T(1) h = h)
    SampleCtl* pin = (SampleCtl*)ctx->host_pinned; // decide_batch leaves the last group's control block there
    int64_t q0 = 0; // parents expanded so far; run.n is the queue's length
    for (;;) {
        const int64_t q1 = std::min(run.n, q0 + par_max), first = q0 * per;
        B = (q1 - q0) * per;
        const int64_t room = std::min(B, max_points - (run.n - ns)); // rows the batch can append
        const int64_t bwant = pow2_at_least(std::max(B, kBatchFirst));
        if (bwant > S.bcap && (rc = sync(ctx))) return rc; // the last batch's law pass still reads the batch buffers
        if ((rc = ensure_batch<T>(ctx, bwant))) return rc;
        if ((rc = batch_prepare<T>(ctx, run, first, room, true))) return rc;
        if ((rc = enqueue_candidates<T>(ctx, seed, (const Pt<T>*)S.pts.p, q0, first, B, per))) return rc;
        // a stall limit no miss run can reach: only max_points ends the scan
        const BatchArgs args{B, run.n, first, ns, max_points, (int64_t)LLONG_MAX, (const uint8_t*)S.b_in.p, (const int32_t*)nullptr,
                             (int32_t)q0, (int32_t)per};
        if ((rc = decide_batch<T, true>(ctx, run, args))) return rc;
        // an accepted point of an earlier batch whose own h is bad (the rows of this batch are evaluated below)
        if (pin->bad != kEmpty) return bad_h(pin->bad);
        const int64_t n_new = pin->n_new;
        if (n_new > room) return fail(ctx, WTP_ERR_INTERNAL, "a batch appended more rows than it had room for");
        if (law && n_new > 0 && (rc = front_own_h<T>(ctx, sp, run.n, n_new))) return rc;
        run.n += n_new;
        q0 = q1;
        if (pin->stopped) break;  // max_points
        if (q0 == run.n) break;   // nothing was appended and every entry has been expanded: the front has died out
    }
    WTP_HIP(ctx, hipMemcpyAsync(pin, S.ctl.p, sizeof(SampleCtl), hipMemcpyDeviceToHost, ctx->stream)); // the last rows' bad values
    if ((rc = sync(ctx))) return rc;
    if (pin->bad != kEmpty) return bad_h(pin->bad);
    if ((rc = run_finish<T>(ctx, run, SampleKind::front, info))) return rc;
    S.front_per = per;
    info->batch = B / per;
    info->stop_reason = info->stop_reason ? 2 : 1; // max_points ended the scan, or the front has died out
    return WTP_OK;
}

template <typename T> int sample_unpack(wtp_ctx* ctx, const void* pts, int64_t n, T* d_xyz, T* d_r) {
    hipLaunchKernelGGL(sample_unpack_kernel<T>, dim3(sm_stride_grid(n)), dim3(kSmThreads), 0, ctx->stream, (const Pt<T>*)pts, n,
                       d_xyz, d_r);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

template <typename T> int sample_unpack_xy(wtp_ctx* ctx, const T* src, int stride, int64_t n, T* d_xy) {
    hipLaunchKernelGGL(sample_unpack_xy_kernel<T>, dim3(sm_stride_grid(n)), dim3(kSmThreads), 0, ctx->stream, src, stride, n, d_xy);
    WTP_HIP(ctx, hipGetLastError());
    return WTP_OK;
}

#define INST(T)                                                            \
    template int ensure_batch<T>(wtp_ctx*, int64_t);                       \
    template int sample_unpack<T>(wtp_ctx*, const void*, int64_t, T*, T*); \
    template int sample_unpack_xy<T>(wtp_ctx*, const T*, int, int64_t, T*);
INST(float)
INST(double)
#undef INST

} // namespace wtp

using namespace wtp;
#define WTP_API extern "C"

// max_points, batch and the seeds (wtp_mesh_sample takes none)
static int check_size_args(wtp_ctx* ctx, int64_t max_points, int64_t batch, const void* seeds, int64_t n_seeds) {
    if (max_points < 1) return fail(ctx, WTP_ERR_ARG, "max_points must be positive");
    if (batch < 0 || batch > (int64_t(1) << 24)) return fail(ctx, WTP_ERR_ARG, "batch must be in [0, 2^24]");
    if (n_seeds < 0) return fail(ctx, WTP_ERR_ARG, "n_seeds must not be negative");
    if (n_seeds > 0 && !seeds) return fail(ctx, WTP_ERR_ARG, "seeds is NULL");
    return WTP_OK;
}

// the argument rows wtp_mesh_sample and wtp_mesh_fill share
static int check_run_args(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, int64_t max_points, int64_t stall_limit,
                          uint64_t seed, int64_t batch, const void* seeds, int64_t n_seeds, bool loops = false) {
    const int rc = check_sample_args(ctx, spacing, factor, seed, loops);
    if (rc) return rc;
    if (stall_limit < 1) return fail(ctx, WTP_ERR_ARG, "stall_limit must be positive");
    return check_size_args(ctx, max_points, batch, seeds, n_seeds);
}

WTP_API int wtp_mesh_sample(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, int64_t max_points,
                            int64_t stall_limit, uint64_t seed, int64_t batch, wtp_sample_info* info) {
    if (!ctx) return WTP_ERR_ARG;
    int rc = check_run_args(ctx, spacing, factor, max_points, stall_limit, seed, batch, nullptr, 0);
    if (rc) return rc;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    RunInfo ri{};
    rc = by_dtype(ctx->mesh.dtype, [&](auto t) {
        using T = decltype(t);
        return sample_run<T>(ctx, mesh_domain(ctx), spacing, factor, max_points, stall_limit, seed, batch, SampleKind::sample,
                             (const T*)nullptr, 0, &ri);
    });
    if (rc || !info) return rc;
    info->n_points = ri.n_points, info->n_darts = ri.n_darts, info->batch = ri.batch;
    info->stop_reason = ri.stop_reason;
    info->n_batches = ri.n_batches, info->rounds_max = ri.rounds_max, info->host_syncs = ri.host_syncs;
    info->total_area = ctx->mesh.total_area, info->r_min = ri.r_min, info->r_max = ri.r_max;
    return WTP_OK;
}

// is a result of kind k resident?  `missing`: what to say if not
static int check_resident(wtp_ctx* ctx, SampleKind k, const char* missing) {
    if (!ctx) return WTP_ERR_ARG;
    if (ctx->sample.kind != k) return fail(ctx, WTP_ERR_STATE, missing);
    return WTP_OK;
}

// xyz and r of the resident rows behind the seeds, into host arrays (through the context's scratch block) or, dev, into
// device arrays; either may be absent.  cols = 2: the area fill's xy rows
static int rows_out(wtp_ctx* ctx, bool dev, void* xyz_out, void* r_out, int cols = 3) {
    SampleState& S = ctx->sample;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    if (!xyz_out && !r_out) return WTP_OK;
    const size_t ts = tsize(S.dtype), n = (size_t)S.n;
    int rc;
    if (!dev && (rc = ensure(ctx, ctx->scratch, ts * 4 * n))) return rc;
    char* d_xyz = dev ? (char*)xyz_out : (char*)ctx->scratch.p;
    char* d_r = dev ? (char*)r_out : d_xyz + ts * 3 * n;
    rc = by_dtype(S.dtype, [&](auto t) {
        using T = decltype(t);
        const Pt<T>* rows = (const Pt<T>*)S.pts.p + S.n_seeds;
        if (cols == 3) return sample_unpack<T>(ctx, rows, S.n, (T*)d_xyz, (T*)d_r);
        if (d_xyz && S.n > 0 && sample_unpack_xy<T>(ctx, (const T*)rows, 4, S.n, (T*)d_xyz)) return (int)WTP_ERR_HIP;
        return d_r ? sample_unpack<T>(ctx, rows, S.n, (T*)nullptr, (T*)d_r) : (int)WTP_OK;
    });
    if (rc || dev) return rc;
    if (xyz_out) WTP_HIP(ctx, hipMemcpyAsync(xyz_out, d_xyz, ts * cols * n, hipMemcpyDeviceToHost, ctx->stream));
    if (r_out) WTP_HIP(ctx, hipMemcpyAsync(r_out, d_r, ts * n, hipMemcpyDeviceToHost, ctx->stream));
    return WTP_OK;
}

static const char kNoSample[] = "no sample: call wtp_mesh_sample first";
static const char kNoFill[] = "no fill: call wtp_mesh_fill first";
static const char kNoFront[] = "no front: call wtp_mesh_front first";

WTP_API int wtp_mesh_sample_get(wtp_ctx* ctx, void* xyz_out, int32_t* tri_out, void* r_out, int64_t* dart_out) {
    int rc = check_resident(ctx, SampleKind::sample, kNoSample);
    if (rc || (rc = rows_out(ctx, false, xyz_out, r_out))) return rc;
    const SampleState& S = ctx->sample;
    if (tri_out) WTP_HIP(ctx, hipMemcpyAsync(tri_out, S.tri.p, 4 * (size_t)S.n, hipMemcpyDeviceToHost, ctx->stream));
    if (dart_out) WTP_HIP(ctx, hipMemcpyAsync(dart_out, S.dart.p, 8 * (size_t)S.n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_mesh_sample_get_dev(wtp_ctx* ctx, void* d_xyz_out, int32_t* d_tri_out, void* d_r_out) {
    int rc = check_resident(ctx, SampleKind::sample, kNoSample);
    if (rc || (rc = rows_out(ctx, true, d_xyz_out, d_r_out))) return rc;
    const SampleState& S = ctx->sample;
    if (d_tri_out) WTP_HIP(ctx, hipMemcpyAsync(d_tri_out, S.tri.p, 4 * (size_t)S.n, hipMemcpyDeviceToDevice, ctx->stream));
    return sync(ctx);
}

static int check_dart_range(wtp_ctx* ctx, int64_t first, int64_t n) {
    if (first < 0 || n < 0 || first > (int64_t(1) << 62) - n) return fail(ctx, WTP_ERR_ARG, "bad dart range");
    return WTP_OK;
}

WTP_API int wtp_mesh_sample_darts(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, uint64_t seed, int64_t first,
                                  int64_t n, void* xyz_out, int32_t* tri_out, void* r_out) {
    if (!ctx) return WTP_ERR_ARG;
    int rc = check_sample_args(ctx, spacing, factor, seed);
    if (rc || (rc = check_dart_range(ctx, first, n))) return rc;
    if (n == 0) return WTP_OK;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    return by_dtype(ctx->mesh.dtype, [&](auto t) {
        using T = decltype(t);
        return sample_darts<T>(ctx, mesh_domain(ctx), spacing, factor, seed, first, n, false, (T*)xyz_out, tri_out, nullptr, (T*)r_out);
    });
}

// ---- the volume fill ---------------------------------------------------------------------------------------------------
WTP_API int wtp_mesh_fill(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, const void* seeds, int64_t n_seeds,
                          int64_t max_points, int64_t stall_limit, uint64_t seed, int64_t batch, wtp_fill_info* info) {
    if (!ctx) return WTP_ERR_ARG;
    int rc = check_run_args(ctx, spacing, factor, max_points, stall_limit, seed, batch, seeds, n_seeds);
    if (rc) return rc;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    RunInfo ri{};
    rc = by_dtype(ctx->mesh.dtype, [&](auto t) {
        using T = decltype(t);
        return sample_run<T>(ctx, mesh_domain(ctx), spacing, factor, max_points, stall_limit, seed, batch, SampleKind::fill,
                             (const T*)seeds, n_seeds, &ri);
    });
    if (rc || !info) return rc;
    const double* b = ctx->mesh.bbox;
    info->n_points = ri.n_points, info->n_darts = ri.n_darts, info->n_inside = ri.n_inside, info->n_seeds = n_seeds;
    info->batch = ri.batch;
    info->stop_reason = ri.stop_reason;
    info->n_batches = ri.n_batches, info->rounds_max = ri.rounds_max, info->host_syncs = ri.host_syncs;
    info->bbox_volume = ((b[3] - b[0]) * (b[4] - b[1])) * (b[5] - b[2]);
    info->r_min = ri.r_min, info->r_max = ri.r_max;
    return WTP_OK;
}

WTP_API int wtp_mesh_fill_get(wtp_ctx* ctx, void* xyz_out, void* r_out, int64_t* dart_out) {
    int rc = check_resident(ctx, SampleKind::fill, kNoFill);
    if (rc || (rc = rows_out(ctx, false, xyz_out, r_out))) return rc;
    const SampleState& S = ctx->sample;
    if (dart_out)
        WTP_HIP(ctx, hipMemcpyAsync(dart_out, (const int64_t*)S.dart.p + S.n_seeds, 8 * (size_t)S.n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_mesh_fill_get_dev(wtp_ctx* ctx, void* d_xyz_out, void* d_r_out) {
    int rc = check_resident(ctx, SampleKind::fill, kNoFill);
    if (rc || (rc = rows_out(ctx, true, d_xyz_out, d_r_out))) return rc;
    return sync(ctx);
}

WTP_API int wtp_mesh_fill_darts(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, uint64_t seed, int64_t first,
                                int64_t n, void* xyz_out, uint8_t* inside_out, void* r_out) {
    if (!ctx) return WTP_ERR_ARG;
    int rc = check_sample_args(ctx, spacing, factor, seed);
    if (rc || (rc = check_dart_range(ctx, first, n))) return rc;
    if (n == 0) return WTP_OK;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    return by_dtype(ctx->mesh.dtype, [&](auto t) {
        using T = decltype(t);
        return sample_darts<T>(ctx, mesh_domain(ctx), spacing, factor, seed, first, n, true, (T*)xyz_out, nullptr, inside_out, (T*)r_out);
    });
}

// ---- the advancing front -------------------------------------------------------------------------------------------------
static int check_front_args(wtp_ctx* ctx, const wtp_spacing_desc* spacing, int64_t n, uint64_t seed) {
    const int rc = check_sample_args(ctx, spacing, 1.0, seed);
    if (rc) return rc;
    if (n < 1 || n > 64) return fail(ctx, WTP_ERR_ARG, "n (candidates per parent) must be in [1, 64]");
    return WTP_OK;
}

WTP_API int wtp_mesh_front(wtp_ctx* ctx, const wtp_spacing_desc* spacing, int64_t n, const void* seeds, int64_t n_seeds,
                           int64_t max_points, uint64_t seed, int64_t batch, wtp_front_info* info) {
    if (!ctx) return WTP_ERR_ARG;
    int rc = check_front_args(ctx, spacing, n, seed);
    if (rc || (rc = check_size_args(ctx, max_points, batch, seeds, n_seeds))) return rc;
    // the queue holds at most n_seeds + max_points rows, indexed in int32: refused here, not in the middle of a run
    if (n_seeds >= (int64_t(1) << 31) || max_points >= (int64_t(1) << 31) || n_seeds + max_points >= (int64_t(1) << 31) - 1)
        return fail(ctx, WTP_ERR_ARG, "n_seeds + max_points exceed the int32 index space of the queue");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    RunInfo ri{};
    rc = by_dtype(ctx->mesh.dtype, [&](auto t) {
        using T = decltype(t);
        return front_run<T>(ctx, spacing, (int)n, (const T*)seeds, n_seeds, max_points, seed, batch, &ri);
    });
    if (rc || !info) return rc;
    info->n_points = ri.n_points, info->n_parents = (ri.n_darts + n - 1) / n, info->n_candidates = ri.n_darts;
    info->n_inside = ri.n_inside, info->n_seeds = n_seeds, info->batch = ri.batch;
    info->stop_reason = ri.stop_reason;
    info->n_batches = ri.n_batches, info->rounds_max = ri.rounds_max, info->host_syncs = ri.host_syncs;
    info->r_min = ri.r_min, info->r_max = ri.r_max;
    return WTP_OK;
}

WTP_API int wtp_mesh_front_get(wtp_ctx* ctx, void* xyz_out, void* h_out, int64_t* cand_out, int32_t* parent_out) {
    int rc = check_resident(ctx, SampleKind::front, kNoFront);
    if (rc || ctx->sample.n == 0 || (rc = rows_out(ctx, false, xyz_out, h_out))) return rc;
    const SampleState& S = ctx->sample;
    std::vector<int64_t> cand;
    int64_t* c = cand_out;
    if (parent_out && !c) cand.resize((size_t)S.n), c = cand.data();
    if (c) WTP_HIP(ctx, hipMemcpyAsync(c, (const int64_t*)S.dart.p + S.n_seeds, 8 * (size_t)S.n, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = sync(ctx))) return rc;
    if (parent_out)
        for (int64_t i = 0; i < S.n; ++i) parent_out[i] = (int32_t)(c[i] / S.front_per); // candidate j = q n + s
    return WTP_OK;
}

WTP_API int wtp_mesh_front_get_dev(wtp_ctx* ctx, void* d_xyz_out, void* d_h_out) {
    int rc = check_resident(ctx, SampleKind::front, kNoFront);
    if (rc || ctx->sample.n == 0 || (rc = rows_out(ctx, true, d_xyz_out, d_h_out))) return rc;
    return sync(ctx);
}

WTP_API int wtp_mesh_front_candidates(wtp_ctx* ctx, const wtp_spacing_desc* spacing, uint64_t seed, const void* parents_xyz,
                                      int64_t n_parents, int64_t first_parent, int64_t n, void* xyz_out, uint8_t* inside_out,
                                      void* r_out) {
    if (!ctx) return WTP_ERR_ARG;
    int rc = check_front_args(ctx, spacing, n, seed);
    if (rc) return rc;
    if (n_parents < 0 || first_parent < 0 || n_parents > (int64_t(1) << 31) || first_parent > (int64_t(1) << 31))
        return fail(ctx, WTP_ERR_ARG, "bad parent range");
    if (n_parents == 0) return WTP_OK;
    if (!parents_xyz) return fail(ctx, WTP_ERR_ARG, "parents_xyz is NULL");
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    return by_dtype(ctx->mesh.dtype, [&](auto t) {
        using T = decltype(t);
        return front_candidates<T>(ctx, spacing, seed, (const T*)parents_xyz, n_parents, first_parent, (int)n, (T*)xyz_out,
                                   inside_out, (T*)r_out);
    });
}

// ---- the area fill: wtp_mesh_fill's run over the boundary loops of wtp_loops_set -----------------------
static const char kNoArea[] = "no area fill: call wtp_loops_fill first";

WTP_API int wtp_loops_fill(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, const void* seeds, int64_t n_seeds,
                           int64_t max_points, int64_t stall_limit, uint64_t seed, int64_t batch, wtp_fill_info* info) {
    if (!ctx) return WTP_ERR_ARG;
    int rc = check_run_args(ctx, spacing, factor, max_points, stall_limit, seed, batch, seeds, n_seeds, true);
    if (rc) return rc;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    RunInfo ri{};
    const SampleDomain dom = loops_domain(ctx);
    rc = by_dtype(dom.dtype, [&](auto t) {
        using T = decltype(t);
        return sample_run<T>(ctx, dom, spacing, factor, max_points, stall_limit, seed, batch, SampleKind::area, (const T*)seeds,
                             n_seeds, &ri);
    });
    if (rc || !info) return rc;
    info->n_points = ri.n_points, info->n_darts = ri.n_darts, info->n_inside = ri.n_inside, info->n_seeds = n_seeds;
    info->batch = ri.batch;
    info->stop_reason = ri.stop_reason;
    info->n_batches = ri.n_batches, info->rounds_max = ri.rounds_max, info->host_syncs = ri.host_syncs;
    info->bbox_volume = (dom.hi[0] - dom.lo[0]) * (dom.hi[1] - dom.lo[1]);
    info->r_min = ri.r_min, info->r_max = ri.r_max;
    return WTP_OK;
}

WTP_API int wtp_loops_fill_get(wtp_ctx* ctx, void* xy_out, void* r_out, int64_t* dart_out) {
    int rc = check_resident(ctx, SampleKind::area, kNoArea);
    if (rc || (rc = rows_out(ctx, false, xy_out, r_out, 2))) return rc;
    const SampleState& S = ctx->sample;
    if (dart_out)
        WTP_HIP(ctx, hipMemcpyAsync(dart_out, (const int64_t*)S.dart.p + S.n_seeds, 8 * (size_t)S.n, hipMemcpyDeviceToHost, ctx->stream));
    return sync(ctx);
}

WTP_API int wtp_loops_fill_get_dev(wtp_ctx* ctx, void* d_xy_out, void* d_r_out) {
    int rc = check_resident(ctx, SampleKind::area, kNoArea);
    if (rc || (rc = rows_out(ctx, true, d_xy_out, d_r_out, 2))) return rc;
    return sync(ctx);
}

WTP_API int wtp_loops_fill_darts(wtp_ctx* ctx, const wtp_spacing_desc* spacing, double factor, uint64_t seed, int64_t first,
                                 int64_t n, void* xy_out, uint8_t* inside_out, void* r_out) {
    if (!ctx) return WTP_ERR_ARG;
    int rc = check_sample_args(ctx, spacing, factor, seed, true);
    if (rc || (rc = check_dart_range(ctx, first, n))) return rc;
    if (n == 0) return WTP_OK;
    WTP_HIP(ctx, hipSetDevice(ctx->device));
    const SampleDomain dom = loops_domain(ctx);
    return by_dtype(dom.dtype, [&](auto t) {
        using T = decltype(t);
        return sample_darts<T>(ctx, dom, spacing, factor, seed, first, n, true, (T*)xy_out, nullptr, inside_out, (T*)r_out);
    });
}
