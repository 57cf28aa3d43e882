// wtp_stats.hip — the third consumer of the k-NN rows: the reductions of metrics / spacing_metrics /
// spacing_fidelity_metrics (src/metrics.jl:19-129) over the distance rows the topology kernels left in device memory
// (include/wtp.h: wtp_knn_stats).  The n x k matrix is read where it is and never crosses the bus.
//
//   knn_stats_kernel    256 points per block, one per thread.  The block's rows are one contiguous piece of the matrix; it is
//                       loaded in tiles of 256 rows x TK slots (TK slots = 128 bytes of a row: consecutive lanes read
//                       consecutive addresses) into LDS with a row stride of TK + 1 elements, so that thread r then walks
//                       row r without a bank conflict (stride odd in elements: the 32 lanes of a half wave hit 32 banks).
//                       Per point, in double and in slot order: mean, two-pass sample deviation, max, nearest (slot 1),
//                       and with a spacing e = |mean - h| / h, u = nn / h, c = #{d <= coord_radius h}.  Then lane -> wave
//                       (xor butterflies) -> block: one KnnStats per block, its squared deviations of e and u taken
//                       about the block's own means.
//   knn_stats_finish    4096 partials per block into one (16 per thread in order, then a tree in LDS); launched level by
//                       level until one is left.  Partials merge as (count, sum, M2) triples (Chan et al.), never as
//                       sum x^2 - (sum x)^2 / n.
//
// No floating-point atomics and a fixed order everywhere: two calls on one cloud return the same bits.  The longest chain
// of additions is the k - 1 slots of a row (<= 127); across points it is 16 + 8 per level.
#include "wtp_device.hpp"

namespace wtp {

static constexpr int kStatThreads = 256;
static constexpr int kStatFan = 16;                          // partials a finishing thread merges in order
static constexpr int kStatGroup = kStatThreads * kStatFan;   // partials per finishing block

__host__ __device__ inline KnnStats knn_stats_empty() {
    KnnStats s{};
    s.nn_min = __builtin_huge_val();
    s.nn_max = -__builtin_huge_val();
    s.nn_min_i = s.nn_max_i = -1;
    return s;
}

__host__ __device__ inline void knn_stats_merge_into(KnnStats& a, const KnnStats& b) {
    if (b.n == 0) return;
    if (a.n == 0) {
        a = b;
        return;
    }
    const double na = (double)a.n, nb = (double)b.n, w = na * nb / (na + nb);
    const double de = b.sum_err / nb - a.sum_err / na, du = b.sum_u / nb - a.sum_u / na;
    a.ssd_err = (a.ssd_err + b.ssd_err) + de * de * w;
    a.ssd_u = (a.ssd_u + b.ssd_u) + du * du * w;
    a.n += b.n;
    a.sum_mean += b.sum_mean, a.sum_std += b.sum_std, a.sum_max += b.sum_max, a.sum_min += b.sum_min;
    a.sum_err += b.sum_err, a.sum_u += b.sum_u;
    a.sum_coord += b.sum_coord;
    a.max_err = b.max_err > a.max_err ? b.max_err : a.max_err;
    a.has_spacing |= b.has_spacing;
    if (b.nn_min < a.nn_min || (b.nn_min == a.nn_min && b.nn_min_i < a.nn_min_i)) a.nn_min = b.nn_min, a.nn_min_i = b.nn_min_i;
    if (b.nn_max > a.nn_max || (b.nn_max == a.nn_max && b.nn_max_i < a.nn_max_i)) a.nn_max = b.nn_max, a.nn_max_i = b.nn_max_i;
}

void knn_stats_merge(KnnStats& a, const KnnStats& b) { knn_stats_merge_into(a, b); }
KnnStats knn_stats_neutral() { return knn_stats_empty(); }

// sums of N values over the block, in a fixed order, to every thread (sm: N * 4 doubles)
template <int N> __device__ inline void block_sums(double (&v)[N], double* sm) {
#pragma unroll
    for (int i = 0; i < N; ++i)
        for (int m = 32; m > 0; m >>= 1) v[i] = v[i] + __shfl_xor(v[i], m);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < N; ++i) sm[wave * N + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ((sm[i] + sm[N + i]) + sm[2 * N + i]) + sm[3 * N + i];
    __syncthreads();
}

// extreme of (v, i) over the block to every thread: the smallest v (sign = +1) or the largest (sign = -1), ties to the
// smaller i (sm: 4 doubles, smi: 4 indices)
__device__ inline void block_extreme(double& v, long long& i, bool want_min, double* sm, long long* smi) {
    auto better = [&](double ov, long long oi) { return (want_min ? ov < v : ov > v) || (ov == v && oi < i); };
    for (int m = 32; m > 0; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        const long long oi = __shfl_xor(i, m);
        if (better(ov, oi)) v = ov, i = oi;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sm[wave] = v, smi[wave] = i;
    __syncthreads();
    v = sm[0], i = smi[0];
    for (int w = 1; w < kStatThreads / 64; ++w)
        if (better(sm[w], smi[w])) v = sm[w], i = smi[w];
    __syncthreads();
}

template <typename T>
__global__ void __launch_bounds__(kStatThreads)
knn_stats_kernel(const T* __restrict__ dist, int64_t n, int k, const double* __restrict__ h, double h_const, int has_spacing,
                 double coord_radius, const int64_t* __restrict__ gid, T* __restrict__ nn_out, double* __restrict__ mean_out,
                 KnnStats* __restrict__ parts, unsigned long long* __restrict__ bad_h) {
    constexpr int TK = 128 / (int)sizeof(T); // slots per tile: 128 bytes of a row
    constexpr int LD = TK + 1;               // LDS row stride (elements)
    __shared__ T tile[kStatThreads * LD];
    __shared__ double sm[6 * (kStatThreads / 64)];
    __shared__ long long smi[kStatThreads / 64];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * kStatThreads;
    const int64_t i = i0 + tid;
    const bool live = i < n;
    const int ke = k - 1;                    // slots 1 .. k - 1: slot 0 is the point itself (or a twin at distance 0)
    const int ntiles = (ke + TK - 1) / TK;

    double hi = 1.0;
    bool h_ok = true;
    if (has_spacing && live) {
        hi = h ? h[i] : h_const;
        h_ok = hi > 0.0 && hi <= 1.79769313486231570815e308; // finite and > 0 (NaN fails both)
        if (!h_ok) atomicMin(bad_h, (unsigned long long)i);
    }
    const double reach = coord_radius * hi;

    double sum = 0.0, mx = 0.0, nn = 0.0, mean = 0.0, ssd = 0.0;
    long long coord = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int t = 0; t < ntiles; ++t) {
            const int s0 = 1 + t * TK;
            if (pass == 0 || ntiles > 1) { // (a single tile stays in LDS for the second pass)
                __syncthreads();
#pragma unroll 4
                for (int m = 0; m < TK; ++m) {
                    const int e = m * kStatThreads + tid;
                    const int r = e / TK, j = e % TK;
                    if (i0 + r < n && s0 + j < k) tile[r * LD + j] = dist[(i0 + r) * k + s0 + j];
                }
                __syncthreads();
            }
            if (live) {
                const int len = k - s0 < TK ? k - s0 : TK;
                const T* row = tile + tid * LD;
                if (pass == 0) {
                    if (t == 0) nn = (double)row[0], mx = nn;
                    for (int j = 0; j < len; ++j) {
                        const double d = (double)row[j];
                        sum = sum + d;
                        mx = d > mx ? d : mx;
                        coord += d <= reach ? 1 : 0;
                    }
                } else {
                    for (int j = 0; j < len; ++j) {
                        const double d = (double)row[j] - mean;
                        ssd = ssd + d * d;
                    }
                }
            }
        }
        if (pass == 0) mean = sum / (double)ke;
    }
    const double sd = wsqrt(ssd / (double)(ke - 1)); // k_eff = 1: 0 / 0 = NaN, as Julia's std of one value
    if (live) {
        if (nn_out) nn_out[i] = (T)nn; // (exact: nn came from a T)
        if (mean_out) mean_out[i] = mean;
    }

    const bool sp = has_spacing && live && h_ok;
    double dev = mean - hi;
    dev = dev < 0 ? -dev : dev;
    const double e = sp ? dev / hi : 0.0, u = sp ? nn / hi : 0.0;

    double v[6] = {live ? mean : 0.0, live ? sd : 0.0, live ? mx : 0.0, live ? nn : 0.0, e, u};
    block_sums<6>(v, sm);
    const int64_t cnt = n - i0 < kStatThreads ? n - i0 : kStatThreads;
    // squared deviations about the block's own means
    const double me = v[4] / (double)cnt, mu = v[5] / (double)cnt;
    double q[2] = {sp ? (e - me) * (e - me) : 0.0, sp ? (u - mu) * (u - mu) : 0.0};
    block_sums<2>(q, sm);
    const long long id = live ? (gid ? (long long)gid[i] : (long long)i) : 0x7fffffffffffffffLL;
    double lo = live ? nn : __builtin_huge_val(), hi_nn = live ? nn : -__builtin_huge_val(), emax = e;
    long long lo_i = id, hi_i = id, e_i = id;
    block_extreme(lo, lo_i, true, sm, smi);
    block_extreme(hi_nn, hi_i, false, sm, smi);
    block_extreme(emax, e_i, false, sm, smi);
    // sum of the counts: integers, any order gives the same sum
    long long c = sp ? coord : 0;
    for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
    if ((tid & 63) == 0) smi[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        KnnStats s{};
        s.n = cnt;
        s.k_eff = ke;
        s.has_spacing = has_spacing ? 1 : 0;
        s.sum_mean = v[0], s.sum_std = v[1], s.sum_max = v[2], s.sum_min = v[3];
        s.nn_min = lo, s.nn_min_i = lo_i, s.nn_max = hi_nn, s.nn_max_i = hi_i;
        s.sum_err = v[4], s.ssd_err = q[0], s.max_err = emax;
        s.sum_u = v[5], s.ssd_u = q[1];
        s.sum_coord = (smi[0] + smi[1]) + (smi[2] + smi[3]);
        parts[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(kStatThreads)
knn_stats_finish_kernel(const KnnStats* __restrict__ in, int64_t m, KnnStats* __restrict__ out) {
    __shared__ KnnStats s[kStatThreads];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * kStatGroup + (int64_t)tid * kStatFan;
    KnnStats a = knn_stats_empty();
    for (int j = 0; j < kStatFan; ++j)
        if (first + j < m) knn_stats_merge_into(a, in[first + j]);
    s[tid] = a;
    __syncthreads();
    for (int stride = kStatThreads / 2; stride > 0; stride >>= 1) {
        if (tid < stride) {
            KnnStats x = s[tid];
            knn_stats_merge_into(x, s[tid + stride]);
            s[tid] = x;
        }
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = s[0];
}

size_t knn_stats_tmp_bytes(int64_t n) {
    const int64_t nb = (n + kStatThreads - 1) / kStatThreads;
    const int64_t l1 = (nb + kStatGroup - 1) / kStatGroup;
    return sizeof(KnnStats) * (size_t)(nb + l1 + 2) + 64;
}

// d_tmp: knn_stats_tmp_bytes(n).  The result lands in d_tmp as one KnnStats at *d_result_out, behind it (8 bytes) the
// smallest index whose spacing is not finite and > 0 (all ones: none) at *d_bad_out.  n >= 1, k >= 2.
template <typename T>
int launch_knn_stats(wtp_ctx* ctx, const T* d_dist, int64_t n, int k, const double* d_h, double h_const, int has_spacing,
                     double coord_radius, const int64_t* d_gid, T* d_nn_out, double* d_mean_out, void* d_tmp,
                     const KnnStats** d_result_out, const unsigned long long** d_bad_out) {
    const int64_t nb = (n + kStatThreads - 1) / kStatThreads;
    const int64_t l1 = (nb + kStatGroup - 1) / kStatGroup;
    KnnStats* a = (KnnStats*)d_tmp;          // nb partials, later the third level's
    KnnStats* b = a + nb;                         // l1 partials
    KnnStats* fin = b + l1;                       // the result
    unsigned long long* bad = (unsigned long long*)(fin + 1);
    WTP_HIP(ctx, hipMemsetAsync(bad, 0xFF, 8, ctx->stream));
    hipLaunchKernelGGL(knn_stats_kernel<T>, dim3((unsigned)nb), dim3(kStatThreads), 0, ctx->stream, d_dist, n, k, d_h, h_const,
                       has_spacing, coord_radius, d_gid, d_nn_out, d_mean_out, a, bad);
    // level by level: nb -> l1 -> ... -> 1 (two buffers in turn; a level's output is shorter than the space it overwrites)
    const KnnStats* src = a;
    int64_t m = nb;
    bool into_b = true;
    do {
        const int64_t mo = (m + kStatGroup - 1) / kStatGroup;
        KnnStats* dst = mo == 1 ? fin : (into_b ? b : a);
        hipLaunchKernelGGL(knn_stats_finish_kernel, dim3((unsigned)mo), dim3(kStatThreads), 0, ctx->stream, src, m, dst);
        src = dst;
        m = mo;
        into_b = !into_b;
    } while (m > 1);
    WTP_HIP(ctx, hipGetLastError());
    *d_result_out = fin;
    *d_bad_out = bad;
    return WTP_OK;
}

#define INST(T)                                                                                                          \
    template int launch_knn_stats<T>(wtp_ctx*, const T*, int64_t, int, const double*, double, int, double, const int64_t*, T*, \
                                     double*, void*, const KnnStats**, const unsigned long long**);
INST(float)
INST(double)
#undef INST

} // namespace wtp
