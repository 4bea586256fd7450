// Ranking metrics from the ranks the device already holds (reference evaluation.py:94-164 with rank_metrics_with_std.py: mrr, map,
// p; eval/mpd/mpd_metrics.py:43-144: r-precision, ndcg, playlist-extender clicks).  Every one of them is a function of a row's
// held-out ranks in ascending order, r_1 <= r_2 <= ... <= r_m, and the cap k alone:
//
//   mrr[@k]    1 / r_1 if r_1 <= k, else 0
//   map[@k]    (sum_{j <= h} fl(j / r_j)) / h,  h = #{r_j <= k}; 0 if h = 0
//   p@k        h / k
//   ndcg@k     (sum_{j <= h} d[r_j]) / (sum_{i = 1 .. min(k, m)} d[i]),  d the caller's table (d[i] at index i - 1)
//   r-prec@k   #{r_j <= min(m, k)} / m
//   clicks@k   floor((r_1 - 1) / 10) if r_1 <= k, else k / 10 + 1
//
// k = 0 is "unbounded" (mrr, map only): every stored rank counts.  A row without entries scores 0, clicks@k = k / 10 + 1.
// A stored rank kRankAbsent (INT32_MAX) is "not retrieved": it counts towards m and satisfies no r <= k, unbounded included.
// A row with a rank below 1, or longer than kMetricRowMax, is NaN in every metric.
//
//   metric_rows_kernel    kMetricRows rows per workgroup, one wavefront each.  Entries order by (rank, position in the row) - the
//                         stable order of the host's lexsort - as one 64-bit key.  A row of up to 64 entries is ranked in
//                         registers (a lane counts the keys below its own over 64 shuffles) and written to the wave's 64 LDS
//                         slots in order.  A longer row is sorted by the whole workgroup in LDS (bitonic, padded to a power of
//                         two with the largest key: 4096 keys = 32 KB) one row after the other, and wave 0 evaluates it.
//   metric_finish_kernel  one workgroup per metric: mean, then the mean of the squared deviations, then sqrt - two passes, each a
//                         strided partial sum per thread and one LDS tree.
//   ranks_from_lists_kernel  the bridge from [n, K] lists (best first, -1 padding) to ranks: one wavefront per row; a list id is
//                         looked up among the row's ascending truth ids (binary search) and its position + 1 goes to that truth
//                         entry by an int32 atomicMin - a duplicated id keeps its smaller position; the rest stays kRankAbsent.
//
// ARITHMETIC: h, m and every count are integers.  Each sum runs in ascending j, one term after the other, the same on every
// lane of the evaluating wave - no tree, no atomics: the bits do not depend on the launch.  The kernel takes no logarithm.
// BOUNDS: a row's length is checked against kMetricRowMax before LDS is indexed; the sort indexes [0, P), P <= kMetricRowMax;
// the table is read at r_j - 1 < k and at i - 1 < min(k, m), and the caller has k <= the table's length checked on the host.
#pragma once
#include <math.h>

#include "popular.h"

namespace aae {

constexpr int kMetricNT = 256;                  // threads of every workgroup here
constexpr int kMetricRows = kMetricNT / 64;     // rows of a workgroup: one wavefront each
constexpr int kMetricRowMax = 4096;             // longest row (AAE_METRIC_ROW_MAX): 4096 keys of 8 bytes = 32 KB of LDS
constexpr int kMetricMax = 32;                  // most specs of one call (AAE_METRIC_MAX)
constexpr int kRankAbsent = 2147483647;         // AAE_RANK_ABSENT
enum { kMetMRR = 0, kMetMAP = 1, kMetP = 2, kMetNDCG = 3, kMetRPrec = 4, kMetClicks = 5, kMetKinds = 6 };

struct MetricSpecs { int n; int kind[kMetricMax]; int k[kMetricMax]; };
// indptr [n_rows + 1], ranks in CSR order; disc [n_disc]; out [n][ld]
struct MetricRowsArgs {
    const int64_t* indptr; const int32_t* ranks; int n_rows;
    const double* disc; int n_disc;
    double* out; long long ld;
};

__device__ __forceinline__ unsigned long long metric_key(int rank, int pos) {
    return ((unsigned long long)(unsigned)rank << 32) | (unsigned)pos;
}
__device__ __forceinline__ int metric_rank_of(unsigned long long key) { return (int)(unsigned)(key >> 32); }

// #{entries of the sorted keys [0, m) whose rank is <= k}: they are its first ones.  Never counts kRankAbsent
__device__ __forceinline__ int metric_hits(const unsigned long long* s, int m, int k) {
    const int cap = (k <= 0 || k >= kRankAbsent) ? kRankAbsent - 1 : k;
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (metric_rank_of(s[mid]) <= cap) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// sum_{j = 1 .. h} term(j) in ascending j on every lane of the wave alike: 64 terms are formed at a time, one per lane, and
// added one after the other from a shuffle
template <class Term>
__device__ __forceinline__ double metric_seq_sum(int h, int lane, Term term) {
    double acc = 0.0;
    for (int base = 0; base < h; base += 64) {
        const int j = base + lane + 1;
        const double t = j <= h ? term(j) : 0.0;
        const int n = h - base < 64 ? h - base : 64;
        for (int i = 0; i < n; ++i) acc += __shfl(t, i, 64);
    }
    return acc;
}

// every metric of one row from its sorted keys s[0, m) (LDS), by one wavefront; lane 0 writes
__device__ __forceinline__ void metric_eval_row(const unsigned long long* s, int m, bool bad, const MetricSpecs& sp,
                                                const MetricRowsArgs& a, long long row, int lane) {
    const int r1 = m > 0 ? metric_rank_of(s[0]) : kRankAbsent;
    for (int q = 0; q < sp.n; ++q) {
        const int kind = sp.kind[q], k = sp.k[q];
        double v = 0.0;
        if (bad) {
            v = __builtin_nan("");
        } else if (kind == kMetClicks) {
            const bool in = m > 0 && r1 != kRankAbsent && r1 <= k;
            v = in ? (double)((r1 - 1) / 10) : (double)k / 10.0 + 1.0;
        } else if (m > 0) {
            if (kind == kMetMRR) {
                const bool in = r1 != kRankAbsent && (k <= 0 || r1 <= k);
                v = in ? 1.0 / (double)r1 : 0.0;
            } else if (kind == kMetP) {
                v = (double)metric_hits(s, m, k) / (double)k;
            } else if (kind == kMetRPrec) {
                v = (double)metric_hits(s, m, m < k ? m : k) / (double)m;
            } else if (kind == kMetMAP) {
                const int h = metric_hits(s, m, k);
                if (h > 0) {
                    const double sum = metric_seq_sum(h, lane, [&](int j) { return (double)j / (double)metric_rank_of(s[j - 1]); });
                    v = sum / (double)h;
                }
            } else if (kind == kMetNDCG) {
                const int h = metric_hits(s, m, k);
                if (h > 0) {
                    const double* d = a.disc;
                    const double num = metric_seq_sum(h, lane, [&](int j) { return d[metric_rank_of(s[j - 1]) - 1]; });
                    const double den = metric_seq_sum(m < k ? m : k, lane, [&](int i) { return d[i - 1]; });
                    v = num / den;
                }
            }
        }
        if (lane == 0) a.out[(long long)q * a.ld + row] = v;
    }
}

__global__ __launch_bounds__(kMetricNT) void metric_rows_kernel(MetricRowsArgs a, MetricSpecs sp) {
    __shared__ unsigned long long s_long[kMetricRowMax];
    __shared__ unsigned long long s_short[kMetricRows][64];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * kMetricRows;

    // ---- rows of up to 64 entries: one wavefront each
    const long long row = row0 + wave;
    long long lo = 0, len = 0;
    if (row < a.n_rows) { lo = a.indptr[row]; len = a.indptr[row + 1] - lo; }
    if (len < 0) len = 0;
    const bool is_short = row < a.n_rows && len <= 64;
    bool bad_short = false;
    if (is_short) {
        const int m = (int)len;
        const int r = lane < m ? a.ranks[lo + lane] : kRankAbsent;
        const unsigned long long key = lane < m ? metric_key(r, lane) : ~0ull;
        bad_short = __ballot(lane < m && r < 1) != 0ull;
        int below = 0;
        for (int i = 0; i < 64; ++i) below += __shfl(key, i, 64) < key ? 1 : 0;          // (keys differ: the position is in them)
        if (lane < m) s_short[wave][below] = key;
    }
    __syncthreads();
    if (is_short) metric_eval_row(s_short[wave], (int)len, bad_short, sp, a, row, lane);

    // ---- longer rows: the whole workgroup sorts one after the other (every condition below is the same on all threads)
    for (int w = 0; w < kMetricRows; ++w) {
        const long long rw = row0 + w;
        if (rw >= a.n_rows) break;
        const long long lw = a.indptr[rw];
        const long long mw = a.indptr[rw + 1] - lw;
        if (mw <= 64) continue;
        if (mw > kMetricRowMax) {                                    // never indexes LDS: NaN everywhere
            if (wave == 0) metric_eval_row(s_long, 0, true, sp, a, rw, lane);
            continue;
        }
        const int m = (int)mw;
        int P = 128;
        while (P < m) P <<= 1;                                       // (P <= kMetricRowMax: m <= kMetricRowMax, a power of two)
        if (tid == 0) s_bad = 0;
        __syncthreads();
        int bad = 0;
        for (int e = tid; e < P; e += kMetricNT) {
            const int r = e < m ? a.ranks[lw + e] : kRankAbsent;
            bad |= (e < m && r < 1) ? 1 : 0;
            s_long[e] = e < m ? metric_key(r, e) : ~0ull;
        }
        if (bad) s_bad = 1;
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (P >> 1); t += kMetricNT) {
                    const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));       // (i < P - stride, i + stride < P)
                    const int j = i + stride;
                    const bool up = (i & size) == 0;
                    const unsigned long long x = s_long[i], y = s_long[j];
                    if ((x > y) == up) { s_long[i] = y; s_long[j] = x; }
                }
                __syncthreads();
            }
        }
        const bool row_bad = s_bad != 0;
        if (wave == 0) metric_eval_row(s_long, m, row_bad, sp, a, rw, lane);
        __syncthreads();                                             // (the next long row rewrites s_long and s_bad)
    }
}

// mean and population standard deviation of the n doubles of each metric's row of `per_row` [metrics][ld] -> out [metrics][2].
// n = 0 gives NaN, as np.mean of nothing
__device__ __forceinline__ double metric_block_sum(double v, double* s_red, int tid) {
    s_red[tid] = v;
    __syncthreads();
    for (int o = kMetricNT >> 1; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    const double total = s_red[0];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(kMetricNT) void metric_finish_kernel(const double* __restrict__ per_row, long long ld, int n,
                                                                  double* __restrict__ out) {
    __shared__ double s_red[kMetricNT];
    const int tid = threadIdx.x;
    const double* x = per_row + (long long)blockIdx.x * ld;
    double acc = 0.0;
    for (int i = tid; i < n; i += kMetricNT) acc += x[i];
    const double mean = metric_block_sum(acc, s_red, tid) / (double)n;
    acc = 0.0;
    for (int i = tid; i < n; i += kMetricNT) { const double d = x[i] - mean; acc += d * d; }
    const double var = metric_block_sum(acc, s_red, tid) / (double)n;
    if (tid == 0) { out[2 * blockIdx.x] = mean; out[2 * blockIdx.x + 1] = sqrt(var); }
}

// ids [n_rows][ld], the first K of a row its list; tv the canonical truth rows (ascending ids); out in the call's CSR order
__global__ __launch_bounds__(kMetricNT) void ranks_from_lists_kernel(const int32_t* __restrict__ ids, long long ld, int K, BatchView tv,
                                                                     int* __restrict__ ranks_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kMetricRows + (threadIdx.x >> 6);
    if (row >= tv.n_rows) return;                                   // (a whole wavefront: nothing here meets at a barrier)
    const int dt = tv.doc((int)row);
    const int64_t tlo = tv.indptr[dt], thi = tv.indptr[dt + 1];
    if (tlo >= thi) return;
    int* out = ranks_out + pop_truth_offset(tv, row, lane);
    for (int64_t e = tlo + lane; e < thi; e += 64) __hip_atomic_store(&out[e - tlo], kRankAbsent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the wave's own stores are complete before its atomics on the same words start
    __threadfence();
    __builtin_amdgcn_wave_barrier();
    const int32_t* list = ids + row * ld;
    for (int p = lane; p < K; p += 64) {
        const int id = list[p];
        if (id < 0) continue;
        const int64_t at = pop_lower_bound(tv.indices, tlo, thi, id);
        if (at < thi && tv.indices[at] == id) atomicMin(&out[at - tlo], p + 1);
    }
}

}  // namespace aae
