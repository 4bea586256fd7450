// The random baseline (reference baselines.py:7-19, RandomBaseline: predict = rand(rows, items)) from the library's keyed
// generator, so that a seed determines the floor line under every table of results.  A score is never stored:
//
//   key    = rng_key(seed, draw, 0) ^ 15 * 0xA0761D6478BD642F          stream 15 of the generator (device_common.h)
//   s(r,j) = hash_cell(key, r, j) >> (32 - bits)                       an integer in [0, 2^bits), bits in [1, 24]
//   score  = s * 2^-bits                                               exact in fp32
//
// r is the row's index in the WHOLE test set (row0 + the row of the call): chunking the rows of a call changes nothing.
// The ordering is the library's one rule (rank_long.h / rank_full.h): the larger s first, the smaller id at equal s, known
// items left out.  Equal s are common (24-bit values over 100 000 items tie in nearly every row), and the integer order is the
// fp32 order of the scores, so lists and ranks are exact.
//
//   rand_scores_kernel  the dense fp32 block, for predict() and the tests.
//   rand_topk_kernel    one workgroup per row, every thread a contiguous range of the items.  An exact two-level radix select
//                       over the bits-bit values, the draws regenerated on every pass: (1) a histogram of the top 12 bits of the
//                       unknown items and the row's min / max over ALL items; (2) a histogram of the remaining bits inside the
//                       floor bin - the threshold t is then the k-th largest value among the unknown items; (3) every unknown
//                       item with s > t is collected (fewer than k) and a thread counts its items with s == t; (4) a prefix
//                       sum over the threads hands the ties their places in ascending id until the list holds k.  The k pairs
//                       are sorted in LDS (bitonic, (s descending, id ascending) packed into 64 bits).  The candidate buffer is
//                       bounded by k itself.  A row with fewer than k unknown items takes them all and ends in id -1 / score 0.
//   rand_ranks_kernel   one workgroup per row.  The row's held-out draws are sorted in LDS by (s descending, id ascending);
//                       every thread generates its range of the items, finds by binary search how many held-out entries an
//                       unknown item is ordered before, and adds to a counter there; an inclusive prefix sum over the counters
//                       is, per held-out entry, the number of unknown items ordered before it.  A known held-out item ranks
//                       behind every rankable one, among the known items by id; an id outside [0, n_items) ranks 0 (popular.h).
//                       A row of more than `cap` held-out entries (the caller's power of two, at most kRandTruthMax) ranks 0
//                       throughout - the entry point refuses what it can see of that before the launch.
//
// Known items are masked by a merge: a thread's items ascend, so a cursor into the row's ascending ids (one binary search per
// pass) only ever moves forward.  Scaled scores: (score - min) * inv, span = max - min, inv = span > 0 ? 1 / span : 1 in fp32,
// the formula of popular.h over the scores.  CONTRACT (the caller's, as in every dense ranking call): the ids of a batch row lie
// in [0, n_items) and ascend without duplicates.  Every loop is bounded by n_items, a row's length, k or cap.
// No float atomics, no inline assembly: integer LDS atomics, plain loads, vector stores, wave shuffles.
#pragma once
#include "popular.h"

namespace aae {

constexpr int kRandNT = 256;                 // threads of every workgroup here
constexpr int kRandBins = 4096;              // counters of a histogram: 12 bits per level, two levels cover bits <= 24
constexpr int kRandKMax = 1024;              // longest list
constexpr int kRandTruthMax = 4096;          // most held-out entries of a row
constexpr int kRandScoreRows = 1024;         // grid.y of the score kernel: the rows stride over it

struct RandArgs { uint64_t seed; uint64_t draw; uint32_t row0; int bits; int n_items; };

__device__ __forceinline__ uint64_t rand_key(const RandArgs& A) { return rng_key(A.seed, A.draw, 0) ^ (15ull * 0xA0761D6478BD642Full); }
__device__ __forceinline__ uint32_t rand_value(uint64_t key, uint32_t r, int j, int bits) {
    return hash_cell(key, r, (uint32_t)j) >> (32 - bits);
}
// (s descending, id ascending) as one ascending 64-bit key; top = 2^bits - 1.  ~0 orders behind every key
__device__ __forceinline__ unsigned long long rand_pack(uint32_t top, uint32_t s, int j) {
    return ((unsigned long long)(top - s) << 32) | (unsigned long long)(uint32_t)j;
}

// the items [lo, hi) of thread `tid`: contiguous, ascending with the thread
__device__ __forceinline__ void rand_range(int n, int tid, int& lo, int& hi) {
    const int64_t per = ((int64_t)n + kRandNT - 1) / kRandNT;
    const int64_t a = (int64_t)tid * per, b = a + per;
    lo = (int)(a < n ? a : n); hi = (int)(b < n ? b : n);
}

// a cursor into the ascending ids [lo, hi) of a row for queries that ascend
struct RandKnown {
    const int32_t* ids; int64_t p, hi; int cur;
    __device__ __forceinline__ RandKnown(const int32_t* ids_, int64_t lo, int64_t hi_, int first) : ids(ids_), hi(hi_) {
        p = pop_lower_bound(ids, lo, hi, first);
        cur = p < hi ? ids[p] : 0x7FFFFFFF;
    }
    __device__ __forceinline__ bool has(int j) {
        while (cur < j) { ++p; cur = p < hi ? ids[p] : 0x7FFFFFFF; }
        return cur == j;
    }
};

// exclusive prefix sum of v over the workgroup's threads, and the total; wsum: kRandNT / 64 ints of LDS.  Every thread calls it
__device__ __forceinline__ int rand_scan(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    __syncthreads();                                             // (the sums of an earlier call have been read)
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int off = 0; total = 0;
#pragma unroll
    for (int i = 0; i < kRandNT / 64; ++i) { const int s = wsum[i]; if (i < w) off += s; total += s; }
    return off + inc - v;
}

// the bin b of hist[kRandBins] with above = #{entries in bins > b} < need <= above + hist[b]: sel[0] = b, sel[1] = above;
// sel[0] = -1, sel[1] = the total when the histogram holds fewer than `need` entries.  Every thread calls it; hist is complete
__device__ __forceinline__ void rand_floor_bin(const int* hist, int need, int* wsum, int* sel) {
    constexpr int per = kRandBins / kRandNT;
    const int top = kRandBins - 1 - (int)threadIdx.x * per;    // a thread's bins descend from here: thread 0 holds the largest values
    int v = 0;
#pragma unroll
    for (int i = 0; i < per; ++i) v += hist[top - i];
    int total;
    const int excl = rand_scan(v, wsum, total);
    if (threadIdx.x == 0) { sel[0] = -1; sel[1] = total; }
    __syncthreads();
    if (excl < need && need <= excl + v) {                      // (one thread at most)
        int a = excl;
        for (int i = 0; i < per; ++i) {
            const int c = hist[top - i];
            if (a + c >= need) { sel[0] = top - i; sel[1] = a; break; }
            a += c;
        }
    }
    __syncthreads();
}

// ascending bitonic sort of keys[P], P a power of two; every thread calls it
__device__ __forceinline__ void rand_sort(unsigned long long* keys, int P) {
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < (P >> 1); i += kRandNT) {
                const int a = 2 * i - (i & (stride - 1)), b = a + stride;
                const unsigned long long x = keys[a], y = keys[b];
                if ((x > y) == ((a & size) == 0)) { keys[a] = y; keys[b] = x; }
            }
        }
    __syncthreads();
}

__global__ __launch_bounds__(kRandNT) void rand_scores_kernel(RandArgs A, int n_rows, float* __restrict__ out, long long ld) {
    const int64_t col = (int64_t)blockIdx.x * kRandNT + threadIdx.x;
    if (col >= A.n_items) return;
    const int j = (int)col;
    const uint64_t key = rand_key(A);
    const float scale = 1.f / (float)(1u << A.bits);
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y)
        out[(size_t)r * ld + j] = (float)rand_value(key, A.row0 + (uint32_t)r, j, A.bits) * scale;
}

__global__ __launch_bounds__(kRandNT) void rand_topk_kernel(RandArgs A, BatchView kv, int exclude_known, int k,
                                                            int* __restrict__ idx_out, float* __restrict__ val_out) {
    __shared__ int hist[kRandBins];
    __shared__ unsigned long long cand[kRandKMax];
    __shared__ int wsum[kRandNT / 64];
    __shared__ int sel[2];
    __shared__ unsigned ends[2];                                 // the row's smallest and largest value, over all items
    __shared__ int n_above;
    const int tid = threadIdx.x, row = blockIdx.x;
    const int n = A.n_items, bits = A.bits;
    const uint64_t key = rand_key(A);
    const uint32_t r = A.row0 + (uint32_t)row, top = (1u << bits) - 1u;
    const int low = bits > 12 ? bits - 12 : 0;                   // the bits the second histogram refines
    const uint32_t low_mask = (1u << low) - 1u;
    int64_t klo = 0, khi = 0;
    if (exclude_known) { const int dc = kv.doc(row); klo = kv.indptr[dc]; khi = kv.indptr[dc + 1]; }
    int lo, hi;
    rand_range(n, tid, lo, hi);

    // (1) the top 12 bits of the unknown items; min / max over all items
    for (int i = tid; i < kRandBins; i += kRandNT) hist[i] = 0;
    if (tid == 0) { ends[0] = 0xFFFFFFFFu; ends[1] = 0u; n_above = 0; }
    __syncthreads();
    {
        uint32_t smin = 0xFFFFFFFFu, smax = 0u;
        RandKnown kn(kv.indices, klo, khi, lo);
        for (int j = lo; j < hi; ++j) {
            const uint32_t s = rand_value(key, r, j, bits);
            smin = s < smin ? s : smin; smax = s > smax ? s : smax;
            if (!kn.has(j)) atomicAdd(&hist[s >> low], 1);
        }
        if (lo < hi) { atomicMin(&ends[0], smin); atomicMax(&ends[1], smax); }
    }
    __syncthreads();
    rand_floor_bin(hist, k, wsum, sel);
    const int b1 = sel[0];
    const bool all = b1 < 0;                                     // fewer than k unknown items: every one of them is listed
    int above = sel[1];                                          // (all: the number of unknown items)
    uint32_t t = all ? 0u : (uint32_t)b1;
    __syncthreads();                                             // (sel is rewritten below)
    // (2) the remaining bits inside the floor bin
    if (!all && low > 0) {
        for (int i = tid; i < kRandBins; i += kRandNT) hist[i] = 0;
        __syncthreads();
        RandKnown kn(kv.indices, klo, khi, lo);
        for (int j = lo; j < hi; ++j) {
            const uint32_t s = rand_value(key, r, j, bits);
            if ((s >> low) == (uint32_t)b1 && !kn.has(j)) atomicAdd(&hist[s & low_mask], 1);
        }
        __syncthreads();
        rand_floor_bin(hist, k - above, wsum, sel);               // (the bin holds at least k - above entries: always found)
        t = ((uint32_t)b1 << low) | (uint32_t)(sel[0] < 0 ? 0 : sel[0]);
        above += sel[0] < 0 ? 0 : sel[1];
    }
    const int count = all ? above : k;                           // entries of the list
    const int need = all ? 0 : k - above;                        // ties at t the list takes, in ascending id
    // (3) collect the items above t; count a thread's ties
    int ties = 0;
    {
        RandKnown kn(kv.indices, klo, khi, lo);
        for (int j = lo; j < hi; ++j) {
            const uint32_t s = rand_value(key, r, j, bits);
            if ((all || s >= t) && !kn.has(j)) {
                if (all || s > t) {
                    const int p = atomicAdd(&n_above, 1);
                    if (p < kRandKMax) cand[p] = rand_pack(top, s, j);
                } else {
                    ++ties;
                }
            }
        }
    }
    int total_ties;
    int place = rand_scan(ties, wsum, total_ties);
    // (4) the ties in ascending id: a thread's range lies behind the ranges of the threads before it
    if (ties > 0 && place < need) {
        RandKnown kn(kv.indices, klo, khi, lo);
        for (int j = lo; j < hi && place < need; ++j) {
            const uint32_t s = rand_value(key, r, j, bits);
            if (s == t && !kn.has(j)) {
                const int p = above + place++;
                if (p < kRandKMax) cand[p] = rand_pack(top, s, j);
            }
        }
    }
    __syncthreads();
    int P = 1;
    while (P < count) P <<= 1;
    for (int i = count + tid; i < P; i += kRandNT) cand[i] = ~0ull;
    rand_sort(cand, P);

    const float scale = 1.f / (float)(1u << bits);
    const float fmin_ = (float)ends[0] * scale;
    const float span = (float)ends[1] * scale - fmin_;
    const float inv = span > 0.f ? 1.f / span : 1.f;
    int* idx = idx_out + (size_t)row * k;
    float* val = val_out ? val_out + (size_t)row * k : nullptr;
    for (int p = tid; p < k; p += kRandNT) {
        int id = -1; float v = 0.f;
        if (p < count) {
            const unsigned long long c = cand[p];
            id = (int)(uint32_t)c;
            v = ((float)(top - (uint32_t)(c >> 32)) * scale - fmin_) * inv;
        }
        idx[p] = id;
        if (val) val[p] = v;
    }
}

// bytes of dynamic LDS of rand_ranks_kernel for rows of up to `cap` held-out entries: the keys, cap + 1 counters, the scan's sums
inline size_t rand_ranks_lds_bytes(int cap) { return (size_t)cap * 8 + ((size_t)cap + 1 + kRandNT / 64) * 4; }

__global__ __launch_bounds__(kRandNT) void rand_ranks_kernel(RandArgs A, BatchView kv, BatchView tv, int exclude_known, int cap,
                                                             int* __restrict__ ranks_out) {
    extern __shared__ __align__(16) unsigned char rand_lds[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(rand_lds);     // [cap]: the held-out entries, best first
    int* cnt = reinterpret_cast<int*>(keys + cap);                                  // [cap + 1]
    int* wsum = cnt + cap + 1;                                                      // [kRandNT / 64]
    const int tid = threadIdx.x, row = blockIdx.x;
    const int n = A.n_items, bits = A.bits;
    const int dt = tv.doc(row);
    const int64_t tlo = tv.indptr[dt], thi = tv.indptr[dt + 1];
    if (tlo >= thi) return;                                      // (the whole workgroup: nothing below meets at a barrier)
    const long long off = pop_truth_offset(tv, row, tid & 63);
    if (thi - tlo > cap) {                                       // (the caller's bound did not hold: nothing is ranked)
        for (int64_t e = tid; e < thi - tlo; e += kRandNT) ranks_out[off + e] = 0;
        return;
    }
    const int T = (int)(thi - tlo);
    const uint64_t key = rand_key(A);
    const uint32_t r = A.row0 + (uint32_t)row, top = (1u << bits) - 1u;
    int64_t klo = 0, khi = 0;
    if (exclude_known) { const int dc = kv.doc(row); klo = kv.indptr[dc]; khi = kv.indptr[dc + 1]; }

    // the rankable held-out entries, sorted; everything else orders behind them and counts nothing
    for (int e = tid; e < cap; e += kRandNT) {
        unsigned long long q = ~0ull;
        if (e < T) {
            const int t = tv.indices[tlo + e];
            if (t >= 0 && t < n) {
                const int64_t at = pop_lower_bound(kv.indices, klo, khi, t);
                if (!(at < khi && kv.indices[at] == t)) q = rand_pack(top, rand_value(key, r, t, bits), t);
            }
        }
        keys[e] = q;
    }
    for (int e = tid; e <= cap; e += kRandNT) cnt[e] = 0;
    rand_sort(keys, cap);

    // an unknown item is ordered before the held-out entries from the first key above its own on (never before itself)
    {
        int lo, hi;
        rand_range(n, tid, lo, hi);
        RandKnown kn(kv.indices, klo, khi, lo);
        for (int j = lo; j < hi; ++j) {
            if (kn.has(j)) continue;
            const unsigned long long q = rand_pack(top, rand_value(key, r, j, bits), j);
            int a = 0, b = cap;
            while (a < b) { const int mid = (a + b) >> 1; if (keys[mid] <= q) a = mid + 1; else b = mid; }
            atomicAdd(&cnt[a], 1);
        }
    }
    __syncthreads();
    // inclusive prefix sum over the counters: a thread owns `per` neighbours
    {
        const int per = cap >= kRandNT ? cap / kRandNT : 1;
        const int first = tid * per;
        int v = 0;
        if (first < cap) for (int i = 0; i < per; ++i) v += cnt[first + i];
        int total;
        int a = rand_scan(v, wsum, total);
        if (first < cap) for (int i = 0; i < per; ++i) { a += cnt[first + i]; cnt[first + i] = a; }
    }
    __syncthreads();
    const int m = (int)(khi - klo);
    for (int e = tid; e < T; e += kRandNT) {
        const int t = tv.indices[tlo + e];
        int rank = 0;
        if (t >= 0 && t < n) {
            const int64_t at = pop_lower_bound(kv.indices, klo, khi, t);
            if (at < khi && kv.indices[at] == t) {
                rank = 1 + (n - m) + (int)(at - klo);
            } else {
                const unsigned long long q = rand_pack(top, rand_value(key, r, t, bits), t);
                int a = 0, b = cap;
                while (a < b) { const int mid = (a + b) >> 1; if (keys[mid] < q) a = mid + 1; else b = mid; }
                rank = 1 + (a < cap ? cnt[a] : 0);
            }
        }
        ranks_out[off + e] = rank;
    }
}

}  // namespace aae
