// The most-popular baseline (reference baselines.py:46-58, MostPopular: predict = the item counts of the training set, the same
// vector for every row).  Every row ranks the SAME scores, so the items are ordered once - `order`: the ids by (count descending,
// id ascending), `pos` its inverse, built by the caller - and a row only has to leave its known items out of that order:
//
//   pop_counts_kernel  counts[j] += x_dj, one lane per stored entry of the training matrix, int32 atomicAdd (integer adds: the
//                      result does not depend on their order).  counts is zeroed by the caller.
//   pop_topk_kernel    one wavefront per row, kPopRows rows per workgroup.  The wave walks `order` 64 candidates at a time: a
//                      lane looks its candidate up among the row's ascending ids (binary search), a ballot and the popcount of
//                      the lower lanes give its place in the list, the lane writes id and scaled score.  Stops at k written or
//                      at the end of `order`, then pads with id -1 / score 0.  O(k + m) candidates for a row of m known items.
//   pop_ranks_kernel   one wavefront per row; per held-out item t a binary search says whether it is a known item.  If so its
//                      rank is 1 + (items - m) + #{known j < t} - the index the search returns.  If not, the lanes stride over
//                      the known ids counting pos[j] < pos[t] and a wave reduction gives 1 + pos[t] - count.  O(m) per entry.
//
// The ordering is the library's one rule (rank_long.h / rank_full.h): the better score first, the smaller id at equal scores,
// known items left out; a known held-out item behind every rankable one, among the known items by id; an id outside
// [0, n_items) ranks 0 and `pos` is not read for it.  Scaled scores are the min-max scaling over ALL items with the fp32
// formula of the int32 co-occurrence route (rank_long.h): (float(v) - float(min)) * inv, span = float(max) - float(min),
// inv = span > 0 ? 1 / span : 1, where min = counts[order[n_items - 1]] and max = counts[order[0]].
//
// No [rows, items] buffer, no LDS, no limit on m or on k <= n_items.  CONTRACT (the caller's, as in every dense ranking call):
// the ids of a batch row lie in [0, n_items) and ascend without duplicates.  Every loop is bounded by a row's length or by
// n_items; an index read from `order` is used only after it was checked against [0, n_items).
// No float atomics, no inline assembly: plain loads, vector stores, wave ballots and shuffles.
#pragma once
#include "cooc.h"

namespace aae {

constexpr int kPopNT = 256;                 // threads of every workgroup here
constexpr int kPopRows = kPopNT / 64;       // rows of a ranking workgroup: one wavefront each
constexpr int kPopCountBlocks = 2048;       // grid of the grid-stride count kernel

// counts, order, pos: int32 [n_items]
struct PopView {
    const int32_t* counts; const int32_t* order; const int32_t* pos;
    int n_items;
};

__global__ __launch_bounds__(kPopNT) void pop_counts_kernel(CoocView X, int n_items, int* __restrict__ counts) {
    const int64_t nnz = X.indptr[X.n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kPopNT + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kPopNT) {
        const int j = X.indices[e];
        if (j >= 0 && j < n_items) atomicAdd(&counts[j], X.values[e]);
    }
}

// the first entry of the ascending ids [lo, hi) that is >= t (hi when there is none): at most 64 halvings
__device__ __forceinline__ int64_t pop_lower_bound(const int32_t* __restrict__ ids, int64_t lo, int64_t hi, int t) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kPopNT) void pop_topk_kernel(PopView P, BatchView kv, int exclude_known, int k,
                                                          int* __restrict__ idx_out, float* __restrict__ val_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kPopRows + (threadIdx.x >> 6);
    if (row >= kv.n_rows) return;                                   // (a whole wavefront: nothing here meets at a barrier)
    const int n = P.n_items;
    int64_t lo = 0, hi = 0;
    if (exclude_known) { const int dc = kv.doc((int)row); lo = kv.indptr[dc]; hi = kv.indptr[dc + 1]; }
    const int top = P.order[0], bottom = P.order[n - 1];
    const bool ends_ok = top >= 0 && top < n && bottom >= 0 && bottom < n;
    const float fmin_ = ends_ok ? (float)P.counts[bottom] : 0.f;
    const float span = (ends_ok ? (float)P.counts[top] : 0.f) - fmin_;
    const float inv = span > 0.f ? 1.f / span : 1.f;
    int* idx = idx_out + (size_t)row * k;
    float* val = val_out + (size_t)row * k;
    int written = 0;
    for (int base = 0; base < n && written < k; base += 64) {
        const int c = base + lane;
        const int item = c < n ? P.order[c] : -1;
        bool keep = item >= 0 && item < n;
        if (keep && lo < hi) {
            const int64_t e = pop_lower_bound(kv.indices, lo, hi, item);
            keep = !(e < hi && kv.indices[e] == item);
        }
        const unsigned long long mask = __ballot(keep);
        const int p = written + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && p < k) { idx[p] = item; val[p] = ((float)P.counts[item] - fmin_) * inv; }
        written += __popcll(mask);
    }
    for (int p = (written < k ? written : k) + lane; p < k; p += 64) { idx[p] = -1; val[p] = 0.f; }
}

// where the entries of call row `row` begin in the call's output (entries of the rows before it, CSR order): the wave's sum
__device__ __forceinline__ long long pop_truth_offset(const BatchView& tv, int64_t row, int lane) {
    if (!tv.rows) return tv.indptr[tv.row_start + row] - tv.indptr[tv.row_start];
    long long sum = 0;
    for (int64_t r = lane; r < row; r += 64) { const int dc = tv.rows[r]; sum += tv.indptr[dc + 1] - tv.indptr[dc]; }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    return sum;
}

__global__ __launch_bounds__(kPopNT) void pop_ranks_kernel(PopView P, BatchView kv, BatchView tv, int exclude_known,
                                                           int* __restrict__ ranks_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kPopRows + (threadIdx.x >> 6);
    if (row >= kv.n_rows) return;
    const int n = P.n_items;
    const int dt = tv.doc((int)row);
    const int64_t tlo = tv.indptr[dt], thi = tv.indptr[dt + 1];
    if (tlo >= thi) return;
    int64_t lo = 0, hi = 0;
    if (exclude_known) { const int dc = kv.doc((int)row); lo = kv.indptr[dc]; hi = kv.indptr[dc + 1]; }
    const long long off = pop_truth_offset(tv, row, lane);
    for (int64_t e = tlo; e < thi; ++e) {                            // (wave-uniform: every lane holds the same entry)
        const int t = tv.indices[e];
        int rank = 0;
        if (t >= 0 && t < n) {
            const int64_t at = pop_lower_bound(kv.indices, lo, hi, t);
            if (at < hi && kv.indices[at] == t) {
                rank = 1 + (n - (int)(hi - lo)) + (int)(at - lo);
            } else {
                const int pt = P.pos[t];
                int ahead = 0;
                for (int64_t q = lo + lane; q < hi; q += 64) {
                    const int j = kv.indices[q];
                    ahead += (j >= 0 && j < n && P.pos[j] < pt) ? 1 : 0;
                }
                for (int o = 32; o > 0; o >>= 1) ahead += __shfl_xor(ahead, o, 64);
                rank = 1 + pt - ahead;
            }
        }
        if (lane == 0) ranks_out[off + (e - tlo)] = rank;
    }
}

}  // namespace aae
