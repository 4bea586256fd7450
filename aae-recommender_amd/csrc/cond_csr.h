// Trainable bag conditions from a resident CSR: cond_bag.h's five reductions, their backward and the optimiser step over the
// value lists of a corpus that was uploaded once, without the padded [rows][width] rectangle and without the quadratic
// duplicate scan of bag_update_kernel.  The arithmetic is cond_bag.h's helpers; this file adds the source and the grouping.
//
//   bag CSR   indptr int64 [n_docs + 1], indices int32 (table rows), optionally weights fp32 (per_sample_weights, sum only).
//             NOT canonical: a row may name a table row several times, and the order of its entries is the order of the value
//             list.  A step names its rows by row_ids int32 [rows] (a window of the epoch's permutation) or, row_ids NULL, as
//             row0 .. row0 + rows.  A row id outside [0, n_docs) is an empty row; offsets are clamped into [0, nnz].
//   entry e   the step's entries numbered in (position of the row in the batch, position in the row) order - the slot order
//             of the padded route with its padding slots left out.
//   width     the longest list among the step's rows, dead entries counted, at least 1: what _pad_batch pads to.  It is
//             computed by bagcsr_rowinfo_kernel and read from the scratch by the launches behind it - the host never sees it.
//
// Encode: bag_reduce_col over a row's entries with the step's width; the slots the padded form would add behind them are the
// dead slots it accounts for.  Same operations in the same order: the same bits as aae_bag_encode / aae_cat_encode on the
// padded form.
//
// Update, the grouping: every entry becomes the 64-bit key (table row << 32 | e), a dead entry (padding row, out of range)
// (0xFFFFFFFF << 32 | e).  The keys are distinct, so their ascending order is unique whatever sorts them, and it lists the
// entries of a table row next to each other in entry order - the order the padded route sums them in.
//   bagcsr_rowinfo_kernel   one workgroup: the rows' lengths, their exclusive scan off[rows + 1], E and the width
//   bagcsr_sort_kernel      a workgroup per run of kBagCsrSort entries: builds the run's keys (the row of entry e by a binary
//                           search in off) and sorts them in LDS (bitonic, 32 KB: four workgroups a CU)
//   bagcsr_merge_kernel     one launch per doubling of the run width: a thread per key, its place is its index in its own
//                           run plus a lower-bound search in the sibling run.  The number of passes follows from the
//                           caller's entry bound (the host does not know E); a pass whose runs already span E copies.
//   bagcsr_rowpass_kernel   max modes: the winner of every (row, column), recomputed from the untouched table; kBagMeanCount:
//                           the live entries of every row.  Once per row, not once per contributing entry.
//   bagcsr_update_kernel    a wavefront per sorted position (grid-stride): the first key of a table row owns it, walks the
//                           row's run, sums the contributions in that order (bag_grad_add) and hands the row on as
//                           bag_update_kernel does (bag_write_row; the max modes' second pass: bag_apply_row).
// Renorm (max_norm): the same sort with no padding row (pad -1), so a padding-row entry keeps its row in the key; the first
// key of a table row owns it and scales it once (bagcsr_renorm_kernel -> bag_row_renorm).
// Work: O(E) for everything but the sort; the sort is O(E log^2 kBagCsrSort) in LDS plus log2(bound / kBagCsrSort) merge passes
// of O(E log E) each.  Nothing is quadratic, nothing is proportional to vocab but dense Adam itself, there is no [vocab]
// marker, no atomic of any kind, and every loop is bounded by a length read once (E, a row's length, the row count).
// Entries beyond the caller's bound are dropped (hdr[2] is raised), never written.
#pragma once
#include "cond_bag.h"

namespace aae {

constexpr int kBagCsrSort = 4096;             // keys a workgroup sorts in LDS in one go; the run length the merges start from
constexpr int kBagCsrNT = 256;                // threads of the sort and merge workgroups
constexpr int kBagCsrScanNT = 1024;           // rows bagcsr_rowinfo_kernel scans in one round
constexpr int kBagCsrMaxGrid = 4096;          // workgroups of the update launch (grid-stride over the sorted keys)
constexpr int kBagCsrMaxEntries = 1 << 22;    // entries of a step
constexpr unsigned kBagCsrDead = 0xFFFFFFFFu;
static_assert((kBagCsrSort & (kBagCsrSort - 1)) == 0, "the bitonic network runs over powers of two");

struct BagCsr {
    const long long* indptr; const int* indices; const float* weights;      // weights NULL: none
    long long n_docs, nnz;
    const int* row_ids; long long row0; int rows;
    // the scratch (abi_condition.h: bag_csr_carve)
    unsigned long long* keys_a; unsigned long long* keys_b;                 // [max_entries] each
    int* hdr;                                                               // [0] E, [1] width, [2] entries were dropped
    int* off;                                                               // [rows + 1] first entry of every row of the step
    int* live;                                                              // [rows] kBagMeanCount's divisors
    int* rowof;                                                             // [max_entries] the row of entry e
    int* win;                                                               // [rows][dim] max modes: the winning position
    int max_entries;
};

// the entries [lo, hi) of row r of the step
__device__ __forceinline__ void bagcsr_row(const BagCsr& c, int r, long long* lo, long long* hi) {
    const long long id = c.row_ids ? (long long)c.row_ids[r] : c.row0 + r;
    long long a = 0, b = 0;
    if (id >= 0 && id < c.n_docs) { a = c.indptr[id]; b = c.indptr[id + 1]; }
    a = a < 0 ? 0 : (a > c.nnz ? c.nnz : a);
    b = b < a ? a : (b > c.nnz ? c.nnz : b);
    *lo = a; *hi = b;
}

__global__ void __launch_bounds__(kBagCsrScanNT)
bagcsr_rowinfo_kernel(BagCsr c) {
    __shared__ long long part[kBagCsrScanNT / 64];
    __shared__ long long wmax[kBagCsrScanNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0, longest = 1;
    for (int base = 0; base < c.rows; base += kBagCsrScanNT) {
        const int r = base + tid;
        long long len = 0;
        if (r < c.rows) { long long lo, hi; bagcsr_row(c, r, &lo, &hi); len = hi - lo; }
        longest = len > longest ? len : longest;
        long long x = len;                                          // inclusive scan of the wavefront
        for (int d = 1; d < 64; d <<= 1) { const long long y = __shfl_up(x, d); if (lane >= d) x += y; }
        if (lane == 63) part[wave] = x;
        __syncthreads();
        long long pre = carry, tot = carry;
        for (int w = 0; w < kBagCsrScanNT / 64; ++w) { if (w < wave) pre += part[w]; tot += part[w]; }
        if (r < c.rows) {
            const long long at = pre + x - len;
            c.off[r] = (int)(at < (long long)c.max_entries ? at : (long long)c.max_entries);
        }
        carry = tot;
        __syncthreads();
    }
    for (int d = 32; d > 0; d >>= 1) { const long long y = __shfl_xor(longest, d); longest = y > longest ? y : longest; }
    if (lane == 0) wmax[wave] = longest;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kBagCsrScanNT / 64; ++w) longest = wmax[w] > longest ? wmax[w] : longest;
        const int E = (int)(carry < (long long)c.max_entries ? carry : (long long)c.max_entries);
        c.off[c.rows] = E;
        c.hdr[0] = E;
        c.hdr[1] = (int)(longest < 0x7fffffffll ? longest : 0x7fffffffll);
        c.hdr[2] = carry > (long long)c.max_entries;
    }
}

__global__ void __launch_bounds__(64)
bagcsr_encode_kernel(BagCsr c, const float* __restrict__ table, int vocab, int dim, int reduce, int pad, float* __restrict__ out,
                     long long ldo) {
    const int r = blockIdx.x, col = blockIdx.y * 64 + threadIdx.x;
    if (col >= dim) return;
    long long lo, hi;
    bagcsr_row(c, r, &lo, &hi);
    const int width = (reduce == kBagMeanWidth || reduce == kBagMaxPad0) ? c.hdr[1] : 1;
    int win, cnt;
    out[(size_t)r * ldo + col] = bag_reduce_col(table, vocab, dim, c.indices + lo, c.weights ? c.weights + lo : nullptr, hi - lo,
                                                   width, reduce, pad, col, &win, &cnt);
}

// bitonic sort of keys[0, cap) in LDS, ascending; cap a power of two
__device__ __forceinline__ void bagcsr_bitonic(unsigned long long* keys, int cap, int tid) {
    for (int k = 2; k <= cap; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (cap >> 1); t += kBagCsrNT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long ki = keys[i], kl = keys[l];
                if ((ki > kl) == ((i & k) == 0)) { keys[i] = kl; keys[l] = ki; }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(kBagCsrNT)
bagcsr_sort_kernel(BagCsr c, int vocab, int pad) {
    __shared__ unsigned long long keys[kBagCsrSort];
    const int tid = threadIdx.x;
    const int E = c.hdr[0];
    const long long e0 = (long long)blockIdx.x * kBagCsrSort;
    if (e0 >= E) return;
    const int n = E - e0 < kBagCsrSort ? (int)(E - e0) : kBagCsrSort;
    int cap = 2;
    while (cap < n) cap <<= 1;
    for (int i = tid; i < cap; i += kBagCsrNT) {
        unsigned long long key = ~0ull;                             // (padding of the network: above every key, never stored)
        if (i < n) {
            const int e = (int)e0 + i;
            int a = 0, b = c.rows;                                  // the row of e: the last one with off[row] <= e
            while (a < b) {
                const int m = (a + b) >> 1;
                if (c.off[m] <= e) a = m + 1; else b = m;
            }
            const int row = a - 1;
            long long lo, hi;
            bagcsr_row(c, row, &lo, &hi);
            const int j = c.indices[lo + (e - c.off[row])];
            c.rowof[e] = row;
            key = ((unsigned long long)(bag_live(j, vocab, pad) ? (unsigned)j : kBagCsrDead) << 32) | (unsigned)e;
        }
        keys[i] = key;
    }
    __syncthreads();
    bagcsr_bitonic(keys, cap, tid);
    for (int i = tid; i < n; i += kBagCsrNT) c.keys_a[e0 + i] = keys[i];
}

// runs of w keys in src, merged pairwise into runs of 2 w in dst
__global__ void __launch_bounds__(kBagCsrNT)
bagcsr_merge_kernel(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst, const int* __restrict__ hdr,
                    int w) {
    const long long E = hdr[0];
    const long long i = (long long)blockIdx.x * kBagCsrNT + threadIdx.x;
    if (i >= E) return;
    const long long base = i / (2ll * w) * (2ll * w);
    const long long mid = base + w < E ? base + w : E;
    const long long end = base + 2ll * w < E ? base + 2ll * w : E;
    const unsigned long long key = src[i];
    // the sibling run, and how many of its keys are smaller (distinct keys: a lower bound on either side)
    long long a = i < mid ? mid : base, b = i < mid ? end : mid;
    const long long sib = a;
    while (a < b) {
        const long long m = a + ((b - a) >> 1);
        if (src[m] < key) a = m + 1; else b = m;
    }
    dst[base + (i - (i < mid ? base : mid)) + (a - sib)] = key;
}

__global__ void __launch_bounds__(64)
bagcsr_rowpass_kernel(BagCsr c, const float* __restrict__ table, int vocab, int dim, int reduce, int pad) {
    const int r = blockIdx.x, lane = threadIdx.x;
    long long lo, hi;
    bagcsr_row(c, r, &lo, &hi);
    const int len = c.off[r + 1] - c.off[r];                        // (the entries the step holds: all of them within the bound)
    if (reduce == kBagMeanCount) {
        if (blockIdx.y) return;
        int n = 0;
        for (int i = lane; i < len; i += 64) n += bag_live(c.indices[lo + i], vocab, pad);
        for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d);
        if (lane == 0) c.live[r] = n;
        return;
    }
    const int col = blockIdx.y * 64 + lane;
    if (col >= dim) return;
    int win, cnt;
    bag_reduce_col(table, vocab, dim, c.indices + lo, nullptr, len, c.hdr[1], reduce, pad, col, &win, &cnt);
    c.win[(size_t)r * dim + col] = win;
}

__global__ void __launch_bounds__(64 * kCatWaves)
bagcsr_update_kernel(BagTable a, BagCsr c, const unsigned long long* __restrict__ sorted, int apply_only) {
    const int lane = threadIdx.x & 63;
    const int E = c.hdr[0], width = c.hdr[1];
    const int stride = gridDim.x * kCatWaves;
    for (int k = blockIdx.x * kCatWaves + (threadIdx.x >> 6); k < E; k += stride) {
        const unsigned j = (unsigned)(sorted[k] >> 32);
        if (j == kBagCsrDead) continue;
        if (k > 0 && (unsigned)(sorted[k - 1] >> 32) == j) continue;          // an earlier entry of the same table row owns it
        if (apply_only) { bag_apply_row(a, (int)j, lane); continue; }
        // gradient of row j: its run of the sorted keys, in entry order
        float g[kCatMaxDim / 64];
#pragma unroll
        for (int q = 0; q < kCatMaxDim / 64; ++q) g[q] = 0.f;
        int named = 0;                                              // entries naming row j (scale_grad_by_freq)
        for (int k2 = k; k2 < E; ++k2) {
            const unsigned long long key = sorted[k2];
            if ((unsigned)(key >> 32) != j) break;
            ++named;
            const int e = (int)(unsigned)key;
            const int b = c.rowof[e];
            const int w = e - c.off[b];
            float wt = 1.f;
            if (c.weights) { long long lo, hi; bagcsr_row(c, b, &lo, &hi); wt = c.weights[lo + w]; }
            const int live = a.reduce == kBagMeanCount ? c.live[b] : 1;
#pragma unroll
            for (int q = 0; q < kCatMaxDim / 64; ++q) {
                const int col = lane + 64 * q;
                if (col >= a.dim) continue;
                const bool winner = a.reduce >= kBagMaxPad0 && c.win[(size_t)b * a.dim + col] == w;
                bag_grad_add(g[q], a.reduce, a.d[(size_t)b * a.ldd + col], width, live, winner, c.weights != nullptr, wt);
            }
        }
        bag_freq_scale(a, g, named);
        bag_write_row(a, (int)j, lane, g);
    }
}

// max_norm over the keys sorted with no padding row: a wavefront per sorted position, the first key of a table row scales it
__global__ void __launch_bounds__(64 * kCatWaves)
bagcsr_renorm_kernel(float* __restrict__ table, int dim, BagCsr c, const unsigned long long* __restrict__ sorted, float max_norm,
                     int norm_type) {
    const int lane = threadIdx.x & 63;
    const int E = c.hdr[0];
    const int stride = gridDim.x * kCatWaves;
    for (int k = blockIdx.x * kCatWaves + (threadIdx.x >> 6); k < E; k += stride) {
        const unsigned j = (unsigned)(sorted[k] >> 32);
        if (j == kBagCsrDead) continue;
        if (k > 0 && (unsigned)(sorted[k - 1] >> 32) == j) continue;
        bag_row_renorm(table, dim, (int)j, lane, max_norm, norm_type);
    }
}

}  // namespace aae
