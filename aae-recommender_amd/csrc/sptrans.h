// Transpose of a canonical CSR matrix on the device: T = A^T for A [n_rows x n_cols] with int64 indptr, int32 indices ascending
// within a row and without duplicates, and 4-byte values that are MOVED AS RAW BITS (uint32 here) - one code path serves the int32
// operands of the co-occurrence build (spgemm.h) and the fp32 feature rows of the truncated-SVD fit (lowrank.h).  T has the same
// layout, its rows (A's columns) ascending and duplicate-free: indptr, indices and the value bits are scipy's A.T.tocsr() after
// sort_indices(), the same bits every run.
//
// Two calls, the shape of spgemm.h: Count writes the entries of every row of T, the caller's exclusive scan gives T's indptr,
// Fill writes indices (the source row ids) and values.
//
//   sptrans_count_kernel    flat over A's stored entries (grid-stride): one 64-bit integer atomic per entry on col_nnz[c].  The
//                           histogram does not depend on the order of the adds.
//   sptrans_scatter_kernel  one wave per row of A: entry (r, c, v) takes the slot cursor[c]++ (a 64-bit integer atomic) of T's
//                           row c and stores (r, v) there - inside [indptr[c], indptr[c + 1]) or not at all.  The order inside a
//                           segment is whatever the atomics gave; the set is not.
//   sptrans_sort_kernel     one workgroup (4 waves) per row of T sorts the min(cursor[c], segment length) pairs it holds by
//                           source row.  A canonical A names every (r, c) once, so the keys of a segment are distinct and the
//                           sorted segment is unique: that is what makes the bits repeat.  Up to kSptransLds = 4096 pairs: one
//                           bitonic sort in LDS over the power of two >= the length (32 KB: four workgroups fit a CU's 160 KB),
//                           the padding keys ~0u compared as unsigned, as spgemm_hash_kernel's Fill does.  Longer segments - a
//                           popular item's holds 10^5 - 10^6 - sort every run of 4096 in LDS in place, then merge runs pairwise,
//                           width doubling, ping-pong between the segment and the same range of the caller's scratch of nnz
//                           pairs: every pair finds its place by its index in its own run plus a lower-bound search in the
//                           sibling run (distinct keys: no tie rule needed), O(len log^2 len) in all, never quadratic.  A
//                           barrier separates the passes (one workgroup: __syncthreads orders its global stores before the
//                           next pass's loads); an odd number of passes ends with a copy back.
//
// Every loop is bounded by a segment length, the row count or a fixed grid: a wrong indptr from the caller may drop entries, it
// does not spin.  A column id outside [0, n_cols) is skipped, not dereferenced.  Fill never stores outside its row's segment (in
// the outputs and in the scratch alike).  No float atomics, no inline assembly.  Offsets are 64-bit throughout.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace aae {

constexpr int kSptransLds = 4096;       // the longest segment sorted in LDS in one go, and the run length of the merge
constexpr int kSptransNT = 256;
constexpr int kSptransCountBlocks = 2048;   // grid of the flat Count pass (grid-stride)
static_assert((kSptransLds & (kSptransLds - 1)) == 0, "the bitonic network runs over powers of two");

struct SptransArgs {
    const int64_t* indptr;              // A [n_rows + 1]
    const int32_t* indices;
    const uint32_t* values;
    int n_rows, n_cols;
    unsigned long long* col_nnz;        // Count: [n_cols], zero on entry
    const int64_t* t_indptr;            // Fill: [n_cols + 1]
    int32_t* t_indices;
    uint32_t* t_values;
    unsigned long long* cursor;         // Fill: [n_cols], zero on entry
    int2* scratch;                      // Fill: (row, value bits) pairs, addressed like t_indices; NULL when no segment can be long
    int64_t scratch_pairs;              // pairs the scratch holds: a long segment that does not lie inside it is left unsorted
};

__global__ __launch_bounds__(kSptransNT) void sptrans_count_kernel(SptransArgs g) {
    const int64_t lo = g.indptr[0], hi = g.indptr[g.n_rows];
    const int64_t stride = (int64_t)gridDim.x * kSptransNT;
    for (int64_t e = lo + (int64_t)blockIdx.x * kSptransNT + threadIdx.x; e < hi; e += stride) {
        const int c = g.indices[e];
        if (c >= 0 && c < g.n_cols) atomicAdd(&g.col_nnz[c], 1ull);
    }
}

__global__ __launch_bounds__(kSptransNT) void sptrans_scatter_kernel(SptransArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kSptransNT / 64) + (threadIdx.x >> 6);
    if (row >= g.n_rows) return;
    for (int64_t e = g.indptr[row] + lane, hi = g.indptr[row + 1]; e < hi; e += 64) {
        const int c = g.indices[e];
        if (c < 0 || c >= g.n_cols) continue;
        const int64_t at = g.t_indptr[c] + (int64_t)atomicAdd(&g.cursor[c], 1ull);
        if (at < g.t_indptr[c + 1]) { g.t_indices[at] = (int32_t)row; g.t_values[at] = g.values[e]; }
    }
}

// bitonic sort of keys[0, cap) / vals[0, cap) in LDS, ascending, keys compared as unsigned; cap a power of two
__device__ __forceinline__ void sptrans_bitonic(unsigned* keys, unsigned* vals, int cap, int tid) {
    for (int k = 2; k <= cap; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (cap >> 1); t += kSptransNT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned ki = keys[i], kl = keys[l];
                if ((ki > kl) == ((i & k) == 0)) {
                    keys[i] = kl; keys[l] = ki;
                    const unsigned v = vals[i]; vals[i] = vals[l]; vals[l] = v;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kSptransNT) void sptrans_sort_kernel(SptransArgs g) {
    __shared__ unsigned keys[kSptransLds];
    __shared__ unsigned vals[kSptransLds];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int64_t lo = g.t_indptr[c];
    const int64_t seg = g.t_indptr[c + 1] - lo;
    const unsigned long long held = g.cursor[c];
    const int64_t cnt = seg < 0 ? 0 : ((unsigned long long)seg < held ? seg : (int64_t)held);       // pairs the scatter stored
    if (cnt < 2) return;
    int32_t* idx = g.t_indices + lo;
    uint32_t* val = g.t_values + lo;
    // every run of kSptransLds pairs (the whole segment when it is no longer) sorted in LDS, in place
    const bool is_long = cnt > kSptransLds;
    if (is_long && (!g.scratch || lo < 0 || lo + cnt > g.scratch_pairs)) return;                   // (refused on the host: abi_sptrans.h)
    for (int64_t r0 = 0; r0 < cnt; r0 += kSptransLds) {
        const int n = (int)(cnt - r0 < (int64_t)kSptransLds ? cnt - r0 : (int64_t)kSptransLds);
        int cap = 2;
        while (cap < n) cap <<= 1;
        for (int j = tid; j < cap; j += kSptransNT) {
            keys[j] = j < n ? (unsigned)idx[r0 + j] : ~0u;
            vals[j] = j < n ? val[r0 + j] : 0u;
        }
        __syncthreads();
        sptrans_bitonic(keys, vals, cap, tid);
        for (int j = tid; j < n; j += kSptransNT) { idx[r0 + j] = (int32_t)keys[j]; val[r0 + j] = vals[j]; }
        __syncthreads();                                    // (the LDS arrays are free for the next run; the stores are visible)
    }
    if (!is_long) return;
    // pairwise merges, the run width doubling: src -> dst, then the two change places
    int2* scr = g.scratch + lo;
    bool in_scratch = false;                                // where the current runs live
    for (int64_t w = kSptransLds; w < cnt; w <<= 1) {
        for (int64_t i = tid; i < cnt; i += kSptransNT) {
            const int64_t base = i / (2 * w) * (2 * w);
            const int64_t mid = base + w < cnt ? base + w : cnt;
            const int64_t end = base + 2 * w < cnt ? base + 2 * w : cnt;
            const unsigned key = in_scratch ? (unsigned)scr[i].x : (unsigned)idx[i];
            const unsigned bits = in_scratch ? (unsigned)scr[i].y : val[i];
            // the sibling run, and how many of its keys are smaller (distinct keys: lower bound on either side)
            int64_t a = i < mid ? mid : base, b = i < mid ? end : mid;
            const int64_t sib = a;
            while (a < b) {
                const int64_t m = a + ((b - a) >> 1);
                const unsigned km = in_scratch ? (unsigned)scr[m].x : (unsigned)idx[m];
                if (km < key) a = m + 1; else b = m;
            }
            const int64_t at = base + (i - (i < mid ? base : mid)) + (a - sib);
            if (in_scratch) { idx[at] = (int32_t)key; val[at] = bits; }
            else scr[at] = make_int2((int)key, (int)bits);
        }
        __syncthreads();
        in_scratch = !in_scratch;
    }
    if (in_scratch)
        for (int64_t i = tid; i < cnt; i += kSptransNT) { const int2 p = scr[i]; idx[i] = p.x; val[i] = (uint32_t)p.y; }
}

}  // namespace aae
