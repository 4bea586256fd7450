// Exact sparse product in int32: C = A . B for CSR operands in the layout of the co-occurrence matrix (cooc.h CoocView: int64
// indptr, int32 indices ascending within a row and without duplicates, int32 values), the result in the same layout with the
// columns ascending in every row - what cooc_scores_kernel's lower-bound search needs.  It builds the co-occurrence matrix of
// the Countbased baseline on the device: C = X^T . X, and C . C for every further order (aaerec/cooc.py).
//
// Gustavson, row-wise: row i of C = sum over the entries (d, a) of A's row i of a * B[d, :].  Every accumulation is an int32 add
// (an LDS integer atomic), so a row's values do not depend on the order of the adds: the same bits every run.  The caller
// guarantees that no sum leaves int32 (aaerec/cooc.py device_build_ok) and that every value is strictly positive: "touched" is
// "non-zero" on the tile path.  No float atomics, no inline assembly.  Offsets into indices / values are 64-bit throughout.
//
// Two passes of the same code (template flag FILL): Count writes the entries of every result row, the caller's exclusive scan
// gives indptr, Fill writes columns and values.  Rows are dealt to two kernels by their product upper bound
// u_i = sum over A's row i of nnz(B_d) (spgemm_bound_kernel); both kernels are launched over every row and a workgroup whose row
// belongs to the other one leaves at once.
//
//   spgemm_hash_kernel   u_i <= kSpgemmHashProducts.  One workgroup (4 waves) per row, an open-addressing table in LDS: int32 keys
//                        (-1 = empty), int32 values, kSpgemmHashCap = 2 * kSpgemmHashProducts slots = 64 KB - two workgroups fit
//                        the CU's 160 KB, the reasoning of kCoocTile.  A row uses the first cap_i = the power of two >=
//                        max(64, 2 u_i) slots and initialises only those, so its load never exceeds 1/2 and linear probing ends
//                        (the probe loop is bounded by cap_i all the same: a wrong u from the caller drops products, it does
//                        not hang).  Slot = column & (cap_i - 1): consecutive columns are consecutive banks.  16 lanes take one
//                        entry of A's row and stride over B's row; insert = LDS atomicCAS on the key, then atomicAdd on the
//                        value.  Count stops behind a barrier with the number of successful inserts.  Fill sorts the used part
//                        of the table in place, bitonic over cap_i with the keys compared as unsigned - an empty slot
//                        (0xFFFFFFFF) is the largest key, so the sort is the compaction as well - and stores the row's pairs with
//                        plain coalesced stores.
//   spgemm_tile_kernel   every longer row.  One workgroup (16 waves) per row walks the column range a tile of kCoocTile items at
//                        a time.  Per tile: zero an int32 LDS tile; stage the row's A entries through LDS kSpgemmStage at a time
//                        (value and the bounds of B's row: one coalesced pass, nothing assumes the row fits); 16 lanes take a
//                        staged entry, find by lower-bound search the first column of B's row inside the tile and stride over the
//                        segment adding into the tile, as cooc_scores_kernel does (Count only marks the cell).  Behind a barrier
//                        each wave counts the non-zero cells of its 1/16 of the tile (ballot / popcount), the counts meet in LDS,
//                        and each wave stores its cells from its prefix + the row's running offset, lanes in column order: a
//                        tile emits ascending columns by construction, so this path has no sort.
//
// An empty A row gives an empty C row; an empty B row adds nothing; a column id of A outside [0, p) or of B outside [0, n) is
// skipped, not dereferenced.  Fill never stores outside [indptr[i], indptr[i + 1]) of its row.
#pragma once
#include "cooc.h"

namespace aae {

constexpr int kSpgemmHashProducts = 4096;                   // the largest u_i of the hash path
constexpr int kSpgemmHashCap = 2 * kSpgemmHashProducts;     // slots of the LDS table (a power of two)
constexpr int kSpgemmHashNT = 256;
constexpr int kSpgemmTileNT = 1024;
constexpr int kSpgemmStage = 512;                           // A entries staged per piece on the tile path
constexpr int kSpgemmGroup = 16;                            // lanes that share one A entry
static_assert((kSpgemmHashCap & (kSpgemmHashCap - 1)) == 0, "the table is masked, not divided");
static_assert(kCoocTile % (kSpgemmTileNT / 64 * 64) == 0, "each wave owns a whole number of 64-cell steps of the tile");

// A [m x p], B [p x n]; u [m] from spgemm_bound_kernel.  Count: row_nnz [m] is written.  Fill: indptr [m + 1] is read, indices and
// values are written.
struct SpgemmArgs {
    CoocView A, B;
    int p, n;
    const int64_t* u;
    int64_t* row_nnz;
    const int64_t* indptr;
    int32_t* indices;
    int32_t* values;
};

// u_i = sum over the entries (d, .) of A's row i, d in [0, p), of nnz(B_d): one wave per row
__global__ __launch_bounds__(256) void spgemm_bound_kernel(CoocView A, CoocView B, int p, int64_t* __restrict__ u) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= A.n_rows) return;
    long long sum = 0;
    for (int64_t e = A.indptr[row] + lane, hi = A.indptr[row + 1]; e < hi; e += 64) {
        const int d = A.indices[e];
        if (d >= 0 && d < p) sum += B.indptr[d + 1] - B.indptr[d];
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (lane == 0) u[row] = sum;
}

// The accumulation phases of the two paths as device functions: the product kernels below and the row kernels of mutinfo.h
// (which reduce a row where these store it) run the same code.
//
// Hash path: cap = the slots row `row` uses (0: the row is the tile kernel's).  Initialises them, inserts every product of the
// row; returns this thread's count of fresh inserts.  No barrier behind the inserts: the caller's.
__device__ __forceinline__ int spgemm_hash_cap(int64_t u) {
    if (u > kSpgemmHashProducts) return 0;
    int cap = 64;
    while (cap < 2 * u) cap <<= 1;
    return cap;
}
template <bool FILL>
__device__ __forceinline__ int spgemm_hash_accumulate(const CoocView& A, const CoocView& B, int p, int n, int row, int cap,
                                                      int* keys, int* vals) {
    const int tid = threadIdx.x, mask = cap - 1;
    for (int j = tid; j < cap; j += kSpgemmHashNT) { keys[j] = -1; if (FILL) vals[j] = 0; }
    __syncthreads();
    const int grp = tid / kSpgemmGroup, gl = tid % kSpgemmGroup;
    int fresh = 0;
    for (int64_t e = A.indptr[row] + grp, ehi = A.indptr[row + 1]; e < ehi; e += kSpgemmHashNT / kSpgemmGroup) {
        const int d = A.indices[e];
        if (d < 0 || d >= p) continue;
        const int a = A.values[e];
        for (int64_t q = B.indptr[d] + gl, qhi = B.indptr[d + 1]; q < qhi; q += kSpgemmGroup) {
            const int c = B.indices[q];
            if (c < 0 || c >= n) continue;
            int h = c & mask;
            for (int probe = 0; probe < cap; ++probe) {                     // (load <= 1/2: an empty slot comes long before cap)
                const int prev = atomicCAS(&keys[h], -1, c);
                if (prev == -1 || prev == c) {
                    fresh += prev == -1;
                    if (FILL) atomicAdd(&vals[h], a * B.values[q]);
                    break;
                }
                h = (h + 1) & mask;
            }
        }
    }
    return fresh;
}
// bitonic over the cap slots in use, keys as unsigned: the occupied slots come first, ascending; empty ones (~0u) last.  The
// caller's barrier stands between the last insert and this; a barrier closes every stage, the last one included
__device__ __forceinline__ void spgemm_hash_sort(int cap, int* keys, int* vals) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= cap; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (cap >> 1); t += kSpgemmHashNT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned ki = (unsigned)keys[i], kl = (unsigned)keys[l];
                if ((ki > kl) == ((i & k) == 0)) {
                    keys[i] = (int)kl; keys[l] = (int)ki;
                    const int v = vals[i]; vals[i] = vals[l]; vals[l] = v;
                }
            }
            __syncthreads();
        }
    }
}

template <bool FILL>
__global__ __launch_bounds__(kSpgemmHashNT) void spgemm_hash_kernel(SpgemmArgs g) {
    __shared__ int keys[kSpgemmHashCap];
    __shared__ int vals[kSpgemmHashCap];
    __shared__ int inserted;
    const int tid = threadIdx.x, row = blockIdx.x;
    const int cap = spgemm_hash_cap(g.u[row]);
    if (cap == 0) return;                                                   // the tile kernel's row
    if (tid == 0) inserted = 0;
    const int fresh = spgemm_hash_accumulate<FILL>(g.A, g.B, g.p, g.n, row, cap, keys, vals);
    if (!FILL) {
        if (fresh) atomicAdd(&inserted, fresh);
        __syncthreads();
        if (tid == 0) g.row_nnz[row] = inserted;
        return;
    }
    __syncthreads();
    spgemm_hash_sort(cap, keys, vals);
    const int64_t lo = g.indptr[row];
    const int64_t cnt = min(g.indptr[row + 1] - lo, (int64_t)cap);
    for (int j = tid; j < cnt; j += kSpgemmHashNT) {
        if (keys[j] < 0) break;                                             // (fewer entries than indptr promised: never under the contract)
        g.indices[lo + j] = keys[j];
        g.values[lo + j] = vals[j];
    }
}

// Tile path: the cells [col0, col1) of one row into `tile` (kCoocTile ints: zeroed here, then every product of the row whose
// column is inside the span added - Count only marks the cell), the row's A entries [alo, ahi) staged kSpgemmStage at a time
// through s_lo / s_hi / s_val.  Ends behind a barrier: the tile is complete for every thread.
template <bool FILL>
__device__ __forceinline__ void spgemm_tile_accumulate(const CoocView& A, const CoocView& B, int p, int64_t alo, int64_t ahi,
                                                       int col0, int col1, int* tile, int64_t* s_lo, int64_t* s_hi, int* s_val) {
    const int tid = threadIdx.x, grp = tid / kSpgemmGroup, gl = tid % kSpgemmGroup;
    for (int j = tid; j < kCoocTile; j += kSpgemmTileNT) tile[j] = 0;
    for (int64_t e0 = alo; e0 < ahi; e0 += kSpgemmStage) {
        const int piece = (int)min((int64_t)kSpgemmStage, ahi - e0);
        __syncthreads();                                                    // the tile is zero / the last piece has been read
        if (tid < piece) {
            const int d = A.indices[e0 + tid];
            const bool ok = d >= 0 && d < p;
            s_val[tid] = A.values[e0 + tid];
            s_lo[tid] = ok ? B.indptr[d] : 0;
            s_hi[tid] = ok ? B.indptr[d + 1] : 0;
        }
        __syncthreads();
        for (int s = grp; s < piece; s += kSpgemmTileNT / kSpgemmGroup) {
            const int64_t bhi = s_hi[s];
            int64_t a = s_lo[s], b = bhi;                                   // the first entry of B's row with column >= col0
            while (a < b) {
                const int64_t mid = a + ((b - a) >> 1);
                if (B.indices[mid] < col0) a = mid + 1; else b = mid;
            }
            const int x = s_val[s];
            for (int64_t q = a + gl; q < bhi; q += kSpgemmGroup) {
                const int c = B.indices[q];
                if (c >= col1) break;
                if (c < col0) continue;
                if (FILL) atomicAdd(&tile[c - col0], x * B.values[q]); else tile[c - col0] = 1;
            }
        }
    }
    __syncthreads();
}

template <bool FILL>
__global__ __launch_bounds__(kSpgemmTileNT) void spgemm_tile_kernel(SpgemmArgs g) {
    __shared__ __attribute__((aligned(16))) int tile[kCoocTile];
    __shared__ int64_t s_lo[kSpgemmStage], s_hi[kSpgemmStage];
    __shared__ int s_val[kSpgemmStage];
    __shared__ int wcnt[kSpgemmTileNT / 64];
    constexpr int kWaves = kSpgemmTileNT / 64, kSeg = kCoocTile / kWaves;       // cells of the tile one wave compacts
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    if (g.u[row] <= kSpgemmHashProducts) return;                            // the hash kernel's row
    const int64_t alo = g.A.indptr[row], ahi = g.A.indptr[row + 1];
    const int64_t out0 = FILL ? g.indptr[row] : 0, out1 = FILL ? g.indptr[row + 1] : 0;
    int64_t running = 0;                                                    // entries of the row emitted by the tiles so far
    for (int col0 = 0; col0 < g.n; col0 += kCoocTile) {
        const int col1 = min(col0 + kCoocTile, g.n), width = col1 - col0;
        spgemm_tile_accumulate<FILL>(g.A, g.B, g.p, alo, ahi, col0, col1, tile, s_lo, s_hi, s_val);
        int mine = 0;                                                       // non-zero cells of this wave's segment
        for (int j = wave * kSeg + lane; j < (wave + 1) * kSeg; j += 64)
            mine += __popcll(__ballot(j < width && tile[j] != 0));
        if (lane == 0) wcnt[wave] = mine;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kWaves; ++w) { const int c = wcnt[w]; total += c; before += w < wave ? c : 0; }
        if (FILL) {
            int64_t pos = out0 + running + before;
            for (int j = wave * kSeg + lane; j < (wave + 1) * kSeg; j += 64) {
                const int v = j < width ? tile[j] : 0;
                const unsigned long long m = __ballot(v != 0);
                const int64_t at = pos + __popcll(m & ((1ull << lane) - 1));
                if (v != 0 && at < out1) { g.indices[at] = col0 + j; g.values[at] = v; }
                pos += __popcll(m);
            }
        }
        running += total;
        __syncthreads();                                                    // wcnt and the tile are free again
    }
    if (!FILL && tid == 0) g.row_nnz[row] = running;
}

}  // namespace aae
