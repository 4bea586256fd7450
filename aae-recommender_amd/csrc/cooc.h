// Item co-occurrence scores (the reference's Countbased baseline, baselines.py:22-43: predict = X @ C with C = X^T X of the
// training set): for call row r with entries (i, x_i) and the co-occurrence matrix C in CSR form
//
//   scores[r][j] = sum_i x_i * C[i][j]            fp32 or int32 [rows][ld] in HBM, every column j < n_items written
//
// - a sparse row times a sparse matrix with INTEGER values.  The sum is formed in int32, so it is exact and does not depend on
// the order the terms arrive in: the same bits from run to run and however the caller chunks its rows.  Two stored types
// (OUT; kernel_pick.h names both): float - the sum converted once (the caller keeps every sum below 2^24, aaerec/cooc.py
// device_route's "f32", so the fp32 it reads is that integer) - and int32_t - the sum as it is (the caller keeps every sum
// inside int32, device_route's "i32"), for the integer form of the dense rank kernels (rank_long.h DenseScore).
//
//   cooc_scores_kernel       one workgroup per (row, tile of kCoocTile items).  The workgroup zeroes an int32 tile in LDS; its
//                            16 waves take the row's entries in turn; for entry (i, x_i) the wave finds, by a lower-bound search
//                            in the ascending columns of C's row i, the first column inside the tile, and its lanes stride over
//                            the segment from there while the column stays below the tile's end, each adding x_i * C[i][j] to
//                            tile[j] with an integer LDS atomic.  Behind a barrier the tile is stored with plain coalesced
//                            stores - converted (float4) or as it is (int4) where the matrix is 16-byte aligned.
//
// kCoocTile = 16384 items = 64 KB of the CU's 160 KB of LDS: two workgroups fit a CU by LDS, and two workgroups of 16 waves
// are the CU's 32 wave slots as well, so one workgroup's atomics run beside the other's zeroing and stores.  A wider tile
// (32768: 128 KB) halves the searches per entry but leaves one workgroup per CU and nothing to overlap with; a narrower one
// adds a search per (entry, tile) - log2(nnz of C's row) dependent loads each - for no more residency than the wave slots allow.
//
// An input id outside [0, n_items) or without a row in C is skipped; an item whose C row is empty adds nothing; a row without
// entries is a row of zeros.  Columns of C outside the tile's span - or, against the contract, descending - are never added.
// No float atomics, no inline assembly.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace aae {

constexpr int kCoocTile = 16384;
constexpr int kCoocNT = 1024;

struct CoocView { const int64_t* indptr; const int32_t* indices; const int32_t* values; int n_rows; };

template <class OUT>
__global__ __launch_bounds__(kCoocNT) void cooc_scores_kernel(CoocView C, int n_items, int ntiles, BatchView bv,
                                                              OUT* __restrict__ scores, long long ld) {
    static_assert(std::is_same_v<OUT, float> || std::is_same_v<OUT, int32_t>, "the score matrix is fp32 or int32");
    __shared__ __attribute__((aligned(16))) int tile[kCoocTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x / ntiles, t = blockIdx.x - row * ntiles;
    const int col0 = t * kCoocTile, col1 = min(col0 + kCoocTile, n_items), width = col1 - col0;
    for (int j = tid; j < kCoocTile; j += kCoocNT) tile[j] = 0;
    __syncthreads();
    const int dc = bv.doc(row);
    const int64_t lo = bv.indptr[dc], hi = bv.indptr[dc + 1];
    for (int64_t e = lo + wave; e < hi; e += kCoocNT / 64) {
        const int i = bv.indices[e];
        const int x = __float2int_rn(bv.values[e]);
        if (i < 0 || i >= n_items || i >= C.n_rows || x == 0) continue;
        const int64_t clo = C.indptr[i], chi = C.indptr[i + 1];
        int64_t a = clo, b = chi;                   // the first entry of C's row i with column >= col0 (every lane the same search)
        while (a < b) {
            const int64_t mid = a + ((b - a) >> 1);
            if (C.indices[mid] < col0) a = mid + 1; else b = mid;
        }
        for (int64_t p = a + lane; p < chi; p += 64) {
            const int c = C.indices[p];
            if (c >= col1) break;
            if (c >= col0) atomicAdd(&tile[c - col0], x * C.values[p]);
        }
    }
    __syncthreads();
    OUT* out = scores + (size_t)row * (size_t)ld + col0;        // (col0 is a multiple of 4: a float4 / int4 of the row is one of the matrix)
    if ((ld & 3) == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0) {
        const int w4 = width >> 2;
        for (int j = tid; j < w4; j += kCoocNT) {
            const int4 v = reinterpret_cast<const int4*>(tile)[j];
            if constexpr (std::is_same_v<OUT, float>) reinterpret_cast<float4*>(out)[j] = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
            else reinterpret_cast<int4*>(out)[j] = v;
        }
        for (int j = 4 * w4 + tid; j < width; j += kCoocNT) out[j] = (OUT)tile[j];
    } else {
        for (int j = tid; j < width; j += kCoocNT) out[j] = (OUT)tile[j];
    }
}

}  // namespace aae
