// Mutual information of a contingency table that is never stored: C = A . B for CSR operands in the layout of spgemm.h (A = X^T
// [m x p], B = Y [p x n], int32 values, strictly positive, every c_ij below 2^31 by the caller's guard - aaerec/utils.py
// device_mi_ok), reduced row by row while it sits in LDS.  scikit-learn's mutual_info_score(contingency=C), rearranged per row:
//
//   MI = (1/T) sum_i [ S1_i + pi_i (ln T - ln pi_i) ],   S1_i = sum_j c_ij (ln c_ij - ln pj_j),   pi_i = sum_j c_ij,   T = sum_i pi_i
//
// with the column sums formed from the operands' own entries before the product: a_d = sum_i A_id, pj_j = sum_d B_dj a_d.
//
//   mi_colsum_kernel / mi_pj_kernel   a_d and pj_j by int64 integer atomics: order-free, the same bits every run.
//   mi_lnpj_kernel                    lnpj[j] = log((double)pj_j) (0 where pj_j = 0: no product ever lands in such a column).
//   mi_hash_kernel / mi_tile_kernel   row i of C accumulated in LDS by spgemm.h's own accumulation phases (rows dealt by the
//                                     product bound u_i exactly as spgemm deals them), then reduced on the spot: pi_i in int64,
//                                     S1_i in fp64.  The order of the fp64 sum is fixed: the hash row is first sorted by column
//                                     (the slot a column lands in depends on which lane wins an insert; the sorted table does
//                                     not), lane t takes the sorted entries t, t + 256, ... in turn, a shuffle tree per wave, the
//                                     wave partials in wave order.  A tile row: lane l of wave w takes cells w * 1024 + l + 64 k,
//                                     k ascending, a shuffle tree per wave, the 16 wave partials in wave order, and the tiles'
//                                     partial sums in column order.
//   mi_finish_kernel                  one workgroup: T = sum pi_i (integer), then the row terms with a fixed stride per thread,
//                                     a fixed shuffle / LDS tree; mi = max(sum / T, 0), mi = 0 when T = 0.
//
// No float atomics, no inline assembly.  Every loop is bounded as in spgemm.h; ids outside their range are skipped, not
// dereferenced; an empty row writes row_pi = 0, row_s1 = 0.  LDS: the row kernels claim what spgemm's claim plus the wave
// partials (at most 256 bytes): two workgroups per CU, kCoocTile's reasoning.
#pragma once
#include "spgemm.h"

namespace aae {

constexpr int kMiNT = 256;                  // marginals
constexpr int kMiBlocks = 1024;             // grid of the grid-stride column-sum kernel
constexpr int kMiFinishNT = 1024;

// A [m x p], B [p x n]; u [m] from spgemm_bound_kernel; lnpj [n] from mi_lnpj_kernel.  row_s1 / row_pi [m] are written.
struct MiRowArgs {
    CoocView A, B;
    int p, n;
    const int64_t* u;
    const double* lnpj;
    double* row_s1;
    int64_t* row_pi;
};

// sum over the wave, the same tree every run; the total in lane 0
__device__ __forceinline__ double mi_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ long long mi_wave_sum(long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// a[d] += A's values of column d, d in [0, p): grid-stride over the stored entries (a zeroed by the caller)
__global__ __launch_bounds__(kMiNT) void mi_colsum_kernel(CoocView A, int p, unsigned long long* __restrict__ a) {
    const int64_t nnz = A.indptr[A.n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kMiNT + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kMiNT) {
        const int d = A.indices[e];
        if (d >= 0 && d < p) atomicAdd(&a[d], (unsigned long long)(long long)A.values[e]);
    }
}

// pj[j] += B_dj * a[d] over B's rows d in [0, p): one wave per row (pj zeroed by the caller)
__global__ __launch_bounds__(kMiNT) void mi_pj_kernel(CoocView B, int p, int n, const unsigned long long* __restrict__ a,
                                                      unsigned long long* __restrict__ pj) {
    const int lane = threadIdx.x & 63;
    const int64_t d = (int64_t)blockIdx.x * (kMiNT / 64) + (threadIdx.x >> 6);
    if (d >= p || d >= B.n_rows) return;
    const unsigned long long ad = a[d];
    if (ad == 0) return;
    for (int64_t q = B.indptr[d] + lane, qhi = B.indptr[d + 1]; q < qhi; q += 64) {
        const int c = B.indices[q];
        if (c >= 0 && c < n) atomicAdd(&pj[c], (unsigned long long)(long long)B.values[q] * ad);
    }
}

__global__ __launch_bounds__(kMiNT) void mi_lnpj_kernel(const int64_t* __restrict__ pj, int n, double* __restrict__ lnpj) {
    const int64_t j = (int64_t)blockIdx.x * kMiNT + threadIdx.x;
    if (j >= n) return;
    const int64_t v = pj[j];
    lnpj[j] = v > 0 ? log((double)v) : 0.0;
}

__global__ __launch_bounds__(kSpgemmHashNT) void mi_hash_kernel(MiRowArgs g) {
    __shared__ int keys[kSpgemmHashCap];
    __shared__ int vals[kSpgemmHashCap];
    __shared__ double w_s1[kSpgemmHashNT / 64];
    __shared__ long long w_pi[kSpgemmHashNT / 64];
    constexpr int kWaves = kSpgemmHashNT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    const int cap = spgemm_hash_cap(g.u[row]);
    if (cap == 0) return;                                                   // the tile kernel's row
    (void)spgemm_hash_accumulate<true>(g.A, g.B, g.p, g.n, row, cap, keys, vals);
    __syncthreads();
    spgemm_hash_sort(cap, keys, vals);                                      // ascending columns first, the empty slots last
    double s1 = 0.0;
    long long pi = 0;
    for (int j = tid; j < cap; j += kSpgemmHashNT) {
        const int col = keys[j];
        if (col < 0) break;                                                 // sorted: nothing occupied lies behind an empty slot
        const int c = vals[j];
        if (c <= 0) continue;                                               // (never under the contract)
        pi += c;
        s1 += (double)c * (log((double)c) - g.lnpj[col]);
    }
    s1 = mi_wave_sum(s1);
    pi = mi_wave_sum(pi);
    if (lane == 0) { w_s1[wave] = s1; w_pi[wave] = pi; }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        long long t = 0;
        for (int w = 0; w < kWaves; ++w) { s += w_s1[w]; t += w_pi[w]; }
        g.row_s1[row] = s;
        g.row_pi[row] = t;
    }
}

// (8 waves per SIMD: two workgroups of 16 waves on a CU need the kernel inside 64 vector registers - without the bound the
//  fp64 logarithm takes 78 and the LDS claim's second workgroup never arrives; 64 without a spill with it)
__global__ __launch_bounds__(kSpgemmTileNT, 8) void mi_tile_kernel(MiRowArgs g) {
    __shared__ __attribute__((aligned(16))) int tile[kCoocTile];
    __shared__ int64_t s_lo[kSpgemmStage], s_hi[kSpgemmStage];
    __shared__ int s_val[kSpgemmStage];
    __shared__ double w_s1[kSpgemmTileNT / 64];
    __shared__ long long w_pi[kSpgemmTileNT / 64];
    constexpr int kWaves = kSpgemmTileNT / 64, kSeg = kCoocTile / kWaves;       // cells of the tile one wave reduces
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    if (g.u[row] <= kSpgemmHashProducts) return;                            // the hash kernel's row
    const int64_t alo = g.A.indptr[row], ahi = g.A.indptr[row + 1];
    double row_s1 = 0.0;                                                    // (every thread keeps the same running sums)
    long long row_pi = 0;
    for (int col0 = 0; col0 < g.n; col0 += kCoocTile) {
        const int col1 = min(col0 + kCoocTile, g.n), width = col1 - col0;
        spgemm_tile_accumulate<true>(g.A, g.B, g.p, alo, ahi, col0, col1, tile, s_lo, s_hi, s_val);
        double s1 = 0.0;
        long long pi = 0;
        for (int j = wave * kSeg + lane; j < (wave + 1) * kSeg; j += 64) {
            const int c = j < width ? tile[j] : 0;
            if (c > 0) {
                pi += c;
                s1 += (double)c * (log((double)c) - g.lnpj[col0 + j]);
            }
        }
        s1 = mi_wave_sum(s1);
        pi = mi_wave_sum(pi);
        if (lane == 0) { w_s1[wave] = s1; w_pi[wave] = pi; }
        __syncthreads();
        double ts = 0.0;
        long long tp = 0;
        for (int w = 0; w < kWaves; ++w) { ts += w_s1[w]; tp += w_pi[w]; }
        row_s1 += ts;
        row_pi += tp;
        __syncthreads();                                                    // the partials and the tile are free again
    }
    if (tid == 0) { g.row_s1[row] = row_s1; g.row_pi[row] = row_pi; }
}

// out: double mi at byte 0, int64 T at byte 8
__global__ __launch_bounds__(kMiFinishNT) void mi_finish_kernel(int m, const double* __restrict__ row_s1,
                                                                const int64_t* __restrict__ row_pi, void* out) {
    __shared__ double w_s[kMiFinishNT / 64];
    __shared__ long long w_t[kMiFinishNT / 64];
    constexpr int kWaves = kMiFinishNT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long t = 0;
    for (int i = tid; i < m; i += kMiFinishNT) t += row_pi[i];
    t = mi_wave_sum(t);
    if (lane == 0) w_t[wave] = t;
    __syncthreads();
    long long T = 0;
    for (int w = 0; w < kWaves; ++w) T += w_t[w];
    const double lnT = T > 0 ? log((double)T) : 0.0;
    double s = 0.0;
    for (int i = tid; i < m; i += kMiFinishNT) {
        const int64_t pi = row_pi[i];
        if (pi > 0) s += row_s1[i] + (double)pi * (lnT - log((double)pi));
    }
    s = mi_wave_sum(s);
    if (lane == 0) w_s[wave] = s;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int w = 0; w < kWaves; ++w) sum += w_s[w];
        const double mi = T > 0 ? sum / (double)T : 0.0;
        *static_cast<double*>(out) = mi > 0.0 ? mi : 0.0;
        *reinterpret_cast<int64_t*>(static_cast<char*>(out) + 8) = T;
    }
}

}  // namespace aae
