// Long recommendation lists: top-k for 32 < k <= 1024 (the reference's MPD driver ranks 500 items per row with the same
// predict -> remove_non_missing -> argtopk, evaluation.py:183-199, 20-58).  rank_x3.h keeps a sorted list of K <= 32 entries
// per thread in registers; a list of 500 does not fit there, so the long path selects by THRESHOLD:
//
//   fused form (handles with rank_ok)
//     1. rank_x3_kernel<NB, 32>          unchanged: [rows][wgs][32] candidates + (min, max) per (row, workgroup)
//     2. rank_floor_kernel               per row the k-th best logit among its candidates = tau0, a lower bound of the row's true
//                                        k-th best (the candidates are rankable items of the row); fewer than k candidates:
//                                        tau0 = -inf.  Zeroes the row's counter.
//     3. rank_x3_kernel<NB, 1, WIN, true> the same front end (same products, same bits) with the COLLECT epilogue: every
//                                        rankable cell with logit >= tau0 is appended to the row's list (int32 counter per row,
//                                        64-bit entries: order-preserving key of the logit | ~item)
//     4. rank_long_sort_kernel           one workgroup per row: bitonic sort of the row's entries in LDS (logit descending,
//                                        smaller item id first at equal logits - the entry's integer order, so the output does
//                                        not depend on the order the appends arrived in), sigmoid + min-max scaling as
//                                        rank_merge_kernel, the k best written.  A row with more entries than the list holds
//                                        is left to the host (abi_rank.h: the dense form ranks it).
//   dense form (every other handle; the overflow fallback)
//     rank_long_dense_kernel             one workgroup per row of the [rows][N] score matrix: known items masked as
//                                        topk_rows_kernel (kernels.h) masks them, radix select (4 x 8 bits of the key) of the k-th
//                                        best value T, every item above T + the smallest ids among the items equal to T, the
//                                        same LDS sort.  Templated on the score type (DenseScore): float, what every caller
//                                        but one launches, and int32_t - the co-occurrence scores ranked as the integers they
//                                        are (abi_cooc.h aae_cooc_topk_i32): the keys are the scores, so the order is exact up to
//                                        2^31 where fp32 keys tie from 2^24 on.
// A row with fewer than k rankable items: its items, then id -1 / score 0 - what topk_rows_kernel and rank_merge_kernel emit.
#pragma once
#include <limits.h>

#include "rank_x3.h"

namespace aae {

constexpr int kLongKMax = 1024;        // longest list
constexpr int kLongCap = 4096;         // entries of a row's collect list (and of the LDS sort): 32 KB per row
constexpr int kLongNT = 1024;

// order-preserving map float -> unsigned (a < b <=> key(a) < key(b); -0 < +0) and back
__device__ __forceinline__ unsigned ord_key(float v) {
    const unsigned u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ord_val(unsigned k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
// The score type of the dense rank kernels (rank_long_dense_kernel, rank_full.h rank_full_dense_kernel): the value a known item
// is masked to (below every real score), its counterpart above every score, the order-preserving key and its inverse, the
// conversion to float (round to nearest) the scaled value is formed from.  int32_t: lowest() is key 0, and the caller keeps
// every real score strictly above it.
template <class SC> struct DenseScore;
template <> struct DenseScore<float> {
    static __device__ __forceinline__ float lowest() { return -INFINITY; }
    static __device__ __forceinline__ float highest() { return INFINITY; }
    static __device__ __forceinline__ unsigned key(float v) { return ord_key(v); }
    static __device__ __forceinline__ float unkey(unsigned k) { return ord_val(k); }
    static __device__ __forceinline__ float to_float(float v) { return v; }
    static __device__ __forceinline__ float lesser(float a, float b) { return fminf(a, b); }
    static __device__ __forceinline__ float greater(float a, float b) { return fmaxf(a, b); }
};
template <> struct DenseScore<int32_t> {
    static __device__ __forceinline__ int32_t lowest() { return INT_MIN; }
    static __device__ __forceinline__ int32_t highest() { return INT_MAX; }
    static __device__ __forceinline__ unsigned key(int32_t v) { return (unsigned)v ^ 0x80000000u; }
    static __device__ __forceinline__ int32_t unkey(unsigned k) { return (int32_t)(k ^ 0x80000000u); }
    static __device__ __forceinline__ float to_float(int32_t v) { return __int2float_rn(v); }
    static __device__ __forceinline__ int32_t lesser(int32_t a, int32_t b) { return min(a, b); }
    static __device__ __forceinline__ int32_t greater(int32_t a, int32_t b) { return max(a, b); }
};
__device__ __forceinline__ unsigned long long long_entry(unsigned key, int item) {
    return ((unsigned long long)key << 32) | (unsigned)~item;        // (descending: larger key, then smaller item; 0 = no item)
}

// The k-th largest of n keys (1 <= k <= n), by the whole workgroup: four passes of an 8-bit histogram, most significant
// byte first.  Returns the key; *ties = how many of the keys EQUAL to it belong to the k best (k - *ties keys are larger).
// hist: int[256] + int[2] of LDS.  All threads call it; it ends behind a barrier.
template <class KeyOf>
__device__ unsigned block_select_kth(KeyOf key_of, int n, int k, int* hist, int* ties) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    int* state = hist + 256;
    unsigned prefix = 0u; int kk = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += nt) hist[i] = 0;
        __syncthreads();
        const unsigned mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int i = tid; i < n; i += nt) {
            const unsigned key = key_of(i);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid < 64) {     // lane l: bins 255 - 4 l .. 252 - 4 l; the bin in which the running count from the top reaches kk
            int c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = hist[255 - (4 * lane + j)];
            const int sum = c[0] + c[1] + c[2] + c[3];
            int incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
            int excl = incl - sum;
            if (excl < kk && kk <= incl) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (kk <= excl + c[j]) { state[0] = 255 - (4 * lane + j); state[1] = kk - excl; break; }
                    excl += c[j];
                }
            }
        }
        __syncthreads();
        prefix |= (unsigned)state[0] << shift; kk = state[1];
        __syncthreads();
    }
    *ties = kk;
    return prefix;
}

// bitonic sort of P (a power of two) 64-bit entries in LDS, descending; ends behind a barrier
__device__ __forceinline__ void block_sort_desc(unsigned long long* e, int P) {
    const int tid = threadIdx.x, nt = blockDim.x;
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += nt) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = e[i], b = e[x];
                    const bool desc = (i & k2) == 0;
                    if (desc ? a < b : a > b) { e[i] = b; e[x] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// ---- fused form -------------------------------------------------------------------------------------------------
// One workgroup per row: tau[row] = the k-th best logit of the row's n = wgs * 32 candidates (unused slots carry item -1),
// -inf where it has fewer than k; count[row] = 0 for the collect launch.
__global__ __launch_bounds__(256) void rank_floor_kernel(const float* __restrict__ cand_v, const int* __restrict__ cand_i, int n,
                                                         int k, float* __restrict__ tau, int* __restrict__ count) {
    __shared__ int hist[258];
    const int row = blockIdx.x;
    const float* cv = cand_v + (size_t)row * n;
    const int* ci = cand_i + (size_t)row * n;
    if (threadIdx.x == 0) count[row] = 0;
    if (n < k) { if (threadIdx.x == 0) tau[row] = -INFINITY; return; }
    int ties;
    const unsigned T = block_select_kth([&](int i) { return ci[i] >= 0 ? ord_key(cv[i]) : 0u; }, n, k, hist, &ties);
    if (threadIdx.x == 0) tau[row] = T ? ord_val(T) : -INFINITY;
}

// One workgroup per row: the row's collected entries sorted, the k best scaled and written.  count[row] > cap: nothing is
// written for the row (the host sees the count and ranks the row through the score matrix).
__global__ __launch_bounds__(kLongNT) void rank_long_sort_kernel(const unsigned long long* __restrict__ list,
                                                                 const int* __restrict__ count, int cap,
                                                                 const float* __restrict__ mm, int wgs, int k_out,
                                                                 int* __restrict__ idx_out, float* __restrict__ val_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ent[];
    __shared__ float s_min[kLongNT / 64], s_max[kLongNT / 64];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = count[row];
    if (n > cap) return;
    int P = 2;
    while (P < n) P <<= 1;
    const unsigned long long* src = list + (size_t)row * cap;
    for (int i = tid; i < P; i += kLongNT) ent[i] = i < n ? src[i] : 0ull;
    float vmin = INFINITY, vmax = -INFINITY;
    for (int w = tid; w < wgs; w += kLongNT) {
        const size_t slot = (size_t)row * wgs + w;
        vmin = fminf(vmin, mm[2 * slot]); vmax = fmaxf(vmax, mm[2 * slot + 1]);
    }
    for (int o = 32; o > 0; o >>= 1) { vmin = fminf(vmin, __shfl_xor(vmin, o, 64)); vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64)); }
    if (lane == 0) { s_min[wave] = vmin; s_max[wave] = vmax; }
    block_sort_desc(ent, P);
    for (int w = 0; w < kLongNT / 64; ++w) { vmin = fminf(vmin, s_min[w]); vmax = fmaxf(vmax, s_max[w]); }
    const float smin = sigmoidf_(vmin), smax = sigmoidf_(vmax);
    const float span = smax - smin;
    const float inv = span > 0.f ? 1.f / span : 1.f;
    for (int r = tid; r < k_out; r += kLongNT) {
        const unsigned long long e = r < n ? ent[r] : 0ull;
        const int item = (int)~(unsigned)e;
        idx_out[(size_t)row * k_out + r] = item;
        val_out[(size_t)row * k_out + r] = item >= 0 ? (sigmoidf_(ord_val((unsigned)(e >> 32))) - smin) * inv : 0.f;
    }
}

// ---- dense form -------------------------------------------------------------------------------------------------
// One workgroup per row of the score matrix (sigmoids; SC = int32_t: whole-number scores).  As topk_rows_kernel: known items
// are masked to -inf (DenseScore<SC>::lowest()) in place, their scores still enter the row minimum / maximum - kept in SC, so
// the integer form's are exact.  Ties of the k-th value go to the smaller item ids.
// The scaled value is (float(v) - float(min)) * inv, span = float(max) - float(min), inv = span > 0 ? 1 / span : 1.
template <class SC>
__global__ __launch_bounds__(kLongNT) void rank_long_dense_kernel(SC* __restrict__ scores, int ld, int n_items, BatchView bv,
                                                                  int exclude_known, int k_out, int* __restrict__ idx_out,
                                                                  float* __restrict__ val_out) {
    using D = DenseScore<SC>;
    __shared__ unsigned long long ent[kLongKMax];
    __shared__ int hist[258];
    __shared__ SC s_min[kLongNT / 64], s_max[kLongNT / 64];
    __shared__ int s_w[kLongNT / 64];
    __shared__ int s_n;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SC* sc = scores + (size_t)row * ld;
    SC vmin = D::highest(), vmax = D::lowest();
    if (exclude_known) {
        const int dc = bv.doc(row);
        const int64_t lo = bv.indptr[dc], hi = bv.indptr[dc + 1];
        for (int64_t e = lo + tid; e < hi; e += kLongNT) {
            const int i = bv.indices[e];
            const SC v = sc[i];
            vmin = D::lesser(vmin, v); vmax = D::greater(vmax, v);
            sc[i] = D::lowest();
        }
    }
    if (tid == 0) s_n = 0;
    for (int i = tid; i < kLongKMax; i += kLongNT) ent[i] = 0ull;
    __syncthreads();
    for (int i = tid; i < n_items; i += kLongNT) {
        const SC v = sc[i];
        if (v != D::lowest()) { vmin = D::lesser(vmin, v); vmax = D::greater(vmax, v); }
    }
    for (int o = 32; o > 0; o >>= 1) { vmin = D::lesser(vmin, __shfl_xor(vmin, o, 64)); vmax = D::greater(vmax, __shfl_xor(vmax, o, 64)); }
    if (lane == 0) { s_min[wave] = vmin; s_max[wave] = vmax; }
    int ties;
    const unsigned T = block_select_kth([&](int i) { return D::key(sc[i]); }, n_items, k_out, hist, &ties);
    for (int w = 0; w < kLongNT / 64; ++w) { vmin = D::lesser(vmin, s_min[w]); vmax = D::greater(vmax, s_max[w]); }
    const float fmin_ = D::to_float(vmin);
    const float span = D::to_float(vmax) - fmin_;
    const float inv = span > 0.f ? 1.f / span : 1.f;
    const int above = k_out - ties;                 // items strictly better than T: all of them belong to the list
    for (int i = tid; i < n_items; i += kLongNT) {
        const unsigned key = D::key(sc[i]);
        if (key > T) { const int pos = atomicAdd(&s_n, 1); if (pos < kLongKMax) ent[pos] = long_entry(key, i); }
    }
    // the `ties` smallest ids among the items equal to T (T = a masked item's -inf - key 0 in the integer form: the row has
    // fewer than k rankable items, the rest of the list stays empty)
    if (T != D::key(D::lowest())) {
        int base = 0;
        for (int i0 = 0; i0 < n_items && base < ties; i0 += kLongNT) {
            const int i = i0 + tid;
            const bool hit = i < n_items && D::key(sc[i]) == T;
            const unsigned long long bal = __ballot(hit);
            if (lane == 0) s_w[wave] = __popcll(bal);
            __syncthreads();
            int before = base, total = base;
            for (int w = 0; w < kLongNT / 64; ++w) { if (w < wave) before += s_w[w]; total += s_w[w]; }
            before += __popcll(bal & ((1ull << lane) - 1ull));
            if (hit && before < ties) ent[above + before] = long_entry(T, i);
            base = total;
            __syncthreads();
        }
    }
    int P = 2;
    while (P < k_out) P <<= 1;
    block_sort_desc(ent, P);
    for (int r = tid; r < k_out; r += kLongNT) {
        const unsigned long long e = ent[r];
        const int item = (int)~(unsigned)e;
        idx_out[(size_t)row * k_out + r] = item;
        val_out[(size_t)row * k_out + r] = item >= 0 ? (D::to_float(D::unkey((unsigned)(e >> 32))) - fmin_) * inv : 0.f;
    }
}

}  // namespace aae
